"""Reverse NAT of service replies on the conntrack paths
(cgpu_classify_v{4,6}_ct_rnat / _ctlb_rnat, Engine rev_nat=True).

The compiled-reference harness mocks cilium_lb{4,6}_reverse_nat as always
missing, so the reference for the new outputs is the numpy restatement below
of bpf/lib/lb.h:218-294, :485-576 and of the four call sites in
bpf/bpf_lxc.c, applied to batches whose hit entry (its rev_nat_index and
lb_loopback) is known by construction: entries installed with ct4_update /
ct6_update, or created earlier in the same stream by packets whose service is
known.  Everything the calls returned before (verdict, ct_ret, identity, stage,
the translated daddr / dport, the CT map, the policy counters) is checked to
be what it is without the output."""
import itertools

import numpy as np
import pytest

from cilium_amd import build, layouts as L, synth

pytestmark = pytest.mark.gpu

LOOPBACK = 0x1ffff50a  # IPV4_LOOPBACK (node_config.h:45), the raw network-order word
TCP, UDP, ICMP, ICMP6 = 6, 17, 1, 58
ACK, SYN, SYNACK = (5 << 4) | (16 << 8), (5 << 4) | (2 << 8), (5 << 4) | (18 << 8)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a device"
    build.build()
    return torch


def _engine(**kw):
    from cilium_amd.engine import Engine
    return Engine(device=0, **kw)


def be16(x):
    """host-order port(s) -> the network-order u16 the columns hold"""
    return np.asarray(x).astype(np.uint16).byteswap()


# --------------------------------------------------------------------------
# the restatement
# --------------------------------------------------------------------------
def restate_v4(t, ct_ret, idx, loop, rmap, frame_sa=None, frame_da=None):
    """lb4_rev_nat at its two call sites.  idx / loop: rev_nat_index (raw) and
    lb_loopback of the entry each packet hit (ct_state, conntrack.h ct_lookup4;
    anything for CT_NEW); rmap: {raw index: (address, port)}; frame_sa /
    frame_da: the frame before the step (default: the input columns)."""
    sa = (t["saddr"] if frame_sa is None else frame_sa).astype(np.uint32).copy()
    da = (t["daddr"] if frame_da is None else frame_da).astype(np.uint32).copy()
    sp = t["sport"].astype(np.uint16).copy()
    applied = np.zeros(len(sa), np.uint8)
    for i in range(len(sa)):
        hit = ct_ret[i] in (L.CT_ESTABLISHED, L.CT_REPLY, L.CT_RELATED)
        ix, lo = (int(idx[i]), bool(loop[i])) if hit else (0, False)
        if t["flags"][i] & 1:
            # bpf_lxc.c:531-541: case CT_REPLY / CT_RELATED, if (ct_state.rev_nat_index)
            go = ct_ret[i] in (L.CT_REPLY, L.CT_RELATED) and ix != 0
        else:
            # bpf_lxc.c:909-918: ret == CT_REPLY && rev_nat_index && !loopback
            go = ct_ret[i] == L.CT_REPLY and ix != 0 and not lo
        if not go:
            continue
        nat = rmap.get(ix)  # lb.h:570-572: a miss returns 0, nothing changed
        if nat is None:
            continue
        addr, port = nat
        if port and t["proto"][i] in (TCP, UDP):  # lb.h:496-500, :218-252 (ICMP: break)
            sp[i] = port
        old_sip = sa[i]  # lb.h:502-511 (both flag values: the frame's saddr)
        if lo:           # lb.h:513-535: daddr := old_sip
            da[i] = old_sip
        sa[i] = addr     # lb.h:537
        applied[i] = 1
    return sa, da, sp, applied


def restate_v6(t, ct_ret, idx, rmap):
    """lb6_rev_nat (lb.h:254-317) at bpf_lxc.c:222-235 (egress: CT_REPLY /
    CT_RELATED with rev_nat_index) and :778-785 (ingress: any ct_state with
    rev_nat_index; a CT_NEW packet's ct_state is empty)."""
    sa = t["saddr"].copy()
    sp = t["sport"].astype(np.uint16).copy()
    applied = np.zeros(len(sa), np.uint8)
    for i in range(len(sa)):
        hit = ct_ret[i] in (L.CT_ESTABLISHED, L.CT_REPLY, L.CT_RELATED)
        ix = int(idx[i]) if hit else 0
        if t["flags"][i] & 1:
            go = ct_ret[i] in (L.CT_REPLY, L.CT_RELATED) and ix != 0
        else:
            go = ix != 0
        nat = rmap.get(ix) if go else None  # lb.h:312-314
        if nat is None:
            continue
        addr, port = nat
        if port and t["proto"][i] in (TCP, UDP):  # lb.h:267-271, :218-252
            sp[i] = port
        sa[i] = np.frombuffer(addr, np.uint8)  # lb.h:273-287
        applied[i] = 1
    return sa, sp, applied


def _rn(out, v6=False):
    r = {"sport": out["rn_sport"].cpu().numpy().view(np.uint16),
         "applied": out["rn_applied"].cpu().numpy(),
         "ct_ret": out["ct_ret"].cpu().numpy(), "verdict": out["verdict"].cpu().numpy()}
    if v6:
        r["saddr"] = out["rn_saddr"].cpu().numpy()
    else:
        r["saddr"] = out["rn_saddr"].cpu().numpy().view(np.uint32)
        r["daddr"] = out["rn_daddr"].cpu().numpy().view(np.uint32)
    return r


def _check4(got, exp, msg):
    for f, x in zip(("saddr", "daddr", "sport", "applied"), exp):
        np.testing.assert_array_equal(got[f], x, err_msg=f"{msg} rn_{f}")


# --------------------------------------------------------------------------
# 1. IPv4, pre-installed entries, cgpu_classify_v4_ct_rnat
# --------------------------------------------------------------------------
LOCAL4 = L.ip4_be("10.200.0.1")
# raw indices (the datapath's word): high bit set, both bytes used, byte-swapped twins
IDX_PORT = [0x0100, 0x0007, 0xFFFF, 0x8001]
IDX_PORT0 = [0x0200, 0x1234]
IDX_MISS = [0x0300, 0xFFFE, 0x0001]  # 0x0001: the twin of mapped 0x0100
K_ZERO, K_PORT, K_PORT0, K_MISS = 0, 1, 2, 3
# (index kind, lb_loopback, protocol, egress, port orientation)
CASES4 = list(itertools.product([K_PORT, K_PORT0, K_MISS, K_ZERO], [0, 1], [TCP, UDP, ICMP], [1, 0], [0, 1]))


def _rmap4():
    m = {}
    for j, ix in enumerate(IDX_PORT):
        m[ix] = (L.ip4_be(f"10.96.1.{j + 1}"), int(be16(8000 + j)))
    for j, ix in enumerate(IDX_PORT0):
        m[ix] = (L.ip4_be(f"10.96.2.{j + 1}"), 0)
    return m


def _idx_of(kind, c):
    return {K_ZERO: 0, K_PORT: IDX_PORT[c % len(IDX_PORT)], K_PORT0: IDX_PORT0[c % len(IDX_PORT0)],
            K_MISS: IDX_MISS[c % len(IDX_MISS)]}[kind]


def build_v4_hits(n):
    """n reply-direction packets over ceil(n / 2) connections (n > 256: each
    connection twice), every one a pure hit of an entry installed beforehand.
    Returns (t, entries [(key, val)], expected ct_ret, idx, loop, case)."""
    nconn = n if n <= 257 else (n + 1) // 2
    keys, vals = [], []
    cols = {k: [] for k in ("saddr", "daddr", "sport", "dport", "proto", "l4b", "flags", "len", "ep")}
    meta = []
    for c in range(nconn):
        kind, loop, proto, egress, orient = CASES4[c % len(CASES4)]
        rem = L.ip4_be(0x0B000000 + c + 1)  # one remote per connection: one address pair each
        lp = 2000 + c % 30000
        rp = lp + 7 if orient == 0 else lp - 7  # local port below / above the remote one
        sa, da = (LOCAL4, rem) if egress else (rem, LOCAL4)
        sp, dp = (lp, rp) if egress else (rp, lp)
        idx = _idx_of(kind, c)
        k = np.zeros((), L.CT4_TUPLE)
        k["daddr"], k["saddr"], k["nexthdr"] = da, sa, proto
        k["flags"] = L.TUPLE_F_IN if egress else L.TUPLE_F_OUT
        if proto == ICMP:  # an ICMP error resolves RELATED on the pair's related entry
            k["flags"] |= L.TUPLE_F_RELATED
        else:  # the reply-direction tuple: dport <- the packet's sport (conntrack.h:500-504)
            k["dport"], k["sport"] = int(be16(sp)), int(be16(dp))
        v = np.zeros((), L.CT_ENTRY)
        v["lifetime"], v["rev_nat_index"], v["bits"] = 100000, idx, 16 | (8 if loop else 0)
        v["src_sec_id"] = 5000
        keys.append(k)
        vals.append(v)
        cols["saddr"].append(sa)
        cols["daddr"].append(da)
        cols["sport"].append(int(be16(sp)))
        cols["dport"].append(int(be16(dp)))
        cols["proto"].append(proto)
        cols["l4b"].append(ACK if proto == TCP else [3, 11, 12][c % 3] if proto == ICMP else 0)
        cols["flags"].append(egress)
        cols["len"].append(64 + c % 1000)
        cols["ep"].append(0)
        meta.append((L.CT_RELATED if proto == ICMP else L.CT_REPLY, idx, loop, c % len(CASES4)))
    order = np.arange(n) % nconn  # c0 .. c(nconn-1), then again
    dt = {"saddr": np.uint32, "daddr": np.uint32, "sport": np.uint16, "dport": np.uint16, "proto": np.uint8,
          "l4b": np.uint16, "flags": np.uint8, "len": np.uint32, "ep": np.uint16}
    t = {k: np.array(x, dt[k])[order] for k, x in cols.items()}
    m = np.array(meta, np.int64)[order]
    return t, list(zip(keys, vals)), m[:, 0].astype(np.uint8), m[:, 1], m[:, 2], m[:, 3]


def _env4(e):
    synth.load_lxc(e, [5000])
    for ix, (addr, port) in _rmap4().items():
        v = np.zeros((), L.LB4_REVERSE_NAT)
        v["address"], v["port"] = addr, port
        assert e.revnat4_update(ix, v) == 0


@pytest.mark.parametrize("cfg", [dict(schedule=0), dict(schedule=8 << 8), dict(schedule=0, ct_lru=1)],
                         ids=["default", "sort8", "lru"])
@pytest.mark.parametrize("n", [1, 257, 5000])
def test_v4_preinstalled_hits(torch_cuda, n, cfg):
    t, ents, cr, idx, loop, case = build_v4_hits(n)
    exp = restate_v4(t, cr, idx, loop, _rmap4())
    if n >= 257:  # every category of the issue is in the batch
        eg, ic = (t["flags"] & 1) == 1, t["proto"] == ICMP
        ap = exp[3] == 1
        mapped = np.isin(idx, IDX_PORT + IDX_PORT0)
        assert (~eg & (cr == L.CT_RELATED) & mapped & ~ap).any()           # ingress RELATED: not rewritten
        assert (~eg & (cr == L.CT_REPLY) & mapped & (loop == 1) & ~ap).any()  # ingress REPLY, loopback: not
        assert (~eg & (cr == L.CT_REPLY) & mapped & (loop == 0) & ap).any()
        assert (eg & (cr == L.CT_RELATED) & ap).any()                      # egress RELATED: rewritten
        lo_eg = eg & (cr == L.CT_REPLY) & (loop == 1) & ap
        assert lo_eg.any() and (exp[1][lo_eg] == t["saddr"][lo_eg]).all()  # daddr := old saddr
        assert (ic & ap).any() and (exp[2][ic] == t["sport"][ic]).all()    # ICMP keeps its port word
        assert ((idx == 0) & ~ap).any() and (np.isin(idx, IDX_MISS) & ~ap).any()
        assert (ap & np.isin(idx, IDX_PORT0)).any() and (exp[2][ap & np.isin(idx, IDX_PORT0)] ==
                                                         t["sport"][ap & np.isin(idx, IDX_PORT0)]).all()
        tu = ap & np.isin(idx, IDX_PORT) & ~ic
        assert tu.any() and (exp[2][tu] != t["sport"][tu]).all()
        assert len(set(case.tolist())) == len(CASES4)
    e = _engine(ct_max=1 << 14, **cfg)
    _env4(e)
    e.commit()
    for k, v in ents:
        assert e.ct4_update(k, v) == 0
    got = _rn(e.classify_v4_ct(synth.to_device(t), 1000, rev_nat=True))
    torch_cuda.cuda.synchronize()
    np.testing.assert_array_equal(got["ct_ret"], cr)
    _check4(got, exp, f"n={n} {cfg}")
    e.close()


# --------------------------------------------------------------------------
# 2. IPv4, entries created in the batch, cgpu_classify_v4_ctlb_rnat
# --------------------------------------------------------------------------
# (vip, vip port, backend, backend port, rev_nat index (host order))
SVCS4 = [("10.96.0.1", 80, "10.1.0.1", 8080, 1),       # port translated both ways
         ("10.96.0.2", 443, "10.1.0.2", 443, 2),       # backend port = VIP port
         ("10.96.0.3", 0, "10.1.0.3", 0, 3),           # L3-only service: nat.port 0
         ("10.96.0.4", 80, "10.200.0.1", 8080, 0x0104)]  # the backend is the sender: loopback


def _env_ctlb4(target):
    """The same tables into an Engine or the CPU restatement (Oracle)."""
    for cidr, ident in (("0.0.0.0/0", L.WORLD_ID), ("10.1.0.0/16", 300), ("10.96.0.0/16", 301),
                        ("10.200.0.0/16", 302)):
        assert target.ipcache_update(L.ipcache_key(cidr), L.remote_info(ident)) == 0
    for ident in (300, 301, 302, L.WORLD_ID):
        assert target.policy_update(0, L.policy_key(ident, 0, 0, 1), L.policy_entry()) == 0
    put = target.lb4_update if hasattr(target, "lb4_update") else target.lb_update
    for vip, port, be, bport, rn in SVCS4:
        assert put(L.lb4_key(vip, port, 1), L.lb4_service(be, bport, 0, rn, 1)) == 0
        assert put(L.lb4_key(vip, port, 0), L.lb4_service(0, 0, 1, 0, 1)) == 0
    synth.load_lxc(target, [5000])


def _rmap_ctlb4():
    return {L.revnat_index(rn): (L.ip4_be(vip), int(be16(port))) for vip, port, _, _, rn in SVCS4}


def build_v4_ctlb(nconn, extra_syn=0):
    """Per connection, interleaved over the batch: the egress SYN to the VIP,
    the backend's reply, an egress ACK, a second reply.  Returns (t, expected
    ct_ret, idx, loop, the frame's saddr / daddr after the service step,
    reply mask)."""
    from cilium_amd.shard import flowhash_np
    rows = []
    for rnd in range(4):
        for c in range(nconn + (extra_syn if rnd == 0 else 0)):
            vip, port, be, bport, rn = SVCS4[c % 4]
            loopc = c % 4 == 3
            lp = 20000 + c
            vp = port or 9000  # an L3-only service keeps the packet's port
            bp = bport or vp
            raw = L.revnat_index(rn)
            if rnd in (0, 2):  # egress to the VIP
                rows.append((LOCAL4, L.ip4_be(vip), lp, vp, SYN if rnd == 0 else ACK, 1,
                             L.CT_NEW if rnd == 0 else L.CT_ESTABLISHED, raw, int(loopc),
                             LOOPBACK if loopc else LOCAL4, L.ip4_be(be), 0))
            elif loopc:  # the endpoint answers itself: an egress reply to IPV4_LOOPBACK
                rows.append((LOCAL4, LOOPBACK, bp, lp, SYNACK if rnd == 1 else ACK, 1, L.CT_REPLY, raw, 1,
                             LOCAL4, LOOPBACK, 1))
            else:  # the backend's ingress reply
                rows.append((L.ip4_be(be), LOCAL4, bp, lp, SYNACK if rnd == 1 else ACK, 0, L.CT_REPLY, raw,
                             0, L.ip4_be(be), LOCAL4, 1))
    r = np.array(rows, np.int64)
    n = len(r)
    t = {"saddr": r[:, 0].astype(np.uint32), "daddr": r[:, 1].astype(np.uint32),
         "sport": be16(r[:, 2]), "dport": be16(r[:, 3]), "proto": np.full(n, TCP, np.uint8),
         "l4b": r[:, 4].astype(np.uint16), "flags": r[:, 5].astype(np.uint8),
         "len": np.full(n, 100, np.uint32), "ep": np.zeros(n, np.uint16)}
    t["hash"] = flowhash_np(t["saddr"], t["daddr"], t["sport"], t["dport"], t["proto"]).astype(np.uint32)
    return (t, r[:, 6].astype(np.uint8), r[:, 7], r[:, 8], r[:, 9].astype(np.uint32),
            r[:, 10].astype(np.uint32), r[:, 11].astype(bool))


@pytest.mark.parametrize("nconn,extra", [(64, 1), (1250, 0)], ids=["257", "5000"])
def test_v4_ctlb_in_batch(torch_cuda, nconn, extra):
    t, cr, idx, loop, fsa, fda, reply = build_v4_ctlb(nconn, extra)
    assert len(t["saddr"]) in (257, 5000)
    rmap = _rmap_ctlb4()
    exp = restate_v4(t, cr, idx, loop, rmap, fsa, fda)
    # the replies come back as {VIP, VIP port}; forward packets keep their source
    # (IPV4_LOOPBACK where the backend is the sender); loopback replies get daddr := saddr
    assert (exp[3] == reply).all()
    assert (exp[0][~reply] == fsa[~reply]).all() and (fsa[~reply] == LOOPBACK).any()
    lrep = reply & (loop == 1)
    assert lrep.any() and (exp[1][lrep] == LOCAL4).all() and (exp[0][lrep] == L.ip4_be("10.96.0.4")).all()
    assert (exp[2][reply] != t["sport"][reply]).any() and (exp[2][reply] == t["sport"][reply]).any()
    e = _engine(ct_max=1 << 15)
    _env_ctlb4(e)
    for vip, port, _, _, rn in SVCS4:
        e.UpdateRevNat(rn, vip, port)
    e.commit()
    out = e.classify_v4_ctlb(synth.to_device(t), 1000, rev_nat=True)
    torch_cuda.cuda.synchronize()
    got = _rn(out)
    assert (got["verdict"] == 0).all()
    np.testing.assert_array_equal(got["ct_ret"], cr)
    np.testing.assert_array_equal(out["daddr"].cpu().numpy().view(np.uint32), fda)
    _check4(got, exp, "batch 1")
    # replies only, against the map the first batch left (sizes 1 and all of them)
    for sl in (slice(0, 1), slice(None)):
        t2 = {k: x[reply][sl] for k, x in t.items()}
        exp2 = tuple(x[reply][sl] for x in exp)
        got2 = _rn(e.classify_v4_ctlb(synth.to_device(t2), 1001, rev_nat=True))
        torch_cuda.cuda.synchronize()
        assert (got2["ct_ret"] == L.CT_REPLY).all()
        _check4(got2, exp2, "replies only")
    e.close()


# --------------------------------------------------------------------------
# 3. IPv6
# --------------------------------------------------------------------------
ROUTER6 = bytes.fromhex("f00d0000000000000000000000000001")
LOCAL6 = bytes.fromhex("f00d0000000000000000c0a800000001")  # s6_addr32[3] & 0xFFFF == 0
CASES6 = list(itertools.product([K_PORT, K_PORT0, K_MISS, K_ZERO], [TCP, UDP, ICMP6], [0, 1]))


def _a6(b):
    return np.frombuffer(bytes(b), np.uint8)


def _rmap6():
    m = {}
    for j, ix in enumerate(IDX_PORT):
        m[ix] = (bytes.fromhex("fd000096000000000000000000000000")[:15] + bytes([j + 1]), int(be16(8000 + j)))
    for j, ix in enumerate(IDX_PORT0):
        m[ix] = (bytes.fromhex("fd000097000000000000000000000000")[:15] + bytes([j + 1]), 0)
    return m


def _with_index(addr16, raw):
    """daddr whose s6_addr32[3] & 0xFFFF (bytes 12-13, little endian) is raw"""
    b = bytearray(addr16)
    b[12], b[13] = raw & 0xFF, raw >> 8
    return bytes(b)


def build_v6(n_egress, n_ingress):
    """n_egress pure-hit egress packets (REPLY / RELATED on installed entries,
    the cross product of index kind, protocol and port orientation), then
    n_ingress ingress connections of three packets each, interleaved: the
    first packet (CT_NEW, creates the entry with the index its daddr names),
    a second one (ESTABLISHED), the endpoint's reply (egress, REPLY).
    Returns (t, entries, expected ct_ret, idx)."""
    rows, keys, vals = [], [], []
    for c in range(n_egress):
        kind, proto, orient = CASES6[c % len(CASES6)]
        rem = bytes.fromhex("20010db8000100000000000000000000")[:12] + (c + 1).to_bytes(4, "big")
        lp = 2000 + c % 30000
        rp = lp + 7 if orient == 0 else lp - 7
        idx = _idx_of(kind, c)
        k = np.zeros((), L.CT6_TUPLE)
        k["daddr"][:], k["saddr"][:], k["nexthdr"] = _a6(rem), _a6(LOCAL6), proto
        k["flags"] = L.TUPLE_F_IN
        if proto == ICMP6:
            k["flags"] |= L.TUPLE_F_RELATED
        else:
            k["dport"], k["sport"] = int(be16(lp)), int(be16(rp))
        v = np.zeros((), L.CT_ENTRY)
        v["lifetime"], v["rev_nat_index"], v["bits"], v["src_sec_id"] = 100000, idx, 16, 6000
        keys.append(k)
        vals.append(v)
        rows.append((LOCAL6, rem, lp, rp, proto, ACK if proto == TCP else [1, 2, 3, 4][c % 4] if proto == ICMP6 else 0,
                     1, L.CT_RELATED if proto == ICMP6 else L.CT_REPLY, idx))
    ing = []
    for c in range(n_ingress):
        kind = [K_PORT, K_MISS, K_PORT0][c % 3]
        idx = _idx_of(kind, c)
        rem = bytes.fromhex("20010db8000200000000000000000000")[:12] + (c + 1).to_bytes(4, "big")
        loc = _with_index(LOCAL6, idx)
        lp, rp = 443, 30000 + c
        proto = TCP if c % 2 == 0 else UDP
        ing.append([(rem, loc, rp, lp, proto, SYN if proto == TCP else 0, 0, L.CT_NEW, idx),
                    (rem, loc, rp, lp, proto, ACK if proto == TCP else 0, 0, L.CT_ESTABLISHED, idx),
                    (loc, rem, lp, rp, proto, ACK if proto == TCP else 0, 1, L.CT_REPLY, idx)])
    for rnd in range(3):
        rows += [x[rnd] for x in ing]
    n = len(rows)
    t = {"saddr": np.stack([_a6(r[0]) for r in rows]), "daddr": np.stack([_a6(r[1]) for r in rows]),
         "sport": be16([r[2] for r in rows]), "dport": be16([r[3] for r in rows]),
         "proto": np.array([r[4] for r in rows], np.uint8), "l4b": np.array([r[5] for r in rows], np.uint16),
         "flags": np.array([r[6] for r in rows], np.uint8), "len": np.full(n, 120, np.uint32),
         "ep": np.zeros(n, np.uint16)}
    return (t, list(zip(keys, vals)), np.array([r[7] for r in rows], np.uint8),
            np.array([r[8] for r in rows], np.int64))


def _env6(target):
    assert target.ipcache_update(L.ipcache_key("2001:db8::/32"), L.remote_info(400)) == 0
    for direction in (0, 1):
        assert target.policy_update(0, L.policy_key(400, 0, 0, direction), L.policy_entry()) == 0
    synth.load_lxc(target, [6000])


SVC6 = (bytes.fromhex("fd0000960000000000000000000000aa"), 80,
        bytes.fromhex("20010db80003000000000000000000bb"), 8080, 0x0105)


def _lb6(e):
    vip, port, be, bport, rn = SVC6
    k = np.zeros((), L.LB6_KEY)
    k["address"][:], k["dport"] = _a6(vip), int(be16(port))
    v = np.zeros((), L.LB6_SERVICE)
    v["count"] = 1
    assert e.lb6_update(k, v) == 0
    k["slave"] = 1
    v["count"] = 0
    v["target"][:], v["port"], v["rev_nat_index"] = _a6(be), int(be16(bport)), L.revnat_index(rn)
    v["weight"] = int(be16(1))
    assert e.lb6_update(k, v) == 0


@pytest.mark.parametrize("svc", [False, True], ids=["ct", "ctlb"])
@pytest.mark.parametrize("n_eg,n_in", [(1, 0), (200, 19), (3800, 400)], ids=["1", "257", "5000"])
def test_v6(torch_cuda, n_eg, n_in, svc):
    from cilium_amd.shard import flowhash6_np
    t, ents, cr, idx = build_v6(n_eg, n_in)
    rmap = dict(_rmap6())
    if svc and n_in:
        # one connection to an IPv6 service in the same batch: the egress SYN (the
        # entry takes the service's index), then the backend's reply
        vip, port, be, bport, rn = SVC6
        rmap[L.revnat_index(rn)] = (vip, int(be16(port)))
        add = [(LOCAL6, vip, 40000, port, SYN, 1, L.CT_NEW), (be, LOCAL6, bport, 40000, SYNACK, 0, L.CT_REPLY)]
        t = {k: x.copy() for k, x in t.items()}
        for col, vals in (("saddr", [_a6(a[0]) for a in add]), ("daddr", [_a6(a[1]) for a in add]),
                          ("sport", be16([a[2] for a in add])), ("dport", be16([a[3] for a in add])),
                          ("proto", [TCP, TCP]), ("l4b", [a[4] for a in add]), ("flags", [a[5] for a in add]),
                          ("len", [120, 120]), ("ep", [0, 0])):
            t[col] = np.concatenate([t[col], np.array(vals, t[col].dtype)])
        cr = np.concatenate([cr, np.array([a[6] for a in add], np.uint8)])
        idx = np.concatenate([idx, [L.revnat_index(rn)] * 2])
    n = len(cr)
    exp = restate_v6(t, cr, idx, rmap)
    if n_in:
        eg = (t["flags"] & 1) == 1
        assert (~eg & (cr == L.CT_NEW) & np.isin(idx, IDX_PORT) & (exp[2] == 0)).any()   # first packet: never
        assert (~eg & (cr == L.CT_ESTABLISHED) & (exp[2] == 1)).any()                    # ESTABLISHED: rewritten
        assert (eg & (cr == L.CT_REPLY) & (idx > 0) & (exp[2] == 1)).any()
        assert (~eg & (cr == L.CT_ESTABLISHED) & np.isin(idx, IDX_MISS) & (exp[2] == 0)).any()  # unmapped
        assert (eg & (cr == L.CT_RELATED) & (exp[2] == 1)).any()
        ic = t["proto"] == ICMP6
        assert (exp[1][ic] == t["sport"][ic]).all()
    e = _engine(ct_max=1 << 14, ct6_max=1 << 14, ipv6_router_ip=ROUTER6)
    _env6(e)
    for ix, (addr, port) in rmap.items():
        v = np.zeros((), L.LB6_REVERSE_NAT)
        v["address"][:], v["port"] = _a6(addr), port
        assert e.revnat6_update(ix, v) == 0
    if svc:
        _lb6(e)
    e.commit()
    for k, v in ents:
        assert e.ct6_update(k, v) == 0
    d = synth.to_device(t)
    if svc:
        d["hash"] = synth.to_device({"hash": flowhash6_np(t["saddr"], t["daddr"], t["sport"], t["dport"],
                                                          t["proto"]).astype(np.uint32)})["hash"]
        out = e.classify_v6_ctlb(d, 1000, rev_nat=True)
    else:
        out = e.classify_v6_ct(d, 1000, rev_nat=True)
    torch_cuda.cuda.synchronize()
    got = _rn(out, v6=True)
    np.testing.assert_array_equal(got["ct_ret"], cr)
    np.testing.assert_array_equal(got["applied"], exp[2])
    np.testing.assert_array_equal(got["saddr"], exp[0])
    np.testing.assert_array_equal(got["sport"], exp[1])
    assert e.revnat4_count() == 0
    e.close()


# --------------------------------------------------------------------------
# 4. nothing else moves: the golden streams through the _rnat entry points
# --------------------------------------------------------------------------
def _full_map(e):
    """every index 1..65535 mapped"""
    for ix in range(1, 65536):
        v = np.zeros((), L.LB4_REVERSE_NAT)
        v["address"], v["port"] = 0x0A600000 + ix, ix ^ 0x5555
        assert e.revnat4_update(ix, v) == 0
    assert e.revnat4_count() == 65535


def _golden_run(torch, golden, name, svc, rev_nat):
    g = golden(name)
    e = _engine(ct_max=1 << 20)
    for k, v in zip(g["ipc_keys"], g["ipc_vals"]):
        assert e.ipcache_update(k, v) == 0
    for k, en, ep in zip(g["pol_keys"], g["pol_entries"], g["pol_ep"]):
        assert e.policy_update(int(ep), k, en) == 0
    if svc:
        for k, v in zip(g["lb_keys"], g["lb_vals"]):
            assert e.lb4_update(k, v) == 0
    synth.load_lxc(e, g["seclabels"])
    _full_map(e)
    e.commit()
    for k, v in zip(g["pre_keys"], g["pre_vals"]):
        assert e.ct4_update(k, v) == 0
    t = {k[2:]: g[k] for k in g.files if k.startswith("t_")}
    cuts, nows = g["cuts"], g["nows"]
    off, applied = 0, 0
    for bi in range(4):
        if bi == 2:
            for d in g["pol_del"]:
                assert e.policy_delete(int(g["pol_ep"][d]), g["pol_keys"][d]) == 0
            if svc:
                for d in g["svc_del"]:
                    assert e.lb4_delete(g["lb_keys"][d]) == 0
            e.commit()
        if bi == 3 and svc:
            for d, v in zip(g["svc_readd"], g["readd_vals"]):
                assert e.lb4_update(g["lb_keys"][d], v) == 0
            e.commit()
        sl = slice(int(cuts[bi]), int(cuts[bi + 1]))
        tb = {k: x[sl] for k, x in t.items()}
        fn = e.classify_v4_ctlb if svc else e.classify_v4_ct
        out = fn(synth.to_device(tb), int(nows[bi]), rev_nat=True) if rev_nat else fn(synth.to_device(tb),
                                                                                      int(nows[bi]))
        torch.cuda.synchronize()
        msg = f"{name} batch {bi}"
        np.testing.assert_array_equal(out["verdict"].cpu().numpy(), g["b_verdict"][sl], err_msg=msg)
        np.testing.assert_array_equal(out["ct_ret"].cpu().numpy(), g["b_ct_ret"][sl], err_msg=msg)
        np.testing.assert_array_equal(out["identity"].cpu().numpy().view(np.uint32), g["b_identity"][sl],
                                      err_msg=msg)
        np.testing.assert_array_equal(out["stage"].cpu().numpy(), g["b_stage"][sl], err_msg=msg)
        if svc:
            np.testing.assert_array_equal(out["daddr"].cpu().numpy().view(np.uint32), g["b_xdaddr"][sl],
                                          err_msg=msg)
            m = ((tb["flags"] & 1) == 0) | np.isin(tb["proto"], [6, 17])
            np.testing.assert_array_equal(out["dport"].cpu().numpy().view(np.uint16)[m], g["b_xdport"][sl][m],
                                          err_msg=msg)
        if rev_nat:
            ap = out["rn_applied"].cpu().numpy()
            cr = g["b_ct_ret"][sl]
            assert np.isin(cr[ap == 1], [L.CT_REPLY, L.CT_RELATED]).all()
            applied += int(ap.sum())
        n = int(g["dump_n"][bi])
        keys, vals = e.ct4_dump()
        np.testing.assert_array_equal(keys, g["dump_keys"][off:off + n], err_msg=msg)
        np.testing.assert_array_equal(vals, g["dump_vals"][off:off + n], err_msg=msg)
        assert e.ct4_count() == n
        off += n
    deleted = set(g["pol_del"].tolist())
    for i, (k, ep, fe) in enumerate(zip(g["pol_keys"], g["pol_ep"], g["final_entries"])):
        if i in deleted:
            continue
        rc, got = e.policy_lookup(int(ep), k)
        assert rc == 0
        assert (int(got["packets"]), int(got["bytes"])) == (int(fe["packets"]), int(fe["bytes"]))
    e.close()
    return applied


@pytest.mark.parametrize("name,svc", [("ct4.npz", False), ("ctlb4.npz", True)], ids=["ct4", "ctlb4"])
def test_golden_streams_unmoved(torch_cuda, golden, name, svc):
    """With every index mapped the _rnat calls return the fixture's verdicts,
    ct results, identities, stages, translated daddr / dport, the CT map after
    every batch and the policy counters bit for bit, and so do the calls
    without the output on a context holding the same full map."""
    applied = _golden_run(torch_cuda, golden, name, svc, True)
    if svc:  # the fixture's services carry reverse NAT indices and its stream has their replies
        assert applied > 0
    _golden_run(torch_cuda, golden, name, svc, False)


def test_rn_null_is_the_plain_call(torch_cuda):
    """rn == NULL on the _rnat entry points: the existing calls."""
    import ctypes as C
    from cilium_amd._abi import TuplesV4Ct
    torch = torch_cuda
    t, ents, cr, idx, loop, _ = build_v4_hits(257)
    res = []
    for use_rnat_entry in (False, True):
        e = _engine(ct_max=1 << 14)
        _env4(e)
        e.commit()
        for k, v in ents:
            assert e.ct4_update(k, v) == 0
        d = synth.to_device(t)
        n = len(cr)
        out = {"verdict": torch.empty(n, dtype=torch.int32, device="cuda"),
               "ct_ret": torch.empty(n, dtype=torch.uint8, device="cuda"),
               "identity": torch.empty(n, dtype=torch.int32, device="cuda"),
               "stage": torch.empty(n, dtype=torch.uint8, device="cuda")}
        tv = TuplesV4Ct(*[d[k].data_ptr() for k in ("saddr", "daddr", "sport", "dport", "proto", "l4b", "flags",
                                                    "len", "ep")])
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        args = [e.h, C.byref(tv), n, 1000] + [C.c_void_p(out[k].data_ptr()) for k in ("verdict", "ct_ret",
                                                                                     "identity", "stage")]
        if use_rnat_entry:
            assert e.L.cgpu_classify_v4_ct_rnat(*args, None, st) == 0
        else:
            assert e.L.cgpu_classify_v4_ct(*args, st) == 0
        torch.cuda.synchronize()
        keys, vals = e.ct4_dump()
        res.append([out[k].cpu().numpy() for k in ("verdict", "ct_ret", "identity", "stage")] + [keys, vals])
        e.close()
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


def test_tunnel_and_rev_nat_exclusive(torch_cuda):
    e = _engine(ct_max=1 << 10)
    e.commit()
    t = synth.to_device(build_v4_hits(1)[0])
    with pytest.raises(ValueError):
        e.classify_v4_ct(t, 1, tunnel=True, rev_nat=True)
    with pytest.raises(ValueError):
        e.classify_v6_ct(t, 1, tunnel=True, rev_nat=True)
    e.close()


# --------------------------------------------------------------------------
# 5. properties on a synth stream from an empty map
# --------------------------------------------------------------------------
def test_synth_ctlb_properties(torch_cuda):
    from oracle import Oracle
    T = synth.make_tables(n_prefixes=2000, n_identities=200, n_endpoints=2, keys_per_ep=3000)
    svcs = synth.make_services(T, 300)
    t, locals_be, seclabels, svcs = synth.make_ctlb_workload(T, svcs, 2_500, mean_pkts=8.0, span=0.5)
    n = len(t["saddr"])
    assert 15_000 < n < 25_000
    ns = len(svcs.vip)
    # reverse NAT entries as the agent writes them: every service's index -> {VIP, port}
    rn_of = svcs.vals["rev_nat_index"][ns:]
    rmap = {}
    for k, raw in zip(svcs.keys[ns:], rn_of):
        rmap[int(raw)] = (int(k["address"]), int(k["dport"]))
    # the restatement's ct_ret on the CPU: the stream has replies on service connections
    o = Oracle(**T.oracle_config())
    synth.load_oracle(o, T)
    synth.load_services(o, svcs)
    synth.load_lxc(o, seclabels)
    o.ct_set_max(1 << 18)
    exp = o.classify_v4_ctlb(t, 1000)
    backends = svcs.vals["target"][ns:]
    from_backend = ((t["flags"] & 1) == 0) & np.isin(t["saddr"], backends) & (exp["ct_ret"] == L.CT_REPLY)
    assert from_backend.sum() > 100
    e = _engine(**T.engine_config(), ct_max=1 << 18)
    synth.load_engine(e, T)
    synth.load_services(e, svcs)
    synth.load_lxc(e, seclabels)
    for raw, (addr, port) in rmap.items():
        v = np.zeros((), L.LB4_REVERSE_NAT)
        v["address"], v["port"] = addr, port
        assert e.revnat4_update(raw, v) == 0
    e.commit()
    out = e.classify_v4_ctlb(synth.to_device(t), 1000, rev_nat=True)
    torch_cuda.cuda.synchronize()
    got = _rn(out)
    np.testing.assert_array_equal(got["ct_ret"], exp["ct_ret"])
    np.testing.assert_array_equal(got["verdict"], exp["verdict"])
    ap = got["applied"] == 1
    assert ap.sum() > 0
    assert np.isin(got["ct_ret"][ap], [L.CT_REPLY, L.CT_RELATED]).all()
    assert np.isin(got["saddr"][ap], np.array([a for a, _ in rmap.values()], np.uint32)).all()
    np.testing.assert_array_equal(got["sport"][~ap], t["sport"][~ap])
    assert ((got["saddr"][~ap] == t["saddr"][~ap]) | (got["saddr"][~ap] == LOOPBACK)).all()
    e.close()
