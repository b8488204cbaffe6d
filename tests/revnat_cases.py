"""Builders, environments and the numpy restatement of lb4_rev_nat /
lb6_rev_nat shared by the reverse NAT tests (tests/test_gpu_revnat.py on the
engine, tests/test_oracle_revnat.py on the CPU restatement).

The batches are built so that the entry every packet hits (its rev_nat_index
and lb_loopback) is known by construction: entries installed with ct4_update /
ct6_update, or created earlier in the same stream by packets whose service is
known.  restate_v4 / restate_v6 restate bpf/lib/lb.h:218-294, :485-576 and the
four call sites in bpf/bpf_lxc.c from those known entries.  The environment
loaders take an Engine or an Oracle: both carry the same method names."""
import itertools

import numpy as np

from cilium_amd import layouts as L, synth

LOOPBACK = 0x1ffff50a  # IPV4_LOOPBACK (node_config.h:45), the raw network-order word
TCP, UDP, ICMP, ICMP6 = 6, 17, 1, 58
ACK, SYN, SYNACK = (5 << 4) | (16 << 8), (5 << 4) | (2 << 8), (5 << 4) | (18 << 8)


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


# --------------------------------------------------------------------------
# IPv4, entries installed beforehand
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


# --------------------------------------------------------------------------
# IPv4, entries created in the batch by the service step
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

# --------------------------------------------------------------------------
# IPv6
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
