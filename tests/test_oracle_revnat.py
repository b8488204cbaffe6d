"""Reverse NAT in the CPU restatement (or_classify_*_rnat, Oracle
rev_nat=True): the maps cilium_lb{4,6}_reverse_nat and lb4_rev_nat /
lb6_rev_nat at the four call sites of bpf/bpf_lxc.c.

Two anchors.  (1) The C restatement, written from the reference's source,
against the numpy restatement of tests/revnat_cases.py, written independently,
on batches whose hit entries are known by construction: every output column
exactly.  (2) A table of single packets whose expected frame is written out
as literals, one row per call-site condition and per branch of the rewrite,
which both restatements must reproduce."""
import ipaddress

import numpy as np
import pytest

from cilium_amd import layouts as L
from oracle import Oracle
from revnat_cases import (ACK, ICMP, ICMP6, IDX_MISS, IDX_PORT, IDX_PORT0, LOCAL4, LOCAL6, LOOPBACK, ROUTER6, SVC6,
                          SYN, SYNACK, TCP, UDP, _a6, _env4, _env6, _env_ctlb4, _lb6, _rmap4, _rmap6, _rmap_ctlb4,
                          be16, build_v4_ctlb, build_v4_hits, build_v6, restate_v4, restate_v6)


def _load_rmap(o, rmap, v6=False):
    for ix, (addr, port) in rmap.items():
        if v6:
            v = np.zeros((), L.LB6_REVERSE_NAT)
            v["address"][:], v["port"] = _a6(addr), port
            assert o.revnat6_update(ix, v) == 0
        else:
            v = np.zeros((), L.LB4_REVERSE_NAT)
            v["address"], v["port"] = addr, port
            assert o.revnat4_update(ix, v) == 0


def _same4(rn, exp, msg):
    for f, x in zip(("rn_saddr", "rn_daddr", "rn_sport", "rn_applied"), exp):
        np.testing.assert_array_equal(rn[f], x, err_msg=f"{msg} {f}")


# --------------------------------------------------------------------------
# 1. the C restatement against the numpy restatement
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 5000])
def test_v4_preinstalled_hits(n):
    t, ents, cr, idx, loop, case = build_v4_hits(n)
    exp = restate_v4(t, cr, idx, loop, _rmap4())
    # every category is in the batch (as tests/test_gpu_revnat.py)
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
    p0 = ap & np.isin(idx, IDX_PORT0)
    assert p0.any() and (exp[2][p0] == t["sport"][p0]).all()
    tu = ap & np.isin(idx, IDX_PORT) & ~ic
    assert tu.any() and (exp[2][tu] != t["sport"][tu]).all()
    o = Oracle()
    _env4(o)
    for k, v in ents:
        assert o.ct4_update(k, v) == 0
    got = o.classify_v4_ct(t, 1000, rev_nat=True)
    np.testing.assert_array_equal(got[1], cr)
    _same4(got[5], exp, f"n={n}")
    o.close()


@pytest.mark.parametrize("nconn,extra", [(64, 1), (1250, 0)], ids=["257", "5000"])
def test_v4_ctlb_in_batch(nconn, extra):
    t, cr, idx, loop, fsa, fda, reply = build_v4_ctlb(nconn, extra)
    assert len(t["saddr"]) in (257, 5000)
    rmap = _rmap_ctlb4()
    exp = restate_v4(t, cr, idx, loop, rmap, fsa, fda)
    assert (exp[3] == reply).all()
    assert (exp[0][~reply] == fsa[~reply]).all() and (fsa[~reply] == LOOPBACK).any()
    lrep = reply & (loop == 1)
    assert lrep.any() and (exp[1][lrep] == LOCAL4).all() and (exp[0][lrep] == L.ip4_be("10.96.0.4")).all()
    assert (exp[2][reply] != t["sport"][reply]).any() and (exp[2][reply] == t["sport"][reply]).any()
    o = Oracle()
    _env_ctlb4(o)
    _load_rmap(o, rmap)
    got = o.classify_v4_ctlb(t, 1000, rev_nat=True)
    assert (got["verdict"] == 0).all()
    np.testing.assert_array_equal(got["ct_ret"], cr)
    np.testing.assert_array_equal(got["xdaddr"], fda)
    _same4(got, exp, "batch 1")
    # replies only, against the map the first batch left
    for sl in (slice(0, 1), slice(None)):
        t2 = {k: x[reply][sl] for k, x in t.items()}
        got2 = o.classify_v4_ctlb(t2, 1001, rev_nat=True)
        assert (got2["ct_ret"] == L.CT_REPLY).all()
        _same4(got2, tuple(x[reply][sl] for x in exp), "replies only")
    o.close()


@pytest.mark.parametrize("svc", [False, True], ids=["ct", "ctlb"])
@pytest.mark.parametrize("n_eg,n_in", [(200, 19), (3800, 400)], ids=["257", "5000"])
def test_v6(n_eg, n_in, svc):
    from cilium_amd.shard import flowhash6_np
    t, ents, cr, idx = build_v6(n_eg, n_in)
    rmap = dict(_rmap6())
    if svc:
        # one connection to an IPv6 service in the same batch (as tests/test_gpu_revnat.py)
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
    exp = restate_v6(t, cr, idx, rmap)
    eg = (t["flags"] & 1) == 1
    assert (~eg & (cr == L.CT_NEW) & np.isin(idx, IDX_PORT) & (exp[2] == 0)).any()   # first packet: never
    assert (~eg & (cr == L.CT_ESTABLISHED) & (exp[2] == 1)).any()                    # ESTABLISHED: rewritten
    assert (eg & (cr == L.CT_REPLY) & (idx > 0) & (exp[2] == 1)).any()
    assert (~eg & (cr == L.CT_ESTABLISHED) & np.isin(idx, IDX_MISS) & (exp[2] == 0)).any()  # unmapped
    assert (eg & (cr == L.CT_RELATED) & (exp[2] == 1)).any()
    ic = t["proto"] == ICMP6
    assert (exp[1][ic] == t["sport"][ic]).all()
    if svc:  # the backend's reply comes back as the service
        assert exp[2][-1] == 1 and bytes(exp[0][-1]) == SVC6[0]
    o = Oracle(router_ip=ROUTER6)
    _env6(o)
    _load_rmap(o, rmap, v6=True)
    if svc:
        _lb6(o)
    for k, v in ents:
        assert o.ct6_update(k, v) == 0
    if svc:
        t["hash"] = flowhash6_np(t["saddr"], t["daddr"], t["sport"], t["dport"], t["proto"]).astype(np.uint32)
        got = o.classify_v6_ctlb(t, 1000, rev_nat=True)
        gcr, rn = got["ct_ret"], got
    else:
        got = o.classify_v6_ct(t, 1000, rev_nat=True)
        gcr, rn = got[1], got[5]
    np.testing.assert_array_equal(gcr, cr)
    np.testing.assert_array_equal(rn["rn_applied"], exp[2])
    np.testing.assert_array_equal(rn["rn_saddr"], exp[0])
    np.testing.assert_array_equal(rn["rn_sport"], exp[1])
    o.close()


# --------------------------------------------------------------------------
# 2. literal cases
# --------------------------------------------------------------------------
def _ip4(s):
    """dotted quad -> the raw network-order word (independent of cilium_amd.layouts)"""
    return int.from_bytes(ipaddress.IPv4Address(s).packed, "little")


def _ip6(s):
    return ipaddress.IPv6Address(s).packed


# the reverse NAT maps of the table: raw index -> (address, host-order port)
MAP4 = {0x0100: ("10.96.1.1", 8000), 0x0200: ("10.96.2.1", 0)}
MAP6 = {0x0100: ("fd00:96::1", 8000), 0x0200: ("fd00:97::1", 0)}
EP4, REM4 = "10.200.0.1", "11.0.0.9"
EP6, REM6 = "f00d::c0a8:0:1", "2001:db8:1::9"          # EP6: s6_addr32[3] & 0xFFFF == 0
EP6_IDX = "f00d::c0a8:1:1"                             # bytes 12-13 = 00 01: raw index 0x0100

# name, family, egress, protocol, l4b, (saddr, sport), (daddr, dport), the installed entry (how the
# packet hits it: "reply" = its own tuple, "fwd" = the reversed tuple, None = no entry; rev_nat_index;
# lb_loopback), then the expectation: ct_ret, frame saddr, frame daddr (IPv4), sport, applied.
LITERAL = [
    ("v4 egress REPLY, port mapped", 4, 1, TCP, ACK, (EP4, 8080), (REM4, 40000), ("reply", 0x0100, 0),
     L.CT_REPLY, "10.96.1.1", REM4, 8000, 1),
    ("v4 egress REPLY, nat port 0: the source port is kept", 4, 1, TCP, ACK, (EP4, 8080), (REM4, 40000),
     ("reply", 0x0200, 0), L.CT_REPLY, "10.96.2.1", REM4, 8080, 1),
    ("v4 egress RELATED: ICMP keeps its port word", 4, 1, ICMP, 3, (EP4, 0x1234), (REM4, 0x5678),
     ("reply", 0x0100, 0), L.CT_RELATED, "10.96.1.1", REM4, 0x1234, 1),
    ("v4 egress REPLY, map miss", 4, 1, UDP, 0, (EP4, 8080), (REM4, 40000), ("reply", 0x0300, 0),
     L.CT_REPLY, EP4, REM4, 8080, 0),
    ("v4 egress REPLY, the byte-swapped twin of a mapped index", 4, 1, UDP, 0, (EP4, 8080), (REM4, 40000),
     ("reply", 0x0001, 0), L.CT_REPLY, EP4, REM4, 8080, 0),
    ("v4 egress REPLY, index 0", 4, 1, TCP, ACK, (EP4, 8080), (REM4, 40000), ("reply", 0, 0),
     L.CT_REPLY, EP4, REM4, 8080, 0),
    ("v4 egress REPLY on a loopback entry: daddr becomes the old saddr", 4, 1, TCP, ACK, (EP4, 8080),
     ("10.245.255.31", 40000), ("reply", 0x0100, 1), L.CT_REPLY, "10.96.1.1", EP4, 8000, 1),
    ("v4 egress ESTABLISHED on an entry with an index: never", 4, 1, TCP, ACK, (EP4, 40000), (REM4, 8080),
     ("fwd", 0x0100, 0), L.CT_ESTABLISHED, EP4, REM4, 40000, 0),
    ("v4 ingress REPLY", 4, 0, UDP, 0, (REM4, 8080), (EP4, 40000), ("reply", 0x0100, 0),
     L.CT_REPLY, "10.96.1.1", EP4, 8000, 1),
    ("v4 ingress RELATED: never", 4, 0, ICMP, 11, (REM4, 0), (EP4, 0), ("reply", 0x0100, 0),
     L.CT_RELATED, REM4, EP4, 0, 0),
    ("v4 ingress REPLY on a loopback entry: never", 4, 0, TCP, ACK, (REM4, 8080), (EP4, 40000),
     ("reply", 0x0100, 1), L.CT_REPLY, REM4, EP4, 8080, 0),
    ("v6 egress REPLY", 6, 1, TCP, ACK, (EP6, 8080), (REM6, 40000), ("reply", 0x0100, 0),
     L.CT_REPLY, "fd00:96::1", None, 8000, 1),
    ("v6 ingress ESTABLISHED", 6, 0, TCP, ACK, (REM6, 40000), (EP6, 443), ("fwd", 0x0100, 0),
     L.CT_ESTABLISHED, "fd00:96::1", None, 8000, 1),
    ("v6 ingress ESTABLISHED, nat port 0", 6, 0, UDP, 0, (REM6, 40000), (EP6, 443), ("fwd", 0x0200, 0),
     L.CT_ESTABLISHED, "fd00:97::1", None, 40000, 1),
    ("v6 ingress NEW to an address that names a mapped index: never", 6, 0, TCP, (5 << 4) | (2 << 8),
     (REM6, 40000), (EP6_IDX, 443), (None, 0, 0), L.CT_NEW, REM6, None, 40000, 0),
]


def _literal_batch(row):
    name, fam, egress, proto, l4b, (sa, sp), (da, dp), (how, idx, loop) = row[:8]
    v6 = fam == 6
    if v6:
        t = {"saddr": _a6(_ip6(sa))[None, :].copy(), "daddr": _a6(_ip6(da))[None, :].copy()}
        k = np.zeros((), L.CT6_TUPLE)
    else:
        t = {"saddr": np.array([_ip4(sa)], np.uint32), "daddr": np.array([_ip4(da)], np.uint32)}
        k = np.zeros((), L.CT4_TUPLE)
    t.update(sport=be16([sp]), dport=be16([dp]), proto=np.array([proto], np.uint8),
             l4b=np.array([l4b], np.uint16), flags=np.array([egress], np.uint8),
             len=np.array([100], np.uint32), ep=np.zeros(1, np.uint16))
    if how is None:
        return t, None
    # ct_lookup's tuple: daddr / saddr from the frame, dport <- the L4 sport, sport <- the L4 dport,
    # flags TUPLE_F_IN on egress (conntrack.h:462-530); "fwd" hits after ipv4_ct_tuple_reverse
    icmp = proto in (ICMP, ICMP6)
    own = (t["daddr"][0], t["saddr"][0], 0 if icmp else int(be16(sp)), 0 if icmp else int(be16(dp)),
           L.TUPLE_F_IN if egress else L.TUPLE_F_OUT)
    if how == "fwd":
        own = (own[1], own[0], own[3], own[2], own[4] ^ L.TUPLE_F_IN)
    k["daddr"], k["saddr"], k["dport"], k["sport"], k["flags"] = own
    k["nexthdr"] = proto
    if icmp:
        k["flags"] |= L.TUPLE_F_RELATED
    v = np.zeros((), L.CT_ENTRY)
    v["lifetime"], v["rev_nat_index"], v["bits"] = 100000, idx, 16 | (8 if loop else 0)
    v["src_sec_id"] = 400
    return t, (k, v)


@pytest.mark.parametrize("row", LITERAL, ids=[r[0] for r in LITERAL])
def test_literal(row):
    name, fam = row[0], row[1]
    (how, idx, loop), (cr, xsa, xda, xsp, xap) = row[7], row[8:]
    v6 = fam == 6
    t, ent = _literal_batch(row)
    o = Oracle(router_ip=ROUTER6)
    _env6(o)  # 2001:db8::/32 -> identity 400, allowed both ways on endpoint 0 (the v6 ingress rows)
    for ix, (addr, port) in (MAP6 if v6 else MAP4).items():
        v = L.lb6_reverse_nat(addr, port) if v6 else L.lb4_reverse_nat(addr, port)
        assert (o.revnat6_update if v6 else o.revnat4_update)(ix, v) == 0
    if ent:
        assert (o.ct6_update if v6 else o.ct4_update)(*ent) == 0
    got = (o.classify_v6_ct if v6 else o.classify_v4_ct)(t, 1000, rev_nat=True)
    rn = got[5]
    assert int(got[1][0]) == cr, name
    if v6:
        rmap = {ix: (_ip6(a), int(be16(p))) for ix, (a, p) in MAP6.items()}
        num = restate_v6(t, np.array([cr], np.uint8), np.array([idx]), rmap)
        num = {"saddr": bytes(num[0][0]), "sport": int(num[1][0]), "applied": int(num[2][0])}
        c = {"saddr": bytes(rn["rn_saddr"][0]), "sport": int(rn["rn_sport"][0]), "applied": int(rn["rn_applied"][0])}
        want = {"saddr": _ip6(xsa), "sport": int(be16(xsp)), "applied": xap}
    else:
        rmap = {ix: (_ip4(a), int(be16(p))) for ix, (a, p) in MAP4.items()}
        num = restate_v4(t, np.array([cr], np.uint8), np.array([idx]), np.array([loop]), rmap)
        num = {"saddr": int(num[0][0]), "daddr": int(num[1][0]), "sport": int(num[2][0]), "applied": int(num[3][0])}
        c = {"saddr": int(rn["rn_saddr"][0]), "daddr": int(rn["rn_daddr"][0]), "sport": int(rn["rn_sport"][0]),
             "applied": int(rn["rn_applied"][0])}
        want = {"saddr": _ip4(xsa), "daddr": _ip4(xda), "sport": int(be16(xsp)), "applied": xap}
    assert c == want, f"{name}: the C restatement"
    assert num == want, f"{name}: the numpy restatement"
    o.close()


# --------------------------------------------------------------------------
# 3. unused: nothing changes
# --------------------------------------------------------------------------
def test_outputs_do_not_disturb_the_call():
    """With the output requested and a loaded map, verdicts, ct results,
    identities, stages, the translated frame, the probe count, the conntrack
    map and the metrics are those of the plain call; columns may be NULL."""
    import ctypes as C
    from oracle import OrRnat4Out
    t, cr, *_ = build_v4_ctlb(64, 1)
    res = []
    for rev in (False, True):
        o = Oracle()
        _env_ctlb4(o)
        if rev:
            _load_rmap(o, _rmap_ctlb4())
        out = o.classify_v4_ctlb(t, 1000, rev_nat=rev)
        res.append(([out[k] for k in ("verdict", "ct_ret", "identity", "stage", "xdaddr", "xdport")],
                    out["probes"], o.ct4_dump(), o.metrics()))
        if rev:  # every column NULL: accepted, nothing written
            arrs = [np.ascontiguousarray(t[k], dt) for k, dt in (
                ("saddr", np.uint32), ("daddr", np.uint32), ("sport", np.uint16), ("dport", np.uint16),
                ("proto", np.uint8), ("l4b", np.uint16), ("flags", np.uint8), ("len", np.uint32), ("ep", np.uint16))]
            n = len(cr)
            v, c2 = np.empty(n, np.int32), np.empty(n, np.uint8)
            none = OrRnat4Out(None, None, None, None)
            assert o.L.or_classify_v4_ct_rnat(o.h, n, *[a.ctypes.data_as(C.c_void_p) for a in arrs], 1001,
                                              v.ctypes.data_as(C.c_void_p), c2.ctypes.data_as(C.c_void_p),
                                              None, None, C.byref(none), None) == 0
        o.close()
    (a, pa, (ka, va), ma), (b, pb, (kb, vb), mb) = res
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert pa == pb
    np.testing.assert_array_equal(ka, kb)
    np.testing.assert_array_equal(va, vb)
    np.testing.assert_array_equal(ma, mb)


def test_map_update_delete():
    o = Oracle()
    assert o.revnat4_delete(7) != 0 and o.revnat6_delete(7) != 0
    assert o.revnat4_update(7, L.lb4_reverse_nat("10.96.0.1", 80)) == 0
    assert o.revnat6_delete(7) != 0  # the other family's map is another map
    assert o.revnat4_delete(7) == 0 and o.revnat4_delete(7) != 0
    o.close()
