"""Reverse NAT of service replies on the conntrack paths
(cgpu_classify_v{4,6}_ct_rnat / _ctlb_rnat, Engine rev_nat=True).

The compiled-reference harness mocks cilium_lb{4,6}_reverse_nat as always
missing, so the reference for the new outputs is the numpy restatement (in
tests/revnat_cases.py) of bpf/lib/lb.h:218-294, :485-576 and of the four call sites in
bpf/bpf_lxc.c, applied to batches whose hit entry (its rev_nat_index and
lb_loopback) is known by construction: entries installed with ct4_update /
ct6_update, or created earlier in the same stream by packets whose service is
known.  Everything the calls returned before (verdict, ct_ret, identity, stage,
the translated daddr / dport, the CT map, the policy counters) is checked to
be what it is without the output."""
import numpy as np
import pytest

from cilium_amd import build, layouts as L, synth
from revnat_cases import (CASES4, ICMP, ICMP6, IDX_MISS, IDX_PORT, IDX_PORT0, LOCAL4, LOCAL6, LOOPBACK, ROUTER6,
                          SVC6, SVCS4, SYN, SYNACK, TCP, _a6, _env4, _env6, _env_ctlb4, _lb6, _rmap4, _rmap6,
                          _rmap_ctlb4, be16, build_v4_ctlb, build_v4_hits, build_v6, restate_v4, restate_v6)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a device"
    build.build()
    return torch


def _engine(**kw):
    from cilium_amd.engine import Engine
    return Engine(device=0, **kw)


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
