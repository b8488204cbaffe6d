"""The ipcache tunnel endpoint on the GPU (cgpu_config.ipcache_tunnel): the
batched ipcache lookup and the tunnel output of the stateless classify paths.

Bit-exact against the compiled reference's answers (tests/golden/*.npz) and
Oracle.ipcache_lookup_addr, never against the engine.  Tunnel output buffers
are pre-filled with 0xFFFFFFFF: every element must be written.

tunnel[i] (include/cgpu.h cgpu_classify_v4_tun) = the matched entry's
tunnel_endpoint for an egress tuple that reached the ipcache lookup and matched
an entry with sec_label != 0, else 0 (bpf_lxc.c:488-491 / :177-180).
"""
import errno

import numpy as np
import pytest

import test_tunnel_cpu as TC
from cilium_amd import build, layouts as L, synth
from cilium_amd._abi import CgpuError
from oracle import Oracle

pytestmark = pytest.mark.gpu
FILL = -1  # 0xFFFFFFFF as int32
PER_LANE = 1  # CGPU_SCHED_PER_LANE


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a device"
    build.build()
    return torch


def _engine(**kw):
    from cilium_amd.engine import Engine
    return Engine(device=0, **{"ipcache_tunnel": 1, **kw})


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def lookup(torch, e, q):
    """ipcache_lookup_batch -> (m, 3) uint32 {found, sec_label, tunnel}"""
    q = np.ascontiguousarray(q)
    a = torch.from_numpy(q if q.ndim == 2 else q.view(np.int32)).cuda()
    out = e.ipcache_lookup_batch(a)
    torch.cuda.synchronize()
    return np.stack([out["found"].cpu().numpy().astype(np.uint32), _u32(out["sec_label"]),
                     _u32(out["tunnel"])], 1)


def load_ipcache(e, ents):
    for k, v in ents:
        assert e.ipcache_update(k, v) == 0


# ---- 4. lookup against the golden fixture ------------------------------------
@pytest.mark.parametrize("phase", ["a", "b"])
def test_lookup_golden(torch_cuda, golden, phase):
    g = golden("ipcache_lpm.npz")
    keys, vals = g["keys"], g["vals"]
    upto = len(keys) - int(g["n_static"]) if phase == "a" else len(keys)
    e = _engine()
    load_ipcache(e, zip(keys[:upto], vals[:upto]))
    e.commit()
    for q, r in ((g["q4"], g["r4" + phase]), (g["q6"], g["r6" + phase])):
        r = np.asarray(r, np.uint32)
        for n in (len(q), 63, 1):
            np.testing.assert_array_equal(lookup(torch_cuda, e, q[:n]), r[:n])
    # IPv6 address columns at any alignment: a view one byte into a buffer
    q6 = np.ascontiguousarray(g["q6"])
    buf = torch_cuda.zeros(q6.size + 16, dtype=torch_cuda.uint8, device="cuda")
    for off in (1, 4):
        v = buf[off:off + q6.size].view(-1, 16)
        v.copy_(torch_cuda.from_numpy(q6))
        out = e.ipcache_lookup_batch(v)
        torch_cuda.cuda.synchronize()
        np.testing.assert_array_equal(_u32(out["tunnel"]), np.asarray(g["r6" + phase], np.uint32)[:, 2])
    e.verify()
    e.close()


# ---- 5. classify against the golden fixture ----------------------------------
def _policy(e, labels):
    """a handful of entries on endpoint 1: some labels allowed on egress and
    ingress (L3-only keys), the rest denied"""
    for lab in labels:
        for eg in (0, 1):
            assert e.policy_update(1, L.policy_key(int(lab), 0, 0, eg), L.policy_entry()) == 0


def _tuples_v4(q, rng):
    n = len(q)
    proto = np.where(np.arange(n) % 16 == 0, 132, 6).astype(np.uint8)  # every 16th gated
    return {"saddr": q.astype(np.uint32), "daddr": q.astype(np.uint32),
            "dport": np.full(n, L.htons(80), np.uint16), "proto": proto,
            "flags": (1 - np.arange(n) % 2).astype(np.uint8),  # even index egress, odd ingress
            "len": rng.integers(60, 1500, n).astype(np.uint32), "ep": np.ones(n, np.uint16)}


def _expect(r, t):
    """The expected tunnels of tuples whose daddr answers are r (a fixture's
    rows), with the conditions that keep the test from passing vacuously.
    IPv4 (4000 tuples): >= 1500 non-zero, >= 20 egress label-0 hits that carry
    a tunnel, >= 50 gated egress tuples.  IPv6 has 3000 tuples, 1500 of them
    egress, so the same scheme cannot reach 1500: the fixture gives 1303
    non-zero and 9 label-0 hits, asserted as >= 1000 and >= 8."""
    eg = (t["flags"] & 1) == 1
    gated = ~np.isin(t["proto"], (6, 17, 1 if t["saddr"].ndim == 1 else 58))
    want = eg & ~gated & (r[:, 0] == 1) & (r[:, 1] != 0)
    exp = np.where(want, r[:, 2], 0).astype(np.uint32)
    assert (exp != 0).sum() >= (1500 if t["saddr"].ndim == 1 else 1000)
    assert (eg & ~gated & (r[:, 0] == 1) & (r[:, 1] == 0) & (r[:, 2] != 0)).sum() >= (20 if t["saddr"].ndim == 1 else 8)
    assert (eg & gated).sum() >= 50 and not exp[~eg].any()
    return exp


def _run_tun(torch, e, t, n, v6=False, path=0, shift=False):
    """the _tun call over the first n tuples; shift: the daddr column one
    element into a larger buffer (unaligned for the x4 schedule)"""
    d = synth.to_device({k: v[:n] for k, v in t.items()})
    if shift and not v6:
        big = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        big[1:].copy_(d["daddr"])
        d["daddr"] = big[1:]
    out = {"verdict": torch.empty(n, dtype=torch.int32, device="cuda"),
           "identity": torch.empty(n, dtype=torch.int32, device="cuda"),
           "stage": torch.empty(n, dtype=torch.uint8, device="cuda"),
           "tunnel": torch.full((n + 8,), FILL, dtype=torch.int32, device="cuda")}
    full = out["tunnel"]
    out["tunnel"] = full[:n]
    e._classify_tun(v6, path, d, out, True, None)
    torch.cuda.synchronize()
    assert (full[n:].cpu().numpy() == FILL).all(), "written past n"
    return out


@pytest.mark.parametrize("sched,shift", [(0, False), (PER_LANE, True), (0, True)])
def test_classify_v4_golden_tunnels(torch_cuda, golden, sched, shift):
    g = golden("ipcache_lpm.npz")
    r = np.asarray(g["r4b"], np.uint32)
    t = _tuples_v4(g["q4"], np.random.default_rng(5))
    exp = _expect(r, t)
    e = _engine(ct_proto_gate=1, schedule=sched)
    load_ipcache(e, zip(g["keys"], g["vals"]))
    labs = np.unique(r[:, 1])
    _policy(e, labs[labs != 0][::2])
    e.commit()
    for n in (4000, 3999, 257, 63, 1, 0):
        out = _run_tun(torch_cuda, e, t, n, shift=shift)
        np.testing.assert_array_equal(_u32(out["tunnel"]), exp[:n])
        if n == 4000:
            v = out["verdict"].cpu().numpy()
            assert (v == 0).sum() > 200 and (v == L.DROP_POLICY).sum() > 200  # allowed and denied
            # the tunnel does not depend on the verdict
            assert (exp[v == L.DROP_POLICY] != 0).any() and (exp[v == 0] != 0).any()
    e.close()


@pytest.mark.parametrize("sched", [0, PER_LANE])
def test_classify_v6_golden_tunnels(torch_cuda, golden, sched):
    g = golden("ipcache_lpm.npz")
    r = np.asarray(g["r6b"], np.uint32)
    q = np.ascontiguousarray(g["q6"])
    n = len(q)
    rng = np.random.default_rng(6)
    t = {"saddr": q, "daddr": q, "dport": np.full(n, L.htons(80), np.uint16),
         "proto": np.where(np.arange(n) % 16 == 0, 132, 6).astype(np.uint8),
         "flags": (1 - np.arange(n) % 2).astype(np.uint8),
         "len": rng.integers(60, 1500, n).astype(np.uint32), "ep": np.ones(n, np.uint16)}
    exp = _expect(r, t)
    e = _engine(ct_proto_gate=1, schedule=sched)
    load_ipcache(e, zip(g["keys"], g["vals"]))
    labs = np.unique(r[:, 1])
    _policy(e, labs[labs != 0][::2])
    e.commit()
    for m in (3000, 2999, 257, 63, 1, 0):
        out = _run_tun(torch_cuda, e, t, m, v6=True)
        np.testing.assert_array_equal(_u32(out["tunnel"]), exp[:m])
    e.close()


# ---- 6. nothing else moves ---------------------------------------------------
def _check_fixture(e, g, ci, out):
    np.testing.assert_array_equal(out["verdict"].cpu().numpy(), g[f"c{ci}_verdict"])
    np.testing.assert_array_equal(_u32(out["identity"]), g[f"c{ci}_identity"])
    np.testing.assert_array_equal(out["stage"].cpu().numpy(), g[f"c{ci}_stage"])
    for k, ep, fe in zip(g["pol_keys"], g["pol_ep"], g[f"c{ci}_final_entries"]):
        rc, got = e.policy_lookup(int(ep), k)
        assert rc == 0
        assert (int(got["packets"]), int(got["bytes"])) == (int(fe["packets"]), int(fe["bytes"]))
    np.testing.assert_array_equal(e.metrics(), g[f"c{ci}_metrics"])


def _load_fixture(e, g, tunnel_of=None):
    for i, (k, v) in enumerate(zip(g["ipc_keys"], g["ipc_vals"])):
        if tunnel_of is not None:
            v = v.copy()
            v["tunnel_endpoint"] = tunnel_of(i)
        assert e.ipcache_update(k, v) == 0
    for k, en, ep in zip(g["pol_keys"], g["pol_entries"], g["pol_ep"]):
        assert e.policy_update(int(ep), k, en) == 0


def _expect_plain(g, t, stage):
    """Oracle lookup of the daddr of every egress tuple that reached the
    lookup (the fixture's stage 4 = protocol gate), under a non-zero label.
    (These fixtures' ipcache values carry tunnels, so the expectation is not
    all zero.)"""
    o = Oracle()
    for k, v in zip(g["ipc_keys"], g["ipc_vals"]):
        assert o.ipcache_update(k, v) == 0
    o.set_fast(True)
    eg = (t["flags"] & 1) == 1
    exp = np.zeros(len(eg), np.uint32)
    for i in np.nonzero(eg & (stage != 4))[0]:
        a = t["daddr"][i]
        rc, val = o.ipcache_lookup_addr(bytes(a) if a.ndim else int(a))
        if rc == 0:
            lab, tun = np.frombuffer(val, "<u4")
            exp[i] = tun if lab else 0
    assert (exp != 0).sum() > 100 and not exp[~eg].any()
    return exp


@pytest.mark.parametrize("ci", range(5))
def test_classify_v4_fixture_unmoved(torch_cuda, golden, ci):
    g = golden("classify_v4.npz")
    gate, src, sw = (int(x) for x in g["configs"][ci])
    e = _engine(ct_proto_gate=gate, ingress_src_identity=src, ingress_secctx_world=sw)
    _load_fixture(e, g)
    e.commit()
    t = {k[2:]: g[k] for k in g.files if k.startswith("t_")}
    out = _run_tun(torch_cuda, e, t, len(t["saddr"]))
    _check_fixture(e, g, ci, out)
    np.testing.assert_array_equal(_u32(out["tunnel"]), _expect_plain(g, t, g[f"c{ci}_stage"]))
    e.close()


@pytest.mark.parametrize("ci", range(4))
def test_classify_v6_fixture_unmoved(torch_cuda, golden, ci):
    g = golden("classify_v6.npz")
    gate, src = (int(x) for x in g["configs"][ci])
    e = _engine(ct_proto_gate=gate, ingress_src_identity=src, ipv6_router_ip=g["router_ip"].tobytes())
    _load_fixture(e, g)
    e.commit()
    t = {k[2:]: g[k] for k in g.files if k.startswith("t_")}
    out = _run_tun(torch_cuda, e, t, len(t["flags"]), v6=True)
    _check_fixture(e, g, ci, out)
    np.testing.assert_array_equal(_u32(out["tunnel"]), _expect_plain(g, t, g[f"c{ci}_stage"]))
    e.close()


# ---- 7. service and cascade paths --------------------------------------------
def _tun_of(i):
    return 0x0A000000 + i + 1


def _oracle_of(g, **cfg):
    o = Oracle(**cfg)
    for i, (k, v) in enumerate(zip(g["ipc_keys"], g["ipc_vals"])):
        v = v.copy()
        v["tunnel_endpoint"] = _tun_of(i)
        assert o.ipcache_update(k, v) == 0
    return o


def _expect_lb4(o, g, t, stage):
    """Oracle lookup of the daddr lb4_local leaves in the tuple, for egress
    tuples that reach the lookup"""
    assert o.lb_update_batch(g["lb_keys"], g["lb_vals"]) == 0
    ref, _ = o.lb4(t, L.LB_LXC)
    o.set_fast(True)
    eg = (t["flags"] & 1) == 1
    n = len(eg)
    exp = np.zeros(n, np.uint32)
    xl = 0
    for i in np.nonzero(eg & ~np.isin(stage, (4, 6, 8)))[0]:
        rc, val = o.ipcache_lookup_addr(int(ref["tdaddr"][i]))
        if rc == 0:
            lab, tun = np.frombuffer(val, "<u4")
            if lab:
                exp[i] = tun
                xl += int(ref["tdaddr"][i] != t["daddr"][i])
    assert xl >= 1 and (stage == 6).sum() >= 1  # a translated tuple with a tunnel, a service drop
    assert not exp[stage == 6].any()
    return exp


@pytest.mark.parametrize("ci", range(2))
@pytest.mark.parametrize("name,path", [("classify_v4_lb.npz", 1), ("cascade_v4.npz", 2)])
def test_service_paths_v4(torch_cuda, golden, name, path, ci):
    g = golden(name)
    gate, src, sw = (int(x) for x in g["configs"][ci])
    e = _engine(ct_proto_gate=gate, ingress_src_identity=src, ingress_secctx_world=sw)
    _load_fixture(e, g, _tun_of)
    assert e.lb4_update_batch(g["lb_keys"], g["lb_vals"]) == 0
    if path == 2:
        for w, nm in ((0, "dyn4"), (1, "fix4")):
            for k in g[nm]:
                assert e.cidr_update(w, k) == 0
        for k in g["endpoints"]:
            assert e.endpoint_update(k) == 0
    e.commit()
    t = {k[2:]: g[k] for k in g.files if k.startswith("t_") and k != "t_opts"}
    stage = g[f"c{ci}_stage"]
    exp = _expect_lb4(_oracle_of(g, ct_proto_gate=gate), g, t, stage)
    if path == 2:
        assert (stage == 8).sum() >= 1 and not exp[stage == 8].any()
    out = _run_tun(torch_cuda, e, t, len(t["saddr"]), path=path)
    _check_fixture(e, g, ci, out)
    np.testing.assert_array_equal(_u32(out["tunnel"]), exp)
    e.close()


@pytest.mark.parametrize("sched", [0, PER_LANE])
@pytest.mark.parametrize("ci", range(2))
def test_service_path_v6(torch_cuda, golden, ci, sched):
    """the daddr after lb6_local is the compiled reference's (c*_tdaddr)"""
    g = golden("classify_v6_lb.npz")
    gate, src = (int(x) for x in g["configs"][ci])
    e = _engine(ct_proto_gate=gate, ingress_src_identity=src, ipv6_router_ip=g["router_ip"].tobytes(),
                schedule=sched)
    _load_fixture(e, g, _tun_of)
    assert e.lb6_update_batch(g["lb_keys"], g["lb_vals"]) == 0
    e.commit()
    t = {k[2:]: g[k] for k in g.files if k.startswith("t_")}
    stage, td = g[f"c{ci}_stage"], g[f"c{ci}_tdaddr"]
    o = _oracle_of(g)
    o.set_fast(True)
    eg = (t["flags"] & 1) == 1
    exp = np.zeros(len(eg), np.uint32)
    xl = 0
    for i in np.nonzero(eg & ~np.isin(stage, (4, 6)))[0]:
        rc, val = o.ipcache_lookup_addr(bytes(td[i]))
        if rc == 0:
            lab, tun = np.frombuffer(val, "<u4")
            if lab:
                exp[i] = tun
                xl += int(bytes(td[i]) != bytes(t["daddr"][i]))
    assert xl >= 1 and (stage == 6).sum() >= 1
    out = _run_tun(torch_cuda, e, t, len(eg), v6=True, path=1)
    _check_fixture(e, g, ci, out)
    np.testing.assert_array_equal(_u32(out["tunnel"]), exp)
    e.close()


# ---- 8. table shapes the fixture does not reach ------------------------------
def _egress_v4(q):
    n = len(q)
    return {"saddr": q, "daddr": q, "dport": np.full(n, L.htons(80), np.uint16),
            "proto": np.full(n, 6, np.uint8), "flags": np.ones(n, np.uint8),
            "len": np.full(n, 100, np.uint32), "ep": np.ones(n, np.uint16)}


def test_shapes_v4(torch_cuda):
    ents, q = TC._rand_tables(np.random.default_rng(11))
    A, B, Cc, D = 0xC0A80001, 0xC0A80002, 0xF0000003, 0x0A0B0C0D
    ents += [(TC._v4key(0x0A010000, 16), TC._val(5, A)), (TC._v4key(0x0A010200, 24), TC._val(0, B)),
             (TC._v4key(0x0A010207, 32), TC._val(7, 0)), (TC._v4key(0x0A010309, 32), TC._val(0xC0000001, Cc)),
             (np.zeros((), L.IPCACHE_KEY), TC._val(9, D))]
    shadow = TC._be([0x0A010101, 0x0A010233, 0x0A010207, 0x0A010309, 0x7B000001])
    q = np.concatenate([shadow, q])
    exp = TC.oracle_rows(TC.Oracle_from(ents), q)
    assert exp[:5].tolist() == [[1, 5, A], [1, 0, B], [1, 7, 0], [1, 0xC0000001, Cc], [1, 9, D]]
    assert len(np.unique(exp[:, 2])) > 1200
    e = _engine()
    load_ipcache(e, ents)
    e.commit()
    np.testing.assert_array_equal(lookup(torch_cuda, e, q), exp)
    out = _run_tun(torch_cuda, e, _egress_v4(q), len(q))
    want = np.where(exp[:, 1] != 0, exp[:, 2], 0)
    assert want[:5].tolist() == [A, 0, 0, Cc, D]
    np.testing.assert_array_equal(_u32(out["tunnel"]), want)
    e.close()


def test_shapes_v6(torch_cuda):
    ents, q = TC.v6_tables(np.random.default_rng(13))
    exp = TC.oracle_rows(TC.Oracle_from(ents), q)
    in32 = exp[:, 1] == 77
    assert in32.sum() > 200 and len(np.unique(exp[in32, 2])) > 10
    e = _engine()
    load_ipcache(e, ents)
    e.commit()
    np.testing.assert_array_equal(lookup(torch_cuda, e, q), exp)
    n = len(q)
    t = {"saddr": q, "daddr": q, "dport": np.full(n, L.htons(80), np.uint16),
         "proto": np.full(n, 6, np.uint8), "flags": np.ones(n, np.uint8),
         "len": np.full(n, 100, np.uint32), "ep": np.ones(n, np.uint16)}
    out = _run_tun(torch_cuda, e, t, n, v6=True)
    np.testing.assert_array_equal(_u32(out["tunnel"]), np.where(exp[:, 1] != 0, exp[:, 2], 0))
    e.close()


# ---- 9. incremental commits --------------------------------------------------
def _ipc_commits(e):
    out = np.zeros(2, np.uint64)
    assert TC.hook("cgpu_diag_ipc_commits", [TC.VP, TC.VP])(e.h, out.ctypes.data) == 0
    return int(out[0]), int(out[1])


def test_incremental_commits(torch_cuda):
    rng = np.random.default_rng(12)
    ents, q = TC._rand_tables(rng, n32=3000)
    base24 = 0x0C010300
    q = np.concatenate([q[:1700], TC._be([base24 | x for x in range(256)]),
                        TC._be([0x0C010450 + x for x in range(16)]), TC._be(rng.integers(0, 1 << 32, 28))])
    assert len(q) == 2000
    k0 = np.zeros((), L.IPCACHE_KEY)
    ents.append((k0, TC._val(9, 0x0A0B0C0D)))
    e = _engine()
    o = Oracle()
    for k, v in ents:
        assert e.ipcache_update(k, v) == 0 and o.ipcache_update(k, v) == 0
    e.commit()
    k32, v32 = ents[7]
    steps = [("tunnel only", k32, TC._val(int(v32["sec_label"]), 0xDEAD0001), False, True),
             ("delete /24", TC._v4key(base24, 24), None, True, True),
             ("insert /28", TC._v4key(0x0C010450, 28), TC._val(4242, 0xBEEF0002), False, True),
             ("static-part key", k0, TC._val(9, 0x0D0C0B0A), False, False)]
    prev = None
    for name, k, v, dele, patched in steps:
        b0, p0 = _ipc_commits(e)
        if dele:
            assert e.ipcache_delete(k) == 0 and o.ipcache_delete(k) == 0
        else:
            assert e.ipcache_update(k, v) == 0 and o.ipcache_update(k, v) == 0
        e.commit()
        b1, p1 = _ipc_commits(e)
        if patched:  # published without a full IPv4 build
            assert (b1, p1) == (b0, p0 + 1), name
        o.set_fast(True)
        exp = TC.oracle_rows(o, q)
        assert prev is None or not np.array_equal(prev[:, 2], exp[:, 2]), name
        prev = exp
        np.testing.assert_array_equal(lookup(torch_cuda, e, q), exp, err_msg=name)
        e.verify()
    e.close()


# ---- 11. flag off -------------------------------------------------------------
def test_flag_off(torch_cuda, golden):
    g = golden("classify_v4.npz")
    t = {k[2:]: g[k] for k in g.files if k.startswith("t_")}
    n = len(t["saddr"])
    res, tb = {}, {}
    for flag in (0, 1):
        e = _engine(ipcache_tunnel=flag)
        _load_fixture(e, g, _tun_of)
        e.commit()
        tb[flag] = e.table_bytes()
        d = synth.to_device(t)
        plain = e.classify_v4(d)
        # tunnel == NULL: the plain call's results
        out = {"verdict": torch_cuda.empty(n, dtype=torch_cuda.int32, device="cuda"),
               "identity": torch_cuda.empty(n, dtype=torch_cuda.int32, device="cuda"),
               "stage": torch_cuda.empty(n, dtype=torch_cuda.uint8, device="cuda")}
        from cilium_amd._abi import TuplesV4, check
        import ctypes as C
        tv = TuplesV4(*[d[k].data_ptr() for k in ("saddr", "daddr", "dport", "proto", "flags", "len", "ep")])
        st = C.c_void_p(torch_cuda.cuda.current_stream().cuda_stream)
        check(e.L.cgpu_classify_v4_tun(e.h, C.byref(tv), None, None, 0, n, out["verdict"].data_ptr(),
                                       out["identity"].data_ptr(), out["stage"].data_ptr(), None, st), "tun NULL")
        torch_cuda.cuda.synchronize()
        for k in ("verdict", "identity", "stage"):
            assert torch_cuda.equal(plain[k], out[k])
        res[flag] = plain
        if not flag:
            for call in (lambda: e.classify_v4(d, tunnel=True), lambda: e.classify_v4_lb(d, tunnel=True),
                         lambda: e.classify_v6(d, tunnel=True),
                         lambda: e.ipcache_lookup_batch(d["daddr"], tunnel=True)):
                with pytest.raises(CgpuError) as ex:
                    call()
                assert ex.value.errno == errno.EINVAL and "ipcache_tunnel" in str(ex.value)
            assert e.ipcache_lookup_batch(d["daddr"])["tunnel"] is None
            assert e.L.cgpu_classify_v4_tun(e.h, C.byref(tv), None, None, 7, n, out["verdict"].data_ptr(),
                                            out["identity"].data_ptr(), None, None, st) == -errno.EINVAL
        e.close()
    for k in ("verdict", "identity", "stage"):
        assert torch_cuda.equal(res[0][k], res[1][k])
    assert tb[1]["ipcache"] > tb[0]["ipcache"]
    assert {k: v for k, v in tb[1].items() if k != "ipcache"} == {k: v for k, v in tb[0].items() if k != "ipcache"}


# ---- 10. conntrack ------------------------------------------------------------
@pytest.mark.parametrize("v6", [False, True])
def test_conntrack_golden_stream(torch_cuda, golden, v6):
    """ct4.npz / ct6.npz (their ipcache carries tunnels) replayed through
    cgpu_classify_v{4,6}_ct_tun as test_gpu_ct{,6}.py replay them: verdict,
    ct_ret, identity, stage and every map dump are the fixture's, the tunnel
    the Oracle lookup of the daddr of an egress packet whose ct_lookup
    succeeded, under a non-zero label."""
    g = golden("ct6.npz" if v6 else "ct4.npz")
    assert g["ipc_vals"]["tunnel_endpoint"].any()
    kw = dict(ct_max=1 << 20)
    if v6:
        kw.update(ct6_max=1 << 20, ipv6_router_ip=g["router_ip"].tobytes())
    e = _engine(**kw)
    o = Oracle()
    for k, v in zip(g["ipc_keys"], g["ipc_vals"]):
        assert e.ipcache_update(k, v) == 0 and o.ipcache_update(k, v) == 0
    o.set_fast(True)
    for k, en, ep in zip(g["pol_keys"], g["pol_entries"], g["pol_ep"]):
        assert e.policy_update(int(ep), k, en) == 0
    synth.load_lxc(e, g["seclabels"])
    e.commit()
    upd, dump, count = (e.ct6_update, e.ct6_dump, e.ct6_count) if v6 else (e.ct4_update, e.ct4_dump, e.ct4_count)
    for k, v in zip(g["pre_keys"], g["pre_vals"]):
        assert upd(k, v) == 0
    t = {k[2:]: g[k] for k in g.files if k.startswith("t_")}
    n = len(t["flags"])
    eg = (t["flags"] & 1) == 1
    exp = np.zeros(n, np.uint32)
    for i in np.nonzero(eg & (g["b_ct_ret"] != L.CT_NONE))[0]:
        a = t["daddr"][i]
        rc, val = o.ipcache_lookup_addr(bytes(a) if v6 else int(a))
        if rc == 0:
            lab, tun = np.frombuffer(val, "<u4")
            exp[i] = tun if lab else 0
    assert (eg & (g["b_ct_ret"] == L.CT_REPLY) & (exp != 0)).sum() >= 1
    assert (g["b_ct_ret"] == L.CT_NONE).sum() >= 1 and not exp[g["b_ct_ret"] == L.CT_NONE].any()
    cuts, nows = g["cuts"], g["nows"]
    off = 0
    for bi in range(4):
        if bi == 2:
            for d in g["pol_del"]:
                assert e.policy_delete(int(g["pol_ep"][d]), g["pol_keys"][d]) == 0
            e.commit()
        sl = slice(int(cuts[bi]), int(cuts[bi + 1]))
        m = sl.stop - sl.start
        tun = torch_cuda.full((m + 8,), FILL, dtype=torch_cuda.int32, device="cuda")
        out = {"verdict": torch_cuda.empty(m, dtype=torch_cuda.int32, device="cuda"),
               "ct_ret": torch_cuda.empty(m, dtype=torch_cuda.uint8, device="cuda"),
               "identity": torch_cuda.empty(m, dtype=torch_cuda.int32, device="cuda"),
               "stage": torch_cuda.empty(m, dtype=torch_cuda.uint8, device="cuda"), "tunnel": tun[:m]}
        d = synth.to_device({k: x[sl] for k, x in t.items()})
        (e.classify_v6_ct if v6 else e.classify_v4_ct)(d, int(nows[bi]), out=out, tunnel=True)
        torch_cuda.cuda.synchronize()
        for k, dt in (("verdict", np.int32), ("ct_ret", np.uint8), ("identity", np.uint32), ("stage", np.uint8)):
            np.testing.assert_array_equal(out[k].cpu().numpy().view(dt), g["b_" + k][sl], err_msg=f"{k} batch {bi}")
        np.testing.assert_array_equal(_u32(out["tunnel"]), exp[sl], err_msg=f"tunnel batch {bi}")
        assert (tun[m:].cpu().numpy() == FILL).all()
        nd = int(g["dump_n"][bi])
        keys, vals = dump()
        np.testing.assert_array_equal(keys, g["dump_keys"][off:off + nd], err_msg=f"batch {bi}")
        np.testing.assert_array_equal(vals, g["dump_vals"][off:off + nd], err_msg=f"batch {bi}")
        assert count() == nd
        off += nd
    e.close()
