"""Crafted service frontend tables and forwarding tables through every device
walk of a single-slot neighbourhood hash outside the policy tables.

The cases of hop_cases.py -- full, wrapping, shared and empty-home
neighbourhoods in the lb4 / lb6 frontend tables and the forwarding tables
e4 / e6 / t4 / t6, build_lb's relocations, near-equal keys, absent keys at
planted homes, addresses that only the presence bitmap admits, a second
commit that deletes from a full home, and small tables that doubled -- are
loaded into an engine and walked by

* lb_fe_resolve per lane (k_lb4, k_classify<LB>, lb4_one on the x4 kernel's
  SLOW stage) and in the x4 staged form (lb4_lxc_q of k_classify_x4<LB> and,
  at Q = 2, <XDP>), lb_frontend / lb_row under the stateful service step
  (k_svc_prep*, the service walkers, k_svc_mark*), lb6_get<false> (lb6_one)
  and lb6_get<true> (the stateful IPv6 step), the host-resident forms;
* fwd_find4, fwd_find6<3>, fwd_find6<4> (k_forward) and the hand-copied
  fwd_slot4 / fwd_slot6 (k_forward_frames), whose slot index picks the MAC
  row the rewrite writes.

Expected values are the restatement's (oracle, forward_cases,
forward_frames_cases), computed once per case and configuration; every
comparison is bit-exact.  That the tables hold the shapes, and that every
planted key decides a packet of these batches, is asserted on the CPU in
test_hop_shapes.py.
"""
import numpy as np
import pytest

import cascade_cases as CC
import forward_cases as FC
import forward_frames_cases as FF
import hop_cases as H
from cilium_amd import build, layouts as L, synth
from test_gpu_forward_frames import _run as frames_run, _whole

pytestmark = pytest.mark.gpu

PER_LANE = 1  # CGPU_SCHED_PER_LANE
CT_MAX = 1 << 17
NOW = 1000
SECLABELS = (np.arange(CC.N_EP, dtype=np.uint32) * 7 + 6000).astype(np.uint32)
FCOLS = ("action", "ret", "ifindex", "arg")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a device"
    build.build()
    return torch


# --------------------------------------------------------------------------
# services
# --------------------------------------------------------------------------
class Svc:
    """One family's case over the policy_hops ipcache and policy, with
    everything the restatement says about it, computed once."""

    def __init__(self, v6):
        self.v6 = v6
        self.c = H.lb6_case() if v6 else H.lb4_case()
        self.w = CC.policy_workload()
        self.batch, self.target = H.svc_batch(v6)
        self.ct = H.svc_ct_batches(v6)
        self._exp = {}

    def load(self, t, kind, phase=1, commit=None):
        self.w.load(t, 1)
        if kind == "cascade":
            CC.load_xdp(t)
        if kind == "ctlb":
            synth.load_lxc(t, SECLABELS)
        self.c.load(t, phase, commit)

    def tuples(self, kind):
        return CC.xdp_batch(self.batch) if kind == "cascade" else self.batch

    def expected(self, kind, phase=1):
        key = (kind, phase)
        if key in self._exp:
            return self._exp[key]
        from oracle import Oracle
        o = Oracle(ct_proto_gate=1)
        self.load(o, kind, phase)
        b = self.tuples(kind)
        if kind in ("select0", "select1"):
            r, _ = o.lb4(b, int(kind[-1]), nthreads=4)
        elif kind == "ctlb":
            (o.ct6_set_max if self.v6 else o.ct_set_max)(CT_MAX)
            H.load_ct_preinstall(o, self.v6)
            fn = o.classify_v6_ctlb if self.v6 else o.classify_v4_ctlb
            r = {"batches": []}
            for j, x in enumerate(self.ct):
                x = fn(x, NOW + j)
                r["batches"].append({"daddr" if k == "xdaddr" else "dport" if k == "xdport" else k: v
                                     for k, v in x.items() if k != "probes"})
            r["ct_count"] = o.ct6_count() if self.v6 else o.ct4_count()
            look = o.ct6_lookup if self.v6 else o.ct4_lookup
            r["pre"] = [look(k) for k in H.svc_ct_preinstall(self.v6)[0]]
        else:
            fn = {"lb": o.classify_v6_lb if self.v6 else o.classify_v4_lb, "cascade": o.classify_v4_cascade}[kind]
            v, i, s, _ = fn(b, nthreads=4)
            r = {"verdict": v, "identity": i, "stage": s}
        if not kind.startswith("select"):
            r["counters"] = self.w.counters(o, 1)
            r["metrics"] = o.metrics()
        o.close()
        self._exp[key] = r
        return r

    def engine(self, kind, phase=1, **kw):
        from cilium_amd.engine import Engine
        e = Engine(device=0, ct_proto_gate=1, policy_max_total=1 << 12, max_endpoints=8, **kw)
        self.load(e, kind, phase, commit=e.commit)
        e.commit()
        return e

    def aimed(self, i):
        """the tuples of the batch aimed at frontend i"""
        return self.target == i


@pytest.fixture(scope="module")
def svcs():
    cache = {}

    def get(v6):
        if v6 not in cache:
            cache[v6] = Svc(v6)
        return cache[v6]
    return get


SCOLS = (("verdict", np.int32), ("identity", np.uint32), ("stage", np.uint8), ("ct_ret", np.uint8), ("dport", np.uint16))


def _col(x, dt):
    x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    return x.view(dt) if x.dtype.itemsize == np.dtype(dt).itemsize else x.astype(dt)


def _same(out, exp, what=""):
    for k, dt in SCOLS:
        if k in exp:
            got = _col(out[k], dt)
            bad = np.flatnonzero(got != exp[k])
            assert len(bad) == 0, (what, k, len(bad), bad[:5], got[bad[:5]], exp[k][bad[:5]])
    if "daddr" in exp:
        got = out["daddr"].cpu().numpy()
        got = got.view(np.uint32) if got.ndim == 1 else got.reshape(-1)
        np.testing.assert_array_equal(got, np.asarray(exp["daddr"]).reshape(-1), err_msg=what + " daddr")


def _check(S, e, out, exp):
    """the columns, every policy key's counters, metrics(); the expectation is not flat"""
    if out is not None:
        _same(out, exp)
    assert S.w.counters(e, 1) == exp["counters"]
    np.testing.assert_array_equal(e.metrics(), exp["metrics"])


def _offset1(torch, d):
    """every column as a view one element past an aligned base"""
    out = {}
    for k, x in d.items():
        buf = torch.empty((x.shape[0] + 16,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        out[k] = buf[1:1 + x.shape[0]]
        out[k].copy_(x)
    return out


def _select(torch, e, b, mode):
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16, np.dtype(np.uint8): np.uint8}
    d = {k: torch.from_numpy(np.ascontiguousarray(b[k]).view(view[b[k].dtype])).cuda()
         for k in ("saddr", "daddr", "sport", "dport", "proto", "hash")}
    out = e.lb4_select(d, mode)
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy().view(dt) for k, dt in (("ret", np.int32), ("saddr", np.uint32), ("daddr", np.uint32),
                                                          ("dport", np.uint16), ("rev_nat", np.uint16), ("slave", np.uint16))}


LB_COLS = ("ret", "saddr", "daddr", "dport", "rev_nat", "slave")


@pytest.mark.parametrize("mode", [L.LB_NETDEV, L.LB_LXC], ids=["netdev", "lxc"])
def test_lb4_select(torch_cuda, svcs, mode):
    """k_lb4: lb_frontend / lb_fe_resolve per lane, both programs"""
    S = svcs(False)
    exp = S.expected(f"select{mode}")
    e = S.engine("select")
    got = _select(torch_cuda, e, S.batch, mode)
    ok = exp["ret"] >= 0   # rev_nat and slave are defined where a service was found or none exists
    for k in LB_COLS:
        m = ok if k in ("rev_nat", "slave") else np.ones(len(ok), bool)
        bad = np.flatnonzero((got[k] != exp[k]) & m)
        assert len(bad) == 0, (k, len(bad), bad[:5], S.target[bad[:5]], got[k][bad[:5]], exp[k][bad[:5]])
    if mode == L.LB_LXC:
        assert (exp["ret"] == 1).sum() > 2000 and (exp["ret"] == 2).sum() >= 3 and (exp["ret"] == L.DROP_NO_SERVICE).sum() >= 4
        assert len(np.unique(exp["daddr"][exp["ret"] == 1])) > 500, "many backends"
    e.close()


@pytest.mark.parametrize("v6", [False, True], ids=["lb4", "lb6"])
def test_overfull_tables(torch_cuda, v6):
    """the frontend table that doubled: nine frontends of one home at 64 slots"""
    from oracle import Oracle
    from cilium_amd.engine import Engine
    c = H.lb6_overfull() if v6 else H.lb4_overfull()
    w = CC.policy_workload()
    p, target = H.svc_probes(c)
    p = {k: v[:len(target) - (len(target) % 4 == 0)] for k, v in p.items()}
    o = Oracle(ct_proto_gate=1)
    e = Engine(device=0, ct_proto_gate=1, policy_max_total=1 << 12, max_endpoints=8)
    for t in (o, e):
        w.load(t, 1)
        c.load(t, 1)
    e.commit()
    v, i, s, _ = (o.classify_v6_lb if v6 else o.classify_v4_lb)(p, nthreads=2)
    out = (e.classify_v6_lb if v6 else e.classify_v4_lb)(synth.to_device(p))
    torch_cuda.cuda.synchronize()
    _same(out, {"verdict": v, "identity": i, "stage": s})
    np.testing.assert_array_equal(e.metrics(), o.metrics())
    assert len(np.unique(i)) >= 4, "the nine frontends' backends have several identities"
    if not v6:
        ref, _ = o.lb4(p, L.LB_LXC)
        got = _select(torch_cuda, e, p, L.LB_LXC)
        for k in LB_COLS:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
        assert len(np.unique(ref["daddr"][ref["ret"] == 1])) == 9
    o.close()
    e.close()


# id -> (restatement kind, engine-only config, call)
V4_PATHS = {
    "x4": ("lb", {}, "lb"),                                   # k_classify_x4<LB>: lb4_lxc_q, RETRY and SLOW stages
    "per_lane": ("lb", dict(schedule=PER_LANE), "lb"),         # k_classify<LB>: lb4_one
    "x4_offset1": ("lb", {}, "offset1"),                       # columns of any alignment
    "x4_cascade": ("cascade", {}, "cascade"),                  # k_classify_x4<XDP>: lb4_lxc_q at Q = 2
    "host": ("lb", {}, "host"),                                # cgpu_classify_v4_lb_host
}


@pytest.mark.parametrize("path", sorted(V4_PATHS))
def test_classify_v4_lb(torch_cuda, svcs, path):
    torch = torch_cuda
    S = svcs(False)
    kind, ecfg, call = V4_PATHS[path]
    exp = S.expected(kind)
    e = S.engine(kind, **ecfg)
    b = S.tuples(kind)
    n = len(b["flags"])
    assert n % 4 != 0 and n <= 40_000
    if call == "host":
        out = e.classify_v4_lb_host({k: np.ascontiguousarray(v) for k, v in b.items()})
    else:
        d = synth.to_device(b)
        out = e.classify_v4_lb(_offset1(torch, d) if call == "offset1" else d, xdp=call == "cascade")
    torch.cuda.synchronize()
    _check(S, e, out, exp)
    # translated tuples reach many identities (the backends'); the service step drops some
    # (a frontend without slaves, a gated protocol at a frontend that has them)
    svc = S.target >= 0
    assert len(np.unique(exp["identity"][svc])) >= 50 and (exp["stage"][svc] == 6).sum() >= 10
    assert (exp["verdict"][svc] == 0).sum() > 1000 and (exp["verdict"][svc] == L.DROP_POLICY).sum() > 200
    e.close()


V6_PATHS = {"prepass": ({}, "lb"), "per_lane": (dict(schedule=PER_LANE), "lb"), "host": ({}, "host")}


@pytest.mark.parametrize("path", sorted(V6_PATHS))
def test_classify_v6_lb(torch_cuda, svcs, path):
    """lb6_get<false> under lb6_one: the x4 kernel's V6 service form, k_classify<V6, LB>, the host form"""
    S = svcs(True)
    ecfg, call = V6_PATHS[path]
    exp = S.expected("lb")
    e = S.engine("lb", **ecfg)
    b = S.batch
    assert len(b["flags"]) % 4 != 0
    if call == "host":
        out = e.classify_v6_host({k: np.ascontiguousarray(v) for k, v in b.items()}, lb=True)
    else:
        out = e.classify_v6_lb(synth.to_device(b))
    torch_cuda.cuda.synchronize()
    _check(S, e, out, exp)
    svc = S.target >= 0
    assert len(np.unique(exp["identity"][svc])) >= 50 and (exp["verdict"][svc] == 0).sum() > 1000
    e.close()


@pytest.mark.parametrize("lru", [0, 1], ids=["hash", "lru"])
@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_classify_ctlb(torch_cuda, svcs, v6, lru):
    """three batches on one map: k_svc_prep* / the service walkers /
    k_svc_mark*; the second and third repeat connections, whose CT_SERVICE
    entries name the slave (lb_row, lb6_get<true>).  Entries installed before
    the first batch name slave 0 (the master's own row), slaves past the
    frontend's and missing rows, at displaced frontends (that they occur:
    test_hop_shapes.py).  The map is large enough that the LRU form evicts
    nothing: one expectation serves both."""
    S = svcs(v6)
    exp = S.expected("ctlb")
    e = S.engine("ctlb", ct_max=CT_MAX, ct6_max=CT_MAX, ct_lru=lru)
    H.load_ct_preinstall(e, v6)
    fn = e.classify_v6_ctlb if v6 else e.classify_v4_ctlb
    for j, b in enumerate(S.ct):
        out = fn(synth.to_device(b), NOW + j)
        torch_cuda.cuda.synchronize()
        _same(out, exp["batches"][j], f"batch {j}")
    _check(S, e, None, exp)
    assert (e.ct6_count() if v6 else e.ct4_count()) == exp["ct_count"] > 1000
    # the installed entries afterwards: the stored slave, and in the hash map every byte
    for k, (rc, want) in zip(H.svc_ct_preinstall(v6)[0], exp["pre"]):
        got_rc, got = (e.ct6_lookup if v6 else e.ct4_lookup)(k)
        assert got_rc == rc == 0
        want = np.frombuffer(want, L.CT_ENTRY)[0]
        for f in ("slave", "bits", "rev_nat_index") if lru else L.CT_ENTRY.names:
            assert got[f] == want[f], (f, k, got, want)
    b1, b2, b3 = exp["batches"]
    assert (b1["ct_ret"] == L.CT_NEW).sum() > 1000 and (b2["ct_ret"] == L.CT_ESTABLISHED).sum() > 1000
    assert (b3["ct_ret"] == L.CT_ESTABLISHED).sum() > 500 and (b3["ct_ret"] == L.CT_NEW).sum() > 500
    if lru:
        assert e.ct_lru_stats(v6) == {"evictions": 0, "no_victim": 0}
    e.close()


@pytest.mark.parametrize("v6", [False, True], ids=["lb4", "lb6"])
def test_second_commit_services(torch_cuda, svcs, v6):
    """the frontend at offset 3 of the full home is deleted, one arrives at
    the wrapping home; the table rebuilds: the deleted key now misses, its
    neighbours still hit"""
    S = svcs(v6)
    c = S.c
    e = S.engine("lb", phase=2)
    exp1, exp2 = S.expected("lb", 1), S.expected("lb", 2)
    out = (e.classify_v6_lb if v6 else e.classify_v4_lb)(synth.to_device(S.batch))
    torch_cuda.cuda.synchronize()
    _check(S, e, out, exp2)
    gone = S.aimed(c.info["gone"]) & np.isin(S.batch["proto"], (6, 17))
    assert gone.sum() >= 8 and (exp1["identity"][gone] != exp2["identity"][gone]).any(), "the deleted frontend still translates"
    for i in c.planted["full"]:
        if i != c.info["gone"]:
            m = S.aimed(i)
            assert np.array_equal(exp1["identity"][m], exp2["identity"][m]) and np.array_equal(exp1["verdict"][m], exp2["verdict"][m])
    new = np.flatnonzero([n == "wrap" for n, _, _ in c.absent])[0]   # an absent key of the wrapping home before
    new = S.target == -1 - new
    assert new.sum() == 4
    if not v6:
        ref1, ref2 = S.expected("select1", 1), S.expected("select1", 2)
        got = _select(torch_cuda, e, S.batch, L.LB_LXC)
        for k in LB_COLS:
            np.testing.assert_array_equal(got[k], ref2[k], err_msg=k)
        # (the deleted key's address has an L3 frontend: its tuples go there now)
        mine = np.array([t for t, _ in c.fe[c.info["gone"]]["backends"].values()], np.uint32)
        assert np.isin(ref1["daddr"][gone], mine).any() and not np.isin(ref2["daddr"][gone], mine).any()
        mine = np.array([t for t, _ in c.info["new"]["backends"].values()], np.uint32)
        assert np.isin(ref2["daddr"][new], mine).all() and not np.isin(ref1["daddr"][new], mine).any()
    e.close()


# --------------------------------------------------------------------------
# forwarding
# --------------------------------------------------------------------------
def _fwd_engine(w):
    from cilium_amd.engine import Engine
    e = Engine(device=0, **FC.engine_cfg(w))
    FF.load_frame_world(e, w)
    e.commit()
    return e


@pytest.fixture(scope="module")
def fwd_engine(torch_cuda):
    e = _fwd_engine(H.fwd_case().w)
    yield e
    e.close()


def _fwd_dev(torch, b, v6, offset=0):
    d = {}
    for k, x in b.items():
        if k == "daddr" and v6:
            n = len(x)
            raw = torch.zeros(16 * n + 16, dtype=torch.uint8, device="cuda")
            raw[offset:offset + 16 * n] = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).cuda()
            d[k] = raw[offset:offset + 16 * n].view(n, 16)
        elif k in ("daddr", "tunnel"):
            d[k] = torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32)).cuda()
        else:
            d[k] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return d


def _fwd_run(torch, e, w, mode, v6, b, encap=True, offset=0):
    d = _fwd_dev(torch, b, v6, offset)
    kw = dict(FC.fwd_kwargs(w, mode), encap=encap)
    o = (e.forward_v6 if v6 else e.forward_v4)(d["daddr"], verdict=d["verdict"], tunnel=d["tunnel"], flags=d["flags"],
                                               ttl=d["ttl"], **kw)
    torch.cuda.synchronize()
    return {"action": o["action"].cpu().numpy(), "ret": o["ret"].cpu().numpy(),
            "ifindex": o["ifindex"].cpu().numpy().view(np.uint32), "arg": o["arg"].cpu().numpy().view(np.uint32)}


def _fwd_same(got, exp, who, msg):
    for k in FCOLS:
        bad = np.flatnonzero(got[k] != exp[k])
        assert len(bad) == 0, (msg, k, len(bad), [who[i][0] for i in bad[:5]], got[k][bad[:5]], exp[k][bad[:5]])


def _with_encap(w, encap):
    if encap:
        return w
    return FF.FrameWorld(**{**{k: getattr(w, k) for k in FF.FrameWorld.__dataclass_fields__}, "encap": False})


@pytest.mark.parametrize("encap", [True, False], ids=["encap", "noencap"])
@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
@pytest.mark.parametrize("mode", [FC.LXC, FC.NETDEV], ids=["lxc", "netdev"])
def test_forward(torch_cuda, fwd_engine, mode, v6, encap):
    """k_forward: fwd_find4 over e4 and t4, fwd_find6<4> over e6, fwd_find6<3> over t6"""
    w = _with_encap(H.fwd_case().w, encap)
    b, who = H.fwd_batch(v6)
    exp = FC.restate(w, mode, v6, **b)
    got = _fwd_run(torch_cuda, fwd_engine, w, mode, v6, b, encap, offset=4 if v6 else 0)
    _fwd_same(got, exp, who, f"mode {mode} v6 {v6} encap {encap}")
    assert len(np.unique(exp["arg"][exp["action"] == FC.LOCAL])) > 60
    if encap:
        # (the IPv6 netdev gate passes one /96: one tunnel key)
        assert len(np.unique(exp["arg"][(exp["action"] == FC.OVERLAY) & (b["tunnel"] == 0)])) > (0 if v6 and mode else 60)


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_forward_overfull(torch_cuda, v6):
    """the four tables after a doubling; key 0 absent at a home with hop bits"""
    c = H.fwd_overfull()
    e = _fwd_engine(c.w)
    assert e.forward_table_bytes() == {"endpoints4": 128 * 16, "endpoints6": 128 * 32, "tunnel4": 128 * 16, "tunnel6": 128 * 32}
    b, who = H.fwd_batch(v6, True)
    for mode in (FC.LXC, FC.NETDEV):
        _fwd_same(_fwd_run(torch_cuda, e, c.w, mode, v6, b), FC.restate(c.w, mode, v6, **b), who, f"mode {mode}")
    if not v6:
        zero = np.array([k == FC.key4(0) for _, k in who])
        exp = FC.restate(c.w, FC.NETDEV, False, **b)
        assert zero.sum() == 12 and (exp["action"][zero & (b["tunnel"] == 0)] == FC.STACK).all()
    e.close()


def _mixed_frames(small=False):
    """the two families' batches as frames in one buffer: (frames, verdict, stage, tunnel, who)"""
    parts = []
    for v6 in (False, True):
        b, who = H.fwd_batch(v6, small)
        b = FF.add_stage(b)
        parts.append((b, FF.build_frames(b, v6), who))
    n = sum(len(p[2]) for p in parts)
    perm = np.random.Generator(np.random.PCG64(0xF7 + n)).permutation(n)
    perm = perm[:n - (n % 4 == 0)]
    f = {k: np.ascontiguousarray(np.concatenate([p[1][k] for p in parts])[perm]) for k in ("data", "len", "flags")}
    col = {k: np.concatenate([p[0][k] for p in parts])[perm] for k in ("verdict", "stage", "tunnel")}
    who = [(parts[0][2] + parts[1][2])[i] for i in perm]
    return f, col["verdict"], col["stage"], col["tunnel"], who


@pytest.mark.parametrize("rewrite", [True, False], ids=["rewrite", "decide"])
@pytest.mark.parametrize("mode", [FC.LXC, FC.NETDEV], ids=["lxc", "netdev"])
def test_forward_frames(torch_cuda, fwd_engine, mode, rewrite):
    """k_forward_frames: fwd_slot4 / fwd_slot6; the MAC row is read at the slot the walk returns"""
    w = H.fwd_case().w
    f, verdict, stage, tunnel, who = _mixed_frames()
    exp, data = FF.restate_frames(w, mode, f, verdict, stage, tunnel, rewrite)
    got, raw = frames_run(torch_cuda, fwd_engine, w, mode, f, verdict, stage, tunnel, rewrite=rewrite)
    _fwd_same(got, exp, who, f"frames mode {mode}")
    np.testing.assert_array_equal(raw, _whole(f, data if rewrite else f["data"]))  # every slot, the guard behind them
    if rewrite:
        # every LOCAL frame carries its own endpoint's MAC pair, and each endpoint has its own
        local = np.flatnonzero(exp["action"] == FC.LOCAL)
        assert len(local) > 300
        out = raw[:f["data"].size].reshape(f["data"].shape)
        pairs = set()
        for i in local:
            mac, node = w.macs[who[i][1]]
            want = mac.to_bytes(8, "little")[:6] + node.to_bytes(8, "little")[:6]
            assert out[i, :12].tobytes() == want, who[i]
            pairs.add(want)
        assert len(pairs) > 60


def _ipcache_tunnels(wl, b):
    """the tunnel column of a stateless classify call, from the restatement's
    ipcache: the entry an egress tuple's identity came from (a non-zero
    label) where the conntrack gate passes the protocol, 0 elsewhere"""
    from oracle import Oracle
    v6 = b["daddr"].ndim == 2
    o = Oracle()
    for k, v in wl.ipc1:
        assert o.ipcache_update(k, v) == 0
    o.set_fast(True)
    exp = np.zeros(len(b["flags"]), np.uint32)
    for i in np.flatnonzero(((b["flags"] & 1) == 1) & np.isin(b["proto"], (6, 17, 58 if v6 else 1))):
        a = b["daddr"][i]
        rc, val = o.ipcache_lookup_addr(bytes(a) if v6 else int(a))
        if rc == 0:
            label, tun = np.frombuffer(val, "<u4")[:2]
            exp[i] = tun if label else 0
    o.close()
    return exp


def test_chained_calls(torch_cuda):
    """classify_v4 / classify_v6 / classify_frames with forward=: the chained
    entry points on the crafted tables.  The netdev program reads neither
    verdict nor flags, so the tables decide every packet; verdicts and the
    tunnel column are the restatement's, and the forwarding columns are the
    restatement's on those."""
    from cilium_amd.engine import Engine
    from oracle import Oracle
    torch = torch_cuda
    c, wl = H.fwd_case(), CC.policy_workload()
    w = c.w
    e = Engine(device=0, ct_proto_gate=1, policy_max_total=1 << 12, max_endpoints=8, ipcache_tunnel=1, **FC.engine_cfg(w))
    o = Oracle(ct_proto_gate=1)
    wl.load(e, 1)
    wl.load(o, 1)
    FF.load_frame_world(e, w)
    synth.load_lxc(e, SECLABELS)
    synth.load_lxc(o, SECLABELS)
    e.commit()
    fkw = FC.fwd_kwargs(w, FC.NETDEV)
    for v6 in (False, True):
        fb, who = H.fwd_batch(v6)
        n = len(who)
        base = wl.batch6 if v6 else wl.batch4
        b = {k: v[:n].copy() for k, v in base.items()}
        b["daddr"] = fb["daddr"]
        vo, io, so, _ = (o.classify_v6 if v6 else o.classify_v4)(b, nthreads=4)
        d = synth.to_device(b)
        d["ttl"] = torch.from_numpy(fb["ttl"]).cuda()
        out = (e.classify_v6 if v6 else e.classify_v4)(d, forward=fkw)
        torch.cuda.synchronize()
        _same(out, {"verdict": vo, "identity": io, "stage": so}, f"chained v6 {v6}")
        tun = _ipcache_tunnels(wl, b)
        np.testing.assert_array_equal(out["tunnel"].cpu().numpy().view(np.uint32), tun, err_msg=f"chained v6 {v6} tunnel")
        exp = FC.restate(w, FC.NETDEV, v6, fb["daddr"], vo, tun, b["flags"], fb["ttl"])
        got = {"action": out["fwd_action"].cpu().numpy(), "ret": out["fwd_ret"].cpu().numpy(),
               "ifindex": out["fwd_ifindex"].cpu().numpy().view(np.uint32), "arg": out["fwd_arg"].cpu().numpy().view(np.uint32)}
        _fwd_same(got, exp, who, f"chained v6 {v6}")
        assert len(np.unique(exp["arg"][exp["action"] == FC.LOCAL])) > 60
    # frames: the IPv4 tuples above as frames
    fb, who = H.fwd_batch(False)
    n = len(who)
    b = {k: v[:n].copy() for k, v in wl.batch4.items()}
    b["daddr"] = fb["daddr"]
    f = synth.frames_from_tuples(b, stride=64)
    vo, io, so, _ = o.classify_frames(f, nthreads=4)
    exp, data = FF.restate_frames(w, FC.NETDEV, f, vo, so, None, True)
    d = synth.frames_to_device(f)
    out = e.classify_frames(d, forward=FF.fwdf_kwargs(w, FC.NETDEV))
    torch.cuda.synchronize()
    _same(out, {"verdict": vo, "identity": io, "stage": so}, "chained frames")
    got = {"action": out["fwd_action"].cpu().numpy(), "ret": out["fwd_ret"].cpu().numpy(),
           "ifindex": out["fwd_ifindex"].cpu().numpy().view(np.uint32), "arg": out["fwd_arg"].cpu().numpy().view(np.uint32)}
    _fwd_same(got, exp, who, "chained frames")
    np.testing.assert_array_equal(d["data"].cpu().numpy(), data)
    assert (exp["action"] == FC.LOCAL).sum() > 300
    o.close()
    e.close()


def test_second_commit_forwarding(torch_cuda):
    """per table: the key at offset 3 of the full home is deleted, one arrives
    at the wrapping home; the tables rebuild.  The deleted key now misses, its
    neighbours still hit; columns and frames."""
    c = H.fwd_case()
    w1, w2 = c.w, H.fwd_world2(c)
    dele, add = H.fwd_second_commit(c)
    e = _fwd_engine(w1)
    for t in ("e4", "e6"):
        assert e.endpoint_delete(np.frombuffer(dele[t], L.ENDPOINT_KEY)[0]) == 0
        mac, node = w2.macs[add[t]]
        assert e.endpoint_update(np.frombuffer(add[t], L.ENDPOINT_KEY)[0], 0, L.endpoint_info(*w2.eps[add[t]], mac, node)) == 0
    for t in ("t4", "t6"):
        assert e.tunnel_delete(np.frombuffer(dele[t], L.ENDPOINT_KEY)[0]) == 0
        assert e.tunnel_update(np.frombuffer(add[t], L.ENDPOINT_KEY)[0], np.frombuffer(w2.tun[add[t]], L.ENDPOINT_KEY)[0]) == 0
    e.commit()
    for v6 in (False, True):
        b, who = H.fwd_batch(v6)
        exp1, exp2 = FC.restate(w1, FC.LXC, v6, **b), FC.restate(w2, FC.LXC, v6, **b)
        _fwd_same(_fwd_run(torch_cuda, e, w2, FC.LXC, v6, b), exp2, who, f"second commit v6 {v6}")
        et, tt = ("e6", "t6") if v6 else ("e4", "t4")
        plain = (b["verdict"] == 0) & (b["tunnel"] == 0) & (b["flags"] == 1) & (b["ttl"] == 64)
        for t, act in ((et, FC.LOCAL), (tt, FC.OVERLAY)):
            m = np.array([k == dele[t] for _, k in who]) & plain
            assert m.any() and (exp1["action"][m] == act).all() and (exp2["arg"][m] != exp1["arg"][m]).all()
            m = np.array([k == add[t] for _, k in who]) & plain
            assert m.any() and (exp2["action"][m] == act).all() and (exp1["arg"][m] != exp2["arg"][m]).all()
            for k in c.planted[t]["full"]:
                if k != dele[t]:
                    m = np.array([x == k for _, x in who])
                    assert all(np.array_equal(exp1[col][m], exp2[col][m]) for col in FCOLS)
    f, verdict, stage, tunnel, who = _mixed_frames()
    exp, data = FF.restate_frames(w2, FC.LXC, f, verdict, stage, tunnel, True)
    got, raw = frames_run(torch_cuda, e, w2, FC.LXC, f, verdict, stage, tunnel, rewrite=True)
    _fwd_same(got, exp, who, "second commit frames")
    np.testing.assert_array_equal(raw, _whole(f, data))
    e.close()
