"""The local delivery step on the device (cgpu_deliver_v4 / _v6, Engine.deliver_v4
/ _v6, deliver=True on the classify calls; kernel k_deliver).

The reference is tests/deliver_cases.py: the restatement's ingress classify
with the label as its identity, pinned by the literal table there
(tests/test_deliver_cpu.py).  Every comparison is bit-exact: verdict,
identity, stage, every installed key's {packets, bytes}, metrics()."""
import numpy as np
import pytest

import cascade_cases as CC
import deliver_cases as DC
import forward_cases as FC
from cilium_amd import build, layouts as L

pytestmark = pytest.mark.gpu
GLOBAL_CTR = 2  # CGPU_SCHED_GLOBAL_CTR
OUT = (("verdict", np.int32), ("identity", np.uint32), ("stage", np.uint8))
VIEW = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a device"
    build.build()
    return torch


def _engine(**kw):
    from cilium_amd.engine import Engine
    return Engine(device=0, **kw)


def _dev(torch, b, offset=0):
    """the columns as device tensors; offset: every column is a view that many
    elements into an allocation of its own"""
    d = {}
    for k, x in b.items():
        x = np.ascontiguousarray(x)
        x = x.view(VIEW.get(x.dtype, x.dtype))
        buf = torch.zeros(len(x) + 16, dtype=getattr(torch, x.dtype.name), device="cuda")
        assert buf.data_ptr() % 16 == 0
        d[k] = buf[offset:offset + len(x)]
        d[k].copy_(torch.from_numpy(x))
    return d


def _np(out):
    return {k: out[k].cpu().numpy().view(dt) for k, dt in OUT if out.get(k) is not None}


def _run(torch, e, v6, d, out=None):
    fn = e.deliver_v6 if v6 else e.deliver_v4
    o = fn(d["action"], d["arg"], d["dport"], d["proto"], d["flags"], d["len"], src_label=d.get("src_label"),
           src_ep=d.get("src_ep"), out=out)
    torch.cuda.synchronize()
    return o


def _same(got, exp, what=""):
    for k, _ in OUT:
        if k in got:
            bad = np.flatnonzero(got[k] != exp[k])
            assert len(bad) == 0, (what, k, len(bad), bad[:5], got[k][bad[:5]], exp[k][bad[:5]])


# --------------------------------------------------------------------------
# 1. the literal table
# --------------------------------------------------------------------------
LITERAL = [(v6, gate, ep) for v6 in (False, True) for gate in (1, 0) for ep in (False, True)
           if DC.case_rows(v6, gate, ep)]


def _policy_counters(t):
    out = []
    for ep, lab, dport, proto, _ in DC.POLICY:
        rc, got = t.policy_lookup(ep, L.policy_key(lab, dport, proto, 0))
        assert rc == 0
        got = got if isinstance(got, np.void) else np.frombuffer(got, L.POLICY_ENTRY)[0]
        out.append((int(got["packets"]), int(got["bytes"])))
    return out


@pytest.mark.parametrize("v6,gate,src_ep", LITERAL,
                         ids=[f"{'v6' if a else 'v4'}-gate{b}-{'src_ep' if c else 'src_label'}" for a, b, c in LITERAL])
def test_literal_table(torch_cuda, v6, gate, src_ep):
    rows = DC.case_rows(v6, gate, src_ep)
    c = DC.columns(rows)
    # what the ingress tuples of the classify calls would take the identity
    # from is all set against the label: it must not be read
    e = _engine(ct_proto_gate=gate, max_endpoints=DC.MAX_EP, ingress_secctx_world=1, ingress_src_identity=1003)
    DC.load_policy(e)
    DC.load_lxc(e)
    assert e.ipcache_update(L.ipcache_key("0.0.0.0/0"), L.remote_info(1002)) == 0
    assert e.ipcache_update(L.ipcache_key("::/0"), L.remote_info(1002)) == 0
    e.commit()
    got = _np(_run(torch_cuda, e, v6, _dev(torch_cuda, c)))
    exp = DC.expected(rows)
    for i, r in enumerate(rows):
        assert (int(got["verdict"][i]), int(got["identity"][i]), int(got["stage"][i])) == r[11], r[0]
    o = DC.new_oracle(DC.load_policy, gate)
    ref = DC.reference(o, v6, c["action"], c["arg"], DC.labels(c), c["dport"], c["proto"], c["flags"], c["len"],
                       max_ep=DC.MAX_EP)
    _same(ref, exp, "reference")
    assert _policy_counters(e) == _policy_counters(o)
    np.testing.assert_array_equal(e.metrics(), o.metrics())
    o.close()
    e.close()


# --------------------------------------------------------------------------
# 2.-5. the crafted tables
# --------------------------------------------------------------------------
NS = [1, 63, 257, None]  # None: all 11207 rows (not a multiple of 4)


class Crafted:
    """the crafted batches and what the reference says of them, computed once"""

    def __init__(self):
        self.w = CC.policy_workload()
        self._b, self._exp = {}, {}
        lab = np.unique(DC.crafted_batch()["src_label"])
        # the src_ep form: one lxc entry per distinct label, and one id without
        self.ep_of = {int(x): i for i, x in enumerate(lab)}
        self.no_entry = len(lab)

    def batch(self, v6, form="src_label", actions=None):
        key = (v6, form, actions)
        if key not in self._b:
            b = DC.crafted_batch(v6)
            n = len(b["action"])
            assert n == 11207
            lab = b["src_label"].copy()
            if form == "src_ep":
                ep = np.array([self.ep_of[int(x)] for x in lab], np.uint16)
                ep[5::53] = self.no_entry
                lab[5::53] = 0
                del b["src_label"]
                b["src_ep"] = ep
            if actions == "mixed":
                rng = np.random.Generator(np.random.PCG64(0xD11))
                b["action"] = rng.integers(0, 8, n).astype(np.uint8)
            elif actions == "none":
                b["action"] = (np.arange(n) % 7 + (np.arange(n) % 7 >= DC.LOCAL)).astype(np.uint8)
                assert not (b["action"] == DC.LOCAL).any() and len(np.unique(b["action"])) == 7
            b["arg"] = np.where(b["action"] == DC.LOCAL, b["arg"], 0xFFFFFFFF).astype(np.uint32)
            self._b[key] = (b, lab)
        return self._b[key]

    def expected(self, phase, v6, n=None, form="src_label", actions=None):
        key = (phase, v6, n, form, actions)
        if key not in self._exp:
            b, lab = self.batch(v6, form, actions)
            m = len(lab) if n is None else n
            o = DC.new_oracle(lambda t: DC.load_crafted_policy(t, phase))
            r = DC.reference(o, v6, b["action"][:m], b["arg"][:m], lab[:m], b["dport"][:m], b["proto"][:m],
                             b["flags"][:m], b["len"][:m])
            r["counters"] = self.w.counters(o, phase)
            r["metrics"] = o.metrics()
            o.close()
            self._exp[key] = r
        return self._exp[key]

    def load_lxc(self, e):
        for lab, ep in self.ep_of.items():
            assert e.lxc_update(ep, L.lxc_info(b"\0" * 6, 0, b"\0" * 16, 0, lab)) == 0


@pytest.fixture(scope="module")
def crafted():
    return Crafted()


@pytest.fixture(scope="module")
def engines(torch_cuda, crafted):
    """policy_workload() loaded with Workload.load (ipcache and all) as one
    commit and as two (the second patches), the lxc entries of the src_ep form"""
    made = {}

    def get(phase, **kw):
        key = (phase, tuple(sorted(kw.items())))
        if key not in made:
            e = _engine(ct_proto_gate=1, policy_max_total=1 << 12, max_endpoints=8, **kw)
            crafted.load_lxc(e)
            crafted.w.load(e, phase, commit=e.commit)
            e.commit()
            made[key] = e
        e = made[key]
        e.counters_reset()
        return e
    yield get
    for e in made.values():
        e.close()


def _check(crafted, e, got, exp, phase, flat_ok=False):
    if got is not None:
        _same(got, exp)
    assert crafted.w.counters(e, phase) == exp["counters"]
    np.testing.assert_array_equal(e.metrics(), exp["metrics"])
    if not flat_ok:
        v = exp["verdict"]
        assert (v == 0).sum() > 100 and (v == L.DROP_POLICY).sum() > 100 and (v > 0).sum() > 30
        assert sum(p > 0 for p, _ in exp["counters"]) > 100


@pytest.mark.parametrize("form", ["src_label", "src_ep"])
@pytest.mark.parametrize("n", NS, ids=lambda n: f"n{n or 'all'}")
@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
@pytest.mark.parametrize("phase", [1, 2], ids=["commit1", "commit2"])
def test_crafted_tables(torch_cuda, crafted, engines, phase, v6, n, form):
    b, _ = crafted.batch(v6, form)
    exp = crafted.expected(phase, v6, n, form)
    e = engines(phase)
    got = _np(_run(torch_cuda, e, v6, _dev(torch_cuda, DC.head(b, n or len(b["action"])))))
    _check(crafted, e, got, exp, phase, flat_ok=n is not None)
    if form == "src_ep" and n is None:
        assert (got["identity"][5::53][exp["stage"][5::53] != 4] == 0).all()


@pytest.mark.parametrize("phase", [1, 2], ids=["commit1", "commit2"])
def test_crafted_tables_global_counters(torch_cuda, crafted, engines, phase):
    """CGPU_SCHED_GLOBAL_CTR: no LDS counters, every hit two global atomics"""
    b, _ = crafted.batch(False)
    e = engines(phase, schedule=GLOBAL_CTR)
    got = _np(_run(torch_cuda, e, False, _dev(torch_cuda, b)))
    _check(crafted, e, got, crafted.expected(phase, False), phase)


@pytest.mark.parametrize("form", ["src_label", "src_ep"])
@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_mixed_actions(torch_cuda, crafted, engines, v6, form):
    b, _ = crafted.batch(v6, form, "mixed")
    exp = crafted.expected(2, v6, None, form, "mixed")
    loc = b["action"] == DC.LOCAL
    assert 1000 < loc.sum() < 2000 and len(np.unique(b["action"])) == 8 and (b["arg"][~loc] == 0xFFFFFFFF).all()
    e = engines(2)
    got = _np(_run(torch_cuda, e, v6, _dev(torch_cuda, b)))
    for k, want in (("verdict", 0), ("identity", 0), ("stage", L.STAGE_NOT_LOCAL)):
        assert (got[k][~loc] == want).all(), k
    _check(crafted, e, got, exp, 2, flat_ok=True)
    assert sum(p > 0 for p, _ in exp["counters"]) > 50 and int(exp["metrics"][:, :, 0].sum()) > 800


def test_no_local_packet(torch_cuda, crafted, engines):
    b, _ = crafted.batch(False, "src_label", "none")
    e = engines(1)
    got = _np(_run(torch_cuda, e, False, _dev(torch_cuda, b)))
    assert (got["verdict"] == 0).all() and (got["identity"] == 0).all() and (got["stage"] == L.STAGE_NOT_LOCAL).all()
    assert all(c == (0, 0) for c in crafted.w.counters(e, 1))
    assert not e.metrics().any()


@pytest.mark.parametrize("form", ["src_label", "src_ep"])
@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_unaligned_columns(torch_cuda, crafted, engines, v6, form):
    """every column a view one element into its allocation"""
    b, _ = crafted.batch(v6, form)
    n = len(b["action"])
    d = _dev(torch_cuda, b, offset=1)
    assert all(x.data_ptr() % 16 == x.element_size() for x in d.values())
    out = {k: torch_cuda.full((n + 16,), -1 if k != "stage" else 255, dtype=dt, device="cuda")
           for k, dt in (("verdict", torch_cuda.int32), ("identity", torch_cuda.int32), ("stage", torch_cuda.uint8))}
    e = engines(1)
    _run(torch_cuda, e, v6, d, out={k: x[1:1 + n] for k, x in out.items()})
    got = {k: out[k][1:1 + n].cpu().numpy().view(dt) for k, dt in OUT}
    _check(crafted, e, got, crafted.expected(1, v6, None, form), 1)
    for k, x in out.items():  # nothing outside the views
        fill = 255 if k == "stage" else -1
        assert int(x[0]) == fill and (x[1 + n:].cpu().numpy() == fill).all(), k


@pytest.mark.parametrize("n", [257, None], ids=["n257", "nall"])
def test_null_outputs_and_given_tensors(torch_cuda, crafted, engines, n):
    torch = torch_cuda
    b, _ = crafted.batch(False)
    m = n or len(b["action"])
    exp = crafted.expected(1, False, n)
    d = _dev(torch, DC.head(b, m))
    e = engines(1)
    full = torch.full((m + 8,), -7, dtype=torch.int32, device="cuda")
    out = {"verdict": full[:m], "identity": None, "stage": None}
    r = _run(torch, e, False, d, out=out)
    assert r is out and r["identity"] is None and r["stage"] is None
    np.testing.assert_array_equal(full[:m].cpu().numpy(), exp["verdict"])
    assert (full[m:].cpu().numpy() == -7).all(), "written past n"
    _check(crafted, e, None, exp, 1, flat_ok=True)
    # all three given: written in place
    e.counters_reset()
    out = {"verdict": torch.full((m,), -7, dtype=torch.int32, device="cuda"),
           "identity": torch.full((m,), -7, dtype=torch.int32, device="cuda"),
           "stage": torch.full((m,), 77, dtype=torch.uint8, device="cuda")}
    ptrs = {k: x.data_ptr() for k, x in out.items()}
    r = _run(torch, e, False, d, out=out)
    assert {k: r[k].data_ptr() for k in ptrs} == ptrs
    _same(_np(out), exp)
    # only the stage left out
    e.counters_reset()
    out = {"verdict": torch.empty(m, dtype=torch.int32, device="cuda"),
           "identity": torch.empty(m, dtype=torch.int32, device="cuda"), "stage": None}
    _same(_np(_run(torch, e, False, d, out=out)), exp)
    _check(crafted, e, None, exp, 1, flat_ok=True)


def test_empty_batch(torch_cuda, engines):
    torch = torch_cuda
    e = engines(1)
    z = {k: torch.empty(0, dtype=dt, device="cuda") for k, dt in
         (("action", torch.uint8), ("arg", torch.int32), ("src_label", torch.int32), ("dport", torch.int16),
          ("proto", torch.uint8), ("flags", torch.uint8), ("len", torch.int32))}
    r = _run(torch, e, False, z)
    assert r["verdict"].numel() == 0 and not e.metrics().any()


# --------------------------------------------------------------------------
# 6. classify -> forward -> deliver, end to end
# --------------------------------------------------------------------------
A, B, C3 = 5, 6, 7           # the local endpoints' ids
LAB_A, LAB_B, LAB_C, LAB_REMOTE = 1001, 1002, 1003, 2001
ADDR = {False: {"a": "10.1.0.5", "b": "10.1.0.6", "c": "10.1.0.7", "host": "10.1.0.1", "remote": "10.2.3.4", "world": "8.8.8.8"},
        True: {"a": "fd00::5", "b": "fd00::6", "c": "fd00::7", "host": "fd00::2", "remote": "fd01::9", "world": "2001:db8::8"}}
# (ep, sec_label, dport, proto, egress, proxy port)
E2E_POLICY = [
    (A, LAB_B, 0, 0, 1, 0),             # A may send anything to B ...
    (A, LAB_B, 9090, DC.TCP, 1, 15002),  # ... port 9090 through its own proxy
    (A, LAB_REMOTE, 0, 0, 1, 0), (A, L.HOST_ID, 0, 0, 1, 0),
    (B, LAB_A, 53, DC.UDP, 1, 0), (B, LAB_A, 80, DC.TCP, 1, 0),
    (B, LAB_A, 80, DC.TCP, 0, 0),        # B takes port 80 from A,
    (B, LAB_A, 8080, DC.TCP, 0, 15001),  # 8080 through its ingress proxy, nothing else
    (C3, LAB_A, 0, 0, 1, 0),
    (A, 0, 53, DC.UDP, 0, 0),            # A takes DNS from anyone
    (A, LAB_C, 0, 0, 0, 0),              # and anything from C
]


def _e2e_world(v6):
    w = FC.World(host_ifindex=11, encap_ifindex=22)
    a = ADDR[v6]
    k = (lambda s: FC.key6(FC.ip6(s))) if v6 else (lambda s: FC.key4(FC.ip4(s)))
    w.eps[k(a["a"])] = (7, A, 0)
    w.eps[k(a["b"])] = (8, B, 0)
    w.eps[k(a["c"])] = (9, C3, 0)
    w.eps[k(a["host"])] = (0, 0, FC.ENDPOINT_F_HOST)
    w.tun[FC.key6(FC.ip6("fd01::")) if v6 else FC.key4(FC.ip4("10.2.0.0"))] = FC.key4(FC.NODE2)
    return w


def _e2e_load(t, v6, ipcache=True, policy=True):
    a = ADDR[v6]
    full = "/128" if v6 else "/32"
    if ipcache:
        for cidr, lab in (("::/0" if v6 else "0.0.0.0/0", L.WORLD_ID), (a["a"] + full, LAB_A), (a["b"] + full, LAB_B),
                          (a["c"] + full, LAB_C),                          (a["host"] + full, L.HOST_ID), ("fd01::/96" if v6 else "10.2.0.0/16", LAB_REMOTE)):
            assert t.ipcache_update(L.ipcache_key(cidr), L.remote_info(lab, 0)) == 0
    if policy:
        for ep, lab, dport, proto, egr, proxy in E2E_POLICY:
            assert t.policy_update(ep, L.policy_key(lab, dport, proto, egr), L.policy_entry(proxy)) == 0


def _e2e_batch(v6):
    """(name, ep, saddr, daddr, dport, proto, flags, ttl) rows, each four times
    with lengths of its own"""
    a = ADDR[v6]
    E, F = DC.F_EGRESS, DC.F_FRAGMENT
    rows = [
        ("delivered", A, "a", "b", 80, DC.TCP, E, 64),
        ("allowed on egress, denied at the destination", A, "a", "b", 81, DC.TCP, E, 64),
        ("to the destination's proxy", A, "a", "b", 8080, DC.TCP, E, 64),
        ("to the sender's proxy", A, "a", "b", 9090, DC.TCP, E, 64),
        ("fragment: no L3 key at the destination" if not v6 else "fragment bit on IPv6", A, "a", "b", 80, DC.TCP, E | F, 64),
        ("wildcard at the destination", B, "b", "a", 53, DC.UDP, E, 64),
        ("L3 key at the destination", C3, "c", "a", 80, DC.TCP, E, 64),
        ("allowed by B, denied by A", B, "b", "a", 80, DC.TCP, E, 64),
        ("denied on egress", B, "b", "a", 22, DC.TCP, E, 64),
        ("expired before delivery", A, "a", "b", 80, DC.TCP, E, 1),
        ("gated protocol", A, "a", "b", 0, DC.GRE, E, 64),
        ("to the host", A, "a", "host", 80, DC.TCP, E, 64),
        ("to the overlay", A, "a", "remote", 80, DC.TCP, E, 64),
        ("to the world: denied", A, "a", "world", 80, DC.TCP, E, 64),
        ("an ingress tuple", A, "b", "a", 80, DC.TCP, 0, 64),
    ]
    rows = [r for r in rows for _ in range(4)]
    n = len(rows)
    pack = (lambda s: np.frombuffer(FC.ip6(a[s]), np.uint8)) if v6 else (lambda s: FC.ip4(a[s]))
    t = {"saddr": np.array([pack(r[2]) for r in rows], np.uint8 if v6 else np.uint32),
         "daddr": np.array([pack(r[3]) for r in rows], np.uint8 if v6 else np.uint32),
         "dport": np.array([L.htons(r[4]) for r in rows], np.uint16), "proto": np.array([r[5] for r in rows], np.uint8),
         "flags": np.array([r[6] for r in rows], np.uint8), "len": (100 + 13 * np.arange(n)).astype(np.uint32),
         "ep": np.array([r[1] for r in rows], np.uint16)}
    return [r[0] for r in rows], t, np.array([r[7] for r in rows], np.uint8)


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_classify_forward_deliver(torch_cuda, v6):
    from cilium_amd import synth
    from oracle import Oracle
    torch = torch_cuda
    w = _e2e_world(v6)
    names, t, ttl = _e2e_batch(v6)
    sec = {A: LAB_A, B: LAB_B, C3: LAB_C}
    # the three references: the restatement's classify, the forwarding
    # restatement on its verdicts, the delivery reference on the LOCAL rows
    o1 = Oracle(ct_proto_gate=1)
    _e2e_load(o1, v6)
    v, ident, st, _ = (o1.classify_v6 if v6 else o1.classify_v4)(t)
    f = FC.restate(w, FC.LXC, v6, t["daddr"], v, np.zeros(len(v), np.uint32), t["flags"], ttl)
    o2 = DC.new_oracle(lambda x: _e2e_load(x, v6, ipcache=False))
    dl = DC.reference(o2, v6, f["action"], f["arg"], DC.labels_of(t["ep"], sec), t["dport"], t["proto"], t["flags"],
                      t["len"])
    loc = f["action"] == FC.LOCAL
    by = dict(zip(names, zip(v.tolist(), f["action"].tolist(), dl["verdict"].tolist(), dl["stage"].tolist())))
    assert by["delivered"] == (0, FC.LOCAL, 0, 1)
    assert by["allowed on egress, denied at the destination"] == (0, FC.LOCAL, L.DROP_POLICY, 0)
    assert by["to the destination's proxy"] == (0, FC.LOCAL, L.htons(15001), 1)
    assert by["to the sender's proxy"][1] == FC.PROXY and by["denied on egress"][1] == FC.DROP
    assert by["wildcard at the destination"][2:] == (0, 3) and by["L3 key at the destination"][2:] == (0, 2)
    assert by["allowed by B, denied by A"] == (0, FC.LOCAL, L.DROP_POLICY, 0)
    assert by["gated protocol"][1] == FC.DROP and by["to the host"][1] == FC.HOST
    assert by["to the overlay"][1] == FC.OVERLAY and by["expired before delivery"][1] != FC.LOCAL
    assert by["fragment bit on IPv6" if v6 else "fragment: no L3 key at the destination"][2] == \
        (0 if v6 else L.DROP_POLICY)
    assert (dl["stage"][~loc] == L.STAGE_NOT_LOCAL).all() and loc.sum() >= 24

    e = _engine(ct_proto_gate=1, ipcache_tunnel=1, max_endpoints=16, **FC.engine_cfg(w))
    _e2e_load(e, v6)
    FC.load_world(e, w)
    for ep, lab in sec.items():
        assert e.lxc_update(ep, L.lxc_info(b"\0" * 6, 0, b"\0" * 16, 0, lab)) == 0
    e.commit()
    d = synth.to_device(t)
    d["ttl"] = torch.from_numpy(ttl).cuda()
    fwd = FC.fwd_kwargs(w, FC.LXC)
    out = (e.classify_v6 if v6 else e.classify_v4)(d, forward=fwd, deliver=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out["verdict"].cpu().numpy(), v)
    np.testing.assert_array_equal(out["identity"].cpu().numpy().view(np.uint32), ident)
    np.testing.assert_array_equal(out["stage"].cpu().numpy(), st)
    assert not out["tunnel"].cpu().numpy().any()
    for k in ("action", "ret", "ifindex", "arg"):
        np.testing.assert_array_equal(out["fwd_" + k].cpu().numpy().view(f[k].dtype), f[k], err_msg=k)
    for k, dt in OUT:
        np.testing.assert_array_equal(out["dlv_" + k].cpu().numpy().view(dt), dl[k], err_msg="dlv_" + k)
    # counters and metrics: the classify step's and the delivery step's together
    for ep, lab, dport, proto, egr, _ in E2E_POLICY:
        key = L.policy_key(lab, dport, proto, egr)
        want = [np.frombuffer(o.policy_lookup(ep, key)[1], L.POLICY_ENTRY)[0] for o in (o1, o2)]
        rc, got = e.policy_lookup(ep, key)
        assert rc == 0 and (int(got["packets"]), int(got["bytes"])) == \
            (sum(int(x["packets"]) for x in want), sum(int(x["bytes"]) for x in want)), (ep, lab, dport, egr)
    np.testing.assert_array_equal(e.metrics(), np.asarray(o1.metrics()) + np.asarray(o2.metrics()))
    # the separate calls give what the chained call gave; given dlv_ tensors are written in place
    e.counters_reset()
    sep = (e.deliver_v6 if v6 else e.deliver_v4)(out["fwd_action"], out["fwd_arg"], d["dport"], d["proto"], d["flags"],
                                                 d["len"], src_ep=d["ep"])
    torch.cuda.synchronize()
    for k, _ in OUT:
        assert torch.equal(sep[k], out["dlv_" + k]), k
    np.testing.assert_array_equal(e.metrics(), o2.metrics())
    mine = {"dlv_" + k: torch.zeros_like(x) for k, x in sep.items()}
    again = (e.classify_v6 if v6 else e.classify_v4)(d, out=dict(mine, verdict=out["verdict"], identity=out["identity"],
                                                               stage=out["stage"]), forward=fwd, deliver=True)
    torch.cuda.synchronize()
    for k, x in mine.items():
        assert again[k].data_ptr() == x.data_ptr() and torch.equal(x, out[k]), k
    with pytest.raises(ValueError):
        (e.classify_v6 if v6 else e.classify_v4)(d, forward=dict(fwd, mode=FC.NETDEV), deliver=True)
    for o in (o1, o2, e):
        o.close()
