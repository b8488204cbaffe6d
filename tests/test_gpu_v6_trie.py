"""The IPv6 ipcache trie's hard shapes through every device walk.

The three tables of v6_trie_cases.py (narrow: b24 staged in LDS, the long
node, windows, lists, inline records; wide: more b24 blocks than the x4 walk
stages, so it gathers b24 from global memory; sparse: lookups that match
nothing, shared h64 home slots, the window's outside, indirect labels) are
loaded into an engine and their probe addresses looked up by

* v6_lookup, one lane per address: the batched ipcache lookup, k_classify<V6>
  (CGPU_SCHED_PER_LANE), the per-lane conntrack prep;
* v6t_lookup_q, staged: the lookup pre-pass k_ipc6_pre (default schedule, also
  in front of the conntrack preps, also over the tunnel trie), the x4 kernel's
  own walk without the pre-pass (cluster_id 0 or past the DIRECT payload), its
  service form, and the frames forms over IPv6 frames that carry the probes.

The probes are the daddr of egress tuples and the saddr of ingress tuples
under a reserved handed-in identity; gated protocols (ct_proto_gate) leave
some lanes of a quad without a walk.  A few L3-only and exact policy entries
sit on the labels the tables return most, so a wrong label also moves a
verdict and a per-entry counter.  Expected values are the restatement's
(oracle), computed once per table and path configuration; every comparison is
bit-exact.  The shape conditions themselves are asserted on the CPU in
test_v6_trie.py.
"""
import numpy as np
import pytest

import v6_trie_cases as VC
from cilium_amd import build, layouts as L, synth
from test_frames_golden import frame_oracle

pytestmark = pytest.mark.gpu

PER_LANE = 1      # CGPU_SCHED_PER_LANE
FRAMES_SPLIT = 8  # CGPU_SCHED_FRAMES_SPLIT
WORLD = 2         # the reserved identity handed in for ingress tuples
N_EP = 3
CT_MAX = 1 << 17
NOW = 1000
FILL = -1
TABLES = sorted(VC.CASES)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a device"
    build.build()
    return torch


def _addrs(c):
    """The table's probes and some 40 addresses of the router's /64 (the
    cluster range: the egress fallback is cluster_id where no prefix
    covers them); ragged."""
    rng = np.random.Generator(np.random.PCG64(0xA6))
    k = 41 if (len(c.addrs) + 41) % 4 else 42
    x = rng.integers(0, 256, (k, 16), dtype=np.uint8)
    x[:, :8] = np.frombuffer(synth.ROUTER_IP6[:8], np.uint8)
    a = np.concatenate([c.addrs, x])
    assert len(a) % 4 != 0 and len(a) <= 40_000
    return a


def _batch(A):
    """The addresses as tuples: daddr of egress tuples, saddr of ingress ones;
    the other address is unique per tuple (and sport too), so no 5-tuple
    repeats on the conntrack path."""
    n = len(A)
    rng = np.random.Generator(np.random.PCG64(0xB6 + n))
    eg = rng.random(n) < 0.5
    other = np.zeros((n, 16), np.uint8)
    other[:, 0] = 0xFD
    other[:, 12:] = np.arange(n, dtype=">u4").view(np.uint8).reshape(n, 4)
    proto = rng.choice(np.array([6, 17, 58, 1], np.uint8), n, p=[0.45, 0.2, 0.15, 0.2])
    frag = rng.random(n) < 0.05
    syn = (5 << 4) | (L.TCP_SYN << 8)
    return {"saddr": np.where(eg[:, None], other, A), "daddr": np.where(eg[:, None], A, other),
            "sport": (1024 + np.arange(n)).astype(np.uint16).byteswap(),
            "dport": rng.choice(np.array([80, 443, 53], np.uint16), n).byteswap(),
            "proto": proto, "l4b": np.where(proto == 6, syn, np.where(proto == 58, 128, 0)).astype(np.uint16),
            "flags": (eg.astype(np.uint8) | (frag.astype(np.uint8) << 1)),
            "len": rng.integers(64, 1501, n).astype(np.uint32),
            "ep": rng.integers(0, N_EP, n).astype(np.uint16),
            "hash": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)}


def _frames(A):
    """39999 frames, 3 in 4 of them IPv6 with the probe addresses (the IPv6
    frames of 110k drawn ones and some of the others, in their order: about
    one IPv6 frame in five parses clean in a 64-byte slot); the same frames in
    128- and 64-byte slots."""
    rng = np.random.Generator(np.random.PCG64(0xF6 + len(A)))
    f = synth.make_frames(rng, 110_000, width=128, n_ep=N_EP, addr6=A)
    v6 = (f["data"][:, 12] == 0x86) & (f["data"][:, 13] == 0xDD)
    rest = np.flatnonzero(~v6)
    keep = np.sort(np.concatenate([np.flatnonzero(v6), rng.choice(rest, 39_999 - int(v6.sum()), replace=False)]))
    f = {k: np.ascontiguousarray(v[keep]) for k, v in f.items()}
    return {128: f, 64: dict(f, data=np.ascontiguousarray(f["data"][:, :64]))}


def _policy(rows):
    """(ep, key, entry) on the labels the table returns most often: L3-only
    and exact (port 80 / TCP) entries in both directions, and the fallback
    identity where nothing (or a tombstone) matches."""
    labs, cnt = np.unique(rows[(rows[:, 0] == 1) & (rows[:, 1] != 0), 1], return_counts=True)
    top = labs[np.argsort(-cnt, kind="stable")[:24]]
    out = [(0, L.policy_key(WORLD, 0, 0, 1), L.policy_entry()), (1, L.policy_key(WORLD, 0, 0, 0), L.policy_entry())]
    for j, lab in enumerate(top):
        for eg in (0, 1):
            k = L.policy_key(int(lab), 0, 0, eg) if j % 2 == 0 else L.policy_key(int(lab), 80, 6, eg)
            out.append((j % N_EP, k, L.policy_entry()))
    return out


class Tab:
    """One table with everything the restatement says about it, computed once."""

    def __init__(self, name):
        self.c = VC.CASES[name]()
        self.addrs = _addrs(self.c)
        self.rows = VC.restate(self.c, self.addrs)
        self.batch = _batch(self.addrs)
        self.policy = _policy(self.rows)
        self.seclabels = (np.arange(N_EP, dtype=np.uint32) * 7 + 6000).astype(np.uint32)
        self._frames = None
        self._exp = {}

    @property
    def frames(self):
        if self._frames is None:
            self._frames = _frames(self.addrs)
        return self._frames

    def load(self, t):
        VC.load_ipcache(t, self.c)
        for ep, k, en in self.policy:
            assert t.policy_update(ep, k, en) == 0

    def counters(self, t):
        out = []
        for ep, k, _ in self.policy:
            rc, got = t.policy_lookup(ep, k)
            assert rc == 0
            got = got if isinstance(got, np.void) else np.frombuffer(got, L.POLICY_ENTRY)[0]
            out.append((int(got["packets"]), int(got["bytes"])))
        return out

    def expected(self, kind, stride=0, **cfg):
        """kind: "plain" | "lb" | "ct" | "frames" -> the restatement's columns,
        per-entry counters and metrics under cfg."""
        key = (kind, stride, tuple(sorted(cfg.items())))
        if key in self._exp:
            return self._exp[key]
        from oracle import Oracle
        base = dict(ct_proto_gate=1, ingress_src_identity=WORLD, **cfg)
        o = frame_oracle(1, 7, n_ep=N_EP, ingress_src_identity=WORLD, **cfg) if kind == "frames" else Oracle(**base)
        self.load(o)
        if kind == "plain":
            v, i, s, _ = o.classify_v6(self.batch, nthreads=4)
            r = {"verdict": v, "identity": i, "stage": s}
        elif kind == "lb":
            v, i, s, _ = o.classify_v6_lb(self.batch, nthreads=4)
            r = {"verdict": v, "identity": i, "stage": s}
        elif kind == "ct":
            synth.load_lxc(o, self.seclabels)
            o.ct6_set_max(CT_MAX)
            v, cr, i, s, _ = o.classify_v6_ct(self.batch, NOW)
            r = {"verdict": v, "ct_ret": cr, "identity": i, "stage": s, "ct_count": o.ct6_count()}
        else:
            f = self.frames[stride]
            v, i, s, _ = o.classify_frames(f, nthreads=4)
            p = o.frames_parse(f)
            r = {"verdict": v, "identity": i, "stage": s,
                 "v6_ok": int(((p["status"] == 0) & (p["family"] == 6)).sum())}
        r["counters"] = self.counters(o)
        r["metrics"] = o.metrics()
        o.close()
        self._exp[key] = r
        return r


@pytest.fixture(scope="module")
def tabs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Tab(name)
        return cache[name]
    return get


def _engine(T, frames=False, **kw):
    from cilium_amd.engine import Engine
    e = Engine(device=0, ct_proto_gate=1, ingress_src_identity=WORLD, policy_max_total=1 << 12, max_endpoints=8,
               **kw)
    T.load(e)
    if frames:
        info = L.lxc_info(synth.LXC_MAC, synth.LXC_IPV4_RAW, synth.LXC_IP6, 7)
        for ep in range(N_EP):
            assert e.lxc_update(ep, info) == 0
    return e


def _check(T, e, out, exp):
    """verdict, identity, stage (ct_ret), per-entry counters, metrics"""
    for k, dt in (("verdict", np.int32), ("identity", np.uint32), ("stage", np.uint8), ("ct_ret", np.uint8)):
        if k in exp:
            got = out[k].cpu().numpy().view(dt)
            bad = np.flatnonzero(got != exp[k])
            assert len(bad) == 0, (k, len(bad), bad[:5], got[bad[:5]], exp[k][bad[:5]])
    assert T.counters(e) == exp["counters"]
    np.testing.assert_array_equal(e.metrics(), exp["metrics"])
    # the expectation is not flat: allowed and denied tuples, counted entries
    assert (exp["verdict"] == 0).sum() > 100 and (exp["verdict"] == L.DROP_POLICY).sum() > 100
    assert sum(p for p, _ in exp["counters"]) > 100


# ---- the batched lookup (k_ipcache_lookup -> v6_lookup) ------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("table", TABLES)
def test_lookup(torch_cuda, tabs, table, offset):
    """found and sec_label of every probe; the address column 16-byte aligned
    and as a view one byte into a larger buffer (any alignment)."""
    torch = torch_cuda
    T = tabs(table)
    e = _engine(T)
    e.commit()
    q = T.addrs
    buf = torch.zeros(q.size + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + q.size].view(-1, 16)
    v.copy_(torch.from_numpy(q))
    out = e.ipcache_lookup_batch(v)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out["found"].cpu().numpy(), T.rows[:, 0])
    np.testing.assert_array_equal(out["sec_label"].cpu().numpy().view(np.uint32), T.rows[:, 1])
    assert len(np.unique(T.rows[:, 1])) > 100
    e.close()


# ---- the stateless classify paths ---------------------------------------------
# id -> (restatement kind, engine / restatement config, engine-only config, tunnel output)
CLASSIFY = {
    "per_lane": ("plain", {}, dict(schedule=PER_LANE), False),        # k_classify<V6> -> v6_lookup
    "prepass": ("plain", {}, {}, False),                              # k_ipc6_pre + x4 kernel
    "prepass_tunnel": ("plain", {}, dict(ipcache_tunnel=1), True),    # ... and the tunnel trie t6
    "x4_walk_cluster0": ("plain", dict(cluster_id=0), {}, False),     # no pre-pass: the x4 kernel's Q = 2 walk
    "x4_walk_cluster_big": ("plain", dict(cluster_id=0x7FFFFFFF), {}, False),
    "lb": ("lb", {}, {}, False),                                      # the service form's walk (no services)
}


@pytest.mark.parametrize("path", sorted(CLASSIFY))
@pytest.mark.parametrize("table", TABLES)
def test_classify(torch_cuda, tabs, table, path):
    torch = torch_cuda
    T = tabs(table)
    kind, cfg, ecfg, tunnel = CLASSIFY[path]
    exp = T.expected(kind, **cfg)
    e = _engine(T, **cfg, **ecfg)
    e.commit()
    d = synth.to_device(T.batch)
    n = len(T.addrs)
    if tunnel:
        full = torch.full((n + 8,), FILL, dtype=torch.int32, device="cuda")
        out = {"verdict": torch.empty(n, dtype=torch.int32, device="cuda"),
               "identity": torch.empty(n, dtype=torch.int32, device="cuda"),
               "stage": torch.empty(n, dtype=torch.uint8, device="cuda"), "tunnel": full[:n]}
        out = e.classify_v6(d, out=out, tunnel=True)
    elif kind == "lb":
        out = e.classify_v6_lb(d)
    else:
        out = e.classify_v6(d)
    torch.cuda.synchronize()
    _check(T, e, out, exp)
    if tunnel:
        t, r = T.batch, T.rows
        want = ((t["flags"] & 1) == 1) & np.isin(t["proto"], (6, 17, 58)) & (r[:, 0] == 1) & (r[:, 1] != 0)
        want_tun = np.where(want, r[:, 2], 0).astype(np.uint32)
        assert len(np.unique(want_tun)) > 100
        np.testing.assert_array_equal(out["tunnel"].cpu().numpy().view(np.uint32), want_tun)
        assert (full[n:].cpu().numpy() == FILL).all(), "written past n"
        lk = e.ipcache_lookup_batch(torch.from_numpy(T.addrs).cuda())
        torch.cuda.synchronize()
        got = np.stack([lk["found"].cpu().numpy().astype(np.uint32), lk["sec_label"].cpu().numpy().view(np.uint32),
                        lk["tunnel"].cpu().numpy().view(np.uint32)], 1)
        np.testing.assert_array_equal(got, r)
    e.close()


# ---- the conntrack path -------------------------------------------------------
CT = {
    "prepass": ({}, {}),                              # k_ipc6_pre (every tuple walks) + k_ct_prep6_q
    "per_lane_schedule": ({}, dict(schedule=PER_LANE)),
    "per_lane_prep_cluster0": (dict(cluster_id=0), {}),  # no pre-pass: k_ct_prep6 -> v6_lookup
}


@pytest.mark.parametrize("path", sorted(CT))
@pytest.mark.parametrize("table", TABLES)
def test_classify_ct(torch_cuda, tabs, table, path):
    """A fresh map, one `now`, no 5-tuple twice: every tracked tuple is a
    create or a policy drop, whatever the order the device takes them in."""
    torch = torch_cuda
    T = tabs(table)
    cfg, ecfg = CT[path]
    exp = T.expected("ct", **cfg)
    e = _engine(T, ct_max=CT_MAX, ct6_max=CT_MAX, **cfg, **ecfg)
    synth.load_lxc(e, T.seclabels)
    e.commit()
    out = e.classify_v6_ct(synth.to_device(T.batch), NOW)
    torch.cuda.synchronize()
    _check(T, e, out, exp)
    assert e.ct6_count() == exp["ct_count"] and exp["ct_count"] > 1000
    assert (exp["ct_ret"] == L.CT_NEW).sum() > 1000 and (exp["ct_ret"] == L.CT_NONE).sum() > 1000
    e.close()


# ---- raw IPv6 frames ----------------------------------------------------------
FRAMES = {"fused64": (64, 0), "split64": (64, FRAMES_SPLIT), "slots128": (128, 0)}


@pytest.mark.parametrize("path", sorted(FRAMES))
@pytest.mark.parametrize("table", TABLES)
def test_classify_frames(torch_cuda, tabs, table, path):
    """IPv6 frames whose addresses are the probes, between IPv4, ARP and other
    frames: the x4 frames kernels' own walk over a non-empty trie."""
    torch = torch_cuda
    T = tabs(table)
    stride, sched = FRAMES[path]
    exp = T.expected("frames", stride=stride)
    assert exp["v6_ok"] >= 5000
    e = _engine(T, frames=True, schedule=sched)
    e.commit()
    out = e.classify_frames(synth.frames_to_device(T.frames[stride]))
    torch.cuda.synchronize()
    _check(T, e, out, exp)
    e.close()
