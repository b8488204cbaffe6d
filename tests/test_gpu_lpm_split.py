"""The split x16 slot (tables.h LPMC_SPLIT) through the device walks.

Every address of every crafted /16 of lpm_split_cases.py -- 4, 5 .. 24 run
starts (2 .. 5 children, a last child of one run and of five), 25 (falls
back), run starts at 0xFFFF in a child and as a coarse start, nested prefixes,
a tombstone, a label >= 2^30, a leaf without a code (falls back), the cluster
range, a /16 under a /8 -- runs through

* classify_v4 at n = 65,536 k + 3: the plain k_classify_x4 takes the split
  slot (whole quads, the ragged tail), and every stateless sibling path of
  test_gpu_cascade_shapes.py must ignore the new bits of an overflow slot;
* ipcache_lookup_batch (lpmc_lookup over the identity and the tunnel table);

after one commit and after a second one that patches the /16s in place, and
two small batches make the plain kernel's wave-uniform branches go both ways:
waves without a split lane and waves of split lanes only.  Expected values are
the restatement's, computed once per path kind and commit; every comparison
is exact.  That the tables hold the shapes is asserted on the CPU in
test_lpm_split.py.
"""
import numpy as np
import pytest

import lpm_split_cases as SC
from cilium_amd import layouts as L, synth
from test_gpu_cascade_shapes import FILL, STATELESS, Tab, _engine, _offset1, _same, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


class SplitTab(Tab):
    def __init__(self):
        self.name = "lpm_split"
        self.w = SC.extras()
        self._frames = None
        self._exp = {}
        self._rows = {}


@pytest.fixture(scope="module")
def tab():
    return SplitTab()


def _rows_of_batch(phase):
    """the restatement's ipcache rows of the plain batch's looked-up addresses"""
    r = SC.restate(phase)
    return np.concatenate([r, r[:3]])


def _check(T, e, out, exp, phase):
    _same(out, exp)
    assert T.w.counters(e, phase) == exp["counters"]
    np.testing.assert_array_equal(e.metrics(), exp["metrics"])
    v = exp["verdict"]
    assert (v == 0).sum() > 1000 and (v == L.DROP_POLICY).sum() > 1000 and (v > 0).sum() > 100
    assert sum(p > 0 for p, _ in exp["counters"]) > 20
    assert len(np.unique(exp["identity"])) >= 10


@pytest.mark.parametrize("path", sorted(STATELESS))
@pytest.mark.parametrize("phase", [1, 2])
def test_classify_v4(torch_cuda, tab, phase, path):
    torch = torch_cuda
    kind, ecfg, call = STATELESS[path]
    exp = tab.expected(kind, phase)
    e = _engine(tab, kind, phase, **ecfg)
    b = tab.batch(kind)
    n = len(b["flags"])
    assert n % 65536 == 3
    d = synth.to_device(b)
    if call == "offset1":
        out = e.classify_v4(_offset1(torch, d))
    elif call == "tunnel":
        full = torch.full((n + 8,), FILL, dtype=torch.int32, device="cuda")
        out = {"verdict": torch.empty(n, dtype=torch.int32, device="cuda"),
               "identity": torch.empty(n, dtype=torch.int32, device="cuda"),
               "stage": torch.empty(n, dtype=torch.uint8, device="cuda"), "tunnel": full[:n]}
        out = e.classify_v4(d, out=out, tunnel=True)
    else:
        out = {"plain": e.classify_v4, "lb": e.classify_v4_lb, "cascade": e.classify_v4_cascade}[call](d)
    torch.cuda.synchronize()
    _check(tab, e, out, exp, phase)
    if call == "tunnel":
        # the entry an egress tuple's identity came from (a non-zero label),
        # for the protocols the conntrack gate passes
        r = _rows_of_batch(phase)
        eg = ((b["flags"] & 1) == 1) & np.isin(b["proto"], (6, 17, 1))
        want = np.where(eg & (r[:, 0] == 1) & (r[:, 1] != 0), r[:, 2], 0).astype(np.uint32)
        assert len(np.unique(want)) >= 10
        np.testing.assert_array_equal(out["tunnel"].cpu().numpy().view(np.uint32), want)
        assert (full[n:].cpu().numpy() == FILL).all(), "written past n"
    e.close()


@pytest.mark.parametrize("phase", [1, 2])
def test_ipcache_lookup_batch(torch_cuda, tab, phase):
    """k_ipcache_lookup (lpmc_lookup over both tables): the split slots' word 0
    and bit 63 are an overflow slot's"""
    torch = torch_cuda
    c = SC.split_case()
    exp = SC.restate(phase)
    e = _engine(tab, "plain", phase, ipcache_tunnel=1)
    lk = e.ipcache_lookup_batch(torch.from_numpy(c.probes().view(np.int32)).cuda())
    torch.cuda.synchronize()
    got = np.stack([lk["found"].cpu().numpy().astype(np.uint32), lk["sec_label"].cpu().numpy().view(np.uint32),
                    lk["tunnel"].cpu().numpy().view(np.uint32)], 1)
    bad = np.flatnonzero((got != exp).any(1))
    assert len(bad) == 0, (len(bad), c.probes()[bad[:5]], got[bad[:5]], exp[bad[:5]])
    e.close()


@pytest.mark.parametrize("which", ["no_split_lane", "only_split_lanes"])
@pytest.mark.parametrize("phase", [1, 2])
def test_wave_uniform_branches(torch_cuda, tab, phase, which):
    """4099 tuples (16 waves of the plain kernel and a ragged tail) none of
    which looks up a split /16 -- inline, past 24 run starts, a leaf without a
    code: the node stages run, no lane has a child -- and 4099 that all do
    and all reach the lookup: no wave enters the node stages"""
    c = SC.split_case()
    exp = tab.expected("plain", phase)
    b = tab.batch("plain")
    split = np.array([p for n, p in c.shapes.items() if c.children[n][phase - 1]], np.uint32)
    looked = np.where(b["flags"] & 1, b["daddr"], b["saddr"]).astype(np.uint32).byteswap() >> 16
    is_split = np.isin(looked, split)
    runs = np.isin(b["proto"], (6, 17)) & ((b["flags"] & 2) == 0)
    ix = np.flatnonzero(~is_split if which == "no_split_lane" else is_split & runs)
    ix = ix[np.random.Generator(np.random.PCG64(7 + phase)).permutation(len(ix))[:4099]]
    assert len(ix) == 4099
    if which == "no_split_lane":
        assert len(np.unique(looked[ix])) >= 3
    e = _engine(tab, "plain", phase)
    out = e.classify_v4(synth.to_device({k: np.ascontiguousarray(v[ix]) for k, v in b.items()}))
    torch_cuda.cuda.synchronize()
    sub = {k: exp[k][ix] for k in ("verdict", "identity", "stage")}
    _same(out, sub, which)
    assert len(np.unique(sub["identity"])) >= 3
    e.close()
