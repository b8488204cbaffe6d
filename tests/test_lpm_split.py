"""The split x16 slot (tables.h LPMC_SPLIT) on the CPU: what Lpm16cBuild makes
of the crafted /16s of lpm_split_cases.py (cgpu_diag_ipc4_split,
cgpu_diag_ipc4_shapes) and the library's host walk, which takes the split form
first as the plain x4 kernel does, over all 65,536 addresses of every crafted
/16, after a full build and after a second commit that patches.  Expected
answers are the restatement's; every comparison is exact.
test_gpu_lpm_split.py runs the same /16s through the device walks.
"""
import ctypes as C

import numpy as np
import pytest

import lpm_split_cases as SC
from test_cascade_shapes import ipc4_shapes
from test_tunnel_cpu import diag, hook

VP = C.c_void_p
COLS = ("kids2", "kids3", "kids4", "kids5", "unsplit_nocode", "past24", "kid_words", "live_kid_words")


def ipc4_split(keys, vals, n_first=None):
    """cgpu_diag_ipc4_split -> ([identity table dict, tunnel table dict], [builds, patched])"""
    keys = np.ascontiguousarray(keys, SC.L.IPCACHE_KEY)
    vals = np.ascontiguousarray(vals, SC.L.REMOTE_ENDPOINT_INFO)
    out = np.full(16, 0xDEADBEEF, np.uint32)
    commits = np.zeros(2, np.uint64)
    rc = hook("cgpu_diag_ipc4_split", [VP, VP, VP, C.c_size_t, C.c_size_t, VP, VP])(
        keys.ctypes.data, vals.ctypes.data, None, len(keys), len(keys) if n_first is None else n_first,
        out.ctypes.data, commits.ctypes.data)
    assert rc == 0, rc
    return [dict(zip(COLS, (int(x) for x in row))) for row in out.reshape(2, 8)], commits.tolist()


@pytest.fixture(scope="module")
def case():
    return SC.split_case()


def _expected_counts(c, phase):
    kids = [v[phase - 1] for v in c.children.values()]
    starts = {n: v[phase - 1] for n, v in c.starts.items()}
    unsplit = sum(1 for n, k in starts.items() if 5 <= k <= SC.MAX_STARTS and c.children[n][phase - 1] == 0)
    return {"kids2": kids.count(2), "kids3": kids.count(3), "kids4": kids.count(4), "kids5": kids.count(5),
            "unsplit_nocode": unsplit, "past24": sum(1 for k in starts.values() if k > SC.MAX_STARTS),
            "live_kid_words": 4 * sum(kids)}


def test_the_shapes_cover_every_child_count(case):
    """child counts 2..5, a last child of one run and of five, the fall-backs"""
    k1 = {n: v[0] for n, v in case.children.items()}
    assert {k1[f"s{k}"] for k in (5, 6, 9, 10, 11, 15, 19, 20, 24)} == {2, 3, 4, 5}
    assert (k1["s5"], k1["s9"], k1["s10"], k1["s24"]) == (2, 2, 3, 5)   # 6 = 5 + 1 runs, 10 = 5 + 5, 11, 25
    assert k1["s4"] == 0 and k1["s25"] == 0 and k1["nocode6"] == 0
    assert k1["ffff_coarse"] == 3 and (case.starts["ffff_coarse"][0] + 1) % 5 == 1  # run 10 = child 2 alone


@pytest.mark.parametrize("phase", [1, 2])
def test_split_counts(case, phase):
    """cgpu_diag_ipc4_split: every crafted /16 is split into the children its
    run starts ask for, in the identity table and in the tunnel table"""
    k, v = case.entries(phase)
    tabs, commits = ipc4_split(k, v, n_first=len(case.keys1))
    assert commits == ([1, 0] if phase == 1 else [1, 1]), "the second commit rebuilt instead of patching"
    want = _expected_counts(case, phase)
    for t in tabs:
        for col, n in want.items():
            assert t[col] == n, (col, t, want)
        if phase == 1:
            assert t["kid_words"] == t["live_kid_words"]
        else:
            # s4 -> 6 starts (2 new children), s6 -> 4 (2 dropped), s5 -> 7 with a
            # leaf without a code (2 dropped), s24 -> 26 (5 dropped): replaced
            # children stay behind as garbage
            assert t["kid_words"] - t["live_kid_words"] == 4 * (2 + 2 + 5)


@pytest.mark.parametrize("n", sorted(SC.split_case().shapes))
def test_every_shape_alone(case, n):
    """one crafted /16 at a time (with the coded labels' /16s): its children"""
    first = len(SC.CODED) + 1
    p16 = (case.keys1["ip"][:, 0].astype(np.uint32) << 8) | case.keys1["ip"][:, 1]
    plen = case.keys1["prefixlen"] - SC.L.IPCACHE_STATIC_PREFIX
    p = case.shapes[n]
    keep = (np.arange(len(p16)) < first) | ((p16 == p) & (plen >= 15)) | (plen == 0)
    tabs, _ = ipc4_split(case.keys1[keep], case.vals1[keep])
    kids = case.children[n][0]
    got = [tabs[0][f"kids{j}"] for j in (2, 3, 4, 5)]
    assert got == [int(kids == j) for j in (2, 3, 4, 5)], (n, tabs[0])
    k = case.starts[n][0]
    assert tabs[0]["unsplit_nocode"] == int(5 <= k <= SC.MAX_STARTS and kids == 0), (n, tabs[0])
    assert tabs[0]["past24"] == int(k > SC.MAX_STARTS), (n, tabs[0])
    assert tabs[1] == tabs[0], n


@pytest.mark.parametrize("phase", [1, 2])
def test_old_shapes_stay(case, phase):
    """cgpu_diag_ipc4_shapes keeps its meaning: a split /16 still counts as the
    overflow slot with the run node or array it had"""
    k, v = case.entries(phase)
    sh, _ = ipc4_shapes(k, v, n_first=len(case.keys1))
    starts = [s[phase - 1] for s in case.starts.values()]
    for t in sh:
        assert t[5] >= sum(1 for s in starts if s == 4)                       # inline, 4 run starts
        assert t[9] == sum(1 for s in starts if 5 <= s <= 10)                 # 64-byte run nodes
        assert t[10] == sum(1 for s in starts if s > 10)                      # arrays
        assert t[7] == 0 and t[8] == 0


@pytest.mark.parametrize("phase", [1, 2])
def test_host_walk_every_address(case, phase):
    """the library's host walk of both tables over all 65,536 addresses of
    every crafted /16 against the restatement"""
    k, v = case.entries(phase)
    exp = SC.restate(phase)
    got, commits = diag(k, v, case.probes(), 0, n_first=len(case.keys1))
    assert commits.tolist() == ([1, 0] if phase == 1 else [1, 1])
    bad = np.flatnonzero((got != exp).any(1))
    assert len(bad) == 0, (len(bad), case.probes()[bad[:5]], got[bad[:5]], exp[bad[:5]])
    # the expectation is not flat: tombstones, labels >= 2^30, the /8, the background
    lab = exp[:, 1]
    assert (exp[:, 0] == 1).all() and (lab == 0).sum() > 100 and (lab >= 1 << 30).sum() > 100
    assert (lab == SC.UNDER8).sum() > 1000 and (lab == SC.L.WORLD_ID).sum() > 100_000
    assert len(np.unique(exp[:, 2])) >= 10
