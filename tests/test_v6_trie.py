"""CPU parity of the IPv6 ipcache trie (tables.h v6_lpm, host.cpp build_v6;
VERDICT r2 next 4): the library builds the trie from ipcache keys exactly as
a commit does and answers lookups with its host restatement of the device
walk (cgpu_diag_ipc6_trie, a test hook outside include/cgpu.h); the answers
must equal the restatement's ipcache LPM (oracle/cgpu_oracle.c
or_ipcache_lookup, pinned by tests/golden/classify_v6.npz), address by
address.  The device walks themselves (v6_lookup, v6t_lookup_q staged and
unstaged, the pre-pass, the frames and conntrack forms) run over the same
narrow / wide / sparse tables (v6_trie_cases.py) in test_gpu_v6_trie.py; the
v6 cases of test_gpu_parity / test_gpu_fullsize only meet tables of random
addresses (no long node, hardly a /64 list of several prefixes).  The
conditions that make those three tables hard are asserted here, without a
device.  Shapes: the config-v6 table, a /32 too dense for
64 sub-range lines (the binary-searched long node), boundaries at both ends
of a /32 (a window of the whole range), /64s with several nested or disjoint
/65+ prefixes (lists), static-part entries and ::/0 under everything, /17../32
expansion under longer prefixes, tombstones."""
import ctypes as C

import numpy as np
import pytest

import v6_trie_cases as VC
from cilium_amd import _abi, layouts as L, synth
from v6_trie_cases import edge_table, keys_of, probes

V6T_LONG = 7
V6T_LDS_B24 = 96  # kernels.hip: b24 blocks the x4 walk stages in LDS at most


def trie(keys, labels, addrs):
    f = _abi.lib().cgpu_diag_ipc6_trie
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    keys = np.ascontiguousarray(keys)
    labels = np.ascontiguousarray(labels, np.uint32)
    addrs = np.ascontiguousarray(addrs, np.uint8)
    out = np.empty(len(addrs), np.uint32)
    st = np.zeros(8, np.uint32)
    rc = f(keys.ctypes.data, labels.ctypes.data, len(keys), addrs.ctypes.data, len(addrs),
           out.ctypes.data, st.ctypes.data)
    assert rc == 0
    return out, dict(zip(("nodes", "long", "h64", "lists", "pool", "b24", "b32", "slots"), st.tolist()))


def oracle_labels(keys, labels, addrs):
    from oracle import Oracle
    o = Oracle()
    v = np.zeros(len(keys), L.REMOTE_ENDPOINT_INFO)
    v["sec_label"] = labels
    for k, x in zip(keys, v):
        assert o.ipcache_update(k, x) == 0
    q = np.zeros((), L.IPCACHE_KEY)
    q["prefixlen"] = L.IPCACHE_STATIC_PREFIX + 128
    q["family"] = L.ENDPOINT_KEY_IPV6
    out = np.empty(len(addrs), np.uint32)
    for i, a in enumerate(addrs):
        q["ip"] = a
        r, raw = o.ipcache_lookup(q)
        out[i] = np.frombuffer(raw, L.REMOTE_ENDPOINT_INFO)[0]["sec_label"] if r == 0 else 0xFFFFFFFF
    return out


def check(keys, labels, addrs):
    got, st = trie(keys, labels, addrs)
    exp = oracle_labels(keys, labels, addrs)
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, (len(bad), addrs[bad[:3]], got[bad[:3]], exp[bad[:3]])
    return st


def test_trie_config_v6_table():
    T = synth.make_tables6(n_prefixes=20_000, n_identities=500, n_endpoints=2, keys_per_ep=100)
    rng = np.random.Generator(np.random.PCG64(61))
    pick = rng.choice(len(T.pfx_len), 3000, replace=False)
    addrs = probes(T.pfx_addr[pick], T.pfx_len[pick], rng, 5000)
    addrs = np.concatenate([addrs, synth.make_tuples6(T, 5000)["daddr"]])
    st = check(T.ipc_keys, T.ipc_vals["sec_label"], addrs)
    assert st["nodes"] > 100 and st["h64"] > 1000


def test_trie_edge_shapes():
    keys, labels, addr, plen, rng = edge_table()
    addrs = probes(addr, plen, rng, 20_000)
    st = check(keys, labels, addrs)
    assert st["long"] >= 1           # the dense /32
    assert st["lists"] >= 20         # nested / disjoint /65+ in one /64
    assert st["h64"] > st["lists"]   # and inline records


@pytest.fixture(scope="module", params=sorted(VC.CASES))
def case_stats(request):
    """Every shared table: the host walk equals the restatement on its probe
    addresses; -> (case, trie statistics, restatement rows)."""
    c = VC.CASES[request.param]()
    st = check(c.keys, c.labels, c.addrs)
    return c, st, VC.restate(c)


def test_case_probe_sets(case_stats):
    """What the device tests rely on: ragged, at most 40k, and the
    restatement's batch lookup says what its map lookup says."""
    c, _, rows = case_stats
    assert len(c.addrs) % 4 != 0 and len(c.addrs) <= 40_000
    exp = oracle_labels(c.keys, c.labels, c.addrs[::7])
    np.testing.assert_array_equal(np.where(rows[::7, 0] == 1, rows[::7, 1], 0xFFFFFFFF), exp)
    hit = rows[:, 0] == 1
    assert len(np.unique(rows[hit, 2])) > 100  # a tunnel word per prefix
    assert (hit & (rows[:, 1] == 0)).sum() >= 10  # tombstones are matches


def test_case_shapes(case_stats):
    """The conditions on the inputs (stated for the tables, not for the
    library's answers): which trie levels and arms the probes reach."""
    c, st, rows = case_stats
    print(c.name, st)
    w0, w1 = c.h64_keys()
    assert st["h64"] == len(w0)  # one record per /64 with /65+ prefixes
    if c.name == "narrow":
        assert 1 <= st["b24"] <= V6T_LDS_B24 and st["long"] >= 1
        return
    if c.name == "wide":
        assert st["b24"] > V6T_LDS_B24 and st["long"] >= 1 and st["lists"] >= 20
        return
    miss = (rows[:, 0] == 0).mean()
    n_out = int(c.outside().sum())
    slots = st["slots"]
    assert slots & (slots - 1) == 0
    per_home = np.bincount(VC.mix32(w0, w1) & np.uint32(slots - 1), minlength=slots)
    indirect = np.unique(rows[(rows[:, 0] == 1) & (rows[:, 1] >= 1 << 30), 1])
    print("miss", miss, "outside", n_out, "homes >= 2", (per_home >= 2).sum(), ">= 3", (per_home >= 3).sum(),
          "indirect", len(indirect))
    assert 0.05 <= miss <= 0.60
    assert n_out >= 100
    assert len(w0) >= 3000
    assert (per_home >= 2).sum() >= 50 and (per_home >= 3).sum() >= 5
    assert len(indirect) >= 20


def test_frames_addr6_pool():
    """synth.make_frames(addr6=): IPv6 frames carry pool addresses (about
    90 % of the destinations, of the sources all but the endpoint's own);
    an empty pool draws nothing, so the frames are those of addr6=None."""
    pool = VC.narrow().addrs[:5000]
    mk = lambda **kw: synth.make_frames(np.random.Generator(np.random.PCG64(9)), 20_000, width=128, **kw)  # noqa: E731
    f, f0, fe = mk(addr6=pool), mk(), mk(addr6=pool[:0])
    assert all(np.array_equal(f0[k], fe[k]) for k in f0)
    D = f["data"]
    v6 = (D[:, 12] == 0x86) & (D[:, 13] == 0xDD)
    keys = set(map(bytes, pool))
    d_in = np.array([bytes(r) in keys for r in D[v6, 38:54]])
    s_in = np.array([bytes(r) in keys for r in D[v6, 22:38]])
    lxc = (D[v6, 22:38] == np.frombuffer(synth.LXC_IP6, np.uint8)).all(1)
    assert v6.sum() > 4000 and 0.8 < d_in.mean() < 0.95
    assert not (s_in & lxc).any() and 0.8 < s_in[~lxc].mean() < 0.95
    assert np.array_equal(f["data"][~v6], f0["data"][~v6])  # the other frames are unchanged


def test_mix32_mirror():
    """The numpy mix32 against values worked out with Python integers."""
    def ref(a, b):
        m = (1 << 64) - 1
        h = ((b << 32 | a) * 0x9E3779B97F4A7C15) & m
        h ^= h >> 29
        h = (h * 0xBF58476D1CE4E5B9) & m
        h ^= h >> 32
        return h & 0xFFFFFFFF
    rng = np.random.Generator(np.random.PCG64(5))
    a = rng.integers(0, 1 << 32, 200, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, 200, dtype=np.uint64).astype(np.uint32)
    a[:3], b[:3] = [0, 0xFFFFFFFF, 1], [0, 0xFFFFFFFF, 0]
    assert VC.mix32(a, b).tolist() == [ref(int(x), int(y)) for x, y in zip(a, b)]


def test_trie_static_only_and_empty():
    # only static-part entries: no trie levels below the root
    k = np.zeros(1, L.IPCACHE_KEY)
    k["family"] = L.ENDPOINT_KEY_IPV6
    k["prefixlen"] = 20
    addrs = np.random.Generator(np.random.PCG64(3)).integers(0, 256, (100, 16), dtype=np.uint8)
    check(k, np.array([9], np.uint32), addrs)
    got, _ = trie(np.zeros(0, L.IPCACHE_KEY), np.zeros(0, np.uint32), addrs)
    assert (got == 0xFFFFFFFF).all()


@pytest.mark.parametrize("seed", [1, 2])
def test_trie_random_nested(seed):
    """Random nested prefix sets: every length 0..128 under a few /16 roots."""
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    roots = rng.integers(0, 256, (4, 2), dtype=np.uint8)
    n = 4000
    a = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    a[:, :2] = roots[rng.integers(0, 4, n)]
    # cluster: half the prefixes share longer stems so they nest
    stem = a[rng.integers(0, 64, n)]
    keep = rng.integers(2, 14, n)
    for i in range(n // 2):
        a[i, :keep[i]] = stem[i, :keep[i]]
    plen = rng.integers(0, 129, n)
    a &= synth.MASK6[plen]
    keys = keys_of(a, plen)
    canon = np.zeros(n, np.dtype([("l", "u4"), ("a", "u1", (16,))]))
    canon["l"], canon["a"] = plen, a
    _, first = np.unique(canon.view(np.dtype((np.void, 20))), return_index=True)
    keys, a, plen = keys[first], a[first], plen[first]
    labels = rng.integers(1, 1 << 31, len(keys)).astype(np.uint32)  # indirect labels too
    addrs = probes(a, plen, rng, 10_000)
    check(keys, labels, addrs)
