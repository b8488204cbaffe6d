"""Tables and probe addresses for the IPv6 ipcache trie (tables.h v6_lpm),
shared by the CPU walk test (test_v6_trie.py) and the device walks
(test_gpu_v6_trie.py).  Plain numpy; nothing here asks the library anything.

Three tables, each with the addresses to look up:

* narrow: edge_table() as it is -- one /16 root, so the b24 level is a single
  block (staged in LDS by the x4 walk); the binary-searched long node,
  windows, /64 lists, an inline /65+ record, tombstones, static-part keys.
* wide: narrow plus 128 further /16 roots, each with a chain of nested
  prefixes under one base address: more b24 blocks than the x4 walk stages,
  so that walk gathers b24 from global memory, ending in a b24 leaf, a b24
  GROUP, a b32 leaf, a node and a deep node with records.
* sparse: no ::/0 and no static-part key, so lookups can match nothing; 3200
  /64s with /65+ prefixes (shared h64 home slots: hop rounds); a /32 whose
  longer prefixes sit in one /56 (addresses far from it take the window's
  outer label); random nested prefixes; labels >= 2^30 and tombstones.

Expected answers come from the restatement (restate()), never from the library.
"""
import functools
from dataclasses import dataclass

import numpy as np

from cilium_amd import layouts as L, synth

WIDE_ROOTS = 128
WIDE_LENS = np.array([20, 24, 28, 32, 40, 64, 96, 128])
SPARSE_N64 = 3200
# the /32 of the sparse table whose longer prefixes all lie in one /56
OUT32 = np.array([0x26, 0x07, 0xF8, 0xB0], np.uint8)
OUT56 = np.array([0x5A, 0x5A, 0x5A], np.uint8)  # address bits 32..55


def keys_of(addr, plen, static=False):
    k = np.zeros(len(plen), L.IPCACHE_KEY)
    k["family"] = L.ENDPOINT_KEY_IPV6
    k["prefixlen"] = np.asarray(plen) + (0 if static else L.IPCACHE_STATIC_PREFIX)
    k["ip"] = addr
    return k


def probes(addr, plen, rng, n_rand):
    """Every prefix's first and last address and their outside neighbours,
    random addresses inside prefixes and under their /16s."""
    a = np.asarray(addr, np.uint8)
    m = synth.MASK6[np.asarray(plen)]
    lo, hi = a & m, (a & m) | ~m
    out = [lo, hi]
    M = (1 << 128) - 1
    for x, d in ((lo, -1), (hi, 1)):
        v = [((int.from_bytes(r.tobytes(), "big") + d) & M).to_bytes(16, "big") for r in x]
        out.append(np.frombuffer(b"".join(v), np.uint8).reshape(-1, 16))
    pi = rng.integers(0, len(a), n_rand)
    r = rng.integers(0, 256, (n_rand, 16), dtype=np.uint8)
    out.append((a[pi] & m[pi]) | (r & ~m[pi]))
    r2 = rng.integers(0, 256, (n_rand, 16), dtype=np.uint8)
    r2[:, :2] = a[pi, :2]
    out.append(r2)
    return np.concatenate(out)


def edge_table():
    rng = np.random.Generator(np.random.PCG64(62))
    addr, plen, lab = [], [], []

    def put(a, n, lb):
        a = np.array(a, np.uint8)
        addr.append(a & synth.MASK6[n])
        plen.append(n)
        lab.append(lb)
    base = np.zeros(16, np.uint8)
    # a /32 too dense for 64 sub-range lines: 1500 /64s (3000 boundaries)
    d = base.copy()
    d[:4] = [0x20, 0x01, 0x0d, 0xb8]
    put(d, 32, 1001)
    for i in range(1500):
        x = d.copy()
        x[4:8] = rng.integers(0, 256, 4, dtype=np.uint8)
        put(x, 64, 2000 + i)
    # boundaries at both ends of a /32, nested inside a /24 and a /20
    e = base.copy()
    e[:4] = [0x20, 0x01, 0x0e, 0x77]
    put(e, 20, 1101)
    put(e, 24, 1102)
    lo = e.copy()
    put(lo, 48, 1103)
    hi = e.copy()
    hi[4:8] = 0xFF
    put(hi, 64, 1104)
    mid = e.copy()
    mid[4:6] = [0x80, 0x00]
    put(mid, 33, 1105)
    put(mid, 40, 1106)
    # /64s with nested and disjoint /65+ prefixes (lists) and one inline
    for j in range(40):
        s = base.copy()
        s[:8] = [0x20, 0x01, 0x0f, 0x00, 0x00, j, 0x12, 0x34]
        put(s, 64, 3000 + j)
        t = s.copy()
        t[8:] = rng.integers(0, 256, 8, dtype=np.uint8)
        put(t, 96, 3100 + j)
        put(t, 112, 3200 + j)
        put(t, 128, 3300 + j)
        if j % 2:
            u = s.copy()
            u[8:] = rng.integers(0, 256, 8, dtype=np.uint8)
            put(u, 128, 3400 + j)
            put(u, 65, 3500 + j)
        if j % 5 == 0:
            v = s.copy()
            v[8:] = 0xFF
            put(v, 128, 3600 + j)  # ends at the /64's last address
    inl = base.copy()
    inl[:8] = [0x20, 0x01, 0x0f, 0x01, 0, 0, 0, 1]
    put(inl, 100, 3700)  # a /64 whose only /65+ prefix is inline
    # /65+ only under a /32 (no /33../64): a deep node of one line
    o = base.copy()
    o[:4] = [0x20, 0x01, 0x0f, 0x02]
    o[8:] = rng.integers(0, 256, 8, dtype=np.uint8)
    put(o, 128, 3800)
    # /17../32 expansion around a /48, tombstones
    f = base.copy()
    f[:6] = [0x20, 0x01, 0x0a, 0x0b, 0x0c, 0x0d]
    put(f, 17, 4001)
    put(f, 23, 4002)
    put(f, 29, 0)  # tombstone (sec_label 0: a match that shadows)
    put(f, 31, 4004)
    put(f, 48, 4005)
    put(f, 56, 0)
    # ::/0 and two static-part entries (rank below /0)
    put(base, 0, 2)
    keys = keys_of(np.array(addr), plen)
    st_keys = np.zeros(2, L.IPCACHE_KEY)
    st_keys["family"] = L.ENDPOINT_KEY_IPV6
    st_keys["prefixlen"] = [0, 31]
    return (np.concatenate([keys, st_keys]), np.array(lab + [7, 8], np.uint32),
            np.array(addr), np.array(plen), rng)


def mix32(a, b):
    """tables.h mix32 over uint32 arrays."""
    with np.errstate(over="ignore"):
        h = (np.asarray(b, np.uint64) << np.uint64(32) | np.asarray(a, np.uint64)) * np.uint64(0x9E3779B97F4A7C15)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
    return h.astype(np.uint32)


def words64(addr):
    """(w0, w1): address bits 0..31 and 32..63 as host-order words."""
    a = np.ascontiguousarray(np.asarray(addr, np.uint8)[:, :8])
    w = a.view(">u4").astype(np.uint32)
    return w[:, 0], w[:, 1]


@dataclass
class Case:
    name: str
    keys: np.ndarray     # IPCACHE_KEY
    vals: np.ndarray     # REMOTE_ENDPOINT_INFO, a distinct tunnel word per key
    addrs: np.ndarray    # (m, 16) uint8 probe addresses, m % 4 != 0, m <= 40000
    pfx_addr: np.ndarray  # the address-part prefixes (masked) ...
    pfx_len: np.ndarray   # ... and their lengths

    @property
    def labels(self):
        return np.ascontiguousarray(self.vals["sec_label"])

    def h64_keys(self):
        """The distinct /64s that hold a prefix longer than /64 (one h64
        record each), as (w0, w1)."""
        deep = self.pfx_addr[self.pfx_len > 64]
        w0, w1 = words64(deep)
        u = np.unique(w0.astype(np.uint64) << np.uint64(32) | w1.astype(np.uint64))
        return (u >> np.uint64(32)).astype(np.uint32), u.astype(np.uint32)

    def outside(self):
        """Probes of OUT32 farther than 2^10 from its one /56 in bits 32..63:
        outside every window the builder can choose for that /32 (all its
        boundaries lie in the /56, 2^8 wide: w is 9 or 10)."""
        w0, w1 = words64(self.addrs)
        x = int.from_bytes(bytes(OUT56) + b"\0", "big")
        return (w0 == int.from_bytes(bytes(OUT32), "big")) & ((w1 >> 10) != (x >> 10))


def _case(name, keys, labels, addr, plen, addrs):
    vals = np.zeros(len(keys), L.REMOTE_ENDPOINT_INFO)
    vals["sec_label"] = labels
    vals["tunnel_endpoint"] = 0x0A000000 + 1 + np.arange(len(keys))
    addrs = np.ascontiguousarray(addrs[:40_000])
    if len(addrs) % 4 == 0:
        addrs = addrs[:-1]
    return Case(name, keys, vals, addrs, np.asarray(addr, np.uint8), np.asarray(plen))


@functools.lru_cache(None)
def narrow():
    keys, labels, addr, plen, rng = edge_table()
    return _case("narrow", keys, labels, addr, plen, probes(addr, plen, rng, 8000))


@functools.lru_cache(None)
def wide():
    keys, labels, addr, plen, _ = edge_table()
    rng = np.random.Generator(np.random.PCG64(63))
    roots = rng.choice(np.setdiff1d(np.arange(0x3000, 0xF000), [0x2001]), WIDE_ROOTS, replace=False)
    xa, xl, xlab = [], [], []
    for i, r in enumerate(roots):
        base = rng.integers(0, 256, 16, dtype=np.uint8)
        base[:2] = [r >> 8, r & 0xFF]
        lens = np.sort(rng.choice(WIDE_LENS, int(rng.integers(3, len(WIDE_LENS) + 1)), replace=False))
        for n in lens:
            xa.append(base & synth.MASK6[n])
            xl.append(int(n))
            # every 16th label indirect (>= 2^30), every 23rd a tombstone
            k = len(xl)
            xlab.append(0 if k % 23 == 0 else (0x40000000 + k if k % 16 == 0 else 10_000 + k))
    addr = np.concatenate([addr, np.array(xa)])
    plen = np.concatenate([plen, np.array(xl)])
    keys = np.concatenate([keys[:-2], keys_of(np.array(xa), xl), keys[-2:]])
    labels = np.concatenate([labels[:-2], np.array(xlab, np.uint32), labels[-2:]])
    return _case("wide", keys, labels, addr, plen, probes(addr, plen, rng, 6000))


@functools.lru_cache(None)
def sparse():
    rng = np.random.Generator(np.random.PCG64(64))
    addr, plen, lab = [], [], []

    def put(a, n, lb):
        addr.append(np.asarray(a, np.uint8) & synth.MASK6[n])
        plen.append(int(n))
        lab.append(int(lb))

    def label(i):
        r = rng.random()
        return 0 if r < 0.03 else (0x40000000 + 7 * i if r < 0.10 else 5000 + i)
    # 3200 /64s with /65+ prefixes under 8 /32s (4 /16 roots); every other
    # /32 has a /32 prefix of its own, a quarter of the /64s a /64 prefix
    r32 = rng.integers(0, 256, (8, 4), dtype=np.uint8)
    r32[:, 0] = 0x2A
    r32[:, 1] = np.arange(8) // 2
    for j in range(0, 8, 2):
        put(np.concatenate([r32[j], np.zeros(12, np.uint8)]), 32, 4000 + j)
    deep_lens = np.array([65, 72, 80, 96, 112, 120, 127, 128])
    for i in range(SPARSE_N64):
        a = rng.integers(0, 256, 16, dtype=np.uint8)
        a[:4] = r32[rng.integers(0, 8)]
        if i % 4 == 0:
            put(a, 64, label(i))
        k = int(rng.integers(1, 4))
        ls = np.sort(rng.choice(deep_lens, k, replace=False))
        nest = rng.random() < 0.5  # nested under the first, or elsewhere in the /64
        for q, n in enumerate(ls):
            b = a.copy()
            if q and not nest:
                b[8:] = rng.integers(0, 256, 8, dtype=np.uint8)
            put(b, n, label(3 * i + q))
    # a /32 whose longer prefixes all lie in one /56
    o = np.zeros(16, np.uint8)
    o[:4] = OUT32
    put(o, 32, 4100)
    o[4:7] = OUT56
    put(o, 56, 4101)
    for q, (b7, n) in enumerate([(0x00, 60), (0x10, 62), (0x20, 64), (0x21, 64), (0x80, 64), (0xFF, 64)]):
        x = o.copy()
        x[7] = b7
        put(x, n, 4110 + q)
    for q, b7 in enumerate([0x21, 0x42]):
        x = o.copy()
        x[7] = b7
        x[8:] = rng.integers(0, 256, 8, dtype=np.uint8)
        put(x, 96, 4120 + q)
        put(x, 128, 0x40000100 + q)
    # random nested prefix sets (as test_trie_random_nested), lengths /17 up
    roots = np.array([[0x2B, 0x10], [0x2B, 0x11], [0x2C, 0x00], [0x2C, 0xFF]], np.uint8)
    n = 1500
    a = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    a[:, :2] = roots[rng.integers(0, 4, n)]
    stem = a[rng.integers(0, 64, n)]
    keep = rng.integers(2, 14, n)
    for i in range(n // 2):
        a[i, :keep[i]] = stem[i, :keep[i]]
    pl = rng.integers(17, 129, n)
    rl = rng.integers(1, 1 << 31, n)
    for i in range(n):
        put(a[i], pl[i], rl[i])
    addr, plen, lab = np.array(addr), np.array(plen), np.array(lab, np.uint32)
    canon = np.zeros(len(plen), np.dtype([("l", "u4"), ("a", "u1", (16,))]))
    canon["l"], canon["a"] = plen, addr
    _, first = np.unique(canon.view(np.dtype((np.void, 20))), return_index=True)
    first = np.sort(first)
    addr, plen, lab = addr[first], plen[first], lab[first]
    far = rng.integers(0, 256, (300, 16), dtype=np.uint8)  # in OUT32, far from its /56
    far[:, :4] = OUT32
    pr = probes(addr, plen, rng, 2500)
    return _case("sparse", keys_of(addr, plen), lab, addr, plen, np.concatenate([far, pr]))


CASES = {"narrow": narrow, "wide": wide, "sparse": sparse}


def load_ipcache(target, case):
    """The case's ipcache into an Engine or an Oracle."""
    for k, v in zip(case.keys, case.vals):
        assert target.ipcache_update(k, v) == 0


def restate(case, addrs=None):
    """(m, 3) uint32 {found, sec_label, tunnel} of the restatement's ipcache
    lookup (its kernel-like trie) of every probe address."""
    from oracle import Oracle
    o = Oracle()
    load_ipcache(o, case)
    addrs = case.addrs if addrs is None else addrs
    r = np.zeros((len(addrs), 3), np.uint32)
    for i, a in enumerate(addrs):
        rc, val = o.ipcache_lookup_addr(bytes(a))
        if rc == 0:
            r[i] = (1,) + tuple(np.frombuffer(val, "<u4"))
    o.close()
    return r
