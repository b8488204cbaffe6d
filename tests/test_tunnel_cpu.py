"""The ipcache tunnel endpoint, CPU side (cgpu_config.ipcache_tunnel).

The table compile is checked through the test hook cgpu_diag_ipc_tunnel, which
compiles the identity and tunnel tables as cgpu_commit does with the flag set
and walks them on the host as the kernels walk them.  Expectations are the
compiled reference's answers (tests/golden/ipcache_lpm.npz) and
Oracle.ipcache_lookup_addr (pinned to that fixture, tunnel included, by
tests/test_oracle_golden.py); every comparison is bit-exact.
"""
import ctypes as C
import errno

import numpy as np
import pytest

from cilium_amd import layouts as L
from cilium_amd._abi import CgpuConfig, lib
from cilium_amd.engine import Engine
from oracle import Oracle


def hook(name, argtypes):
    """a test hook of the library (exported, in no header): typed by its caller"""
    f = getattr(lib(), name)
    f.restype, f.argtypes = C.c_int, argtypes
    return f


VP = C.c_void_p
DIAG_ARGS = [VP, VP, VP, C.c_size_t, C.c_size_t, VP, C.c_size_t, C.c_int, VP, VP]


def diag(keys, vals, q, v6, n_first=None, delete=None):
    """cgpu_diag_ipc_tunnel -> ((m, 3) uint32 {found, sec_label, tunnel}, {builds, patched})."""
    keys = np.ascontiguousarray(keys, L.IPCACHE_KEY)
    vals = np.ascontiguousarray(vals, L.REMOTE_ENDPOINT_INFO)
    q = np.ascontiguousarray(q, np.uint8 if v6 else np.uint32)
    m = len(q)
    out = np.full((m, 3), 0xDEADBEEF, np.uint32)
    commits = np.zeros(2, np.uint64)
    dl = None if delete is None else np.ascontiguousarray(delete, np.uint8)
    rc = hook("cgpu_diag_ipc_tunnel", DIAG_ARGS)(keys.ctypes.data, vals.ctypes.data,
                                    None if dl is None else dl.ctypes.data, len(keys),
                                    len(keys) if n_first is None else n_first, q.ctypes.data, m,
                                    int(v6), out.ctypes.data, commits.ctypes.data)
    assert rc == 0, rc
    return out, commits


def oracle_rows(o, q):
    """(m, 3) {found, sec_label, tunnel} of Oracle.ipcache_lookup_addr."""
    r = np.zeros((len(q), 3), np.uint32)
    for i, a in enumerate(q):
        rc, val = o.ipcache_lookup_addr(bytes(a) if getattr(a, "ndim", 0) else int(a))
        if rc == 0:
            r[i] = (1,) + tuple(np.frombuffer(val, "<u4"))
    return r


@pytest.mark.parametrize("phase", ["a", "b"])
def test_compile_vs_reference_fixture(golden, phase):
    """ipcache_lpm.npz: found, sec_label and tunnel of every query address as
    the compiled reference answered, for the keys without (a) and with (b)
    the static-part entries."""
    g = golden("ipcache_lpm.npz")
    keys, vals = g["keys"], g["vals"]
    upto = len(keys) - int(g["n_static"]) if phase == "a" else len(keys)
    assert len(keys) == 707 and len(g["q4"]) == 4000 and len(g["q6"]) == 3000
    for v6, q, r in ((0, g["q4"], g["r4" + phase]), (1, g["q6"], g["r6" + phase])):
        r = np.asarray(r, np.uint32)
        # the fixture reaches what the tunnel adds: label-0 hits that carry a
        # tunnel, misses, non-zero tunnels
        tomb = (r[:, 0] == 1) & (r[:, 1] == 0) & (r[:, 2] != 0)
        assert tomb.sum() == (29 if v6 else 60)
        if phase == "a" and not v6:
            assert (r[:, 0] == 0).sum() >= 219  # (424 in the fixture as committed)
        assert (r[:, 2] >= 1 << 30).sum() > 100
        got, _ = diag(keys[:upto], vals[:upto], q, v6)
        assert np.array_equal(got, r)


def test_fixture_prefix_lengths(golden):
    """the fixture's keys run from the static part up to /32 and /128"""
    k = golden("ipcache_lpm.npz")["keys"]
    v4, v6 = k[k["family"] == 1]["prefixlen"], k[k["family"] == 2]["prefixlen"]
    assert k["prefixlen"].min() < 32 and v4.max() == 64 and v6.max() == 160


def _v4key(addr, plen):
    k = np.zeros((), L.IPCACHE_KEY)
    k["prefixlen"] = 32 + plen
    k["family"] = 1
    k["ip"][:4] = np.frombuffer(int(addr).to_bytes(4, "big"), np.uint8)
    return k


def _val(label, tunnel):
    v = np.zeros((), L.REMOTE_ENDPOINT_INFO)
    v["sec_label"], v["tunnel_endpoint"] = label, tunnel
    return v


def _be(addrs):
    """host-order addresses -> the network-order u32 column the lookups take"""
    return np.asarray(addrs, np.uint32).byteswap()


def test_shadow_case():
    """A tombstone shadows the /16's tunnel, a label's tunnel 0 stays 0, a
    label >= 2^30 keeps its tunnel, and a static-part key (prefixlen 0) ranks
    below every address prefix."""
    A, B, Cc, D = 0xC0A80001, 0xC0A80002, 0xF0000003, 0x0A0B0C0D
    ents = [(_v4key(0x0A010000, 16), _val(5, A)), (_v4key(0x0A010200, 24), _val(0, B)),
            (_v4key(0x0A010207, 32), _val(7, 0)), (_v4key(0x0A010309, 32), _val(0xC0000001, Cc))]
    k0 = np.zeros((), L.IPCACHE_KEY)  # prefixlen 0: matches every lookup key
    ents.append((k0, _val(9, D)))
    q = _be([0x0A010101, 0x0A010233, 0x0A010207, 0x0A010309, 0x0B000001])
    got, _ = diag([e[0] for e in ents], [e[1] for e in ents], q, 0)
    assert got.tolist() == [[1, 5, A], [1, 0, B], [1, 7, 0], [1, 0xC0000001, Cc], [1, 9, D]]
    o = Oracle()
    for k, v in ents:
        assert o.ipcache_update(k, v) == 0
    assert np.array_equal(got, oracle_rows(o, q))


def _rand_tables(rng, n32=6000):
    """6000 /32s in 40 /16s with distinct tunnels, /25../31 under /24s under a
    /16.  As cgpu_diag_ipc4_shapes reports it: all 41 /16s overflow to kind-3
    arrays (about 150 /32s each), below them byte-level run nodes of every kind
    and a few 256-leaf arrays.  No /16 is inline-able, so the leaf dictionary
    holds one code (the empty leaf): a full dictionary and run nodes directly
    under d16 are cascade_cases.lpm4_full_dict's."""
    ents, seen = [], set()
    tun = rng.permutation(np.arange(1 << 30, (1 << 30) + 4 * n32, dtype=np.uint32))
    p16 = rng.choice(np.arange(0x0B00, 0x0C00), 40, replace=False)
    while len(ents) < n32:
        a = (int(rng.choice(p16)) << 16) | int(rng.integers(0, 1 << 16))
        if a not in seen:
            seen.add(a)
            ents.append((_v4key(a, 32), _val(int(rng.integers(1, 1 << 31)), int(tun[len(ents)]))))
    ents.append((_v4key(0x0C010000, 16), _val(100, 0xAC100001)))
    for j in range(24):
        base = 0x0C010000 | (j << 8)
        ents.append((_v4key(base, 24), _val(200 + j, 0xAC100100 + j)))
        for plen in range(25, 32):
            a = base | (int(rng.integers(0, 256)) & (0xFF << (32 - plen)) & 0xFF)
            if (a, plen) not in seen:
                seen.add((a, plen))
                ents.append((_v4key(a, plen), _val(int(rng.integers(0, 3)) * 1000 + plen,
                                                   int(rng.integers(1, 1 << 32)))))
    qs = [a for a in list(seen)[:1500] if isinstance(a, int)]
    qs += [0x0C010000 | int(x) for x in rng.integers(0, 1 << 16, 1500)]
    qs += [(int(rng.choice(p16)) << 16) | int(x) for x in rng.integers(0, 1 << 16, 500)]
    return ents, _be(qs)


def test_shapes_beyond_the_fixture():
    rng = np.random.default_rng(11)
    ents, q = _rand_tables(rng)
    o = Oracle()
    for k, v in ents:
        assert o.ipcache_update(k, v) == 0
    o.set_fast(True)
    exp = oracle_rows(o, q)
    assert len(np.unique(exp[:, 2])) > 1200 and (exp[:, 0] == 0).sum() > 50
    got, _ = diag([e[0] for e in ents], [e[1] for e in ents], q, 0)
    assert np.array_equal(got, exp)


def Oracle_from(ents):
    o = Oracle()
    for k, v in ents:
        assert o.ipcache_update(k, v) == 0
    o.set_fast(True)
    return o


def test_patch_path_keeps_tunnels_current():
    """Second commits of one key go through the in-place patch (no IPv4 full
    build): a tunnel-only change with the label equal, a deleted covering /24,
    a new /28."""
    rng = np.random.default_rng(12)
    ents, q = _rand_tables(rng, n32=1500)
    base24 = 0x0C010300
    q = np.concatenate([q, _be([base24 | x for x in range(256)]), _be([0x0C010450 + x for x in range(16)])])
    state = {bytes(k.tobytes()): (k, v) for k, v in ents}
    k32, v32 = ents[7]  # one of the /32s: the tunnel changes, the label stays
    assert int(k32["prefixlen"]) == 64
    steps = [(k32, _val(int(v32["sec_label"]), 0xDEAD0001), 0),
             (_v4key(base24, 24), _val(0, 0), 1),
             (_v4key(0x0C010450, 28), _val(4242, 0xBEEF0002), 0)]
    for k, v, dele in steps:
        base = list(state.values())
        before = oracle_rows(Oracle_from(base), q)
        if dele:
            del state[bytes(k.tobytes())]
        else:
            state[bytes(k.tobytes())] = (k, v)
        exp = oracle_rows(Oracle_from(list(state.values())), q)
        assert not np.array_equal(before[:, 2], exp[:, 2])  # the step moves a probed tunnel
        got, commits = diag([e[0] for e in base] + [k], [e[1] for e in base] + [v], q, 0,
                            n_first=len(base), delete=[0] * len(base) + [dele])
        assert commits.tolist() == [1, 1]  # one full build, then one commit that patched
        assert np.array_equal(got, exp)


def _v6key(addr16, plen):
    k = np.zeros((), L.IPCACHE_KEY)
    k["prefixlen"] = 32 + plen
    k["family"] = 2
    k["ip"][:] = np.frombuffer(addr16, np.uint8)
    return k


def v6_tables(rng):
    """One /32 whose /33../64 prefixes carry different tunnels under ONE label
    (the label lines merge where the tunnel lines must not), one /64 with
    /65+ prefixes (h64 records), a tombstone and a static-part key."""
    def a(hi, lo=0):
        return int(hi).to_bytes(8, "big") + int(lo).to_bytes(8, "big")
    P = 0x20010DB8 << 32
    ents = [(_v6key(a(P), 32), _val(77, 0xAC100001))]
    for j, plen in enumerate(range(33, 65)):
        hi = P | (int(rng.integers(0, 1 << 32)) & (0xFFFFFFFF << (64 - plen)) & 0xFFFFFFFF)
        ents.append((_v6key(a(hi), plen), _val(77, 0xAC110000 + j)))
    Q = (0x20010DB9 << 32) | 0x00010002
    ents.append((_v6key(a(Q), 64), _val(88, 0xAC120001)))
    for j, plen in enumerate((65, 72, 96, 120, 128)):
        lo = int(rng.integers(0, 1 << 63)) & ((1 << 64) - (1 << (128 - plen)))
        ents.append((_v6key(a(Q, lo), plen), _val(88 + (j & 1), 0xAC130000 + j)))
    ents.append((_v6key(a(0x20010DBA << 32), 32), _val(0, 0xAC140001)))  # tombstone
    k0 = np.zeros((), L.IPCACHE_KEY)
    k0["prefixlen"] = 31  # static part {pad, family 2} minus its last bit: family 2 or 3
    k0["family"] = 2
    ents.append((k0, _val(9, 0xAC150001)))
    qs = []
    for k, _ in ents:
        b = bytearray(bytes(k["ip"]))
        qs.append(bytes(b))
        for _ in range(6):
            c = bytearray(b)
            i = int(rng.integers(4, 16))
            c[i] ^= 1 << int(rng.integers(0, 8))
            qs.append(bytes(c))
    qs += [a(P | int(x)) for x in rng.integers(0, 1 << 32, 300)]
    qs += [a(Q, int(x)) for x in rng.integers(0, 1 << 63, 200)]
    qs += [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(50)]
    return ents, np.frombuffer(b"".join(qs), np.uint8).reshape(-1, 16).copy()


def test_v6_labels_merge_where_tunnels_differ():
    rng = np.random.default_rng(13)
    ents, q = v6_tables(rng)
    o = Oracle_from(ents)
    exp = oracle_rows(o, q)
    in32 = exp[:, 1] == 77
    assert in32.sum() > 200 and len(np.unique(exp[in32, 2])) > 10
    assert ((exp[:, 1] == 0) & (exp[:, 0] == 1) & (exp[:, 2] == 0xAC140001)).any()
    assert (exp[:, 2] == 0xAC150001).any() and np.isin(exp[:, 2], 0xAC130000 + np.arange(5)).any()
    got, _ = diag([e[0] for e in ents], [e[1] for e in ents], q, 1)
    assert np.array_equal(got, exp)


def test_config_default_and_host_only_context():
    cfg = CgpuConfig()
    lib().cgpu_config_default(C.byref(cfg))
    assert cfg.ipcache_tunnel == 0 and C.sizeof(CgpuConfig) == 128  # the struct size stays
    e = Engine(device=-1, ipcache_tunnel=1)
    try:
        k, v = _v4key(0x0A000001, 32), _val(5, 0xC0A80063)
        assert e.ipcache_update(k, v) == 0
        rc, got = e.ipcache_lookup(k)
        assert rc == 0 and int(got["tunnel_endpoint"]) == 0xC0A80063  # the mirror keeps it
        buf = (C.c_uint32 * 4)()
        p = C.cast(buf, C.c_void_p)
        for fn in ("cgpu_ipcache_lookup_v4", "cgpu_ipcache_lookup_v6"):
            assert getattr(e.L, fn)(e.h, p, 1, None, p, p, None) == -errno.ENODEV
            assert getattr(e.L, fn)(e.h, p, 1, None, p, None, None) == -errno.ENODEV
        from cilium_amd._abi import TuplesV4, TuplesV4Ct, TuplesV6, TuplesV6Ct
        for fn, tv in (("cgpu_classify_v4_tun", TuplesV4()), ("cgpu_classify_v6_tun", TuplesV6())):
            assert getattr(e.L, fn)(e.h, C.byref(tv), None, None, 0, 1, p, p, None, p, None) == -errno.ENODEV
        for fn, tv in (("cgpu_classify_v4_ct_tun", TuplesV4Ct()), ("cgpu_classify_v6_ct_tun", TuplesV6Ct())):
            assert getattr(e.L, fn)(e.h, C.byref(tv), 1, 0, p, p, p, None, p, None) == -errno.ENODEV
        assert b"host-only" in e.L.cgpu_last_error()
    finally:
        e.close()
