"""The gather stages of the IPv4 x4 classify kernel (k_classify_x4, plain
tuple columns): each stage issues the loads of a lane's four tuples together,
a tuple that skips a stage loading a fixed in-range slot, and the hop slots of
the policy and group tables are resolved in quad-wide rounds.  Every check is
bit-exact against the restatement: verdict, identity and stage of every tuple,
every per-entry counter through policy_lookup, and metrics().

Only the plain IPv4 instantiation has these stages; the service (LB / XDP),
IPv6, frames and tunnel instantiations keep the per-tuple form and are
covered by their own files."""
import numpy as np
import pytest

from cascade_cases import key_hi as _key_hi, lpm_shapes as _lpm_shapes, pg_bloom as _pg_bloom, pol_hash as _pol_hash
from cilium_amd import build, layouts as L, synth

pytestmark = pytest.mark.gpu

NO_CCACHE = 4  # CGPU_SCHED_NO_CCACHE


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a device"
    build.build()
    return torch


def _engine(**kw):
    from cilium_amd.engine import Engine
    return Engine(device=0, **kw)


def _gpu_matches(torch, e, t, exp, o, keys, eps):
    """classify t on e; exp = the restatement's (verdict, identity, stage) and
    o the restatement that produced them (its counters and metrics)."""
    out = e.classify_v4(synth.to_device(t))
    torch.cuda.synchronize()
    v0, i0, s0 = exp
    np.testing.assert_array_equal(out["verdict"].cpu().numpy(), v0)
    np.testing.assert_array_equal(out["identity"].cpu().numpy().view(np.uint32), i0)
    np.testing.assert_array_equal(out["stage"].cpu().numpy(), s0)
    for k, ep in zip(keys, eps):
        rc, got = e.policy_lookup(int(ep), k)
        rc0, raw = o.policy_lookup(int(ep), k)
        want = np.frombuffer(raw, L.POLICY_ENTRY)[0]
        assert rc == 0 and rc0 == 0
        assert (int(got["packets"]), int(got["bytes"])) == (int(want["packets"]), int(want["bytes"]))
    np.testing.assert_array_equal(e.metrics(), o.metrics())


# --------------------------------------------------------------------------
# several loop iterations of the resident grid
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loops_case(torch_cuda):
    """Config "cpu" tables and n = 2 * CUs * 4096 + 3 * 4096 + 1 tuples: one
    pass of the resident grid (one workgroup of 1024 lanes x 4 tuples per CU)
    is CUs * 4096 tuples, so workgroups run 2 and 3 iterations of the loop,
    the last pass is partial and the last quad ragged."""
    from oracle import Oracle
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    n = 2 * cus * 4096 + 3 * 4096 + 1
    T = synth.make_tables(**synth.CONFIGS["cpu"])
    t = synth.make_tuples(T, n)
    o = Oracle(**T.oracle_config())
    synth.load_oracle(o, T)
    v, idt, st, _ = o.classify_v4(t, nthreads=8)
    return T, t, o, (v, idt, st)


@pytest.mark.parametrize("sched", [0, NO_CCACHE])
def test_several_loop_iterations(torch_cuda, loops_case, sched):
    T, t, o, exp = loops_case
    assert len(t["saddr"]) % 4 == 1
    e = _engine(**T.engine_config(), schedule=sched)
    synth.load_engine(e, T)
    e.commit()
    _gpu_matches(torch_cuda, e, t, exp, o, T.pol_keys, T.pol_ep)
    e.close()


# --------------------------------------------------------------------------
# hop neighbourhoods of the policy table
# --------------------------------------------------------------------------
POL_SLOTS = 1 << 16  # the table the key set below is laid out for (asserted)


def _hop_keys(rng):
    """One endpoint's keys: > 4096 exact keys chosen, with the mirror of
    pol_hash, so that home slots are shared by 2, 3 and 4 keys; identity-0
    (wildcard) keys; L3-only keys.  Returns the exact keys (id, dport_be,
    proto, egress), the absent candidates left at occupied home slots, the
    wildcard and the L3 keys."""
    ids = np.arange(300, 348, dtype=np.uint32)
    m = 300_000
    cand = np.stack([rng.choice(ids, m), rng.integers(1, 65536, m).astype(np.uint32),
                     rng.choice(np.array([6, 17], np.uint32), m),
                     rng.integers(0, 2, m).astype(np.uint32)], 1)
    cand = np.unique(cand, axis=0)
    rng.shuffle(cand)
    home = _pol_hash(cand[:, 0], _key_hi(cand[:, 1], cand[:, 2], cand[:, 3]), 0) & np.uint32(POL_SLOTS - 1)
    order = np.argsort(home, kind="stable")
    cand, home = cand[order], home[order]
    first = np.flatnonzero(np.r_[True, home[1:] != home[:-1]])
    count = np.diff(np.r_[first, len(home)])
    take = np.zeros(len(cand), bool)
    absent = np.zeros(len(cand), bool)
    # (keys taken of a home, homes of that kind); a home gives one key more
    # than it installs, so that an absent key shares it
    plan = [(4, 24), (3, 150), (2, 400), (1, 2900)]
    slots = list(rng.permutation(len(first)))
    for k, homes in plan:
        got = 0
        while got < homes:
            j = slots.pop()
            if count[j] < k + 1:
                continue
            take[first[j]:first[j] + k] = True
            absent[first[j] + k] = True
            got += 1
    exact = cand[take]
    assert len(exact) > 4096
    wild = np.array([(0, L.htons(int(p)), pr, d) for p in synth.PORTS64[:40] for pr in (6, 17) for d in (0, 1)],
                    np.uint32)
    l3 = np.array([(i, 0, 0, d) for i in ids[::2] for d in (0, 1)], np.uint32)
    return ids, exact, cand[absent], wild, l3


def test_hop_neighbourhoods(torch_cuda):
    """Tuples that hit every installed key (probe 1, probe 2 and probe 3
    hits), absent keys whose home slot carries hop bits, fragments (no probe
    1 or 3) and lengths >= 2048 (the two-word counter path), in quads that
    hold 0, 1 and >= 2 tuples with hop loads of different numbers of rounds.

    What the mirror can say about a probe-1 lookup without mirroring the
    table's placement of keys: a home slot shared by m installed keys has m
    hop bits, at most one of them bit 0.  An absent key reads every slot but
    the home itself: m - 1 or m hop rounds.  An installed key reads at most
    m - 1.  The probe runs when the tuple is no fragment and the bloom of its
    {identity, direction} group admits its (dport, proto)."""
    from oracle import Oracle
    rng = np.random.default_rng(11)
    ids, exact, absent, wild, l3 = _hop_keys(rng)
    keys_all = np.concatenate([exact, wild, l3])
    pk = np.zeros(len(keys_all), L.POLICY_KEY)
    pk["sec_label"], pk["dport"], pk["protocol"], pk["egress"] = keys_all.T
    pe = np.zeros(len(pk), L.POLICY_ENTRY)
    pe["proxy_port"] = np.where(rng.random(len(pk)) < 0.1, rng.integers(10000, 20000, len(pk)), 0).astype(
        np.uint16).byteswap()
    cidrs = [("0.0.0.0/0", L.WORLD_ID)] + [(f"30.0.{i}.0/24", int(v)) for i, v in enumerate(ids)]
    e = _engine(policy_max_total=1 << 14, max_endpoints=4)
    o = Oracle()
    for c, v in cidrs:
        k, val = L.ipcache_key(c), L.remote_info(v, 0)
        assert e.ipcache_update(k, val) == 0 and o.ipcache_update(k, val) == 0
    assert e.policy_update_batch(np.zeros(len(pk), np.uint32), pk, pe) == 0
    for k, en in zip(pk, pe):
        assert o.policy_update(0, k, en) == 0
    e.commit()
    # the policy group's bytes: the key table and the {identity, direction}
    # group table, a smaller power of two (98 groups) -- the mask of the key
    # table is the larger one's
    slots = e.table_bytes()["policy"] // 16
    assert slots - POL_SLOTS > 0 and slots - POL_SLOTS < POL_SLOTS and \
        (slots - POL_SLOTS) & (slots - POL_SLOTS - 1) == 0
    mask = np.uint32(POL_SLOTS - 1)

    def home_of(k):
        return _pol_hash(k[:, 0], _key_hi(k[:, 1], k[:, 2], k[:, 3]), 0) & mask

    share = np.bincount(home_of(keys_all), minlength=POL_SLOTS)
    assert (share == 2).any() and (share == 3).any() and (share >= 4).any()

    # the tuple stream: (id, dport_be, proto, egress) rows
    n = 1 << 18
    nx = len(exact)
    rows = np.concatenate([
        exact[rng.integers(0, nx, n // 2)],                       # probe-1 hits
        absent[rng.integers(0, len(absent), n // 8)],             # absent, home with hop bits
        np.stack([rng.choice(ids[1::2], n // 8), wild[rng.integers(0, len(wild), n // 8), 1],
                  wild[rng.integers(0, len(wild), n // 8), 2],
                  rng.integers(0, 2, n // 8).astype(np.uint32)], 1),  # probe 3 (no L3 key)
        np.stack([rng.choice(ids[::2], n // 8), rng.integers(1, 65536, n // 8).astype(np.uint32),
                  np.full(n // 8, 6, np.uint32), rng.integers(0, 2, n // 8).astype(np.uint32)], 1),  # probe 2
        np.stack([rng.choice(ids, n // 8), rng.integers(1, 65536, n // 8).astype(np.uint32),
                  rng.choice(np.array([6, 17], np.uint32), n // 8),
                  rng.integers(0, 2, n // 8).astype(np.uint32)], 1)])
    rng.shuffle(rows)
    frag = (rng.random(n) < 0.1) & (rows[:, 3] == 0)
    # planted quads (below): two absent keys of homes shared by 2 and by >= 4
    # keys, and ingress fragments around them
    am = share[home_of(absent)]
    bl_grp = {}
    for (i, dp, pr, d), b in zip(keys_all, _pg_bloom(keys_all[:, 1], keys_all[:, 2])):
        bl_grp[(int(i), int(d))] = bl_grp.get((int(i), int(d)), 0) | int(b)

    def admitted(k):
        b = _pg_bloom(k[:, 1], k[:, 2])
        g = np.array([bl_grp.get((int(i), int(d)), 0) for i, d in zip(k[:, 0], k[:, 3])], np.uint32)
        return (g & b) == b

    adm = admitted(absent)
    a2 = absent[(am == 2) & adm][0]
    a4 = absent[(am >= 4) & adm][0]
    fr = np.array([ids[0], L.htons(80), 6, 0], np.uint32)
    rows[0:4] = fr                      # no tuple with hop loads
    frag[0:4] = True
    rows[4:8] = [a2, fr, fr, fr]        # one
    frag[4:8] = [False, True, True, True]
    rows[8:12] = [a2, a4, fr, fr]       # two, of different rounds
    frag[8:12] = [False, False, True, True]

    idx = np.searchsorted(ids, rows[:, 0])
    addr = ((30 << 24) | (idx.astype(np.uint32) << np.uint32(8)) |
            rng.integers(0, 256, n).astype(np.uint32)).astype(np.uint32).byteswap()
    other = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    eg = rows[:, 3] == 1
    ln = rng.integers(64, 1501, n).astype(np.uint32)
    ln[rng.random(n) < 0.001] = 2048 + 7
    ln[13] = 9000
    t = {"saddr": np.where(eg, other, addr), "daddr": np.where(eg, addr, other),
         "dport": rows[:, 1].astype(np.uint16), "proto": rows[:, 2].astype(np.uint8),
         "flags": (rows[:, 3] | (frag.astype(np.uint32) << 1)).astype(np.uint8), "len": ln,
         "ep": np.zeros(n, np.uint16)}

    # bounds on the probe-1 hop rounds of every tuple
    installed = {tuple(int(x) for x in k) for k in keys_all}
    m_of = share[home_of(rows)]
    inst = np.array([tuple(int(x) for x in r) in installed for r in rows])
    runs = admitted(rows) & ~frag
    lo = np.where(runs, np.where(inst, 0, np.maximum(m_of - 1, 0)), 0)
    hi = np.where(runs, np.where(inst, np.maximum(m_of - 1, 0), m_of), 0)
    q_lo, q_hi = lo[:n - n % 4].reshape(-1, 4), hi[:n - n % 4].reshape(-1, 4)
    sure, none = q_lo >= 1, q_hi == 0
    assert (none.sum(1) == 4).any()
    assert ((sure.sum(1) == 1) & (none.sum(1) == 3)).any()
    two = np.flatnonzero(sure.sum(1) >= 2)
    assert any(q_hi[q][sure[q]].min() < q_lo[q][sure[q]].max() for q in two), \
        "a quad whose tuples need different numbers of hop rounds"
    assert (ln >= 2048).sum() > 10 and frag.sum() > 1000

    v0, i0, s0, _ = o.classify_v4(t, nthreads=8)
    assert all((s0 == k).sum() > 1000 for k in (0, 1, 2, 3))
    _gpu_matches(torch_cuda, e, t, (v0, i0, s0), o, pk, np.zeros(len(pk), np.uint32))
    e.close()


# --------------------------------------------------------------------------
# inactive lanes at every stage
# --------------------------------------------------------------------------
@pytest.mark.parametrize("tables", ["both", "empty_policy", "ipcache_default_only"])
def test_inactive_lanes(torch_cuda, tables):
    """n = 4099 tuples whose quads mix gated protocols (ct_proto_gate),
    ingress and egress, fragments, addresses without an ipcache match, and
    tuples that stop at probe 1, probe 2, probe 3 and DROP_POLICY: the
    branch-free loads see every mask.  Also against an engine with an empty
    policy map and one whose ipcache holds only 0.0.0.0/0."""
    from oracle import Oracle
    rng = np.random.default_rng(5)
    n = 4099
    ids = [400, 401, 402, (1 << 30) + 5, L.WORLD_ID]
    cidrs = [] if tables == "ipcache_default_only" else \
        [(f"40.{i}.0.0/16", v) for i, v in enumerate(ids[:4])] + [("40.9.1.0/24", 401), ("40.9.2.128/25", 402)]
    cidrs += [("0.0.0.0/0", L.WORLD_ID)] if tables != "both" else []
    pol = []
    if tables != "empty_policy":
        for i in ids:
            pol += [L.policy_key(i, 80, 6, d) for d in (0, 1)]           # probe 1
        pol += [L.policy_key(401, 0, 0, 0), L.policy_key(401, 0, 0, 1), L.policy_key(L.WORLD_ID, 0, 0, 0)]  # probe 2
        pol += [L.policy_key(0, p, pr, d) for p, pr in ((53, 17), (443, 6)) for d in (0, 1)]  # probe 3
    e = _engine(policy_max_total=1 << 12, max_endpoints=4, ct_proto_gate=1)
    o = Oracle(ct_proto_gate=1)
    for c, v in cidrs:
        k, val = L.ipcache_key(c), L.remote_info(v, 0)
        assert e.ipcache_update(k, val) == 0 and o.ipcache_update(k, val) == 0
    for i, k in enumerate(pol):
        en = L.policy_entry(15000 if i % 5 == 0 else 0)
        assert e.policy_update(0, k, en) == 0 and o.policy_update(0, k, en) == 0
    e.commit()
    hi = rng.choice(np.array([0x2800, 0x2801, 0x2802, 0x2803, 0x2809, 0x0A07, 0x5000], np.uint32), n)
    addr = ((hi << np.uint32(16)) | rng.choice(np.array([0x0101, 0x0180, 0x02FF, 0x0280, 0x7777], np.uint32), n)
            ).astype(np.uint32).byteswap()
    eg = rng.random(n) < 0.5
    t = {"saddr": addr, "daddr": addr[::-1].copy(),
         "dport": np.array([L.htons(int(p)) for p in rng.choice([80, 53, 443, 8080], n)], np.uint16),
         "proto": rng.choice(np.array([1, 6, 17, 47, 132], np.uint8), n, p=[0.1, 0.4, 0.3, 0.1, 0.1]),
         "flags": (eg | (((rng.random(n) < 0.1) & ~eg) << 1)).astype(np.uint8),
         "len": rng.choice(np.array([64, 1500, 2047, 2048, 65535], np.uint32), n),
         "ep": np.zeros(n, np.uint16)}
    v0, i0, s0, _ = o.classify_v4(t, nthreads=4)
    seen = set(np.unique(s0).tolist())
    assert {0, 4} <= seen and (tables == "empty_policy" or {1, 2, 3} <= seen), seen
    q = s0[:n - n % 4].reshape(-1, 4)
    assert ((q == 4).any(1) & (q != 4).any(1)).any(), "gated and classified tuples in one quad"
    _gpu_matches(torch_cuda, e, t, (v0, i0, s0), o, pol, np.zeros(len(pol), np.uint32))
    e.close()


# --------------------------------------------------------------------------
# every shape of the compressed ipcache table
# --------------------------------------------------------------------------
def test_lpm_shapes_in_quads(torch_cuda):
    """Addresses drawn per tuple over the /16s of every shape, so that the
    four tuples of a quad take different paths through the table: inline
    /16s, 16/32/64-byte nodes (the 64-byte node's far leaves too), both array
    levels, and labels >= 2^30."""
    from oracle import Oracle
    rng = np.random.default_rng(7)
    n = 1 << 18
    hi = rng.choice(np.array([0x1401, 0x1402, 0x1403, 0x1404, 0x1405, 0x1406, 0x1407, 0x1408,
                              0x1409, 0x140A, 0x0A07, 0x0B00], np.uint32), n)
    lo = rng.integers(0, 1 << 16, n, dtype=np.uint32)
    lo = np.where(rng.random(n) < 0.2,
                  rng.choice(np.array([0, 1, 255, 256, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF], np.uint32), n), lo)
    addr = ((hi << np.uint32(16)) | lo).astype(np.uint32).byteswap()
    t = {"saddr": addr, "daddr": addr[::-1].copy(),
         "dport": np.full(n, L.htons(80), np.uint16), "proto": np.full(n, 6, np.uint8),
         "flags": (rng.random(n) < 0.5).astype(np.uint8), "len": np.full(n, 100, np.uint32),
         "ep": np.zeros(n, np.uint16)}
    e = _engine(policy_max_total=1 << 12, max_endpoints=4)
    o = Oracle()
    for k, v in _lpm_shapes(rng):
        assert e.ipcache_update(k, v) == 0 and o.ipcache_update(k, v) == 0
    pol = [L.policy_key(0, 80, 6, 1), L.policy_key(L.WORLD_ID, 0, 0, 0)]
    for k in pol:
        assert e.policy_update(0, k, L.policy_entry(0)) == 0 and o.policy_update(0, k, L.policy_entry(0)) == 0
    e.commit()
    v0, i0, s0, _ = o.classify_v4(t, nthreads=8)
    assert len(np.unique(i0)) > 1000 and (i0 >= 1 << 30).sum() > 1000
    big = (i0[:n].reshape(-1, 4) >= 1 << 30).sum(1)
    assert (big == 0).any() and (big == 1).any() and (big >= 2).any()
    _gpu_matches(torch_cuda, e, t, (v0, i0, s0), o, pol, [0, 0])
    e.close()
