"""What the table builders make of the cases of hop_cases.py, asserted on the
CPU through the test hook cgpu_diag_hop_tables: where every service frontend,
endpoint and tunnel key landed, the masks, build_lb's relocations, the
doublings, and the MAC row at every endpoint's slot.  test_gpu_hop_shapes.py
runs the same cases through every device walk; a shape that silently
disappeared from a table would leave those runs passing for nothing, so every
shape is an assertion of its own here.  The restatement alone also has to
find the batches non-flat: every planted key decides a packet.  All
comparisons are exact.
"""
import ctypes as C

import numpy as np
import pytest

import cascade_cases as CC
import forward_cases as FC
import hop_cases as H
from cilium_amd import layouts as L, synth
from test_tunnel_cpu import hook

VP = C.c_void_p
NONE = 0xFFFFFFFF
TABLES = ("lb4", "lb6", "e4", "e6", "t4", "t6")
SECLABELS = (np.arange(CC.N_EP, dtype=np.uint32) * 7 + 6000).astype(np.uint32)


def world_structs(w):
    """a forward_frames_cases.FrameWorld as (ENDPOINT_KEY, ENDPOINT_INFO, tunnel keys, tunnel values)"""
    ek = np.array([np.frombuffer(k, L.ENDPOINT_KEY)[0] for k in w.eps], L.ENDPOINT_KEY)
    ei = np.array([L.endpoint_info(*v, *w.macs.get(k, (0, 0))) for k, v in w.eps.items()], L.ENDPOINT_INFO)
    tk = np.array([np.frombuffer(k, L.ENDPOINT_KEY)[0] for k in w.tun], L.ENDPOINT_KEY)
    tv = np.array([np.frombuffer(v, L.ENDPOINT_KEY)[0] for v in w.tun.values()], L.ENDPOINT_KEY)
    return ek, ei, tk, tv


def hop_tables(lb4=None, lb6=None, world=None):
    """cgpu_diag_hop_tables -> ({family: (n, 2) {home, slot}}, MAC rows, stats
    {table: {mask, reloc, doubled}})"""
    def arr(x, dt):
        return np.zeros(0, dt) if x is None else np.ascontiguousarray(x, dt)
    k4, v4 = (arr(lb4 and lb4[i], dt) for i, dt in ((0, L.LB4_KEY), (1, L.LB4_SERVICE)))
    k6, v6 = (arr(lb6 and lb6[i], dt) for i, dt in ((0, L.LB6_KEY), (1, L.LB6_SERVICE)))
    ek, ei, tk, tv = world_structs(world) if world is not None else \
        (np.zeros(0, L.ENDPOINT_KEY), np.zeros(0, L.ENDPOINT_INFO), np.zeros(0, L.ENDPOINT_KEY), np.zeros(0, L.ENDPOINT_KEY))
    rows = {n: np.full((len(k), 2), 0xDEADBEEF, np.uint32) for n, k in (("lb4", k4), ("lb6", k6), ("ep", ek), ("tun", tk))}
    macs = np.full((len(ek), 16), 0xEE, np.uint8)
    st = np.zeros(18, np.uint64)
    S = C.c_size_t
    rc = hook("cgpu_diag_hop_tables", [VP, VP, S, VP, VP, S, VP, VP, S, VP, VP, S, VP, VP, VP, VP, VP, VP])(
        k4.ctypes.data, v4.ctypes.data, len(k4), k6.ctypes.data, v6.ctypes.data, len(k6),
        ek.ctypes.data, ei.ctypes.data, len(ek), tk.ctypes.data, tv.ctypes.data, len(tk),
        rows["lb4"].ctypes.data, rows["lb6"].ctypes.data, rows["ep"].ctypes.data, macs.ctypes.data,
        rows["tun"].ctypes.data, st.ctypes.data)
    assert rc == 0, rc
    stats = {t: dict(zip(("mask", "reloc", "doubled"), (int(x) for x in st[3 * i:3 * i + 3]))) for i, t in enumerate(TABLES)}
    return rows, macs, stats


def fe_rows(c, rows):
    """per frontend of a SvcCase {home, slot}: every map entry of a frontend reports the same"""
    out = np.zeros((len(c.fe), 2), np.uint32)
    for i in range(len(c.fe)):
        r = rows[c.fe_of == i]
        assert len(r) and (r == r[0]).all()
        out[i] = r[0]
    return out


def key_rows(w, rows_e, rows_t):
    """{raw key: (home, slot)} of the endpoints and of the tunnel keys"""
    return ({k: tuple(int(x) for x in r) for k, r in zip(w.eps, rows_e)},
            {k: tuple(int(x) for x in r) for k, r in zip(w.tun, rows_t)})


@pytest.fixture(scope="module")
def svc():
    """family -> (case, per-frontend rows, the table's stats)"""
    out = {}
    for fam, c in (("lb4", H.lb4_case()), ("lb6", H.lb6_case())):
        rows, _, st = hop_tables(**{fam: (c.keys, c.vals)})
        out[fam] = (c, fe_rows(c, rows[fam]), st[fam])
    return out


@pytest.fixture(scope="module")
def fwd():
    c = H.fwd_case()
    rows, macs, st = hop_tables(world=c.w)
    by_e, by_t = key_rows(c.w, rows["ep"], rows["tun"])
    return c, {"e4": by_e, "e6": by_e, "t4": by_t, "t6": by_t}, macs, st


def _off(r, mask):
    return (r[:, 1].astype(np.int64) - r[:, 0]) & mask


def _planted_rows(svc, fwd, table):
    """(homes, {name: (n, 2) rows in insertion order}, mask, every installed key's rows)"""
    if table in ("lb4", "lb6"):
        c, r, st = svc[table]
        return c.homes, {n: r[v] for n, v in c.planted.items()}, st["mask"], r
    c, by, _, st = fwd
    rows = {n: np.array([by[table][k] for k in ks], np.uint32) for n, ks in c.planted[table].items()}
    return c.homes[table], rows, st[table]["mask"], np.concatenate(list(rows.values()))


# ---- the masks, and the mirrors of the hashes ---------------------------------
def test_masks_and_counts(svc, fwd):
    for fam in ("lb4", "lb6"):
        c, r, st = svc[fam]
        assert 513 <= len(c.fe) <= 1024
        assert st["mask"] == H.LB_SLOTS - 1 and st["doubled"] == 0, "a planted neighbourhood overflowed"
        assert (r != NONE).all(), "a frontend of the map is not in the table"
    assert svc["lb4"][2]["reloc"] == 5, "reloc: 1 move, reloc2: 2, reloc_o: 2, none anywhere else"
    c, by, _, st = fwd
    for t in ("e4", "e6", "t4", "t6"):
        assert st[t]["mask"] == c.slots[t] - 1 and st[t]["doubled"] == 0 and st[t]["reloc"] == 0, t
        n = sum(len(v) for v in c.planted[t].values())
        assert c.slots[t] // 4 < n <= c.slots[t] // 2
        assert all(by[t][k][1] != NONE for ks in c.planted[t].values() for k in ks), t


def test_mirror_homes(svc, fwd):
    """the numpy mirrors of lb_hash / lb6_hash / fold6 / fwd_hash4 place every key where the library does"""
    for fam in ("lb4", "lb6"):
        c, r, _ = svc[fam]
        assert np.array_equal(r[:, 0], [f["home"] for f in c.fe])
    c, by, _, _ = fwd
    m = {t: c.slots[t] - 1 for t in c.slots}
    for k in c.w.eps:
        if k[16] == 1:
            want = int(H.fwd_hash4(np.frombuffer(k[:4], "<u4"))[0]) & m["e4"]
        else:
            want = int(H.fold6_bytes(np.frombuffer(k[:16], np.uint8))[0]) & m["e6"]
        assert by["e4"][k][0] == want
    for k in c.w.tun:
        if k[16] == 1:
            want = int(H.fwd_hash4(np.frombuffer(k[:4], "<u4"))[0]) & m["t4"]
        else:
            want = int(H.fold6_bytes(np.frombuffer(k[:16], np.uint8), 3)[0]) & m["t6"]
        assert by["t4"][k][0] == want


# ---- the planted neighbourhoods, in every table ---------------------------------
@pytest.mark.parametrize("table", TABLES)
def test_planted_neighbourhoods_are_isolated(svc, fwd, table):
    homes, rows, mask, every = _planted_rows(svc, fwd, table)
    mine = np.concatenate([r for n, r in rows.items() if n not in ("fill", "l3", "near", "router96")])
    key = every[:, 0].astype(np.int64) * (mask + 1) + every[:, 1]
    rest = every[~np.isin(key, mine[:, 0].astype(np.int64) * (mask + 1) + mine[:, 1])]
    assert len(rest) > 100
    # every other key sits in its home slot, no home within 8 of a planted key's
    assert (rest[:, 0] == rest[:, 1]).all()
    for h in np.unique(mine[:, 0]).astype(np.int64):
        d = (rest[:, 0].astype(np.int64) - h) & mask
        assert (np.minimum(d, mask + 1 - d) >= 8).all(), f"a foreign home near planted home {h}"


@pytest.mark.parametrize("table", TABLES)
def test_full_home(svc, fwd, table):
    homes, rows, mask, _ = _planted_rows(svc, fwd, table)
    r = rows["full"]
    assert (r[:, 0] == homes["full"]).all()
    assert _off(r, mask).tolist() == list(range(8)), "8 keys at offsets 0..7, in insertion order"


@pytest.mark.parametrize("table", TABLES)
def test_wrap(svc, fwd, table):
    homes, rows, mask, _ = _planted_rows(svc, fwd, table)
    r = rows["wrap"]
    assert homes["wrap"] == mask - 1 and (r[:, 0] == mask - 1).all()
    assert r[:, 1].tolist() == [mask - 1, mask, 0, 1, 2], "slots 0..2 hold keys of home mask - 1"


@pytest.mark.parametrize("table", TABLES)
def test_shared_homes_interleave(svc, fwd, table):
    homes, rows, mask, _ = _planted_rows(svc, fwd, table)
    s = homes["shared"]
    a, b = rows["shared_a"], rows["shared_b"]
    assert (a[:, 0] == s).all() and (b[:, 0] == s + 3).all()
    assert a[:, 1].tolist() == [s, s + 1, s + 2, s + 6, s + 7] and b[:, 1].tolist() == [s + 3, s + 4, s + 5]


@pytest.mark.parametrize("table", TABLES)
def test_empty_home_holds_a_foreign_key(svc, fwd, table):
    homes, rows, mask, _ = _planted_rows(svc, fwd, table)
    e = homes["empty"]
    assert rows["empty_a"].tolist() == [[e, e], [e, e + 1]]
    assert rows["empty_b"].tolist() == [[e + 1, e + 2]], "home e + 1: bit 0 clear, its slot holds a key of home e"


@pytest.mark.parametrize("table", TABLES)
def test_every_offset_is_occupied(svc, fwd, table):
    """by planted keys of more than one neighbourhood: the full home's alone would do"""
    homes, rows, mask, _ = _planted_rows(svc, fwd, table)
    for off in range(8):
        at = [n for n, r in rows.items() if n != "fill" and off in _off(r, mask).tolist()]
        assert len(at) >= (2 if off in (0, 1, 2, 6, 7) else 1), (off, at)   # full; wrap 0..4; shared_a 0 1 2 6 7


@pytest.mark.parametrize("table", ["e4", "t4"])
def test_key_zero_with_hop_bits(fwd, table):
    c, by, _, st = fwd
    ks = c.planted[table]["zero"]
    assert ks[0] == FC.key4(0)
    r = np.array([by[table][k] for k in ks])
    assert (r[:, 0] == c.homes[table]["zero"]).all() and _off(r, st[table]["mask"]).tolist() == [0, 1, 2, 3]


def test_absent_keys_at_planted_homes(svc, fwd):
    for fam in ("lb4", "lb6"):
        c, r, st = svc[fam]
        inst = {(bytes(np.asarray(f["addr"]).tobytes()), f["dport"]) for f in c.fe}
        names = [n for n, _, _ in c.absent]
        assert names.count("full") >= 3 and names.count("wrap") >= 1 and names.count("shared") == 2 and \
            names.count("empty") == 2
        for n, a, p in c.absent:
            assert (np.asarray(a).tobytes(), p) not in inst
            f = H.fold6_bytes(a) if c.v6 else None
            home = int((H.lb6_hash(f, p) if c.v6 else H.lb_hash(a, p)).reshape(-1)[0]) & st["mask"]
            assert home in (c.homes[n], c.homes[n] + (1 if n == "empty" else 3)), n
            vb = int((H.lb6_vip_bit(f) if c.v6 else H.lb_vip_bit(a)).reshape(-1)[0]) & (H.VIP_BITS - 1)
            assert c.info["vip_bits"][vb], "the presence bitmap hides the absent key: its probe never runs"
    c, by, _, st = fwd
    for t in ("e4", "e6", "t4", "t6"):
        names = [n for n, _ in c.absent[t]]
        assert names.count("full") >= 3 and names.count("wrap") >= 1
        for n, k in c.absent[t]:
            assert k not in c.w.eps and k not in c.w.tun


def test_false_positive_addresses(svc):
    """addresses of no frontend whose vip bit some frontend sets; some with
    the L3 key's home, some with an L4 key's, the planted full home"""
    for fam in ("lb4", "lb6"):
        c, r, st = svc[fam]
        addrs = {np.asarray(f["addr"]).tobytes() for f in c.fe}
        kinds = [n for n, _, _ in c.false_pos]
        assert kinds.count("l4_full") >= 4 and kinds.count("l3_full") >= 1 and len(kinds) >= 30
        for n, a, p in c.false_pos:
            assert np.asarray(a).tobytes() not in addrs
            f = H.fold6_bytes(a) if c.v6 else None
            vb = int((H.lb6_vip_bit(f) if c.v6 else H.lb_vip_bit(a)).reshape(-1)[0]) & (H.VIP_BITS - 1)
            assert c.info["vip_bits"][vb]
            if n != "any":
                home = int((H.lb6_hash(f, p) if c.v6 else H.lb_hash(a, p)).reshape(-1)[0]) & st["mask"]
                assert home == c.homes["full"]


# ---- lb4: build_lb's relocation ---------------------------------------------------
def test_lb4_relocation(svc):
    c, r, st = svc["lb4"]
    R = c.homes["reloc"]
    own = r[c.planted["reloc"]]
    assert own[:, 0].tolist() == list(range(R, R + 8))
    # the key of home R + 1 moved to R + 8 (offset 7), the late key took its slot
    want = [R + j for j in range(8)]
    want[1] = R + 8
    assert own[:, 1].tolist() == want
    assert r[c.planted["reloc_late"]].tolist() == [[R, R + 1]]


def test_lb4_double_relocation(svc):
    c, r, st = svc["lb4"]
    D = c.homes["reloc2"]
    own = r[c.planted["reloc2"]]
    assert own[:, 0].tolist() == list(range(D, D + 15))
    want = [D + j for j in range(15)]
    want[8] = D + 15   # first move: the key of home D + 8, the free slot still 8 from home D
    want[1] = D + 8    # second move: the key of home D + 1
    assert own[:, 1].tolist() == want
    assert r[c.planted["reloc2_late"]].tolist() == [[D, D + 1]]


def test_lb4_relocation_of_a_displaced_key(svc):
    """moves of keys that sat at offsets 6 and 1 of their homes: the free slot
    comes 1 and 6 nearer (d -= j - o), and the second key leaves a slot whose
    hop bits belong to another home's key"""
    c, r, st = svc["lb4"]
    X = c.homes["reloc_o"]
    own = r[c.planted["reloc_o"]]
    assert own.tolist() == [[X, X], [X, X + 1]] + [[X + j, X + j] for j in range(3, 8)]
    assert r[c.planted["reloc_o_far"]].tolist() == [[X + 2, X + 9]], "first at X + 8, moved one slot"
    assert r[c.planted["reloc_o_moved"]].tolist() == [[X + 1, X + 8]], "first at X + 2, moved six slots"
    assert r[c.planted["reloc_o_late"]].tolist() == [[X, X + 2]]


# ---- near-equal keys, value shapes --------------------------------------------------
def test_near_equal_service_keys(svc):
    for fam in ("lb4", "lb6"):
        c, r, _ = svc[fam]
        near = c.fe[c.planted["near"][0]]
        same = [f for f in c.fe if np.asarray(f["addr"]).tobytes() == np.asarray(near["addr"]).tobytes()]
        ports = {f["dport"] for f in same}
        assert 0 in ports and len(ports - {0}) >= 2, "one address with two dports and the L3 key"
        assert any(f["shape"] == "retry" and f["name"] != "fill" for f in same)


def test_service_shapes_sit_on_displaced_frontends(svc):
    for fam in ("lb4", "lb6"):
        c, r, st = svc[fam]
        off = _off(r, st["mask"])
        for shape in ("retry", "slow_count", "slow_hole", "master_only", "no_master", "n1", "n4"):
            at = [int(off[i]) for i, f in enumerate(c.fe) if f["shape"] == shape and f["name"] != "fill"]
            assert any(d > 0 for d in at), shape
        l3 = {np.asarray(c.fe[i]["addr"]).tobytes() for i in c.planted["l3"]}
        for i, f in enumerate(c.fe):
            if f["shape"] == "retry":
                assert np.asarray(f["addr"]).tobytes() in l3, "a retry frontend without its L3 frontend"
        # backend ports equal to the key's dport, and different
        k, v = c.keys, c.vals
        sl = k["slave"] != 0
        assert (v["port"][sl] == k["dport"][sl]).sum() > 100 and (v["port"][sl] != k["dport"][sl]).sum() > 100


def test_near_equal_forwarding_keys(fwd):
    c, by, _, _ = fwd
    e6 = [k for ks in c.planted["e6"].values() for k in ks]
    assert len({k[:12] for k in e6}) == 1, "every e6 address differs from the others in word 3 alone"
    full = c.planted["e6"]["full"]
    assert len({by["e6"][k][0] for k in full}) == 1
    assert FC.key6(H.ROUTER6) in c.w.tun and full[0][:12] == H.ROUTER6[:12], "a t6 key with the /96 of the e6 addresses"


# ---- the MAC rows ---------------------------------------------------------------------
def test_mac_rows_at_the_keys_slots(fwd):
    c, by, macs, _ = fwd
    seen = set()
    for i, k in enumerate(c.w.eps):
        mac, node = c.w.macs.get(k, (0, 0))
        want = mac.to_bytes(8, "little")[:6] + node.to_bytes(8, "little")[:6] + bytes(4)
        assert macs[i].tobytes() == want, "an endpoint's MAC row is not at its slot"
        seen.add(want)
    assert len(seen) == len(c.w.eps), "a distinct MAC pair per endpoint"


# ---- the overfull cases: one doubling ---------------------------------------------------
def test_overfull_doubles_once():
    c4, c6, f = H.lb4_overfull(), H.lb6_overfull(), H.fwd_overfull()
    rows, _, st = hop_tables(lb4=(c4.keys, c4.vals), lb6=(c6.keys, c6.vals), world=f.w)
    for t in TABLES:
        assert st[t] == {"mask": H.SMALL_SLOTS - 1, "reloc": 0, "doubled": 1}, (t, st[t])
    for fam, c in (("lb4", c4), ("lb6", c6)):
        r = fe_rows(c, rows[fam])
        assert len(r) == 9 and (r != NONE).all()
        assert sorted(np.bincount(r[:, 0], minlength=128)[[c.homes["nine"], c.homes["nine"] + 64]]) == [4, 5]
    by_e, by_t = key_rows(f.w, rows["ep"], rows["tun"])
    for t, by in (("e4", by_e), ("e6", by_e), ("t4", by_t), ("t6", by_t)):
        r = np.array([by[k] for k in f.planted[t]["nine"]])
        assert (r != NONE).all() and set(r[:, 0]) == {f.homes[t]["nine"], f.homes[t]["nine"] + 64}
        if t in ("e4", "t4"):   # key 0 is absent, its home carries three hop bits
            z = np.array([by[k] for k in f.planted[t]["zero"]])
            assert (z[:, 0] == f.homes[t]["zero"]).all() and _off(z, 127).tolist() == [0, 1, 2]
            assert FC.key4(0) not in f.w.eps and FC.key4(0) not in f.w.tun


# ---- the second commit --------------------------------------------------------------------
def test_second_commit_tables(svc, fwd):
    for fam in ("lb4", "lb6"):
        c, r1, st1 = svc[fam]
        k, v = c.entries(2)
        rows, _, st = hop_tables(**{fam: (k, v)})
        assert st[fam]["mask"] == H.LB_SLOTS - 1
        gone = c.fe[c.info["gone"]]
        assert c.info["gone"] == c.planted["full"][3] and int(_off(r1[[c.info["gone"]]], st1["mask"])[0]) == 3
        def same(x, f):
            return x["address"].tobytes() == np.asarray(f["addr"], x["address"].dtype).tobytes() and x["dport"] == f["dport"]
        assert sum(same(x, gone) for x in c.keys) == 3 and not any(same(x, gone) for x in k)
        new = c.info["new"]
        mine = np.array([same(x, new) for x in k])
        assert mine.sum() == 3 and (rows[fam][mine][:, 0] == st[fam]["mask"] - 1).all()
        assert (rows[fam] != NONE).all()
    c = fwd[0]
    w2 = H.fwd_world2(c)
    dele, add = H.fwd_second_commit(c)
    rows, _, st = hop_tables(world=w2)
    by_e, by_t = key_rows(w2, rows["ep"], rows["tun"])
    for t, by in (("e4", by_e), ("e6", by_e), ("t4", by_t), ("t6", by_t)):
        assert dele[t] not in by and by[add[t]][0] == c.slots[t] - 2
        full = [by[k] for k in c.planted[t]["full"] if k != dele[t]]
        assert [s - h for h, s in full] == list(range(7)), "the other seven keys of the full home close up"


# ---- the batches: every planted key decides a packet ---------------------------------------
def _svc_oracle(c, v6):
    from oracle import Oracle
    o = Oracle(ct_proto_gate=1)
    CC.policy_workload().load(o, 1)
    c.load(o, 1)
    synth.load_lxc(o, SECLABELS)
    return o


@pytest.mark.parametrize("v6", [False, True], ids=["lb4", "lb6"])
def test_service_batch_reaches_every_planted_frontend(svc, v6):
    c, r, st = svc["lb6" if v6 else "lb4"]
    b, target = H.svc_batch(v6)
    n = len(target)
    assert n <= 40_000 and n % 4 != 0
    assert {6, 17, 58 if v6 else 1, H.GATED} <= set(np.unique(b["proto"]).tolist())
    # the translation of every tuple: the stateful restatement on an empty map
    o = _svc_oracle(c, v6)
    (o.ct6_set_max if v6 else o.ct_set_max)(1 << 17)
    x = (o.classify_v6_ctlb if v6 else o.classify_v4_ctlb)(b, 1000)
    o.close()
    if v6:
        moved = (x["xdaddr"].reshape(n, 16) != b["daddr"]).any(1)
    else:
        moved = x["xdaddr"] != b["daddr"]
    l3 = {np.asarray(c.fe[i]["addr"]).tobytes() for i in c.planted["l3"]}
    for i, f in enumerate(c.fe):
        mine = target == i
        assert mine.sum() >= 3
        has_l3 = np.asarray(f["addr"]).tobytes() in l3
        if f["shape"] == "master_only":
            # the selected slave has no row, and the fallback keeps that slave: an
            # L3 frontend's slave entries carry no count, so it cannot answer either
            l4 = mine & np.isin(b["proto"], (6, 17))
            assert l4.sum() >= 2 and not moved[l4].any(), "a frontend without slaves translated"
            assert (x["verdict"][l4] == L.DROP_NO_SERVICE).all()
        elif f["shape"] in ("retry", "no_master") and not has_l3:
            assert not moved[mine].any()
        else:
            assert moved[mine].any(), f"planted frontend {i} ({f['name']}, {f['shape']}) translates no packet"
    for i in range(len(c.absent)):
        assert (target == -1 - i).sum() == 4
    for i in range(len(c.false_pos)):
        mine = target == -1000 - i
        assert mine.sum() == 4 and not moved[mine].any()
    absent_moved = moved[(target < 0) & (target > -1000)]
    assert not absent_moved.all()
    # candidates of the x4 kernel's RETRY and SLOW stages: conditions on the inputs
    l4 = np.isin(b["proto"], (6, 17))
    shape = np.array([c.fe[t]["shape"] if t >= 0 else "" for t in target])
    has = np.array([t >= 0 and np.asarray(c.fe[t]["addr"]).tobytes() in l3 for t in target])
    assert (l4 & np.isin(shape, ("retry", "no_master")) & has).sum() >= 8, "RETRY: the L4 key has no count, the L3 key exists"
    assert (l4 & (shape == "slow_count") & (b["hash"] % 5 + 1 > 3)).sum() >= 4, "SLOW: a slave past nslaves"
    assert (l4 & (shape == "slow_hole") & (b["hash"] % 3 + 1 == 2)).sum() >= 4, "SLOW: a missing slave row"
    q = shape[:n - n % 4].reshape(-1, 4)
    assert ((q != "").any(1) & (q == "").any(1)).sum() > 100, "service and policy tuples in one quad"
    if not v6:   # lb4_local's loopback case (ret 2: translated, the source is the selected backend)
        o = _svc_oracle(c, v6)
        ref, _ = o.lb4(b, L.LB_LXC, nthreads=4)
        o.close()
        lo = ref["ret"] == 2
        assert lo.sum() >= 3 and (target[lo] >= 0).all() and (ref["tdaddr"][lo] == b["daddr"][lo]).all()
        assert (ref["ret"] == L.DROP_NO_SERVICE).sum() >= 4


@pytest.mark.parametrize("v6", [False, True], ids=["lb4", "lb6"])
def test_stateful_batches_repeat_connections(svc, v6):
    c = svc["lb6" if v6 else "lb4"][0]
    b1, b2, b3 = H.svc_ct_batches(v6)
    o = _svc_oracle(c, v6)
    (o.ct6_set_max if v6 else o.ct_set_max)(1 << 17)
    fn = o.classify_v6_ctlb if v6 else o.classify_v4_ctlb
    x = [fn(b, 1000 + j) for j, b in enumerate((b1, b2, b3))]
    o.close()
    for b in (b1, b2, b3):
        assert len(b["flags"]) <= 8000 and len(b["flags"]) % 4 != 0
    assert (x[0]["ct_ret"] == L.CT_NEW).sum() > 1000
    est = x[1]["ct_ret"] == L.CT_ESTABLISHED
    assert est.sum() > 1000, "the second batch finds the first's connections"
    # an established connection keeps the backend its CT_SERVICE entry names
    np.testing.assert_array_equal(x[1]["xdaddr"][est], x[0]["xdaddr"][est])
    assert (x[2]["ct_ret"] == L.CT_ESTABLISHED).sum() > 500 and (x[2]["ct_ret"] == L.CT_NEW).sum() > 500


@pytest.mark.parametrize("v6", [False, True], ids=["lb4", "lb6"])
def test_stateful_batches_meet_stored_slaves(svc, v6):
    """No packet stores slave 0 (a selected slave is >= 1), so CT_SERVICE
    entries installed beforehand name it: lb4_lookup_slave / lb6_lookup_slave
    then read the master's own entry (target 0), at frontends that are not in
    their home slot.  Others name a slave past the frontend's or a missing row
    (the fallback finds no service: DROP_NO_SERVICE).  A frontend without a
    master entry is never reached with a stored slave: lb*_lookup_service
    passes only a key whose master has a count, so its packets go to the L3
    frontend of its address or are not service packets at all."""
    c, r, st = svc["lb6" if v6 else "lb4"]
    off = _off(r, st["mask"])
    b1, b2, b3 = H.svc_ct_batches(v6)
    k, v, rows, fe, slave = H.svc_ct_preinstall(v6)
    o = _svc_oracle(c, v6)
    (o.ct6_set_max if v6 else o.ct_set_max)(1 << 17)
    H.load_ct_preinstall(o, v6)
    fn = o.classify_v6_ctlb if v6 else o.classify_v4_ctlb
    x = [fn(b, 1000 + j) for j, b in enumerate((b1, b2, b3))]
    after = [np.frombuffer((o.ct6_lookup if v6 else o.ct4_lookup)(a)[1], L.CT_ENTRY)[0] for a in k]
    o.close()
    n = len(b1["flags"])
    shape = np.array([c.fe[i]["shape"] for i in fe])
    l3 = {np.asarray(c.fe[i]["addr"]).tobytes() for i in c.planted["l3"]}
    has_l3 = np.array([np.asarray(c.fe[i]["addr"]).tobytes() in l3 for i in fe])
    own = np.isin(shape, ("n1", "n2", "n3", "n4", "slow_count", "slow_hole", "master_only"))  # the L4 key has a count
    zero = (x[0]["xdaddr"].reshape(n, -1)[rows] == 0).all(1)
    for j in (0, 1):   # the second batch is the first again: the stored slave 0 stays
        z = (x[j]["xdaddr"].reshape(n, -1)[rows] == 0).all(1)
        assert z[own & (slave == 0)].all(), "a stored slave 0 reads the master's entry: target 0"
        assert not z[own & (slave == 1)].any()
    assert (zero & own & (slave == 0) & (off[fe] > 0)).sum() >= 10, "slave 0 at displaced frontends"
    assert len(set(off[fe][zero & own & (slave == 0)].tolist())) >= 6, "at most offsets"
    assert (own & (slave == 0) & (v["bits"] == L.CTB_LB_LOOPBACK)).sum() >= 5
    # a slave past the frontend's, the missing row: lb*_lookup_service with the slave kept finds nothing
    gone = own & ((slave == 40) | ((slave == 2) & np.isin(shape, ("n1", "slow_hole", "master_only"))))
    assert gone.sum() >= 10 and (x[0]["verdict"][rows][gone] == L.DROP_NO_SERVICE).all()
    assert (x[0]["verdict"][rows][own & (slave == 0)] != L.DROP_NO_SERVICE).all()
    # the L4 key has no count: with the L3 frontend of its address the L3 master's entry is read ...
    weak = np.isin(shape, ("retry", "no_master"))
    assert (weak & has_l3 & (slave == 0)).sum() >= 2 and zero[weak & has_l3 & (slave == 0)].all()
    # ... without it there is no service lookup in conntrack: the entry stays as installed
    alone = np.flatnonzero(weak & ~has_l3)
    assert (shape[weak & (slave == 0)] == "no_master").any() and (shape[weak & (slave == 0)] == "retry").any()
    for i in alone:
        assert after[i] == v[i] and not zero[i]
    # every other entry was hit: the packets of both batches are counted
    for i in np.flatnonzero(own | (weak & has_l3)):
        assert after[i]["tx_packets"] + after[i]["rx_packets"] > v[i]["tx_packets"]


@pytest.mark.parametrize("small", [False, True], ids=["main", "overfull"])
@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_forward_batch_reaches_every_planted_key(v6, small):
    c = H.fwd_overfull() if small else H.fwd_case()
    b, who = H.fwd_batch(v6, small)
    n = len(who)
    assert n <= 40_000 and n % 4 != 0 and set(np.unique(b["ttl"]).tolist()) == {0, 1, 2, 64}
    exp = FC.restate(c.w, FC.LXC, v6, **b)
    e, t = ("e6", "t6") if v6 else ("e4", "t4")
    local = {k: v for k, v in c.w.eps.items()}
    hit = {}
    for i, (tab, k) in enumerate(who):
        if tab == e and k in local:
            ifx, lid, fl = local[k]
            ok = exp["action"][i] == (FC.HOST if fl & 1 else FC.LOCAL) and (fl & 1 or exp["arg"][i] == lid)
        elif tab == t and k in c.w.tun:
            ok = exp["action"][i] == FC.OVERLAY and b["tunnel"][i] == 0 and \
                exp["arg"][i] == int.from_bytes(c.w.tun[k][:4], "little")
        else:
            hit.setdefault((tab, k, "absent"), 0)
            hit[(tab, k, "absent")] += 1
            continue
        hit[(tab, k)] = hit.get((tab, k), 0) + bool(ok)
    for tab in (e, t):
        for name, ks in c.planted[tab].items():
            for k in (ks if name != "fill" else ks[:60]):
                assert hit.get((tab, k), 0) >= 1, f"planted {tab} key of '{name}' decides no packet"
        for name, k in c.absent[tab]:
            assert hit[(tab, k, "absent")] == 6
    if not small:   # every row of the decision list but the tunnel value 0 (forward_cases has it)
        for name, m in FC.categories(c.w, FC.LXC, v6, b).items():
            assert m.any() or name == "map value 0", name
