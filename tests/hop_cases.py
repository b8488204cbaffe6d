"""Crafted service frontend tables and forwarding tables, shared by the CPU
shape test (test_hop_shapes.py) and the device walks (test_gpu_hop_shapes.py).
Plain numpy with fixed PCG64 seeds; nothing here asks the library anything:
the keys are found with mirrors of the tables.h hashes, and what the builders
made of them is asserted through the test hook cgpu_diag_hop_tables on the CPU.

Six single-slot neighbourhood tables (tables.h POL_HOP): the lb4 and lb6
frontends (2048 slots each), the forwarding tables e4 / e6 (1024 slots) and
t4 / t6 (512 slots).  Every table gets the same planted neighbourhoods (a home
slot and the keys that hash to it), each isolated by a margin of 8 homes, the
rest of the table being keys of distinct homes elsewhere (they all sit in
their home slot):

  full     8 keys of one home, offsets 0..7, and >= 3 absent keys of that home;
  wrap     5 keys of home mask - 1 (slots mask - 1, mask, 0, 1, 2), absent keys;
  shared   homes S and S + 3: keys a1 a2 a3 b1 b2 b3 a4 a5 in insertion order
           fill S .. S + 7, so a4 / a5 lie behind every key of S + 3;
  empty    two keys of home E (slots E, E + 1), then one of home E + 1 (slot
           E + 2): slot E + 1 holds a foreign key, its own bit 0 is clear.

The builders insert in key order, not call order: lb4 by address << 32 |
dport << 16 (the raw words), lb6 and the forwarding maps by key bytes.  Every
candidate carries that rank and the shapes are chosen by it.

lb4 only (build_lb relocates, the others only double): "reloc" (slots R ..
R + 7 each hold the key of that home, then a later key of home R: the key of
R + 1 moves to R + 8, offset 7), "reloc2" (15 such slots: two moves) and
"reloc_o" (two moves again: a key at offset 6 of its home moves one slot, then
a key at offset 1 of its home moves six, out of a slot that is itself the home
of a displaced key).

The small second case of every family (`*_overfull`) holds nine keys of one
home at the base size of 64 slots: the table doubles once, to 128.

Expected answers come from the restatement (oracle, forward_cases), never from
the library.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

import cascade_cases as CC
import forward_cases as FC
import forward_frames_cases as FF
from cascade_cases import HOP, _Zones, mix32
from cilium_amd import layouts as L

LB_SLOTS = 1 << 11    # asserted through cgpu_diag_hop_tables
EP_SLOTS = 1 << 10
TUN_SLOTS = 1 << 9
SMALL_SLOTS = 1 << 7  # the overfull cases after their doubling (base 64)
VIP_BITS = 1 << 15    # tables.h lb_table.vip at <= 4096 frontends
_M = np.uint64(0xFFFFFFFF)


# --------------------------------------------------------------------------
# tables.h hashes, vectorised
# --------------------------------------------------------------------------
def _u64(x):
    return np.asarray(x).astype(np.uint64)


def lb_hash(addr, dport):
    """tables.h lb_hash: the raw address word and the raw (network-order) dport"""
    return mix32(addr, (_u64(dport) ^ np.uint64(0x1b5e0000)).astype(np.uint32))


def lb_vip_bit(addr):
    return mix32(addr, 0x5f1b7e11)


def fmix32(h):
    h = _u64(h) & _M
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85ebca6b)) & _M
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xc2b2ae35)) & _M
    return h ^ (h >> np.uint64(16))


def fold6(w0, w1, w2, w3):
    """tables.h fold6 over the four little-endian words of an address"""
    h = fmix32(_u64(w3) ^ np.uint64(0x6B43A9B5))
    h = fmix32(_u64(w2) ^ h)
    h = fmix32(_u64(w1) ^ h)
    return fmix32(_u64(w0) ^ h).astype(np.uint32)


def fold6_bytes(a16, words=4):
    """fold6 of (n, 16) address bytes; words = 3: the /96 (word 3 taken as 0)"""
    w = np.ascontiguousarray(a16, np.uint8).reshape(-1, 16).view("<u4")
    return fold6(w[:, 0], w[:, 1], w[:, 2], w[:, 3] if words == 4 else np.zeros(len(w), np.uint32))


def lb6_hash(f, dport):
    return mix32(f, (_u64(dport) ^ np.uint64(0x6d5e0000)).astype(np.uint32))


def lb6_vip_bit(f):
    return mix32(f, 0x2f6b1e17)


def fwd_hash4(a):
    return mix32(a, 0x46574434)


def _be16(x):
    return np.asarray(x).astype(np.uint16).byteswap()


def _be32(x):
    return np.asarray(x).astype(np.uint32).byteswap()


# --------------------------------------------------------------------------
# candidates of one table and the planted neighbourhoods
# --------------------------------------------------------------------------
class Cands:
    """Candidate keys of one table by index: their home at `slots`, the rank
    the builder inserts them in, the zones claimed by planted neighbourhoods
    and the homes given to single keys."""

    def __init__(self, slots, hash32, rank):
        self.slots, self.mask = slots, slots - 1
        self.hash32 = np.asarray(hash32, np.uint32)
        self.home = (self.hash32 & np.uint32(self.mask)).astype(np.int64)
        self.rank = np.asarray(rank)
        self.order = np.lexsort((self.rank, self.home))
        self.first = np.searchsorted(self.home[self.order], np.arange(slots + 1))
        self.used = np.zeros(len(self.home), bool)
        self.z = _Zones(slots)
        self.single = np.zeros(slots, bool)   # homes of keys that sit alone
        self.homes, self.planted, self.absent = {}, {}, {}

    def at(self, h):
        """the unused candidates of home h, in insertion order"""
        h &= self.mask
        ix = self.order[self.first[h]:self.first[h + 1]]
        return ix[~self.used[ix]]

    def take(self, name, ix):
        ix = np.atleast_1d(ix)
        assert not self.used[ix].any()
        self.used[ix] = True
        self.planted.setdefault(name, []).extend(int(i) for i in ix)

    def leave(self, name, ix):
        """candidates of a planted home that stay absent"""
        ix = np.atleast_1d(ix)
        assert len(ix) and not self.used[ix].any()
        self.used[ix] = True
        self.absent.setdefault(name, []).extend(int(i) for i in ix)

    def free_home(self, h):
        return not self.z.taken[h & self.mask] and not self.single[h & self.mask]

    def reserve(self, h):
        """a home for a key that sits alone in it (outside every zone)"""
        if not self.free_home(h):
            return False
        self.single[h & self.mask] = True
        return True

    def fillers(self, n, rng, ok=None):
        """n unused candidates of distinct free homes"""
        ix = rng.permutation(len(self.home))[:400_000]
        keep = ~self.used[ix] & ~self.z.taken[self.home[ix]] & ~self.single[self.home[ix]]
        if ok is not None:
            keep &= ok[ix]
        ix = ix[keep]
        _, f = np.unique(self.home[ix], return_index=True)
        ix = ix[np.sort(f)][:n]
        assert len(ix) == n, (len(ix), n)
        self.used[ix] = True
        self.single[self.home[ix]] = True
        return ix

    def all_planted(self):
        return np.array(sorted(i for v in self.planted.values() for i in v), np.int64)


def plant_common(t, start=40):
    """full, wrap, shared and empty into t; returns the next free scan start"""
    r = t.rank
    f = t.homes["full"] = t.z.scan(start, HOP)
    c = t.at(f)
    assert len(c) >= 12, len(c)
    t.take("full", c[:8])
    t.leave("full", c[[8, len(c) // 3, len(c) // 2, len(c) - 1]])   # of the first address and of later ones
    w = t.homes["wrap"] = t.mask - 1
    assert t.z.claim(w, 5)
    c = t.at(w)
    assert len(c) >= 7
    t.take("wrap", c[:5])
    t.leave("wrap", c[[5, len(c) - 1]])
    s = t.homes["shared"] = t.z.scan(f + 40, 3 + HOP)
    a, b = t.at(s), t.at(s + 3)
    assert len(a) >= 8
    b = b[(r[b] > r[a[2]]) & (r[b] < r[a[-2]])]
    assert len(b) >= 4
    t.take("shared_a", np.concatenate([a[:3], a[-2:]]))
    t.take("shared_b", b[:3])
    t.leave("shared", [a[3], b[3]])
    e = t.homes["empty"] = t.z.scan(s + 40, 4)
    a, b = t.at(e), t.at(e + 1)
    assert len(a) >= 3 and len(b) >= 2 and r[b[-1]] > r[a[1]]
    t.take("empty_a", a[:2])
    t.take("empty_b", b[-1:])
    t.leave("empty", [a[2], b[0]])
    return e + 40


def overfull_pick(hash32, rank, extra_home=None):
    """nine candidates of one home at 64 slots that split 5 / 4 at 128, lowest
    rank first; with extra_home (a home at 128 slots): three more of that home,
    8 homes or more away from the nine's"""
    h64 = (hash32 & 63).astype(np.int64)
    h128 = (hash32 & 127).astype(np.int64)
    for h in range(8, 56):
        if extra_home is not None and min((h - extra_home) & 127, (extra_home - h) & 127,
                                          (h + 64 - extra_home) & 127, (extra_home - h - 64) & 127) < 16:
            continue
        lo = np.flatnonzero((h64 == h) & (h128 == h))
        hi = np.flatnonzero((h64 == h) & (h128 == h + 64))
        if len(lo) >= 5 and len(hi) >= 4:
            ix = np.concatenate([lo[:5], hi[:4]])
            ix = ix[np.argsort(rank[ix], kind="stable")]
            if extra_home is None:
                return ix, h
            ex = np.flatnonzero(h128 == extra_home)
            assert len(ex) >= 3
            return np.concatenate([ix, ex[:3]]), h
    raise AssertionError("no overfull home")


# --------------------------------------------------------------------------
# services
# --------------------------------------------------------------------------
# value shapes of a frontend (its map entries):
#   n1..n4       master with count n, slaves 1..n
#   retry        master with count 0 and no slave; the L3 frontend of its address exists
#   slow_count   master with count 5, slaves 1..3: a selected slave 4 / 5 is past nslaves
#   slow_hole    master with count 3, slaves 1 and 3: slave 2's row is missing
#   master_only  master with count 2, no slave
#   no_master    slaves 1 and 2, no master entry (LB_FE_MASTER clear)
SHAPES = {"n1": (1, (1,)), "n2": (2, (1, 2)), "n3": (3, (1, 2, 3)), "n4": (4, (1, 2, 3, 4)),
          "retry": (0, ()), "slow_count": (5, (1, 2, 3)), "slow_hole": (3, (1, 3)),
          "master_only": (2, ()), "no_master": (None, (1, 2))}
# the shapes of the full home's keys by offset, of the wrap's, of the shared a-keys'
FULL_SHAPES = ("n2", "retry", "slow_count", "slow_hole", "master_only", "no_master", "n1", "n4")
WRAP_SHAPES = ("n1", "n3", "slow_hole", "retry", "slow_count")
SHARED_A_SHAPES = ("n2", "n1", "n3", "retry", "slow_count")


@dataclass
class SvcCase:
    v6: bool
    fe: list                 # frontends: dicts {addr (u32 raw / 16 bytes), dport (raw), shape, name, backends}
    keys: np.ndarray         # LB4_KEY / LB6_KEY of the first commit ...
    vals: np.ndarray         # ... LB4_SERVICE / LB6_SERVICE
    fe_of: np.ndarray        # per map entry: index into fe
    homes: dict              # planted name -> home slot
    planted: dict            # planted name -> indices into fe, in insertion order
    absent: list             # (addr, dport raw) never installed, at planted homes (name, addr, dport)
    false_pos: list          # (name, addr, dport raw): no frontend has the address; its vip bit is set
    keys2: np.ndarray = None  # the second commit: entries deleted (del2 = 1) or added
    vals2: np.ndarray = None
    del2: np.ndarray = None
    info: dict = field(default_factory=dict)

    def entries(self, phase=1):
        """(keys, vals) present after commit `phase`"""
        if phase == 1:
            return self.keys, self.vals
        gone = {k.tobytes() for k in self.keys2[self.del2 == 1]}
        keep = np.array([k.tobytes() not in gone for k in self.keys])
        add = self.del2 == 0
        return np.concatenate([self.keys[keep], self.keys2[add]]), np.concatenate([self.vals[keep], self.vals2[add]])

    def load(self, t, phase=1, commit=None):
        """into an Engine or an Oracle; commit: called between the two commits"""
        v6 = self.v6

        def up(k, v):
            if v6:
                return t.lb6_update(k, v)
            return (t.lb4_update if hasattr(t, "lb4_update") else t.lb_update)(k, v)

        def dele(k):
            if v6:
                return t.lb6_delete(k)
            return (t.lb4_delete if hasattr(t, "lb4_delete") else t.lb_delete)(k)
        for k, v in zip(self.keys, self.vals):
            assert up(k, v) == 0
        if phase == 2:
            if commit:
                commit()
            for k, v, d in zip(self.keys2, self.vals2, self.del2):
                assert (dele(k) if d else up(k, v)) == 0


def _backend(case, j, v6):
    """backend j, an address of its own: three in four inside the prefix of a
    fat identity (every endpoint's egress L3 key allows it: the connection is
    created), the others inside identity j's prefix (most are denied)"""
    fat = case.info["fat"]
    ident, low = (case.ids[np.array([j % len(case.ids)])], 77) if j % 4 == 3 else \
        (fat[np.array([j % len(fat)])], 1 + (j // 4) % 250)
    if v6:
        return CC.id_addr6(case, ident, np.array([low], np.uint8))[0]
    return int(_be32(CC.id_addr4(case, ident, np.array([low], np.uint32)))[0])


def _entries(fes, v6, case, first_backend=0):
    """the map entries of the frontends as lbmap writes them; backend ports
    equal the frontend's dport on even backends and differ on odd ones"""
    kd, vd = (L.LB6_KEY, L.LB6_SERVICE) if v6 else (L.LB4_KEY, L.LB4_SERVICE)
    keys, vals, fe_of = [], [], []
    nb = first_backend
    for i, f in enumerate(fes):
        count, slaves = SHAPES[f["shape"]]
        f["backends"] = {}
        for s in ([] if count is None else [0]) + list(slaves):
            k, v = np.zeros((), kd), np.zeros((), vd)
            k["address"], k["dport"], k["slave"] = f["addr"], f["dport"], s
            v["rev_nat_index"] = L.htons(1 + i % 65000)
            v["weight"] = L.htons(1)
            if s == 0:
                v["count"] = count
            else:
                tgt = _backend(case, nb, v6)
                port = int(f["dport"]) if nb % 2 == 0 and f["dport"] else L.htons(9000 + nb % 1000)
                v["target"], v["port"] = tgt, port
                f["backends"][s] = (tgt, port)
                nb += 1
            keys.append(k)
            vals.append(v)
            fe_of.append(i)
    return np.array(keys, kd), np.array(vals, vd), np.array(fe_of, np.int64), nb


def _vip_bits(hashes):
    bits = np.zeros(VIP_BITS, bool)
    bits[np.asarray(hashes, np.uint32) & np.uint32(VIP_BITS - 1)] = True
    return bits


def _svc_case(v6, seed, n_fill):
    """lb4 / lb6: the planted neighbourhoods over 128 addresses x every port"""
    rng = np.random.Generator(np.random.PCG64(seed))
    case = CC.policy_hops()
    n_addr = 128
    ports = _be16(np.arange(1, 65536)).astype(np.uint32)                 # raw dport words
    if v6:
        a16 = np.zeros((n_addr, 16), np.uint8)
        a16[:, 0], a16[:, 1] = 0xFD, 0x64
        a16[:, 12:] = (1 + 37 * np.arange(n_addr)).astype(">u4").view(np.uint8).reshape(n_addr, 4)
        fold = fold6_bytes(a16)
        l3_home = (lb6_hash(fold, 0) & np.uint32(LB_SLOTS - 1)).astype(np.int64)
        ai = np.repeat(np.arange(n_addr), len(ports))
        pp = np.tile(ports, n_addr)
        h32 = lb6_hash(fold[ai], pp)
        # key bytes: the addresses ascend with their index, the dport bytes are the host-order port
        rank = ai.astype(np.int64) * 65536 + _be16(pp).astype(np.int64)
        vbit = lb6_vip_bit(fold)

        def addr_of(i):
            return a16[i].copy()
    else:
        a32 = _be32(0x64400000 + 1 + 37 * np.arange(n_addr))              # 100.64.0.0/10, raw words
        l3_home = (lb_hash(a32, 0) & np.uint32(LB_SLOTS - 1)).astype(np.int64)
        ai = np.repeat(np.arange(n_addr), len(ports))
        pp = np.tile(ports, n_addr)
        h32 = lb_hash(a32[ai], pp)
        rank = (a32[ai].astype(np.uint64) << np.uint64(32)) | (pp.astype(np.uint64) << np.uint64(16))
        vbit = lb_vip_bit(a32)

        def addr_of(i):
            return int(a32[i])
    t = Cands(LB_SLOTS, h32, rank)
    nxt = plant_common(t)
    if not v6:
        # reloc: the keys of homes R .. R + 7 in their home slots, then a later key of home R
        for name, width in (("reloc", 8), ("reloc2", 15)):
            R = t.homes[name] = t.z.scan(nxt, width + 1)
            for j in range(width):
                t.take(name, t.at(R + j)[:1])
            late = t.at(R)[-1]
            assert rank[late] > rank[t.planted[name]].max()
            t.take(name + "_late", [late])
            nxt = R + 40
        # reloc_o: X, X + 1 <- two keys of home X; X + 2 <- the key of home X + 1
        # (offset 1); X + 3 .. X + 7 their own; X + 8 <- a key of home X + 2
        # (offset 6); then a later key of home X: the key of home X + 2 moves
        # to X + 9, then the key of home X + 1 from X + 2, the home of a
        # displaced key, to X + 8
        X = t.homes["reloc_o"] = t.z.scan(nxt, 10)
        a, b = t.at(X), t.at(X + 1)
        mid = b[len(b) // 2]
        assert rank[a[1]] < rank[mid] < rank[a[-1]]
        t.take("reloc_o", a[:2])
        t.take("reloc_o_moved", [mid])
        for j in range(3, 8):
            t.take("reloc_o", t.at(X + j)[:1])
        late = t.at(X)[-1]
        far = t.at(X + 2)
        far = far[rank[far] < rank[late]][-1]
        assert rank[late] > rank[far] > max(rank[t.planted["reloc_o"]].max(), rank[t.planted["reloc_o_moved"][0]])
        t.take("reloc_o_far", [far])
        t.take("reloc_o_late", [late])
    # shapes: which planted frontend gets which value shape; "retry" needs the
    # L3 frontend of its address in a home of its own
    shape_of = {}
    for name, shapes in (("full", FULL_SHAPES), ("wrap", WRAP_SHAPES), ("shared_a", SHARED_A_SHAPES)):
        for i, s in zip(t.planted[name], shapes):
            shape_of[i] = s
    l3_addrs = []
    for i, s in sorted(shape_of.items()):
        if s == "retry":
            a = int(ai[i])
            if a in l3_addrs:
                continue
            assert t.reserve(int(l3_home[a])), "the L3 frontend of a retry address has no home of its own"
            l3_addrs.append(a)
    # two more L3 frontends, of addresses no retry key has
    for a in range(n_addr):
        if len(l3_addrs) >= 5:
            break
        if a not in l3_addrs and t.reserve(int(l3_home[a])):
            l3_addrs.append(a)
    # near-equal keys: the first retry key's address with a second dport
    near_a = l3_addrs[0]
    c = np.flatnonzero((ai == near_a) & ~t.used)
    c = c[[t.free_home(int(h)) for h in t.home[c[:200]]].index(True)]
    t.reserve(int(t.home[c]))
    t.used[c] = True
    fill = t.fillers(n_fill, rng)
    planted_ix = t.all_planted()
    fes, index_of = [], {}
    names = {i: n for n, v in t.planted.items() for i in v}
    cyc = ("n1", "n2", "n3", "n4")
    for j, i in enumerate(np.concatenate([planted_ix, [c], fill])):
        i = int(i)
        index_of[i] = len(fes)
        fes.append({"addr": addr_of(int(ai[i])), "dport": int(pp[i]), "shape": shape_of.get(i, cyc[j % 4]),
                    "name": names.get(i, "near" if i == int(c) else "fill"), "home": int(t.home[i]), "ai": int(ai[i])})
    for a in l3_addrs:
        fes.append({"addr": addr_of(a), "dport": 0, "shape": "n3" if a % 2 else "n1", "name": "l3",
                    "home": int(l3_home[a]), "ai": a})
    keys, vals, fe_of, nb = _entries(fes, v6, case)
    planted = {n: [index_of[i] for i in v] for n, v in t.planted.items()}
    planted["near"] = [index_of[int(c)]]
    planted["l3"] = list(range(len(fes) - len(l3_addrs), len(fes)))
    absent = [(n, addr_of(int(ai[i])), int(pp[i])) for n, v in t.absent.items() for i in v]
    # false positives: addresses of no frontend whose vip bit some frontend
    # sets, with the L3 key's or an L4 key's home the full home
    used_a = sorted({f["ai"] for f in fes})
    bits = _vip_bits(vbit[used_a])
    m = 1 << 21
    if v6:
        q16 = np.zeros((m, 16), np.uint8)
        q16[:, 0], q16[:, 1] = 0xFD, 0x65
        q16[:, 12:] = np.arange(m).astype(">u4").view(np.uint8).reshape(m, 4)
        qf = fold6_bytes(q16)
        hit = np.flatnonzero(bits[lb6_vip_bit(qf) & np.uint32(VIP_BITS - 1)])
        q_l3 = lb6_hash(qf[hit], 0) & np.uint32(LB_SLOTS - 1)
    else:
        q32 = _be32(0x64800000 + np.arange(m))
        hit = np.flatnonzero(bits[lb_vip_bit(q32) & np.uint32(VIP_BITS - 1)])
        q_l3 = lb_hash(q32[hit], 0) & np.uint32(LB_SLOTS - 1)
    assert len(hit) > 200
    false_pos = []
    F = t.homes["full"]
    for k in hit[q_l3 == F][:3]:
        false_pos.append(("l3_full", q16[k].copy() if v6 else int(q32[k]), 0))
    for k in hit[:4]:
        hh = (lb6_hash(qf[k], ports) if v6 else lb_hash(q32[k], ports)) & np.uint32(LB_SLOTS - 1)
        for p in ports[hh == F][:2]:
            false_pos.append(("l4_full", q16[k].copy() if v6 else int(q32[k]), int(p)))
    for k in hit[4:40]:
        false_pos.append(("any", q16[k].copy() if v6 else int(q32[k]), int(ports[rng.integers(len(ports))])))
    # the second commit: the frontend at offset 3 of the full home goes, a new one arrives at the wrap
    gone = planted["full"][3]
    dele = fe_of == gone
    new = {"addr": None, "dport": None, "shape": "n2", "name": "wrap_new", "home": t.homes["wrap"]}
    i = t.absent["wrap"][0]
    new["addr"], new["dport"], new["ai"] = addr_of(int(ai[i])), int(pp[i]), int(ai[i])
    k2, v2, _, _ = _entries([new], v6, case, first_backend=nb)
    keys2 = np.concatenate([keys[dele], k2])
    vals2 = np.concatenate([vals[dele], v2])
    del2 = np.concatenate([np.ones(dele.sum(), np.uint8), np.zeros(len(k2), np.uint8)])
    return SvcCase(v6, fes, keys, vals, fe_of, dict(t.homes), planted, absent, false_pos, keys2, vals2, del2,
                   {"gone": gone, "new": new, "vip_bits": bits})


@functools.lru_cache(None)
def lb4_case():
    return _svc_case(False, 0x1B4, 560)


@functools.lru_cache(None)
def lb6_case():
    return _svc_case(True, 0x1B6, 560)


def _svc_overfull(v6):
    """nine frontends of one home at 64 slots (n1 each)"""
    case = CC.policy_hops()
    ports = _be16(np.arange(1, 65536)).astype(np.uint32)
    if v6:
        a = np.zeros(16, np.uint8)
        a[:2], a[15] = (0xFD, 0x66), 9
        h32 = lb6_hash(np.repeat(fold6_bytes(a[None]), len(ports)), ports)
        rank = _be16(ports).astype(np.int64)
    else:
        a = int(_be32(0x64C00009))
        h32 = lb_hash(np.full(len(ports), a, np.uint32), ports)
        rank = ports.astype(np.int64)
    ix, home = overfull_pick(h32, rank)
    fes = [{"addr": a, "dport": int(ports[i]), "shape": "n1", "name": "nine", "home": int(h32[i] & 127), "ai": 0}
           for i in ix]
    keys, vals, fe_of, _ = _entries(fes, v6, case)
    return SvcCase(v6, fes, keys, vals, fe_of, {"nine": home}, {"nine": list(range(9))}, [], [])


@functools.lru_cache(None)
def lb4_overfull():
    return _svc_overfull(False)


@functools.lru_cache(None)
def lb6_overfull():
    return _svc_overfull(True)


# ---- service batches -------------------------------------------------------
def _aim(base, rows, addr, dport, proto, hashes, v6):
    """rows of the base batch again, as egress tuples aimed at {addr, dport}"""
    b = {k: v[rows].copy() for k, v in base.items()}
    n = len(rows)
    b["daddr"] = np.tile(np.asarray(addr, np.uint8), (n, 1)) if v6 else np.full(n, addr, np.uint32)
    b["dport"] = np.full(n, dport, np.uint16)
    b["proto"] = np.asarray(proto, np.uint8)
    b["l4b"] = CC._l4b(b["proto"])
    b["flags"] = np.ones(n, np.uint8)
    b["hash"] = np.asarray(hashes, np.uint32)
    return b


GATED = 47   # a protocol the conntrack gate refuses (ct_proto_gate = 1)


def svc_probes(c: SvcCase, per_fe=8, seed=0, src=0):
    """(batch of probe tuples, target column): per frontend `per_fe` tuples with
    hash 0, 1, .. (so every slave 1..count is selected, and slaves past
    nslaves), TCP and UDP, one ICMP / ICMPv6 and one gated protocol; the absent
    keys and the false-positive addresses four times each.  The target of a
    tuple: the frontend's index, -1 - i for absent key i, -1000 - i for false
    positive i.  Other columns come from the policy batch, the source address
    and port unique per tuple."""
    w = CC.policy_workload()
    base = w.batch6 if c.v6 else w.batch4
    rng = np.random.Generator(np.random.PCG64(0x5C + seed + len(c.fe)))
    icmp = 58 if c.v6 else 1
    ok = np.flatnonzero(np.isin(base["proto"], (6, 17)) & ((base["flags"] & 2) == 0))
    parts, target, at = [], [], 0

    def rows(n):
        nonlocal at
        r = ok[(at + np.arange(n)) % len(ok)]
        at += n
        return r
    some_port = int(L.htons(4242))
    for i, f in enumerate(c.fe):
        planted = f["name"] != "fill"
        n = per_fe if planted else 3
        proto = np.array([6, 17] * (n // 2) + [6] * (n % 2), np.uint8)
        dport = f["dport"] if f["dport"] else some_port
        parts.append(_aim(base, rows(n), f["addr"], dport, proto, np.arange(n), c.v6))
        target += [i] * n
        if planted:   # ICMP goes to the L3 key alone, the gated protocol is refused after the lookup
            parts.append(_aim(base, rows(2), f["addr"], dport, [icmp, GATED], [3, 4], c.v6))
            target += [i] * 2
    for i, (_, a, p) in enumerate(c.absent):
        parts.append(_aim(base, rows(4), a, p, [6, 17, 6, 17], rng.integers(0, 1 << 32, 4), c.v6))
        target += [-1 - i] * 4
    for i, (_, a, p) in enumerate(c.false_pos):
        parts.append(_aim(base, rows(4), a, p if p else some_port, [6, 17, icmp, 6], rng.integers(0, 1 << 32, 4), c.v6))
        target += [-1000 - i] * 4
    b = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    n = len(target)
    # no 5-tuple twice: a source address and port of its own per tuple
    b["sport"] = _be16(1024 + np.arange(n) % 60000)
    b["saddr"] = CC._unique6(n, (1 << 25) + src) if c.v6 else _be32(0xC6140000 + src + np.arange(n))
    target = np.array(target, np.int64)
    if not c.v6:
        # loopback: the source is the backend the tuple is sent to (n1: always slave 1)
        for i, f in enumerate(c.fe):
            if f["shape"] == "n1" and f["name"] != "fill":
                j = np.flatnonzero((target == i) & (b["proto"] == 6))[:1]
                b["saddr"][j] = f["backends"][1][0]
    return b, target


@functools.lru_cache(None)
def svc_batch(v6):
    """the probes shuffled between policy tuples: <= 40,000, len % 4 != 0;
    (batch, target column with -1 << 40 for a policy tuple)"""
    c = lb6_case() if v6 else lb4_case()
    w = CC.policy_workload()
    base = w.batch6 if v6 else w.batch4
    p, target = svc_probes(c)
    n = min(39_999, len(target) + 20_000)
    n -= n % 4 == 0
    m = n - len(target)
    assert m > 5000
    rng = np.random.Generator(np.random.PCG64(0x5D + v6))
    b = {k: np.concatenate([p[k], base[k][:m]]) for k in p}
    target = np.concatenate([target, np.full(m, -1 << 40, np.int64)])
    perm = rng.permutation(n)
    return {k: np.ascontiguousarray(v[perm]) for k, v in b.items()}, target[perm]


@functools.lru_cache(None)
def svc_ct_batches(v6):
    """the stateful paths: three batches of <= 8,000 packets on one map.  The
    first opens a connection per probe of the planted frontends; the second is
    the first again (the CT_SERVICE entries name the slave: lb4_lookup_slave /
    lb6_lookup_slave read its row); the third repeats half of them between new
    connections."""
    c = lb6_case() if v6 else lb4_case()
    p, target = svc_probes(c, seed=1)
    q, _ = svc_probes(c, seed=2, src=1 << 15)   # the same probes from other sources: new connections
    n1 = min(7999, len(target))
    n1 -= n1 % 4 == 0
    b1 = {k: v[:n1] for k, v in p.items()}
    b3 = {k: np.concatenate([v[:n1:2], q[k][1:n1:2]]) for k, v in p.items()}
    n3 = len(b3["flags"]) - (len(b3["flags"]) % 4 == 0)
    return b1, b1, {k: v[:n3] for k, v in b3.items()}


# stored slaves of the pre-installed CT_SERVICE entries, by the L4 probe of a
# frontend they belong to (hash 0, 1, ..): slave 0 (lb4_lookup_slave reads the
# master's own entry), one past every frontend's slaves, slave 2 (a row, the
# hole of slow_hole, or past n1's), slave 0 with lb_loopback, slave 1
PRE_SLAVES = ((0, 0), (40, 0), (2, 0), (0, L.CTB_LB_LOOPBACK), (1, 0))


@functools.lru_cache(None)
def svc_ct_preinstall(v6):
    """CT_SERVICE entries that are in the map before the first stateful batch:
    (keys, vals, rows, fe, slave) -- for every planted frontend that is not in
    its home slot by construction (offsets 1..7 of the full home, the wrapping
    home, the shared home's a-keys) and for the L3 frontends, the service
    tuples (ct_lookup4 / ct_lookup6 with CT_SERVICE: dport <- the L4 sport) of
    its first TCP / UDP probes of batch 1, with the stored slaves PRE_SLAVES.
    No packet of the batches can store slave 0 (a selected slave is >= 1).
    rows: the probe's index in batch 1; fe: the frontend it is aimed at."""
    c = lb6_case() if v6 else lb4_case()
    b1 = svc_ct_batches(v6)[0]
    _, target = svc_probes(c, seed=1)
    target = target[:len(b1["flags"])]
    who = c.planted["full"][1:] + c.planted["wrap"] + c.planted["shared_a"] + c.planted["l3"]
    rows, fe, ent = [], [], []
    for i in who:
        mine = np.flatnonzero((target == i) & np.isin(b1["proto"], (6, 17)))
        assert len(mine) >= len(PRE_SLAVES) and b1["hash"][mine[0]] == 0
        for r, e in zip(mine, PRE_SLAVES):
            rows.append(int(r))
            fe.append(i)
            ent.append(e)
    rows = np.array(rows)
    m = len(rows)
    k = np.zeros(m, L.CT6_TUPLE if v6 else L.CT4_TUPLE)
    k["daddr"], k["saddr"] = b1["daddr"][rows], b1["saddr"][rows]
    k["dport"], k["sport"] = b1["sport"][rows], b1["dport"][rows]
    k["nexthdr"], k["flags"] = b1["proto"][rows], 4   # TUPLE_F_SERVICE
    v = np.zeros(m, L.CT_ENTRY)
    v["slave"] = [s for s, _ in ent]
    v["bits"] = [x for _, x in ent]
    v["lifetime"] = 5000
    v["rev_nat_index"] = 1 + np.arange(m) % 7
    v["tx_packets"], v["tx_bytes"] = 3, 300
    return k, v, rows, np.array(fe), v["slave"].copy()


def load_ct_preinstall(t, v6):
    """into an Engine (after its commit) or an Oracle"""
    k, v = svc_ct_preinstall(v6)[:2]
    up = t.ct6_update if v6 else t.ct4_update
    for a, b in zip(k, v):
        assert up(a, b) == 0


# --------------------------------------------------------------------------
# forwarding
# --------------------------------------------------------------------------
@dataclass
class FwdCase:
    w: FF.FrameWorld
    homes: dict       # table -> {name: home}
    planted: dict     # table -> {name: [raw 20-byte keys], in insertion order}
    absent: dict      # table -> [(name, raw 20-byte key)] at planted homes, not installed
    slots: dict       # table -> slots asserted through the hook
    info: dict = field(default_factory=dict)


ROUTER6 = FC.ip6("fd00:0:0:0:0:1::")   # the /96 of every e6 candidate (the netdev's gate)


def _k4(raw32):
    return FC.key4(int(raw32))


def _e6_addr(w3):
    return ROUTER6[:12] + int(w3).to_bytes(4, "big")


def _t6_addr(v):
    return bytes([0xFD, 0x10, 0, 0, 0, 0, 0, 0]) + int(v).to_bytes(4, "big") + bytes(4)


def _fwd_cands(rng):
    """the four candidate pools: (Cands, key-of-candidate function)"""
    # e4: 10.1.0.0/16 and 10.2.0.0/16; the 20 key bytes ascend with the host-order address
    h = (0x0A010000 + np.arange(1 << 17)).astype(np.uint32)
    e4 = Cands(EP_SLOTS, fwd_hash4(_be32(h)), h.astype(np.int64))
    # t4: every /16 but 10.1 and 10.2 (tunnel->ip4 of daddr & 0xFFFF)
    p = np.setdiff1d(np.arange(1, 1 << 16), [0x0A01, 0x0A02]).astype(np.uint32)
    t4raw = _be32(p << np.uint32(16))
    t4 = Cands(TUN_SLOTS, fwd_hash4(t4raw), p.astype(np.int64))
    # e6: fd00::1:0:0/96, word 3 = 1 .. 2^17
    v = np.arange(1, (1 << 17) + 1)
    a = np.frombuffer(b"".join(_e6_addr(x) for x in v), np.uint8).reshape(-1, 16)
    e6 = Cands(EP_SLOTS, fold6_bytes(a), v.astype(np.int64))
    # t6: fd10:0:0:0:xxxx:xxxx::/96
    u = np.arange(1, (1 << 16) + 1)
    a = np.frombuffer(b"".join(_t6_addr(x) for x in u), np.uint8).reshape(-1, 16)
    t6 = Cands(TUN_SLOTS, fold6_bytes(a, 3), u.astype(np.int64))
    keyf = {"e4": lambda i: _k4(_be32(h[i])), "t4": lambda i: _k4(t4raw[i]),
            "e6": lambda i: FC.key6(_e6_addr(v[i])), "t6": lambda i: FC.key6(_t6_addr(u[i]))}
    return {"e4": e4, "t4": t4, "e6": e6, "t6": t6}, keyf


@functools.lru_cache(None)
def fwd_case():
    rng = np.random.Generator(np.random.PCG64(0xF3D))
    tabs, keyf = _fwd_cands(rng)
    w = FC.World(host_ifindex=11, encap_ifindex=22, cluster_mask=0, cluster_range=0, router_ip=ROUTER6[:12] + bytes(4))
    homes, planted, absent, order = {}, {}, {}, {}
    zero4 = int(fwd_hash4(0))
    for name, t in tabs.items():
        extra = []
        if name in ("e4", "t4"):
            # key 0 (0.0.0.0 / the prefix 0.0) with three more keys at its home
            z = zero4 & t.mask
            assert t.z.claim(z, 4)
            t.homes["zero"] = z
            c = t.at(z)
            assert len(c) >= 5
            t.take("zero", c[:3])
            t.leave("zero", c[3:5])
            extra.append(("zero", _k4(0)))
        plant_common(t)
        if name == "t6":
            # a tunnel key whose /96 is the e6 addresses' (and the netdev's gate)
            hh = int(fold6_bytes(np.frombuffer(ROUTER6, np.uint8), 3)[0]) & t.mask
            assert t.reserve(hh)
            extra.append(("router96", FC.key6(ROUTER6)))
        n_fill = {"e4": 300, "e6": 300, "t4": 170, "t6": 170}[name]
        fill = t.fillers(n_fill, rng)
        homes[name] = dict(t.homes)
        planted[name] = {n: [keyf[name](i) for i in v] for n, v in t.planted.items()}
        for n, k in extra:
            planted[name].setdefault(n, []).insert(0, k)
        planted[name]["fill"] = [keyf[name](int(i)) for i in fill]
        absent[name] = [(n, keyf[name](i)) for n, v in t.absent.items() for i in v]
    # values: a distinct (ifindex, lxc_id) per endpoint; every fourth planted
    # endpoint past the first of its home is the host; a distinct node per tunnel key
    j = 0
    for name in ("e4", "e6"):
        for n, ks in planted[name].items():
            for i, k in enumerate(ks):
                j += 1
                host = n != "fill" and i % 4 == 2
                w.eps[k] = (0, 0, FC.ENDPOINT_F_HOST) if host else (100 + j, j, 0)
    for name in ("t4", "t6"):
        for n, ks in planted[name].items():
            for k in ks:
                j += 1
                w.tun[k] = FC.key4(int(_be32(0xC0A80000 + j)))
    fw = FF.frame_world(w)
    slots = {"e4": EP_SLOTS, "e6": EP_SLOTS, "t4": TUN_SLOTS, "t6": TUN_SLOTS}
    return FwdCase(fw, homes, planted, absent, slots)


@functools.lru_cache(None)
def fwd_overfull():
    """nine keys of one home at 64 slots in each of the four tables; key 0 is
    absent from e4 and t4, three keys sit at its home (at 128 slots)"""
    rng = np.random.Generator(np.random.PCG64(0xF3E))
    tabs, keyf = _fwd_cands(rng)
    w = FC.World(host_ifindex=11, encap_ifindex=22, cluster_mask=0, cluster_range=0, router_ip=ROUTER6[:12] + bytes(4))
    homes, planted, absent = {}, {}, {}
    z = int(fwd_hash4(0)) & (SMALL_SLOTS - 1)
    j = 0
    for name, t in tabs.items():
        four = name in ("e4", "t4")
        ix, home = overfull_pick(t.hash32, t.rank, z if four else None)
        homes[name] = {"nine": home}
        planted[name] = {"nine": [keyf[name](int(i)) for i in ix[:9]]}
        absent[name] = []
        if four:
            homes[name]["zero"] = z
            planted[name]["zero"] = [keyf[name](int(i)) for i in ix[9:]]
            absent[name].append(("zero", _k4(0)))
        for ks in planted[name].values():
            for k in ks:
                j += 1
                if name[0] == "e":
                    w.eps[k] = (100 + j, j, 0)
                else:
                    w.tun[k] = FC.key4(int(_be32(0xC0A80000 + j)))
    return FwdCase(FF.frame_world(w), homes, planted, absent, {k: SMALL_SLOTS for k in tabs})


def fwd_second_commit(c: FwdCase):
    """(deleted keys, {added key: value}) per table: the key at offset 3 of the
    full home goes, an absent key of the wrap home arrives"""
    dele = {t: c.planted[t]["full"][3] for t in ("e4", "e6", "t4", "t6")}
    add = {t: [k for n, k in c.absent[t] if n == "wrap"][0] for t in ("e4", "e6", "t4", "t6")}
    return dele, add


def fwd_world2(c: FwdCase) -> FF.FrameWorld:
    """the world after the second commit"""
    w = c.w
    w2 = FF.FrameWorld(**{k: (dict(getattr(w, k)) if isinstance(getattr(w, k), dict) else getattr(w, k))
                          for k in FF.FrameWorld.__dataclass_fields__})
    dele, add = fwd_second_commit(c)
    for t in ("e4", "e6"):
        del w2.eps[dele[t]]
        w2.macs.pop(dele[t], None)
        w2.eps[add[t]] = (900 + len(t), 60_000 + (t == "e6"), 0)
        w2.macs[add[t]] = (0x4D00_0000_0902 + (t == "e6"), 0x4E00_0000_0906 + (t == "e6"))
    for t in ("t4", "t6"):
        del w2.tun[dele[t]]
        w2.tun[add[t]] = FC.key4(int(_be32(0xC0A8FF01 + (t == "t6"))))
    return w2


def _daddr_of(table, key, rng, w):
    """a destination that looks the key up: the endpoint's address, or an
    address of the tunnel prefix that is no endpoint"""
    if table == "e4":
        return key[:4]
    if table == "e6":
        return key[:16]
    while True:
        if table == "t4":
            d = key[:2] + bytes(rng.integers(1, 255, 2, dtype=np.uint8))
            if FC.key4(int.from_bytes(d, "little")) not in w.eps:
                return d
        else:
            d = key[:12] + bytes(rng.integers(1, 255, 4, dtype=np.uint8))
            if FC.key6(d) not in w.eps:
                return d


@functools.lru_cache(None)
def fwd_batch(v6, small=False):
    """forward_cases.build_batch's columns over the crafted world: every
    planted and absent key (and a sample of the others) is the destination of
    six packets, the first of them plain (verdict 0, no tunnel word, egress,
    ttl 64: the tables decide it), the others with drawn verdicts, tunnel
    words, flags and ttl 0 / 1 / 2 / 64; (columns, per packet (table, key))"""
    c = fwd_overfull() if small else fwd_case()
    rng = np.random.Generator(np.random.PCG64(0xFB + v6 + 2 * small))
    e, t = ("e6", "t6") if v6 else ("e4", "t4")
    aims = []
    for tab in (e, t):
        for n, ks in c.planted[tab].items():
            for k in (ks if n != "fill" else ks[:60]):
                aims.append((tab, k))
        for n, k in c.absent[tab]:
            aims.append((tab, k))
    if v6 and not small:
        # word 3 alone differs from an endpoint; the /96 of the e6 addresses outside every endpoint
        aims += [("e6", FC.key6(k[:15] + bytes([k[15] ^ 1]))) for k in c.planted["e6"]["full"][:4]]
    per = 6
    who, daddr = [], []
    for tab, k in aims:
        for _ in range(per):
            who.append((tab, k))
            daddr.append(_daddr_of(tab, k, rng, c.w))
    n = len(who)
    first = np.arange(n) % per == 0
    vr = rng.integers(0, 10, n)
    verdict = np.where(first | (vr < 6), 0, np.where(vr == 6, FC.DROP_POLICY, np.where(
        vr == 7, FC.VERDICT_XDP_DROP, rng.integers(1, 65536, n)))).astype(np.int32)
    tunnel = np.where(~first & (rng.integers(0, 4, n) == 0), rng.integers(1, 2 ** 32, n), 0).astype(np.uint32)
    flags = (first | (rng.integers(0, 5, n) != 0)).astype(np.uint8)
    ttl = np.where(first, 64, rng.choice(np.array([0, 1, 2, 64], np.uint8), n)).astype(np.uint8)
    perm = rng.permutation(n)
    perm = perm[:n - (n % 4 == 0)]
    d = np.frombuffer(b"".join(daddr), np.uint8).reshape(n, 16 if v6 else 4)[perm]
    cols = dict(daddr=np.ascontiguousarray(d) if v6 else np.ascontiguousarray(d).view(np.uint32).reshape(-1),
                verdict=verdict[perm], tunnel=tunnel[perm], flags=flags[perm], ttl=ttl[perm])
    return cols, [who[i] for i in perm]
