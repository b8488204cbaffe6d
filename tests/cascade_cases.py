"""Crafted policy / group tables and IPv4 ipcache shapes, shared by the CPU
shape test (test_cascade_shapes.py) and the device cascades
(test_gpu_cascade_shapes.py).  Plain numpy with fixed PCG64 seeds; nothing
here asks the library anything: the keys are found with mirrors of the
tables.h hashes, and what the builders made of them is asserted through the
test hooks on the CPU.

policy_hops(): 3 endpoints, 513..1023 keys (an 8192-slot key table, a 512-slot
group table), with planted neighbourhoods (a home slot and the keys that hash
to it).  A planted neighbourhood is isolated: no other installed key has its
home within 8 slots of it on either side, circularly, so first fit alone
places its keys.  Where two planted homes share a neighbourhood on purpose
("bc", "e", "f"), the later home's keys sit in a higher endpoint: a full
build inserts endpoint by endpoint.

lpm4_full_dict(): more uniform /16s with distinct labels than the leaf
dictionary has codes, and every /16- and byte-level shape of tables.h lpm16c,
with and without dictionary codes for their leaves.

Expected answers come from the restatement (oracle), never from the library.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from cilium_amd import layouts as L

N_EP = 3
POL_SLOTS = 1 << 13   # asserted through cgpu_diag_pol_tables
PG_SLOTS = 1 << 9
HOP = 8               # tables.h POL_HOP
MARGIN = 8            # no foreign home this close to a planted neighbourhood


# --------------------------------------------------------------------------
# tables.h hashes, vectorised
# --------------------------------------------------------------------------
def _u64(x):
    return np.asarray(x).astype(np.uint64)


def mix32(a, b):
    """tables.h mix32"""
    with np.errstate(over="ignore"):
        h = ((_u64(b) << np.uint64(32)) | _u64(a)) * np.uint64(0x9E3779B97F4A7C15)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xbf58476d1ce4e5b9)
        h ^= h >> np.uint64(32)
    return (h & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def pol_hash(lo, hi, ep):
    """tables.h pol_hash"""
    with np.errstate(over="ignore"):
        h = ((_u64(hi) << np.uint64(32)) | _u64(lo)) ^ (_u64(ep) * np.uint64(0x9E3779B97F4A7C15))
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xff51afd7ed558ccd)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xc4ceb9fe1a85ec53)
        h ^= h >> np.uint64(33)
    return (h & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def pg_hash(ident, ep_dir):
    """tables.h pg_hash; ep_dir = ep | egress << 16"""
    return mix32(ident, _u64(ep_dir).astype(np.uint32) ^ np.uint32(0x6a09e667))


def pg_bloom(dport, proto):
    """tables.h pg_bloom: the two bits of a (network-order dport, proto) pair"""
    h = mix32(_u64(dport).astype(np.uint32) | (_u64(proto).astype(np.uint32) << np.uint32(16)), 0x3c6ef372)
    return (np.uint32(1) << (h & np.uint32(31))) | (np.uint32(1) << ((h >> np.uint32(8)) & np.uint32(31)))


def key_hi(dport_be, proto, egress):
    """the policy key's upper word as the table stores it (egress: the whole
    egress_pad byte)"""
    return _u64(dport_be).astype(np.uint32) | (_u64(proto).astype(np.uint32) << np.uint32(16)) | \
        (_u64(egress).astype(np.uint32) << np.uint32(24))


# --------------------------------------------------------------------------
# policy_hops
# --------------------------------------------------------------------------
# a policy key with its endpoint: dport as stored (network order read as a
# little-endian u16), egr the whole egress_pad byte (bit 0 direction)
KEY = np.dtype([("ep", "u4"), ("id", "u4"), ("dport", "u4"), ("proto", "u4"), ("egr", "u4")])
# a probe tuple before it gets addresses
TUP = np.dtype([("ep", "u4"), ("id", "u4"), ("dport", "u4"), ("proto", "u4"), ("dir", "u4"),
                ("frag", "u4"), ("len", "u4")])


def keys_of(ep, ident, dport, proto, egr):
    b = np.broadcast_arrays(ep, ident, dport, proto, egr)
    k = np.zeros(b[0].shape, KEY)
    for f, v in zip(KEY.names, b):
        k[f] = v
    return k.reshape(-1)


def key_home(k, mask=POL_SLOTS - 1, ep=None):
    return pol_hash(k["id"], key_hi(k["dport"], k["proto"], k["egr"]), k["ep"] if ep is None else ep) & np.uint32(mask)


def group_home(ident, ep, egress, mask=PG_SLOTS - 1):
    return pg_hash(ident, _u64(ep).astype(np.uint32) | (_u64(egress).astype(np.uint32) << np.uint32(16))) & np.uint32(mask)


class _Zones:
    """homes of a circular table claimed by planted neighbourhoods"""

    def __init__(self, slots, fixed=()):
        self.slots = slots
        self.taken = np.zeros(slots, bool)
        self.fixed = np.zeros(slots, bool)  # homes of keys that cannot move
        self.fixed[np.asarray(list(fixed), np.int64)] = True

    def span(self, home, width):
        return (home + np.arange(-MARGIN, width + MARGIN)) & (self.slots - 1)

    def claim(self, home, width):
        s = self.span(int(home), width)
        if self.taken[s].any() or self.fixed[s].any():
            return False
        self.taken[s] = True
        return True

    def scan(self, start, width):
        for h in range(start, self.slots - 64):
            if self.claim(h, width):
                return h
        raise AssertionError("no room for a planted neighbourhood")

    def free(self, homes):
        return ~self.taken[np.asarray(homes, np.int64)]


@dataclass
class PolicyCase:
    ids: np.ndarray          # identities of the ipcache: index i has 30.(i >> 8).(i & 255).0/24 and a /64
    keys1: np.ndarray        # KEY rows of the first commit ...
    proxy1: np.ndarray       # ... and their proxy ports (host order), distinct where non-zero
    keys2: np.ndarray        # KEY rows of the second commit
    proxy2: np.ndarray
    del2: np.ndarray         # 1: the row deletes its key
    homes: dict              # name -> planted home slot of the key table
    planted: dict            # name -> indices into keys1 (or, "f_new", into keys2)
    absent: dict             # name -> KEY rows absent from both commits, admitted by their group's bloom
    other_ep: np.ndarray     # KEY rows: the words of an installed key under another endpoint at the same home
    g_homes: dict            # name -> planted home slot of the group table
    g_planted: dict          # name -> (id, ep, egress) rows of installed groups
    g_absent: dict           # name -> (id, ep, egress) rows of absent groups at that home
    tuples: np.ndarray       # TUP rows, len % 4 != 0, <= 40000
    replies: np.ndarray      # KEY rows (egr 0) a conntrack reply is aimed at: planted keys and absent ones
    info: dict = field(default_factory=dict)

    @property
    def pad_key(self):
        return self.planted["g"][-1]

    def keys_after(self, phase):
        """(KEY rows, proxy ports) installed after commit `phase` (1 or 2)"""
        if phase == 1:
            return self.keys1, self.proxy1
        dele = {k.tobytes() for k in self.keys2[self.del2 == 1]}
        keep = np.array([k.tobytes() not in dele for k in self.keys1])
        add = self.del2 == 0
        return np.concatenate([self.keys1[keep], self.keys2[add]]), np.concatenate([self.proxy1[keep], self.proxy2[add]])


def policy_structs(keys, proxy):
    """KEY rows -> (eps u32, POLICY_KEY, POLICY_ENTRY)"""
    pk = np.zeros(len(keys), L.POLICY_KEY)
    pk["sec_label"], pk["dport"], pk["protocol"], pk["egress"] = keys["id"], keys["dport"], keys["proto"], keys["egr"]
    pe = np.zeros(len(keys), L.POLICY_ENTRY)
    pe["proxy_port"] = np.asarray(proxy, np.uint16).byteswap()
    return np.ascontiguousarray(keys["ep"], np.uint32), pk, pe


def _blooms(keys):
    """{(id, ep, dir): bloom} over the groupable keys"""
    out = {}
    ok = keys["egr"] < 2
    for k, b in zip(keys[ok], pg_bloom(keys["dport"][ok], keys["proto"][ok])):
        g = (int(k["id"]), int(k["ep"]), int(k["egr"]))
        out[g] = out.get(g, 0) | int(b)
    return out


def admitted(blooms, k):
    """the bloom of k's group admits its (dport, proto): probe 1 reads the key table"""
    b = pg_bloom(k["dport"], k["proto"])
    g = np.array([blooms.get((int(i), int(e), int(d) & 1), 0) for i, e, d in zip(k["id"], k["ep"], k["egr"])], np.uint32)
    return (g & b) == b


@functools.lru_cache(None)
def policy_hops():
    rng = np.random.Generator(np.random.PCG64(0xCA5C))
    pool = np.unique(np.concatenate([rng.integers(256, 1 << 24, 150_000), rng.integers(1 << 30, 1 << 32, 50_000)])
                     .astype(np.uint32))
    rng.shuffle(pool)
    EDS = [(ep, d) for ep in range(N_EP) for d in (0, 1)]
    ph = np.stack([group_home(pool, ep, d) for ep, d in EDS], 1).astype(np.int64)  # (pool, 6)

    # ---- the group table --------------------------------------------------
    # wildcard (identity 0) keys under every endpoint and direction but one:
    # the group {0, endpoint 0, ingress} would sit at slot 506, inside the
    # neighbourhood that wraps past the last slot
    WILD = [x for x in EDS if x != (0, 0)]
    gz = _Zones(PG_SLOTS, fixed=[int(group_home(0, ep, d)) for ep, d in WILD])
    g_homes, g_planted, g_absent, used_ids = {}, {}, {}, set()

    def groups_at(home, n_inst, n_abs):
        """distinct identities with a group (any endpoint, direction) at `home`"""
        rows = []
        for i, e in zip(*np.nonzero(ph == home)):
            if int(pool[i]) not in used_ids:
                used_ids.add(int(pool[i]))
                rows.append((int(pool[i]),) + EDS[e])
            if len(rows) == n_inst + n_abs:
                break
        assert len(rows) == n_inst + n_abs
        return np.array(rows[:n_inst], np.int64), np.array(rows[n_inst:], np.int64)

    assert gz.claim(PG_SLOTS - 2, 4), "an identity-0 group sits at the end of the group table"
    g_homes["wrap"] = PG_SLOTS - 2
    g_planted["wrap"], g_absent["wrap"] = groups_at(PG_SLOTS - 2, 4, 3)
    g_homes["full"] = gz.scan(40, 8)
    g_planted["full"], g_absent["full"] = groups_at(g_homes["full"], 8, 4)

    def pair(name, a, b, both):
        """an identity whose groups under EDS[a] and EDS[b] share a home; both:
        the two are installed, else the second is the absent one"""
        for i in np.flatnonzero(ph[:, a] == ph[:, b]):
            if int(pool[i]) not in used_ids and gz.claim(ph[i, a], 2):
                used_ids.add(int(pool[i]))
                r = np.array([(int(pool[i]),) + EDS[a], (int(pool[i]),) + EDS[b]], np.int64)
                g_homes[name] = int(ph[i, a])
                g_planted[name], g_absent[name] = (r, r[:0]) if both else (r[:1], r[1:])
                return
        raise AssertionError(name)

    pair("two_eps", EDS.index((0, 1)), EDS.index((1, 1)), True)
    pair("two_dirs", EDS.index((2, 0)), EDS.index((2, 1)), True)
    pair("other_ep", EDS.index((1, 0)), EDS.index((2, 0)), False)
    pair("other_dir", EDS.index((0, 0)), EDS.index((0, 1)), False)

    # fat identities: a group under every endpoint and direction with many
    # keys (a dense bloom), none of them near a planted group home; two of
    # the four are >= 2^30
    okfat = gz.free(ph).all(1) & ~np.isin(pool, list(used_ids))
    fat = np.concatenate([pool[okfat & (pool < 1 << 30)][:2], pool[okfat & (pool >= 1 << 30)][:2]])
    assert len(fat) == 4
    used_ids.update(int(x) for x in fat)
    # filler groups: one identity, one endpoint and direction, one key each
    fill = []
    for i in np.flatnonzero(~np.isin(pool, list(used_ids))):
        e = int(rng.integers(0, 6))
        if gz.free([ph[i, e]])[0]:
            fill.append((int(pool[i]),) + EDS[e])
        if len(fill) == 100:
            break
    fill = np.array(fill, np.int64)

    # ---- the key table ----------------------------------------------------
    mask = POL_SLOTS - 1
    # keys whose words are fixed: the egress L3 key of every fat group (the
    # conntrack batches open connections through them)
    fat_l3 = keys_of(np.repeat(np.arange(N_EP), 4), np.tile(fat, N_EP), 0, 0, 1)
    kz = _Zones(POL_SLOTS, fixed=key_home(fat_l3).astype(np.int64))
    # every exact key a fat group could hold, by home slot
    fg = np.array([(ep, i, d) for ep in range(N_EP) for i in fat for d in (0, 1)], np.int64)
    dports = np.arange(1, 65536, dtype=np.uint32)
    cand = keys_of(np.repeat(fg[:, 0], 2 * len(dports)), np.repeat(fg[:, 1], 2 * len(dports)),
                   np.tile(np.tile(dports, 2), len(fg)), np.tile(np.repeat([6, 17], len(dports)), len(fg)),
                   np.repeat(fg[:, 2], 2 * len(dports)))
    cand = cand[rng.permutation(len(cand))]
    chome = key_home(cand).astype(np.int64)
    order = np.argsort(chome, kind="stable")
    first = np.searchsorted(chome[order], np.arange(POL_SLOTS + 1))
    taken = np.zeros(len(cand), bool)

    def at_home(h, ep=None, egr=None):
        """indices of the unused candidates of home h"""
        ix = order[first[h & mask]:first[(h & mask) + 1]]
        ix = ix[~taken[ix]]
        if ep is not None:
            ix = ix[np.isin(cand["ep"][ix], ep)]
        if egr is not None:
            ix = ix[cand["egr"][ix] == egr]
        return ix

    homes, plant = {}, {}

    def take(name, h, n, ep=None, egr=None):
        ix = at_home(h, ep, egr)[:n]
        assert len(ix) == n, (name, h, len(ix))
        taken[ix] = True
        plant.setdefault(name, []).extend(ix.tolist())

    # (b) + (c): home mask - 3 with 8 keys (slots mask - 3 .. mask, 0 .. 3), then
    # home mask with 2 keys of a higher endpoint
    assert kz.claim(mask - 3, 10), "a fat group's L3 key sits at the end of the key table"
    homes["b"], homes["c"] = mask - 3, mask
    take("b", mask - 3, 8, ep=[0])
    take("c", mask, 2, ep=[1, 2])
    # (d2): the words of one key under two endpoints at one home
    oth = None
    for s in (1, 2):
        ep2 = (cand["ep"] + s) % N_EP
        for i in np.flatnonzero(key_home(cand, ep=ep2) == chome):
            if kz.claim(chome[i], 2):
                oth = (int(i), int(ep2[i]))
                break
        if oth:
            break
    assert oth
    homes["d2"] = int(chome[oth[0]])
    taken[oth[0]] = True
    plant["d2"] = [oth[0]]
    take("d2", homes["d2"], 1)
    other_ep = cand[[oth[0]]].copy()
    other_ep["ep"] = oth[1]
    # (a) a full home; (x) a full home that loses a key in the second commit;
    # (d) 3 and 4 keys; (g) 2 keys and a key with pad bits
    # (a)'s keys are all ingress keys: whatever the order they are placed in,
    # the one at displacement 7 can be the target of a conntrack reply
    for name, n, start in (("a", 8, 500), ("x", 8, 1500), ("d3", 3, 2500), ("d4", 4, 3000)):
        homes[name] = kz.scan(start, n)
        take(name, homes[name], n, egr=0 if name == "a" else None)
    homes["g"] = kz.scan(3500, 3)
    take("g", homes["g"], 2)
    # (e) home h with 2 keys, then home h + 1 with a key of a higher endpoint:
    # it sits at h + 2, and its home slot holds a key of home h
    homes["e"] = kz.scan(4000, 3)
    take("e", homes["e"], 2, ep=[0])
    take("e", homes["e"] + 1, 1, ep=[2])
    # (f) 8 keys at h and one at h + 8; the second commit adds one of home
    # h + 1: h + 1 .. h + 8 are taken, the key at h + 8 moves to h + 9
    homes["f"] = kz.scan(5000, 10)
    take("f", homes["f"], 8)
    take("f", homes["f"] + 8, 1)
    take("f_new", homes["f"] + 1, 1)

    # the key with pad bits: hashed with its pad bits, so searched for
    g_src = cand[plant["g"][0]]
    pk = keys_of(g_src["ep"], g_src["id"], dports, 6, int(g_src["egr"]) | (5 << 1))
    pk = pk[key_home(pk) == homes["g"]][:1]
    assert len(pk) == 1

    def elsewhere(k):
        """the rows of k whose home is outside every planted neighbourhood"""
        return k[kz.free(key_home(k))]

    filler = [elsewhere(fat_l3)]
    assert len(filler[0]) == len(fat_l3)
    for ep, i, d in fg:                       # 18 exact keys per fat group; an ingress L3 key for half of them
        ix = np.flatnonzero((cand["ep"] == ep) & (cand["id"] == i) & (cand["egr"] == d) & ~taken)
        ix = ix[kz.free(chome[ix])][:18]
        taken[ix] = True
        filler.append(cand[ix])
        if d == 0 and (ep + int(i)) % 2:
            filler.append(elsewhere(keys_of(ep, i, 0, 0, 0)))
    wild = []                                 # 10 wildcard (identity 0) keys per endpoint and direction
    for ep, d in WILD:
        w = keys_of(ep, 0, rng.permutation(dports)[:200], rng.choice([6, 17], 200), d)
        wild.append(elsewhere(w)[:10])
    filler += wild
    small = np.concatenate([g_planted[k] for k in sorted(g_planted)] + [fill])
    no_l3 = []
    for j, (i, ep, d) in enumerate(small):    # planted and filler groups: an L3 key or one exact key
        k = elsewhere(keys_of(ep, i, 0, 0, d)) if j % 2 == 0 else []
        if len(k) == 0:
            port = np.array([L.htons(int(p)) for p in rng.permutation([80, 443, 53, 8080, 22, 25])], np.uint32)
            k = elsewhere(keys_of(ep, i, port, 6, d))[:1]
            no_l3.append((int(i), int(ep), int(d)))
        filler.append(k)
    filler = np.concatenate(filler)

    order1 = [n for n in ("a", "b", "c", "d2", "d3", "d4", "e", "f", "g", "x")]
    idx, pos = {}, 0
    rows = []
    for n in order1:
        k = cand[plant[n]]
        if n == "g":
            k = np.concatenate([k, pk])
        idx[n] = np.arange(pos, pos + len(k))
        pos += len(k)
        rows.append(k)
    keys1 = np.concatenate(rows + [filler])
    assert len(np.unique(keys1)) == len(keys1) and 513 <= len(keys1) <= 1023
    # distinct proxy ports, zero for every fourth key
    proxy1 = np.where(np.arange(len(keys1)) % 4 == 3, 0, 1024 + np.arange(len(keys1))).astype(np.uint16)

    # second commit: a key of home f + 1 (relocates the key at f + 8), and the
    # fourth key of x in build order (endpoint, then the key as a u64) goes
    xk = keys1[idx["x"]]
    xo = np.lexsort((xk["id"], key_hi(xk["dport"], xk["proto"], xk["egr"]), xk["ep"]))
    keys2 = np.concatenate([cand[plant["f_new"]], xk[xo[3:4]]])
    proxy2 = np.array([3001, 0], np.uint16)
    del2 = np.array([0, 1], np.uint8)
    idx["f_new"] = np.array([0])
    idx["x_del"] = idx["x"][xo[3:4]]

    # absent keys at the planted homes that the blooms admit.  The deleted
    # key's bits stay in a patched table, so it is admitted after the delete.
    blooms = _blooms(np.concatenate([keys1, keys2]))
    absent = {}
    for n, h in homes.items():
        a = cand[at_home(h)]
        a = a[admitted(blooms, a)]
        a = np.concatenate([a[a["egr"] == 0][:6], a[a["egr"] == 1][:6]])
        assert (a["egr"] == 0).sum() >= 2 and (a["egr"] == 1).sum() >= 2, (n, len(a))
        absent[n] = a
    # the other endpoint must reach the key table with those words: give its
    # group a key with the same two bloom bits if it has none yet
    if not admitted(blooms, other_ep)[0]:
        want = pg_bloom(other_ep["dport"], other_ep["proto"])[0]
        h = keys_of(other_ep["ep"][0], other_ep["id"][0], np.tile(dports, 2), np.repeat([6, 17], len(dports)),
                    other_ep["egr"][0])
        h = elsewhere(h[pg_bloom(h["dport"], h["proto"]) == want])
        have = {k.tobytes() for k in np.concatenate([keys1, keys2, other_ep])}
        h = h[[k.tobytes() not in have for k in h]][:1]
        assert len(h) == 1
        keys1 = np.concatenate([keys1, h])
        proxy1 = np.concatenate([proxy1, [2999]]).astype(np.uint16)
        blooms = _blooms(np.concatenate([keys1, keys2]))
    assert admitted(blooms, other_ep)[0]

    # ---- identities of the ipcache: every group's, installed or absent -----
    ids = [int(x) for x in fat]
    for d_ in (g_planted, g_absent):
        for k in sorted(d_):
            ids += [int(r[0]) for r in d_[k]]
    ids += [int(r[0]) for r in fill]
    ids = np.array(sorted(set(ids)), np.uint32)

    # ---- probe tuples -----------------------------------------------------
    def tup(k, frag=0, ln=None, reps=1):
        k = np.repeat(np.atleast_1d(k), reps)
        t = np.zeros(len(k), TUP)
        t["ep"], t["id"], t["dport"], t["proto"], t["dir"] = k["ep"], k["id"], k["dport"], k["proto"], k["egr"] & 1
        t["frag"] = frag
        t["len"] = rng.integers(64, 1501, len(k)) if ln is None else ln
        return t

    def grp_tup(rows, reps):
        """tuples of groups (id, ep, dir): TCP / UDP at a few ports"""
        rows = np.repeat(np.asarray(rows, np.int64).reshape(-1, 3), reps, 0)
        port = np.array([L.htons(p) for p in (80, 443, 53)], np.uint32)
        return tup(keys_of(rows[:, 1], rows[:, 0], rng.choice(port, len(rows)), rng.choice([6, 17], len(rows)),
                           rows[:, 2]))

    inst = np.concatenate([keys1, cand[plant["f_new"]]])
    inst = inst[inst["egr"] < 2]
    l3 = inst[(inst["dport"] == 0) & (inst["proto"] == 0) & (inst["id"] != 0)]
    exact = inst[(inst["dport"] != 0) & (inst["id"] != 0)]
    wildk = inst[inst["id"] == 0]
    parts = [tup(exact, reps=12)]                                            # probe-1 hits, the deleted key too
    parts += [tup(a, reps=16) for a in absent.values()]                      # absent, admitted, planted homes
    parts.append(tup(other_ep, reps=40))                                    # the same words, another endpoint
    m = 4 * len(l3)                                                         # probe 2: the group's L3 key
    parts.append(tup(keys_of(np.repeat(l3["ep"], 4), np.repeat(l3["id"], 4), rng.integers(1, 65536, m),
                             rng.choice([6, 17], m), np.repeat(l3["egr"], 4))))
    nl = np.array(no_l3, np.int64)                                          # probe 3: groups without an L3 key
    for w in wildk:
        g = nl[(nl[:, 1] == w["ep"]) & (nl[:, 2] == w["egr"])][:6]
        parts.append(tup(keys_of(w["ep"], g[:, 0], w["dport"], w["proto"], w["egr"])))
    # probe-3 misses that read planted homes: wildcard words absent from the table
    p3_miss = 0
    for ep, d in WILD:
        w = keys_of(ep, 0, np.tile(dports, 2), np.repeat([6, 17], len(dports)), d)
        w = w[np.isin(key_home(w), list(homes.values()))]
        w = w[admitted(blooms, w)]
        g = nl[(nl[:, 1] == ep) & (nl[:, 2] == d)][:3]
        for x in w[:20]:
            parts.append(tup(keys_of(ep, g[:, 0], x["dport"], x["proto"], d)))
            p3_miss += len(g)
    assert p3_miss >= 30
    for n in sorted(g_absent):                                              # absent groups at planted group homes
        if len(g_absent[n]):
            parts.append(grp_tup(g_absent[n], 30))
    for n in sorted(g_planted):                                             # installed groups, their own tuples,
        r = g_planted[n]                                                    # the other direction, another endpoint
        parts += [grp_tup(r, 10), grp_tup(np.stack([r[:, 0], r[:, 1], 1 - r[:, 2]], 1), 6),
                  grp_tup(np.stack([r[:, 0], (r[:, 1] + 1) % N_EP, r[:, 2]], 1), 6)]
    parts.append(grp_tup(fill, 4))
    m = 12000                                                               # anything: every identity and WORLD
    anyid = np.concatenate([ids, np.array([L.WORLD_ID], np.uint32)])
    parts.append(tup(keys_of(rng.integers(0, N_EP, m), rng.choice(anyid, m),
                             rng.choice(np.unique(np.concatenate([exact["dport"], wildk["dport"]])), m),
                             rng.choice([6, 17], m), rng.integers(0, 2, m))))
    t = np.concatenate(parts)
    rng.shuffle(t)
    t["frag"] = (rng.random(len(t)) < 0.08) & (t["dir"] == 0)               # ingress fragments: no probe 1 or 3
    gate = rng.random(len(t)) < 0.06                                        # protocols ct_proto_gate leaves out
    t["proto"][gate] = rng.choice([47, 132, 1, 2], int(gate.sum()))
    t["len"][rng.random(len(t)) < 0.004] = 2048 + 7
    t["len"][rng.random(len(t)) < 0.002] = (1 << 18) + 5
    # the first 12 tuples: quads of 0, 1 and 2 hop-loading tuples of different rounds
    fr = tup(exact[:1], frag=1)
    fr["dir"] = 0
    a2, a8 = tup(absent["d2"][:1]), tup(absent["a"][:1])
    head = np.concatenate([fr, fr, fr, fr, a2, fr, fr, fr, a2, a8, fr, fr])
    t = np.concatenate([head, t])[:39_999]
    if len(t) % 4 == 0:
        t = t[:-1]

    # reply targets of the conntrack batches: ingress keys of the planted
    # neighbourhoods, absent ingress keys of the full home
    pl = np.concatenate([keys1[idx[n]] for n in order1] + [cand[plant["f_new"]]])
    replies = np.concatenate([pl[pl["egr"] == 0], absent["a"][absent["a"]["egr"] == 0]])
    return PolicyCase(ids=ids, keys1=keys1, proxy1=proxy1, keys2=keys2, proxy2=proxy2, del2=del2, homes=homes,
                      planted=idx, absent=absent, other_ep=other_ep, g_homes=g_homes, g_planted=g_planted,
                      g_absent=g_absent, tuples=t, replies=replies,
                      info={"fat": fat, "no_l3": nl, "fill": fill, "blooms": blooms})


# ---- addresses -------------------------------------------------------------
def id_addr4(case, ident, low):
    """host-order IPv4 address of an identity: its /24 and a low byte;
    WORLD (no prefix of its own) -> 192.0.2.x under 0.0.0.0/0"""
    i = np.searchsorted(case.ids, ident)
    known = (i < len(case.ids)) & (case.ids[np.minimum(i, len(case.ids) - 1)] == ident)
    return np.where(known, (30 << 24) | (i.astype(np.uint32) << 8) | low, 0xC0000200 | low).astype(np.uint32)


def id_addr6(case, ident, low):
    """(n, 16) IPv6 address of an identity: fd30::/16, its /64, a low byte"""
    i = np.searchsorted(case.ids, ident)
    known = (i < len(case.ids)) & (case.ids[np.minimum(i, len(case.ids) - 1)] == ident)
    a = np.zeros((len(ident), 16), np.uint8)
    a[:, 0] = np.where(known, 0xFD, 0x20)
    a[:, 1] = 0x30
    a[:, 6], a[:, 7] = np.where(known, i >> 8, 0), np.where(known, i & 255, 0)
    a[:, 15] = low
    return a


def policy_ipcache(case):
    """[(IPCACHE_KEY, REMOTE_ENDPOINT_INFO)]: a /24 and a /64 per identity,
    a distinct tunnel each, 0.0.0.0/0 and ::/0 -> WORLD"""
    out = [(L.ipcache_key("0.0.0.0/0"), L.remote_info(L.WORLD_ID, 0)), (L.ipcache_key("::/0"), L.remote_info(L.WORLD_ID, 0))]
    for i, v in enumerate(case.ids):
        out.append((L.ipcache_key(f"30.{i >> 8}.{i & 255}.0/24"), L.remote_info(int(v), 0x0A000001 + 2 * i)))
        out.append((L.ipcache_key(f"fd30:0:0:{i:x}::/64"), L.remote_info(int(v), 0x0A000002 + 2 * i)))
    return out


# --------------------------------------------------------------------------
# lpm4_full_dict
# --------------------------------------------------------------------------
N_UNIFORM = 4200          # uniform /16s with distinct labels: 40.0/16 ...
UNIFORM_P16 = 0x2800
SHAPE_P16 = 0x5000        # the shaped /16s: 80.0/16 ...
CODED = np.array([5001, 5002, 5003, 5004, (1 << 30) + 77], np.uint32)  # labels of many /16s: they get codes


@dataclass
class LpmCase:
    keys1: np.ndarray     # IPCACHE_KEY of the first commit ...
    vals1: np.ndarray     # ... REMOTE_ENDPOINT_INFO, a distinct tunnel per entry
    keys2: np.ndarray     # the second commit (updates only)
    vals2: np.ndarray
    probes: np.ndarray    # network-order u32, len % 4 != 0, <= 40000
    shapes: dict          # name -> /16 (address >> 16) built for that shape
    uniform_new: int      # the /16 the second commit adds

    def entries(self, phase):
        k, v = (self.keys1, self.vals1) if phase == 1 else \
            (np.concatenate([self.keys1, self.keys2]), np.concatenate([self.vals1, self.vals2]))
        return k, v


@functools.lru_cache(None)
def lpm4_full_dict():
    rng = np.random.Generator(np.random.PCG64(0x16C4))
    ents = []   # (host-order address, prefix length, label)
    shapes = {}
    fresh = iter(range((1 << 30) + 1000, (1 << 30) + 100_000))  # labels of one leaf each, >= 2^30: no code

    def put(p16, low, plen, label):
        ents.append(((p16 << 16) | low, plen, int(label)))

    # uniform /16s, one label each, every ninth >= 2^30
    for i in range(N_UNIFORM):
        put(UNIFORM_P16 + i, 0, 16, (1 << 30) + 200_000 + i if i % 9 == 4 else 10_000 + i)
    nxt = iter(range(SHAPE_P16, SHAPE_P16 + 0x400))

    def shape(name, prefixes, coded):
        """one /16 with (low, plen) prefixes; coded: labels of CODED in turn,
        else a fresh label per prefix"""
        p = next(nxt)
        shapes[name] = p
        for j, (low, plen) in enumerate(prefixes):
            put(p, low, plen, CODED[j % len(CODED)] if coded else next(fresh))
        return p

    for coded in (True, False):
        for rep in range(3 if coded else 1):   # the coded labels occur in several /16s
            sfx = (f"{rep}" if rep else "") + ("" if coded else "_nocode")
            shape("s1" + sfx, [(0x8000, 17)], coded)                                   # start 0x8000
            shape("s2" + sfx, [(0x0001, 32)], coded)                                   # starts 1, 2
            shape("s3" + sfx, [(0x0001, 32), (0x8000, 17)], coded)                     # 1, 2, 0x8000
            shape("s4" + sfx, [(0x0000, 32), (0x1234, 32), (0xFFFF, 32)], coded)       # 1, 0x1234, 0x1235, 0xFFFF
    shape("k2", [(0x1000, 24), (0x3000, 24), (0x5000, 24)], False)                     # 6 starts: a 64-byte node
    shape("k2_10", [(0x1000 * j, 24) for j in range(1, 6)], False)                     # 10 starts
    # an array /16: /24s that are leaves, byte-level nodes of every kind, a 256-leaf array
    arr = [(0x0100 * j, 24) for j in range(2, 40, 3)]
    arr += [(0x4080, 25)]                                                # one longer prefix, 1 boundary: kind 0
    arr += [(0x4140, 26)]                                                # one, 2 boundaries: kind 0
    arr += [(0x4240, 26), (0x42C0, 26)]                                  # two, 3 boundaries: kind 1
    arr += [(0x4310, 28), (0x4330, 28)]                                  # two, 4 boundaries: kind 1
    arr += [(0x4400 + 0x20 * j, 28) for j in range(3)]                   # three: kind 2
    arr += [(0x4500 + 0x20 * j + 0x10, 28) for j in range(5)]            # five, 10 boundaries: kind 2
    arr += [(0x4600 + 8 * j, 30) for j in range(12)]                     # > 10: a 256-leaf array
    arr += [(0x47FF, 32), (0x4800, 32)]                                  # the last and first byte of a /24
    shape("array", arr, False)
    shape("array_coded", arr, True)
    # tombstones that shadow a /16
    p = shape("tomb", [(0, 16)], False)
    put(p, 0x4000, 18, 0)
    put(p, 0xFF00, 24, 0)
    p = shape("tomb_all", [(0, 16)], False)
    ents[-1] = (ents[-1][0], 16, 0)
    put(p, 0x0100, 24, next(fresh))
    a = np.array([e[0] for e in ents], np.uint32)
    plen = np.array([e[1] for e in ents], np.uint32)
    lab = np.array([e[2] for e in ents], np.uint32)

    def structs(a, plen, lab, first_tunnel):
        k = np.zeros(len(a), L.IPCACHE_KEY)
        k["family"] = L.ENDPOINT_KEY_IPV4
        k["prefixlen"] = plen + L.IPCACHE_STATIC_PREFIX
        k["ip"][:, :4] = a.astype(">u4").view(np.uint8).reshape(-1, 4)
        v = np.zeros(len(a), L.REMOTE_ENDPOINT_INFO)
        v["sec_label"] = lab
        v["tunnel_endpoint"] = first_tunnel + np.arange(len(a))
        return k, v

    k1, v1 = structs(a, plen, lab, 0x0A000001)
    # 0.0.0.0/0 and, under everything, a static-part entry (prefixlen 31: the
    # {pad, family} words but their last bit)
    kx = np.zeros(2, L.IPCACHE_KEY)
    kx["family"] = L.ENDPOINT_KEY_IPV4
    kx["prefixlen"] = [L.IPCACHE_STATIC_PREFIX, 31]
    vx = np.zeros(2, L.REMOTE_ENDPOINT_INFO)
    vx["sec_label"] = [L.WORLD_ID, 9]
    vx["tunnel_endpoint"] = [0, 0x0AFF0001]
    k1, v1 = np.concatenate([k1, kx]), np.concatenate([v1, vx])
    # second commit: a new uniform /16 (the dictionary is full), a coded label
    # inside an inline /16 (stays inline), a fresh label inside another (overflows)
    uniform_new = UNIFORM_P16 + N_UNIFORM + 5
    a2 = np.array([uniform_new << 16, (shapes["s1"] << 16) | 0x2000, (shapes["s2"] << 16) | 0x9000], np.uint32)
    p2 = np.array([16, 24, 24], np.uint32)
    l2 = np.array([77_777, CODED[1], next(fresh)], np.uint32)
    k2, v2 = structs(a2, p2, l2, 0x0B000001)

    # probes: every boundary of the shaped prefixes with the addresses below
    # and above it, both ends of every shaped /16, the uniform /16s, random
    sh = a >= (SHAPE_P16 << 16)
    A = np.concatenate([a[sh], a2]).astype(np.int64)
    P = np.concatenate([plen[sh], p2]).astype(np.int64)
    last = A + (np.int64(1) << (32 - P)) - 1
    pr = [A - 1, A, A + 1, last - 1, last, last + 1]
    p16 = np.array(sorted(shapes.values()) + [uniform_new], np.int64)
    pr += [p16 << 16, (p16 << 16) | 0xFFFF, (p16 << 16) - 1, ((p16 + 1) << 16)]
    u = (UNIFORM_P16 + np.arange(N_UNIFORM, dtype=np.int64)) << 16
    pr += [u | rng.integers(0, 1 << 16, N_UNIFORM), u[::4], u[1::4] | 0xFFFF]
    pr.append((rng.choice(p16, 9000) << 16) | rng.integers(0, 1 << 16, 9000))
    ar = np.array([shapes["array"], shapes["array_coded"]], np.int64)
    pr.append((rng.choice(ar, 6000) << 16) | rng.integers(0x4000, 0x4900, 6000))
    pr.append(rng.integers(0, 1 << 32, 3000))
    q = np.concatenate(pr) & 0xFFFFFFFF
    q = q[rng.permutation(len(q))][:39_999]
    if len(q) % 4 == 0:
        q = q[:-1]
    return LpmCase(k1, v1, k2, v2, q.astype(np.uint32).byteswap(), shapes, uniform_new)


def lpm_shapes(rng):
    """ipcache contents that force every compressed-LPM shape (tables.h
    lpm16c): uniform /16 leaves, inline /16s, 64-byte run nodes, /16 arrays
    whose /24 entries are leaves, byte-level run nodes or 256-leaf arrays, run
    starts at the last address of a /16, tombstones, and labels >= 2^30 (leaves
    that index `vals`).  The table's few leaves all get dictionary codes, so no
    16- or 32-byte node arises at /16 level (lpm4_full_dict has those)."""
    def lab():
        return int(rng.choice([rng.integers(256, 70000), rng.integers(1 << 30, 1 << 32)]))
    cidrs = [("0.0.0.0/0", L.WORLD_ID), ("10.7.0.0/16", L.CLUSTER_ID)]
    cidrs += [(f"20.1.{16 * i}.0/20", lab()) for i in range(2)]            # two run starts: inline
    cidrs += [(f"20.2.{3 * i}.0/24", lab()) for i in range(5)]             # 64-byte node
    cidrs += [(f"20.3.{7 * i}.0/24", lab()) for i in range(11)]            # /16 array of leaves
    cidrs += [("20.4.255.255/32", lab()), ("20.4.0.0/32", lab()), ("20.5.128.0/17", 0)]
    cidrs += [(f"20.6.{i}.{j}/32", lab()) for i in range(0, 256, 3) for j in rng.choice(256, 40, replace=False)]
    cidrs += [(f"20.6.{i}.{16 * j}/28", lab()) for i in range(1, 256, 3) for j in range(0, 16, 5)]
    cidrs += [(f"20.7.{i}.{4 * j}/30", lab()) for i in range(8) for j in range(0, 64, 2)]
    cidrs += [("20.8.0.0/16", 0), ("20.8.1.0/24", lab()), ("20.9.0.0/15", lab())]
    seen, out = set(), []
    for c, v in cidrs:
        if c not in seen:
            seen.add(c)
            out.append((L.ipcache_key(c), L.remote_info(v, 0)))
    return out


# --------------------------------------------------------------------------
# the two cases as workloads: tables in two commits, tuple batches
# --------------------------------------------------------------------------
SYN = (5 << 4) | (L.TCP_SYN << 8)
SYNACK = (5 << 4) | ((L.TCP_SYN | L.TCP_ACK) << 8)


def _l4b(proto, tcp=SYN):
    return np.where(proto == 6, tcp, np.where(proto == 1, 8, np.where(proto == 58, 128, 0))).astype(np.uint16)


def _be16(x):
    return np.asarray(x).astype(np.uint16).byteswap()


def _be32(x):
    return np.asarray(x).astype(np.uint32).byteswap()


def _unique6(n, base):
    a = np.zeros((n, 16), np.uint8)
    a[:, 0], a[:, 1] = 0xFD, 0x99
    a[:, 12:] = (base + np.arange(n)).astype(">u4").view(np.uint8).reshape(n, 4)
    return a


class Workload:
    """One case: ipcache and policy contents in two commits, an IPv4 (and
    IPv6) tuple batch, the policy keys whose counters are compared."""

    def __init__(self, name, ipc1, ipc2, pol1, pol2, batch4, batch6=None):
        self.name = name
        self.ipc1, self.ipc2 = ipc1, ipc2          # [(IPCACHE_KEY, REMOTE_ENDPOINT_INFO)]
        self.pol1, self.pol2 = pol1, pol2          # [(ep, POLICY_KEY, POLICY_ENTRY or None = delete)]
        self.batch4, self.batch6 = batch4, batch6

    def load(self, t, phase=1, commit=None):
        """the tables into an Engine or an Oracle; commit: called between the
        two commits' contents (an engine commits there: the second one patches)"""
        for k, v in self.ipc1:
            assert t.ipcache_update(k, v) == 0
        for ep, k, e in self.pol1:
            assert t.policy_update(ep, k, e) == 0
        if phase == 2:
            if commit:
                commit()
            for k, v in self.ipc2:
                assert t.ipcache_update(k, v) == 0
            for ep, k, e in self.pol2:
                assert (t.policy_delete(ep, k) if e is None else t.policy_update(ep, k, e)) == 0

    def counter_keys(self, phase):
        """(ep, key) of every policy key present after `phase`"""
        dele = {(ep, k.tobytes()) for ep, k, e in self.pol2 if e is None} if phase == 2 else set()
        rows = self.pol1 + ([r for r in self.pol2 if r[2] is not None] if phase == 2 else [])
        return [(ep, k) for ep, k, _ in rows if (ep, k.tobytes()) not in dele]

    def counters(self, t, phase):
        out = []
        for ep, k in self.counter_keys(phase):
            rc, got = t.policy_lookup(ep, k)
            assert rc == 0
            got = got if isinstance(got, np.void) else np.frombuffer(got, L.POLICY_ENTRY)[0]
            out.append((int(got["packets"]), int(got["bytes"])))
        return out


def _pol_rows(keys, proxy, dele=None):
    eps, pk, pe = policy_structs(keys, proxy)
    return [(int(ep), k, None if dele is not None and dele[i] else e) for i, (ep, k, e) in enumerate(zip(eps, pk, pe))]


def tuples_v4(case, t, base=0):
    """TUP rows -> the IPv4 tuple columns: the identity's address is the
    daddr of egress tuples and the saddr of ingress ones; the other address
    (198.18+, WORLD) and the sport are unique per tuple, so no 5-tuple repeats"""
    n = len(t)
    rng = np.random.Generator(np.random.PCG64(0xB4 + n + base))
    addr = id_addr4(case, t["id"], rng.integers(1, 255, n).astype(np.uint32))
    other = (0xC6120000 + base + np.arange(n)).astype(np.uint32)
    eg = t["dir"] == 1
    proto = t["proto"].astype(np.uint8)
    return {"saddr": _be32(np.where(eg, other, addr)), "daddr": _be32(np.where(eg, addr, other)),
            "sport": _be16(1024 + (base + np.arange(n)) % 60000), "dport": t["dport"].astype(np.uint16),
            "proto": proto, "l4b": _l4b(proto), "flags": (t["dir"] | (t["frag"] << 1)).astype(np.uint8),
            "len": t["len"].astype(np.uint32), "ep": t["ep"].astype(np.uint16),
            "hash": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)}


def tuples_v6(case, t, base=0):
    """the same tuples over the identities' /64s (ICMP becomes ICMPv6)"""
    n = len(t)
    b = tuples_v4(case, t, base)
    rng = np.random.Generator(np.random.PCG64(0xB6 + n + base))
    addr = id_addr6(case, t["id"], rng.integers(1, 255, n).astype(np.uint8))
    other = _unique6(n, base)
    eg = (t["dir"] == 1)[:, None]
    proto = np.where(b["proto"] == 1, 58, b["proto"]).astype(np.uint8)
    return dict(b, saddr=np.where(eg, other, addr), daddr=np.where(eg, addr, other), proto=proto, l4b=_l4b(proto))


@functools.lru_cache(None)
def policy_workload():
    c = policy_hops()
    ipc = policy_ipcache(c)
    return Workload("policy_hops", ipc, [], _pol_rows(c.keys1, c.proxy1), _pol_rows(c.keys2, c.proxy2, c.del2),
                    tuples_v4(c, c.tuples), tuples_v6(c, c.tuples))


def lpm_restate(case, phase, addrs=None):
    """(m, 3) uint32 {found, sec_label, tunnel} of the restatement's ipcache
    lookup of every probe (network-order u32)"""
    from oracle import Oracle
    o = Oracle()
    for k, v in zip(*case.entries(phase)):
        assert o.ipcache_update(k, v) == 0
    o.set_fast(True)
    addrs = case.probes if addrs is None else addrs
    r = np.zeros((len(addrs), 3), np.uint32)
    for i, a in enumerate(addrs):
        rc, val = o.ipcache_lookup_addr(int(a))
        if rc == 0:
            r[i] = (1,) + tuple(np.frombuffer(val, "<u4"))
    o.close()
    return r


@functools.lru_cache(None)
def lpm_workload():
    """the probes as the daddr of egress tuples and the saddr of ingress ones
    (the other address unique per tuple, under 0.0.0.0/0); L3-only and exact
    keys on the labels the probes return most, wildcard keys, WORLD"""
    c = lpm4_full_dict()
    rows = lpm_restate(c, 1)
    n = len(c.probes)
    rng = np.random.Generator(np.random.PCG64(0xA4 + n))
    eg = rng.random(n) < 0.5
    other = _be32(0xC6120000 + np.arange(n))
    proto = rng.choice(np.array([6, 17, 1, 47], np.uint8), n, p=[0.5, 0.3, 0.1, 0.1])
    frag = (rng.random(n) < 0.05) & ~eg
    ln = rng.integers(64, 1501, n).astype(np.uint32)
    ln[rng.random(n) < 0.003] = 2048 + 9
    ln[rng.random(n) < 0.001] = (1 << 18) + 3
    b = {"saddr": np.where(eg, other, c.probes), "daddr": np.where(eg, c.probes, other),
         "sport": _be16(1024 + np.arange(n) % 60000),
         "dport": _be16(rng.choice(np.array([80, 443, 53]), n)), "proto": proto, "l4b": _l4b(proto),
         "flags": (eg.astype(np.uint8) | (frag.astype(np.uint8) << 1)), "len": ln,
         "ep": rng.integers(0, N_EP, n).astype(np.uint16),
         "hash": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)}
    labs, cnt = np.unique(rows[(rows[:, 0] == 1) & (rows[:, 1] != 0), 1], return_counts=True)
    top = labs[np.argsort(-cnt, kind="stable")[:60]]
    pol = []
    for ep in range(N_EP):
        for d in (0, 1):
            pol.append((ep, L.policy_key(0, 53, 17, d), L.policy_entry(0)))
            pol.append((ep, L.policy_key(0, 443, 6, d), L.policy_entry(4000 + ep)))
    pol += [(0, L.policy_key(L.WORLD_ID, 0, 0, 1), L.policy_entry(0)), (1, L.policy_key(L.WORLD_ID, 80, 6, 0), L.policy_entry(0))]
    for j, lab in enumerate(top):
        for ep in range(N_EP):
            for d in (0, 1):
                k = L.policy_key(int(lab), 0, 0, d) if (j + ep) % 3 == 0 else L.policy_key(int(lab), 80, 6, d)
                if (j + ep) % 3 != 2:
                    pol.append((ep, k, L.policy_entry(5000 + j if j % 4 == 0 else 0)))
    return Workload("lpm4_full_dict", list(zip(*c.entries(1))), list(zip(c.keys2, c.vals2)), pol, [], b)


WORKLOADS = {"policy_hops": policy_workload, "lpm4_full_dict": lpm_workload}


# --------------------------------------------------------------------------
# services, the XDP deny set, conntrack batches, frames
# --------------------------------------------------------------------------
VIP4 = 0x64400000          # 100.64.0.0: service addresses
EP4 = 0x0AC80000           # 10.200.0.0: the local endpoints of the XDP step (cilium_lxc)
N_LXC = 32
DENY = [("198.18.7.0/24", 0), ("198.18.9.128/25", 0), ("198.18.11.3/32", 1)]  # (prefix, dyn4 0 / fix4 1)


def _vip6(j):
    a = np.zeros(16, np.uint8)
    a[:2] = [0xFD, 0x64]
    a[15] = j + 1
    return a


def _with_services(w, b4, b6, back4, back6, ports, rows):
    """w.svc4 / w.svc6: one service per backend (address, network-order
    port), VIP 100.64.0.j / fd64::j, port 8000 + j; w.batch4_svc / batch6_svc:
    the batch plus, per service, the tuples `rows[j]` (indices into the batch)
    again, aimed at the VIP"""
    w.svc4, w.svc6 = [], []
    extra4 = {k: [] for k in b4}
    extra6 = {k: [] for k in b6} if b6 is not None else None
    for j, port in enumerate(ports):
        vport = 8000 + j
        w.svc4 += [(L.lb4_key(VIP4 + j + 1, vport, 1), L.lb4_service(int(back4[j]), L.ntohs(int(port)), 0, 0, 1)),
                   (L.lb4_key(VIP4 + j + 1, vport, 0), L.lb4_service(0, 0, 1, 0, 1))]
        ix = np.asarray(rows[j])
        for k in b4:
            extra4[k].append(b4[k][ix])
        extra4["daddr"][-1] = np.full(len(ix), L.ip4_be(VIP4 + j + 1), np.uint32)
        extra4["dport"][-1] = np.full(len(ix), L.htons(vport), np.uint16)
        extra4["flags"][-1] = np.ones(len(ix), np.uint8)
        if b6 is not None:
            for s, cnt in ((1, 0), (0, 1)):
                k6, v6 = np.zeros((), L.LB6_KEY), np.zeros((), L.LB6_SERVICE)
                k6["address"], k6["dport"], k6["slave"] = _vip6(j), L.htons(vport), s
                if s:
                    v6["target"], v6["port"] = back6[j], port
                v6["count"], v6["weight"] = cnt, L.htons(1)
                w.svc6.append((k6, v6))
            for k in b6:
                extra6[k].append(b6[k][ix])
            extra6["daddr"][-1] = np.tile(_vip6(j), (len(ix), 1))
            extra6["dport"][-1] = np.full(len(ix), L.htons(vport), np.uint16)
            extra6["flags"][-1] = np.ones(len(ix), np.uint8)

    def join(b, extra):
        out = {k: np.concatenate([b[k]] + extra[k]) for k in b}
        n = len(out["flags"])
        # the other address and the sport stay unique: the copies get new ones
        m = n - len(b["flags"])
        out["sport"][-m:] = _be16(2000 + np.arange(m))
        if out["saddr"].ndim == 1:
            out["saddr"][-m:] = _be32(0xC6130000 + np.arange(m))
        else:
            out["saddr"][-m:] = _unique6(m, 1 << 24)
        keep = min(n, 39_999)
        keep -= keep % 4 == 0
        return {k: v[n - keep:] for k, v in out.items()}
    w.batch4_svc = join(b4, extra4)
    w.batch6_svc = join(b6, extra6) if b6 is not None else None


def load_services(w, t, v6=False):
    for k, v in (w.svc6 if v6 else w.svc4):
        assert (t.lb6_update(k, v) if v6 else (t.lb4_update if hasattr(t, "lb4_update") else t.lb_update)(k, v)) == 0


def load_xdp(t):
    """a few deny prefixes and the local endpoints of the XDP prefilter"""
    for cidr, which in DENY:
        assert t.cidr_update(which, L.lpm_key(cidr)) == 0
    for j in range(N_LXC):
        assert t.endpoint_update(L.endpoint_key(f"10.200.0.{j + 1}")) == 0


def xdp_batch(b):
    """the ingress tuples' daddr in the endpoint map (1 in 50 is not: dropped
    by XDP), 1 in 30 ingress saddr inside a deny prefix"""
    n = len(b["flags"])
    rng = np.random.Generator(np.random.PCG64(0xD4 + n))
    ing = (b["flags"] & 1) == 0
    b = dict(b)
    local = _be32(EP4 + 1 + rng.integers(0, N_LXC, n))
    b["daddr"] = np.where(ing & (rng.random(n) > 0.02), local, b["daddr"]).astype(np.uint32)
    deny = _be32(rng.choice(np.array([0xC6120700, 0xC6120980, 0xC6120B03], np.uint32), n) |
                 (rng.integers(0, 128, n).astype(np.uint32) * (rng.random(n) < 0.7)))
    b["saddr"] = np.where(ing & (rng.random(n) < 0.033), deny, b["saddr"]).astype(np.uint32)
    return b


def replies_of(b, rows):
    """the reply packets of the (egress) tuples `rows` of batch b"""
    r = {k: v[rows].copy() for k, v in b.items()}
    r["saddr"], r["daddr"] = b["daddr"][rows].copy(), b["saddr"][rows].copy()
    r["sport"], r["dport"] = b["dport"][rows].copy(), b["sport"][rows].copy()
    r["flags"] = np.zeros(len(rows), np.uint8)
    r["l4b"] = _l4b(r["proto"], SYNACK)
    return r


def _concat(*bs):
    return {k: np.concatenate([b[k] for b in bs]) for k in bs[0]}


def _trim(b, n=39_999):
    m = min(len(b["flags"]), n)
    m -= m % 4 == 0
    return {k: v[:m] for k, v in b.items()}


@functools.lru_cache(None)
def policy_extras():
    """policy_workload() with services whose backends are planted egress keys
    (and absent ones of the full home "x"), and two conntrack batches per
    family: the second holds the replies to the first's openers, whose reply
    tuple {identity, sport, proto, ingress} is a planted ingress key"""
    c, w = policy_hops(), policy_workload()
    pl = np.concatenate([c.keys1[c.planted[n]] for n in c.homes])
    pl = pl[pl["egr"] == 1]
    back = np.concatenate([pl[:9], c.absent["x"][c.absent["x"]["egr"] == 1][:3]])
    t = c.tuples
    rows = []
    for k in back:    # tuples of the backend's endpoint and protocol, any direction: they become egress
        ix = np.flatnonzero((t["ep"] == k["ep"]) & (t["proto"] == k["proto"]) & (t["frag"] == 0))[:60]
        assert len(ix) == 60
        rows.append(ix)
    low = np.full(len(back), 77, np.uint32)
    _with_services(w, w.batch4, w.batch6, id_addr4(c, back["id"], low), id_addr6(c, back["id"], low.astype(np.uint8)),
                   back["dport"], rows)
    w.backends = back
    # openers: egress to the reply target's identity and port (allowed by the
    # fat group's egress L3 key), 12 per target
    k = np.repeat(c.replies, 12)
    op = np.zeros(len(k), TUP)
    op["ep"], op["id"], op["dport"], op["proto"], op["dir"] = k["ep"], k["id"], k["dport"], k["proto"], 1
    op["len"] = 100 + np.arange(len(k)) % 1000
    w.reply_target = k
    w.ct = {}
    for v6, (tup, bsvc) in enumerate(((tuples_v4, w.batch4_svc), (tuples_v6, w.batch6_svc))):
        o = tup(c, op, base=1 << 20)
        b1 = _concat(o, _trim(bsvc, 39_000 - len(op)))
        fresh = tup(c, c.tuples[:30_000], base=1 << 22)
        b2 = _concat(replies_of(o, np.arange(len(op))), fresh)
        w.ct[v6] = (_trim(b1), _trim(b2))
    return w


@functools.lru_cache(None)
def lpm_extras():
    """lpm_workload() with services whose backends sit in shaped /16s; the
    second conntrack batch is the first again (established connections)"""
    c, w = lpm4_full_dict(), lpm_workload()
    s = c.shapes
    back = np.array([(s["s4_nocode"] << 16) | 0xFFFF, (s["s4"] << 16) | 0x1234, (s["s3_nocode"] << 16) | 1,
                     (s["k2_10"] << 16) | 0x5000, (s["array"] << 16) | 0x4608, (s["array_coded"] << 16) | 0x4245,
                     (s["tomb"] << 16) | 0x4001, (UNIFORM_P16 + N_UNIFORM - 1) << 16], np.uint32)
    eg = np.flatnonzero(np.isin(w.batch4["proto"], (6, 17)) & ((w.batch4["flags"] & 2) == 0))
    rows = [eg[60 * j:60 * (j + 1)] for j in range(len(back))]
    _with_services(w, w.batch4, None, back, None, np.full(len(back), L.htons(80)), rows)
    w.ct = {0: (w.batch4_svc, w.batch4_svc)}
    return w


EXTRAS = {"policy_hops": policy_extras, "lpm4_full_dict": lpm_extras}


def frames_of(b4):
    """the IPv4 tuples as frames (synth.frames_from_tuples) between 4001 frames
    of every other kind (synth.make_frames), in 128- and 64-byte slots"""
    from cilium_amd import synth
    rng = np.random.Generator(np.random.PCG64(0xF4 + len(b4["flags"])))
    b4 = _trim(b4, 35_000)
    f = synth.frames_from_tuples(b4, stride=128)
    g = synth.make_frames(rng, 4001, width=128, n_ep=N_EP)
    f = {k: np.concatenate([f[k], g[k].astype(f[k].dtype)]) for k in f}
    p = rng.permutation(len(f["len"]))
    p = p[:len(p) - (len(p) % 4 == 0)]
    f = {k: np.ascontiguousarray(v[p]) for k, v in f.items()}
    assert len(p) % 4 != 0 and len(p) <= 40_000
    return {128: f, 64: dict(f, data=np.ascontiguousarray(f["data"][:, :64]))}
