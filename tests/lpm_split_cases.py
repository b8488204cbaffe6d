"""Crafted /16s for the split x16 slot (tables.h LPMC_SPLIT), shared by
test_lpm_split.py (CPU: what the builder made of them, the host walk) and
test_gpu_lpm_split.py (the device walks).  Plain numpy; nothing here asks the
library anything.  Expected answers come from the restatement (oracle).

Every label that must have a dictionary code also fills a uniform /16 of its
own (the dictionary counts leaves of /16s with <= 5 runs); an entry's tunnel
is a function of its label, so the tunnel table has the same runs and codes.
The background is 0.0.0.0/0 -> WORLD.  A /16's run starts are counted here
from its prefixes, per address, and asserted: a shape cannot silently become
another one.
"""
import functools
from dataclasses import dataclass

import numpy as np

import cascade_cases as CC
from cilium_amd import layouts as L

N_EP = CC.N_EP
CODE_P16 = 0x2800        # 40.0/16 ...: one uniform /16 per coded label
SHAPE_P16 = 0x5000       # 80.0/16 ...: the crafted /16s
BIG = (1 << 30) + 77     # a label >= 2^30: its leaf indexes `vals`
CODED = np.array([5001, 5002, 5003, 5004, 5005, 5006, 5007, BIG, 0], np.uint32)  # 0: a tombstone
UNDER8 = 5100            # 30.0.0.0/8
NOCODE = (6001, 6002)    # labels of one leaf each, inside overflowing /16s only: no code
MAX_STARTS = 24          # tables.h LPMC_SPLIT_MAX_RUNS - 1


def tunnel_of(label):
    return 0x0A000000 + (int(label) & 0xFFFF) + (0x10000 if int(label) >= 1 << 30 else 0)


def isolated(k, first=0x0800, step=0x0800):
    """(low, plen) prefixes that make k run starts over a WORLD background:
    k // 2 isolated /24s (two starts each) and, for an odd k, x.x.0.0/24 (its
    start at 0 is no run start)"""
    p = [(first + step * j, 24) for j in range(k // 2)]
    return ([(0, 24)] if k % 2 else []) + p


@dataclass
class SplitCase:
    keys1: np.ndarray     # IPCACHE_KEY of the first commit ...
    vals1: np.ndarray     # ... REMOTE_ENDPOINT_INFO
    keys2: np.ndarray     # the second commit (updates only)
    vals2: np.ndarray
    shapes: dict          # name -> /16 (address >> 16)
    starts: dict          # name -> (run starts after commit 1, after commit 2)
    children: dict        # name -> (children after commit 1, after commit 2); 0: not split

    def entries(self, phase):
        if phase == 1:
            return self.keys1, self.vals1
        return np.concatenate([self.keys1, self.keys2]), np.concatenate([self.vals1, self.vals2])

    def probes(self, names=None):
        """every address of the crafted /16s, network-order u32, /16 by /16"""
        p = np.array([self.shapes[n] for n in (names or sorted(self.shapes))], np.uint32)
        a = (p[:, None] << np.uint32(16)) | np.arange(65536, dtype=np.uint32)[None, :]
        return a.reshape(-1).byteswap()


def _structs(ents):
    a = np.array([e[0] for e in ents], np.uint32)
    k = np.zeros(len(a), L.IPCACHE_KEY)
    k["family"] = L.ENDPOINT_KEY_IPV4
    k["prefixlen"] = np.array([e[1] for e in ents], np.uint32) + L.IPCACHE_STATIC_PREFIX
    k["ip"][:, :4] = a.astype(">u4").view(np.uint8).reshape(-1, 4)
    v = np.zeros(len(a), L.REMOTE_ENDPOINT_INFO)
    v["sec_label"] = [e[2] for e in ents]
    v["tunnel_endpoint"] = [tunnel_of(e[2]) for e in ents]
    return k, v


def _count_starts(p16, ents, under):
    """run starts of /16 p16: the label of every address from the prefixes
    inside it, longest prefix last (`under`: the label below them)"""
    lab = np.full(65536, under, np.int64)
    inside = sorted((e for e in ents if e[1] >= 16 and e[0] >> 16 == p16), key=lambda e: e[1])
    for a, plen, v in inside:
        lo = a & 0xFFFF
        lab[lo:lo + (1 << (32 - plen))] = v
    return int((lab[1:] != lab[:-1]).sum())


@functools.lru_cache(None)
def split_case():
    ents, shapes, under = [], {}, {}
    for j, v in enumerate(CODED):
        ents.append(((CODE_P16 + j) << 16, 16, int(v)))
    ents.append((30 << 24, 8, UNDER8))
    nxt = iter(range(SHAPE_P16, SHAPE_P16 + 0x100))
    lab = [int(x) for x in CODED[:7]]

    def shape(name, prefixes, labels=None, p16=None):
        p = next(nxt) if p16 is None else p16
        shapes[name] = p
        under[name] = UNDER8 if p >> 8 == 30 else L.WORLD_ID
        for j, (low, plen) in enumerate(prefixes):
            ents.append(((p << 16) | low, plen, labels[j] if labels else lab[j % len(lab)]))
        return p

    for k in (4, 5, 6, 9, 10, 11, 15, 19, 20, 24, 25):
        shape(f"s{k}", isolated(k))
    # a real run start at 0xFFFF inside a child: 7 starts, runs 5..7 in child 1
    shape("ffff_child", isolated(6) + [(0xFFFF, 32)])
    # ... and as a coarse start: 10 starts, run 10 begins at 0xFFFF, a last
    # child of one run; x = 0xFFFF also passes the two unused coarse starts
    shape("ffff_coarse", isolated(9) + [(0xFFFF, 32)])
    # run 5 (a coarse start) is one address long: the child's first run start
    # is the coarse start + 1
    shape("coarse_adjacent", [(0x0800, 24), (0x1000, 24), (0x2000, 32), (0x3000, 24)])
    shape("nested", [(0x4000, 20), (0x4400, 24), (0x4440, 28), (0x4444, 32)])
    shape("tombstone", isolated(6), labels=[5001, 0, 5003])
    # a leaf >= 2^30 is one `vals` word per entry: one /15 entry is the leaf of
    # the crafted /16's background and of its uniform neighbour, so it has a code
    shape("big_label", isolated(6), p16=0x5080)
    under["big_label"] = BIG
    ents.append((0x5080 << 16, 15, BIG))
    shape("nocode6", isolated(6), labels=[5001, NOCODE[0], 5003])
    shape("cluster", isolated(6), p16=(10 << 8) | 9)
    shape("under8", isolated(6), p16=(30 << 8) | 5)
    ents.append((0, 0, L.WORLD_ID))
    # the second commit: 4 -> 6 starts, 24 -> 26, 6 -> 4 (a /24 takes the
    # background's label), a split /16 gains a leaf without a code
    ents2 = [((shapes["s4"] << 16) | 0x7000, 24, 5004), ((shapes["s24"] << 16) | 0x7800, 24, 5005),
             ((shapes["s6"] << 16) | 0x0800, 24, L.WORLD_ID), ((shapes["s5"] << 16) | 0x7000, 24, NOCODE[1])]
    starts, children = {}, {}
    for n, p in shapes.items():
        s = (_count_starts(p, ents, under[n]), _count_starts(p, ents + ents2, under[n]))
        starts[n] = s
        nocode = (n == "nocode6", n in ("nocode6", "s5"))
        children[n] = tuple(0 if k < 5 or k > MAX_STARTS or nc else (k + 1 + 4) // 5 for k, nc in zip(s, nocode))
    want = {"s4": (4, 6), "s24": (24, 26), "s6": (6, 4), "s5": (5, 7), "ffff_child": (7, 7), "ffff_coarse": (10, 10),
            "coarse_adjacent": (8, 8), "nested": (8, 8), "s25": (25, 25), "cluster": (6, 6), "under8": (6, 6)}
    for n, s in want.items():
        assert starts[n] == s, (n, starts[n])
    for k in (9, 10, 11, 15, 19, 20):
        assert starts[f"s{k}"] == (k, k)
    k1, v1 = _structs(ents)
    k2, v2 = _structs(ents2)
    return SplitCase(k1, v1, k2, v2, shapes, starts, children)


@functools.lru_cache(None)
def restate(phase):
    """(n, 3) uint32 {found, sec_label, tunnel} of the restatement's ipcache
    lookup of every address of every crafted /16 (SplitCase.probes() order)"""
    import ctypes as C
    from oracle import Oracle
    c = split_case()
    o = Oracle()
    for k, v in zip(*c.entries(phase)):
        assert o.ipcache_update(k, v) == 0
    o.set_fast(True)
    q = c.probes()
    r = np.zeros((len(q), 3), np.uint32)
    buf = (C.c_uint32 * 2)()
    look, h = o.L.or_ipcache_lookup4, o.h
    rows = [(1, buf[0], buf[1]) if look(h, a, buf) == 0 else (0, 0, 0) for a in q.tolist()]
    o.close()
    r[:] = np.array(rows, np.uint32)
    r.setflags(write=False)
    return r


@functools.lru_cache(None)
def workload():
    """the probes as the daddr of egress tuples and the saddr of ingress ones,
    n = 65,536 k + 3 (the three: the first addresses again), with a small
    policy on the labels of the crafted /16s"""
    c = split_case()
    q = c.probes()
    q = np.concatenate([q, q[:3]])
    n = len(q)
    assert n % 65536 == 3
    rng = np.random.Generator(np.random.PCG64(0x5B + n))
    eg = rng.random(n) < 0.5
    other = CC._be32(0xC6120000 + np.arange(n))
    proto = rng.choice(np.array([6, 17, 1, 47], np.uint8), n, p=[0.5, 0.3, 0.1, 0.1])
    frag = (rng.random(n) < 0.05) & ~eg
    b = {"saddr": np.where(eg, other, q), "daddr": np.where(eg, q, other),
         "sport": CC._be16(1024 + np.arange(n) % 60000),
         "dport": CC._be16(rng.choice(np.array([80, 443, 53]), n)), "proto": proto, "l4b": CC._l4b(proto),
         "flags": (eg.astype(np.uint8) | (frag.astype(np.uint8) << 1)),
         "len": rng.integers(64, 1501, n).astype(np.uint32), "ep": rng.integers(0, N_EP, n).astype(np.uint16),
         "hash": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)}
    pol = []
    for ep in range(N_EP):
        for d in (0, 1):
            pol.append((ep, L.policy_key(0, 53, 17, d), L.policy_entry(0)))
            pol.append((ep, L.policy_key(0, 443, 6, d), L.policy_entry(4000 + ep)))
    pol += [(0, L.policy_key(L.WORLD_ID, 0, 0, 1), L.policy_entry(0)), (1, L.policy_key(L.WORLD_ID, 80, 6, 0), L.policy_entry(0))]
    labs = [int(x) for x in CODED if x] + [UNDER8, L.CLUSTER_ID] + list(NOCODE)
    for j, lab in enumerate(labs):
        for ep in range(N_EP):
            for d in (0, 1):
                k = L.policy_key(lab, 0, 0, d) if (j + ep) % 3 == 0 else L.policy_key(lab, 80, 6, d)
                if (j + ep) % 3 != 2:
                    pol.append((ep, k, L.policy_entry(5000 + j if j % 4 == 0 else 0)))
    return CC.Workload("lpm_split", list(zip(*c.entries(1))), list(zip(c.keys2, c.vals2)), pol, [], b)


N_SVC_ROWS = 8192   # tuples aimed at each service: 8 x 8192 = 65,536 more, n stays 65,536 k + 3


@functools.lru_cache(None)
def extras():
    """workload() with eight services whose backends sit in crafted /16s (the
    VIPs as CC.VIP4); batch4_svc: the batch plus, per service, 8192 of its
    TCP / UDP tuples again as egress tuples aimed at the VIP"""
    c, w = split_case(), workload()
    s = c.shapes
    back = np.array([(s["s24"] << 16) | 0x0850, (s["ffff_coarse"] << 16) | 0xFFFF, (s["s9"] << 16) | 0x0001,
                     (s["nocode6"] << 16) | 0x1010, (s["s25"] << 16) | 0x0900, (s["cluster"] << 16) | 0x0801,
                     (s["big_label"] << 16) | 0x4000, (s["s4"] << 16) | 0x0800], np.uint32)
    b4 = w.batch4
    ok = np.flatnonzero(np.isin(b4["proto"], (6, 17)) & ((b4["flags"] & 2) == 0))
    assert len(ok) >= len(back) * N_SVC_ROWS
    w.svc4, extra = [], {k: [] for k in b4}
    for j, a in enumerate(back):
        vport = 8000 + j
        w.svc4 += [(L.lb4_key(CC.VIP4 + j + 1, vport, 1), L.lb4_service(int(a), 80, 0, 0, 1)),
                   (L.lb4_key(CC.VIP4 + j + 1, vport, 0), L.lb4_service(0, 0, 1, 0, 1))]
        ix = ok[N_SVC_ROWS * j:N_SVC_ROWS * (j + 1)]
        for k in b4:
            extra[k].append(b4[k][ix].copy())
        extra["daddr"][-1][:] = L.ip4_be(CC.VIP4 + j + 1)
        extra["dport"][-1][:] = L.htons(vport)
        extra["flags"][-1][:] = 1
    out = {k: np.concatenate([b4[k]] + extra[k]) for k in b4}
    m = len(back) * N_SVC_ROWS
    out["sport"][-m:] = CC._be16(2000 + np.arange(m) % 60000)
    out["saddr"][-m:] = CC._be32(0xC7000000 + np.arange(m))
    w.batch4_svc, w.batch6, w.batch6_svc, w.svc6 = out, None, None, []
    assert len(out["flags"]) % 65536 == 3
    return w
