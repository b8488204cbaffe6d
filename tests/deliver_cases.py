"""Reference for the local delivery step (cgpu_deliver_v4 / _v6).

ipv4_local_delivery / ipv6_local_delivery (bpf/lib/l3.h:71-132) store the
label in CB_SRC_LABEL and tail-call the destination endpoint's ipv4_policy /
ipv6_policy (bpf/bpf_lxc.c:863-978, :1002-1030), which run
policy_can_access_ingress(src_label, dport, proto, ..., is_fragment)
(bpf/lib/policy.h:126-146) on that endpoint's map behind ct_lookup's protocol
gate.  The restatement (oracle) computes exactly that call for an ingress
tuple when its ipcache is empty, ingress_secctx_world is 0 and
ingress_src_identity is the label: nothing can replace the handed-in identity
then.  `reference` configures one restatement once per distinct label of a
batch and classifies that label's LOCAL packets as ingress tuples on ep =
lxc_id; packets that are not LOCAL never reach it.

CASES is a hand-written table of literal packets against the literal policy
world below, the expected (verdict, identity, stage) written out by hand from
the source: it pins the reference.
"""
import numpy as np

from cilium_amd import layouts as L

NONE, DROP, PROXY, LOCAL, HOST, OVERLAY, STACK, TIME_EXCEEDED = range(8)
NOT_LOCAL = 9
DROP_POLICY, DROP_CT_UNKNOWN_PROTO = -133, -137
F_EGRESS, F_FRAGMENT = 1, 2
TCP, UDP, ICMP, ICMP6, GRE = 6, 17, 1, 58, 47
# an endpoint id for which no world here installs a policy key: where `arg`
# names no policy map of the engine the restatement looks this one up (a miss)
NO_MAP = 0xFFFF


def new_oracle(load, gate=1):
    """a restatement for `reference`: policy only (load(o) installs it), an
    empty ipcache, nothing that replaces the handed-in identity"""
    from oracle import Oracle
    o = Oracle(ct_proto_gate=gate, ingress_secctx_world=0, ingress_src_identity=0)
    load(o)
    return o


def labels_of(src_ep, seclabels: dict):
    """the src_ep form: the sending endpoint's SECLABEL, 0 without an lxc entry"""
    return np.array([seclabels.get(int(e), 0) for e in src_ep], np.uint32)


def reference(o, v6, action, arg, label, dport, proto, flags, length, max_ep=65536):
    """{"verdict", "identity", "stage"} of the batch; the restatement `o` keeps
    the counters and metrics of its LOCAL packets (o.policy_lookup, o.metrics)."""
    n = len(action)
    action, arg, label = np.asarray(action), np.asarray(arg, np.uint32), np.asarray(label, np.uint32)
    verdict = np.zeros(n, np.int32)
    identity = np.zeros(n, np.uint32)
    stage = np.full(n, NOT_LOCAL, np.uint8)
    local = action == LOCAL
    ep = np.where((arg > 0xFFFF) | (arg >= max_ep), NO_MAP, arg).astype(np.uint16)
    # is_fragment: the bit on IPv4, false on IPv6 (bpf_lxc.c:1015); direction: ingress
    fl = (np.asarray(flags) & (0 if v6 else F_FRAGMENT)).astype(np.uint8)
    for lab in np.unique(label[local]):
        m = np.flatnonzero(local & (label == lab))
        o.configure(ingress_src_identity=int(lab))
        k = len(m)
        t = {"saddr": np.zeros((k, 16), np.uint8) if v6 else np.zeros(k, np.uint32),
             "daddr": np.zeros((k, 16), np.uint8) if v6 else np.zeros(k, np.uint32),
             "dport": np.asarray(dport, np.uint16)[m], "proto": np.asarray(proto, np.uint8)[m], "flags": fl[m],
             "len": np.asarray(length, np.uint32)[m], "ep": ep[m]}
        v, i, s, _ = (o.classify_v6 if v6 else o.classify_v4)(t)
        verdict[m], identity[m], stage[m] = v, i, s
    return {"verdict": verdict, "identity": identity, "stage": stage}


# --------------------------------------------------------------------------
# the literal policy world and the literal packets
# --------------------------------------------------------------------------
MAX_EP = 64            # the engine's max_endpoints in the literal tests
PROXY_PORT = 15001
PROXY_BE = L.htons(PROXY_PORT)   # the verdict of a redirect: the entry's raw be16 word
# (ep, sec_label, dport host order, proto, proxy port host order): ingress keys of endpoints 5 and 6
POLICY = [
    (5, 1001, 80, TCP, 0),             # exact, no proxy
    (5, 1001, 8080, TCP, PROXY_PORT),  # exact, to the proxy
    (5, 1002, 0, 0, 0),                # L3-only
    (5, 0, 53, UDP, 0),                # identity wildcard
    (5, 1003, 443, TCP, PROXY_PORT),   # an exact key and an L3 key of one identity
    (5, 1003, 0, 0, 0),
    (5, L.HOST_ID, 22, TCP, 0),        # a reserved label as a key
    (6, 1001, 443, TCP, 0),            # another endpoint's map
]
# lxc entries (endpoint id -> SECLABEL); ids 2 (below the last entry) and 9
# (past it) have none
SECLABELS = {3: 1001, 4: 1002}


def load_policy(t):
    for ep, lab, dport, proto, proxy in POLICY:
        assert t.policy_update(ep, L.policy_key(lab, dport, proto, 0), L.policy_entry(proxy)) == 0


def load_lxc(t):
    for ep, lab in SECLABELS.items():
        assert t.lxc_update(ep, L.lxc_info(b"\0" * 6, 0, b"\0" * 16, 0, lab)) == 0


def _p(x):
    return L.htons(x)


# (name, v6, gate, action, arg, src_label | None, src_ep | None, dport (network order), proto, flags, len,
#  expected (verdict, identity, stage))
CASES = [
    # ---- not LOCAL: every other action, arg garbage; nothing is interpreted ----
    *[(f"v4 action {a}", False, 1, a, 0xFFFFFFFF, 1001, None, _p(80), TCP, 0, 100, (0, 0, NOT_LOCAL))
      for a in (NONE, DROP, PROXY, HOST, OVERLAY, STACK, TIME_EXCEEDED)],
    *[(f"v6 action {a}", True, 1, a, 0xFFFFFFFF, 1001, None, _p(80), TCP, 0, 100, (0, 0, NOT_LOCAL))
      for a in (NONE, DROP, PROXY, HOST, OVERLAY, STACK, TIME_EXCEEDED)],
    ("v4 not local, gated protocol", False, 1, STACK, 5, 1002, None, 0, GRE, 0, 100, (0, 0, NOT_LOCAL)),
    # ---- ct_lookup4 / 6 protocol gate ----
    ("v4 gre gated", False, 1, LOCAL, 5, 1002, None, 0, GRE, 0, 100, (DROP_CT_UNKNOWN_PROTO, 0, 4)),
    ("v4 gre, gate off: the L3 key", False, 0, LOCAL, 5, 1002, None, 0, GRE, 0, 100, (0, 1002, 2)),
    ("v4 icmp passes the gate", False, 1, LOCAL, 5, 1002, None, 0, ICMP, 0, 100, (0, 1002, 2)),
    ("v4 icmpv6 number gated", False, 1, LOCAL, 5, 1002, None, 0, ICMP6, 0, 100, (DROP_CT_UNKNOWN_PROTO, 0, 4)),
    ("v6 proto 1 gated", True, 1, LOCAL, 5, 1002, None, 0, ICMP, 0, 100, (DROP_CT_UNKNOWN_PROTO, 0, 4)),
    ("v6 proto 1, gate off: the L3 key", True, 0, LOCAL, 5, 1002, None, 0, ICMP, 0, 100, (0, 1002, 2)),
    ("v6 icmpv6 passes the gate", True, 1, LOCAL, 5, 1002, None, 0, ICMP6, 0, 100, (0, 1002, 2)),
    # ---- the three probes ----
    ("v4 exact", False, 1, LOCAL, 5, 1001, None, _p(80), TCP, 0, 100, (0, 1001, 1)),
    ("v4 exact to the proxy", False, 1, LOCAL, 5, 1001, None, _p(8080), TCP, 0, 100, (PROXY_BE, 1001, 1)),
    ("v4 l3 only", False, 1, LOCAL, 5, 1002, None, _p(9999), UDP, 0, 100, (0, 1002, 2)),
    ("v4 wildcard", False, 1, LOCAL, 5, 1001, None, _p(53), UDP, 0, 100, (0, 1001, 3)),
    ("v4 miss", False, 1, LOCAL, 5, 1001, None, _p(81), TCP, 0, 100, (DROP_POLICY, 1001, 0)),
    ("v4 miss: the key is another endpoint's", False, 1, LOCAL, 5, 1001, None, _p(443), TCP, 0, 100,
     (DROP_POLICY, 1001, 0)),
    ("v4 the other endpoint", False, 1, LOCAL, 6, 1001, None, _p(443), TCP, 0, 100, (0, 1001, 1)),
    ("v4 endpoint without keys", False, 1, LOCAL, 7, 1001, None, _p(80), TCP, 0, 100, (DROP_POLICY, 1001, 0)),
    ("v6 exact", True, 1, LOCAL, 5, 1001, None, _p(80), TCP, 0, 100, (0, 1001, 1)),
    ("v6 exact to the proxy", True, 1, LOCAL, 5, 1001, None, _p(8080), TCP, 0, 100, (PROXY_BE, 1001, 1)),
    ("v6 l3 only", True, 1, LOCAL, 5, 1002, None, _p(9999), UDP, 0, 100, (0, 1002, 2)),
    ("v6 wildcard", True, 1, LOCAL, 5, 1001, None, _p(53), UDP, 0, 100, (0, 1001, 3)),
    ("v6 miss", True, 1, LOCAL, 5, 1001, None, _p(81), TCP, 0, 100, (DROP_POLICY, 1001, 0)),
    # ---- fragments: IPv4 skips probes 1 and 3; IPv6 passes is_fragment = false ----
    ("v4 exact key of 1003, whole packet", False, 1, LOCAL, 5, 1003, None, _p(443), TCP, 0, 100,
     (PROXY_BE, 1003, 1)),
    ("v4 fragment lands on the L3 key", False, 1, LOCAL, 5, 1003, None, _p(443), TCP, F_FRAGMENT, 100,
     (0, 1003, 2)),
    ("v4 fragment, no L3 key", False, 1, LOCAL, 5, 1001, None, _p(80), TCP, F_FRAGMENT, 100,
     (DROP_POLICY, 1001, 0)),
    ("v4 fragment skips the wildcard", False, 1, LOCAL, 5, 1001, None, _p(53), UDP, F_FRAGMENT, 100,
     (DROP_POLICY, 1001, 0)),
    ("v6 fragment bit: still the exact key", True, 1, LOCAL, 5, 1001, None, _p(80), TCP, F_FRAGMENT, 100,
     (0, 1001, 1)),
    ("v6 fragment bit: still the exact key of 1003", True, 1, LOCAL, 5, 1003, None, _p(443), TCP, F_FRAGMENT, 100,
     (PROXY_BE, 1003, 1)),
    # ---- the label is used as handed in ----
    # label 0: probe 1's key {0, 53, UDP} is the wildcard key itself
    ("v4 label 0 on the wildcard port", False, 1, LOCAL, 5, 0, None, _p(53), UDP, 0, 100, (0, 0, 1)),
    ("v4 label 0 miss", False, 1, LOCAL, 5, 0, None, _p(80), TCP, 0, 100, (DROP_POLICY, 0, 0)),
    ("v6 label 0 miss", True, 1, LOCAL, 5, 0, None, _p(80), TCP, 0, 100, (DROP_POLICY, 0, 0)),
    # HOST_ID while the engine's ipcache has every source address under 1002
    # (whose L3 key would allow port 22 at stage 2): the label wins
    ("v4 host label", False, 1, LOCAL, 5, L.HOST_ID, None, _p(22), TCP, 0, 100, (0, L.HOST_ID, 1)),
    ("v4 host label miss", False, 1, LOCAL, 5, L.HOST_ID, None, _p(23), TCP, 0, 100, (DROP_POLICY, L.HOST_ID, 0)),
    ("v6 host label", True, 1, LOCAL, 5, L.HOST_ID, None, _p(22), TCP, 0, 100, (0, L.HOST_ID, 1)),
    ("v4 world label miss", False, 1, LOCAL, 5, L.WORLD_ID, None, _p(22), TCP, 0, 100,
     (DROP_POLICY, L.WORLD_ID, 0)),
    # ---- the src_ep form ----
    ("v4 src_ep 3 is 1001", False, 1, LOCAL, 5, None, 3, _p(80), TCP, 0, 100, (0, 1001, 1)),
    ("v4 src_ep 4 is 1002", False, 1, LOCAL, 5, None, 4, _p(80), TCP, 0, 100, (0, 1002, 2)),
    ("v4 src_ep past the entries", False, 1, LOCAL, 5, None, 9, _p(53), UDP, 0, 100, (0, 0, 1)),
    ("v4 src_ep in a hole of the entries", False, 1, LOCAL, 5, None, 2, _p(80), TCP, 0, 100, (DROP_POLICY, 0, 0)),
    ("v4 src_ep 0xFFFF", False, 1, LOCAL, 5, None, 0xFFFF, _p(80), TCP, 0, 100, (DROP_POLICY, 0, 0)),
    ("v6 src_ep 3 is 1001", True, 1, LOCAL, 5, None, 3, _p(8080), TCP, 0, 100, (PROXY_BE, 1001, 1)),
    ("v6 src_ep past the entries", True, 1, LOCAL, 5, None, 9, _p(80), TCP, 0, 100, (DROP_POLICY, 0, 0)),
    ("v4 src_ep, not local", False, 1, HOST, 0xFFFFFFFF, None, 3, _p(80), TCP, 0, 100, (0, 0, NOT_LOCAL)),
    # ---- arg that names no policy map ----
    ("v4 arg = max_endpoints", False, 1, LOCAL, MAX_EP, 1002, None, _p(80), TCP, 0, 100, (DROP_POLICY, 1002, 0)),
    ("v4 arg 0x10000", False, 1, LOCAL, 0x10000, 1002, None, _p(80), TCP, 0, 100, (DROP_POLICY, 1002, 0)),
    ("v4 arg 0x10005: not endpoint 5", False, 1, LOCAL, 0x10005, 1002, None, _p(80), TCP, 0, 100,
     (DROP_POLICY, 1002, 0)),
    ("v4 arg 0xFFFFFFFF", False, 1, LOCAL, 0xFFFFFFFF, 1002, None, _p(80), TCP, 0, 100, (DROP_POLICY, 1002, 0)),
    ("v4 arg out of range, gated first", False, 1, LOCAL, 0x10000, 1002, None, 0, GRE, 0, 100,
     (DROP_CT_UNKNOWN_PROTO, 0, 4)),
    ("v6 arg = max_endpoints", True, 1, LOCAL, MAX_EP, 1002, None, _p(80), TCP, 0, 100, (DROP_POLICY, 1002, 0)),
    ("v6 arg 0x10005", True, 1, LOCAL, 0x10005, 1002, None, _p(80), TCP, 0, 100, (DROP_POLICY, 1002, 0)),
    # ---- the EGRESS bit is ignored ----
    ("v4 egress bit, exact", False, 1, LOCAL, 5, 1001, None, _p(80), TCP, F_EGRESS, 100, (0, 1001, 1)),
    ("v4 egress bit, fragment", False, 1, LOCAL, 5, 1003, None, _p(443), TCP, F_EGRESS | F_FRAGMENT, 100,
     (0, 1003, 2)),
    ("v6 egress bit, exact", True, 1, LOCAL, 5, 1001, None, _p(80), TCP, F_EGRESS, 100, (0, 1001, 1)),
    # ---- a packet too long for a packed counter takes the two-word path ----
    ("v4 long packet", False, 1, LOCAL, 5, 1001, None, _p(80), TCP, 0, (1 << 18) + 5, (0, 1001, 1)),
]


def case_rows(v6, gate, src_ep):
    """the CASES rows of one family, gate setting and label form"""
    return [c for c in CASES if c[1] == v6 and c[2] == gate and (c[6] is not None) == src_ep]


def columns(rows):
    """CASES rows as the step's columns (src_label or src_ep, whichever the rows carry)"""
    c = {"action": np.array([r[3] for r in rows], np.uint8), "arg": np.array([r[4] for r in rows], np.uint32),
         "dport": np.array([r[7] for r in rows], np.uint16), "proto": np.array([r[8] for r in rows], np.uint8),
         "flags": np.array([r[9] for r in rows], np.uint8), "len": np.array([r[10] for r in rows], np.uint32)}
    if rows and rows[0][6] is not None:
        c["src_ep"] = np.array([r[6] for r in rows], np.uint16)
    else:
        c["src_label"] = np.array([r[5] for r in rows], np.uint32)
    return c


def labels(c):
    """the label column of `columns`' result, whichever form it has"""
    return c["src_label"] if "src_label" in c else labels_of(c["src_ep"], SECLABELS)


def expected(rows):
    e = np.array([r[11] for r in rows], np.int64).reshape(-1, 3)
    return {"verdict": e[:, 0].astype(np.int32), "identity": e[:, 1].astype(np.uint32), "stage": e[:, 2].astype(np.uint8)}


# --------------------------------------------------------------------------
# the crafted policy tables (cascade_cases.policy_hops) as delivery batches
# --------------------------------------------------------------------------
def crafted_batch(v6=False):
    """the ingress rows of policy_workload()'s batch as LOCAL packets: arg =
    ep, label = id (IPv6: ICMP becomes ICMPv6, as tuples_v6 does)"""
    import cascade_cases as CC
    t = CC.policy_hops().tuples
    t = t[t["dir"] == 0]
    proto = t["proto"].astype(np.uint8)
    if v6:
        proto = np.where(proto == ICMP, ICMP6, proto).astype(np.uint8)
    n = len(t)
    return {"action": np.full(n, LOCAL, np.uint8), "arg": t["ep"].astype(np.uint32),
            "src_label": t["id"].astype(np.uint32), "dport": t["dport"].astype(np.uint16), "proto": proto,
            "flags": (t["frag"] << 1).astype(np.uint8), "len": t["len"].astype(np.uint32)}


def load_crafted_policy(t, phase, commit=None):
    """policy_workload()'s policy keys alone (the delivery step reads no ipcache)"""
    import cascade_cases as CC
    w = CC.policy_workload()
    for ep, k, e in w.pol1:
        assert t.policy_update(ep, k, e) == 0
    if phase == 2:
        if commit:
            commit()
        for ep, k, e in w.pol2:
            assert (t.policy_delete(ep, k) if e is None else t.policy_update(ep, k, e)) == 0


def head(b, n):
    return {k: v[:n] for k, v in b.items()}
