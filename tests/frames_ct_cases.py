"""Reference for the stateful path on raw frames (cgpu_frames_parse_ct,
cgpu_classify_frames_ct).

`restate_parse_ct` is the parse: Oracle.frames_parse (the restatement of
cgpu_frames_parse, unchanged) gives status / family / saddr / daddr / proto /
flags, and the three new columns are read here from the frame's bytes at the
offset lb_frames_cases.l4_of finds: the u16 at l4 + 0 and l4 + 2 of TCP / UDP
as loaded, the TCP u16 at l4 + 12, the ICMP / ICMPv6 type byte at l4
(bpf/lib/conntrack.h:471-530, :317-378).  A frame with status != 0 has them 0.

`Chain` restates cgpu_classify_frames_ct: the status-0 frames split by family
in frame order, Oracle.classify_v4_ct / classify_v6_ct on those columns and
the frame's len and ep, the results scattered back; a frame that ended in the
parse gets cgpu_classify_frames' result (verdict = status, 0 when not
classified; identity 0; stage 5, 4 for DROP_CT_UNKNOWN_PROTO, 7 when not
classified; ct_ret CT_NONE; rn columns 0) and is counted once in the metrics
at {(-status) & 0xff, dir} with its len, not-classified and DROP_SNAPLEN
frames not at all.

LITERAL is a table of hand-written bytes with hand-written expected columns.
"""
import numpy as np

from cilium_amd import layouts as L, synth
from forward_frames_cases import hx
from lb_frames_cases import ICMP, ICMP6, TCP, UDP, _h, l4_of, slot

NOW = 1000
SECLABEL = 5000
SIZES = (1, 63, 257, 4099)   # one lane, a partial wave, a partial workgroup, several workgroups


# --------------------------------------------------------------------------
# the world: one endpoint (the LXC addresses of synth, every egress check on),
# an ipcache and an L3 policy that allows some peers in both directions, some
# on ingress only (their egress packets are policy drops) and the rest not
# --------------------------------------------------------------------------
IPCACHE = [("10.1.0.0/16", 300), ("10.2.0.0/16", 301), ("2001:db8:1::/48", 400), ("2001:db8:2::/48", 401)]
# (sec_label, egress)
POLICY = [(300, 1), (300, 0), (301, 0), (400, 1), (400, 0), (401, 0)]
POLICY_KEYS = [L.policy_key(label, 0, 0, eg) for label, eg in POLICY]


def engine_config() -> dict:
    return dict(ct_proto_gate=1, lb_flags=L.LB_L3 | L.LB_L4, ipv6_router_ip=synth.ROUTER_IP6,
                ct_max=1 << 16, ct6_max=1 << 16)


def load_world(t, lxc: bool = True):
    """the tables through the map calls of an Engine or of the restatement"""
    for cidr, label in IPCACHE:
        assert t.ipcache_update(L.ipcache_key(cidr), L.remote_info(label)) == 0
    for k in POLICY_KEYS:
        assert t.policy_update(0, k, L.policy_entry(0)) == 0
    if lxc:
        assert t.lxc_update(0, L.lxc_info(synth.LXC_MAC, synth.LXC_IPV4_RAW, synth.LXC_IP6, 7, SECLABEL)) == 0


def make_oracle(load=load_world):
    from oracle import Oracle
    o = Oracle(ct_proto_gate=1, lb_l3=1, lb_l4=1, router_ip=synth.ROUTER_IP6)
    o.ct_set_max(1 << 16)
    o.ct6_set_max(1 << 16)
    load(o)
    return o


# --------------------------------------------------------------------------
# the parse
# --------------------------------------------------------------------------
PARSE_COLS = ("status", "family", "saddr", "daddr", "sport", "dport", "proto", "l4b", "flags")


def ct_fields(fr, v6: bool):
    """(sport, dport, l4b) of a frame the parse passed, from its bytes"""
    l4, proto = l4_of(fr, v6)
    if proto in (TCP, UDP):
        return _h(fr, l4), _h(fr, l4 + 2), (_h(fr, l4 + 12) if proto == TCP else 0)
    return 0, 0, int(fr[l4])


def restate_parse_ct(o, f: dict) -> dict:
    p = o.frames_parse(f)
    n = len(f["len"])
    out = {k: p[k] for k in ("status", "family", "saddr", "daddr", "proto", "flags")}
    for k in ("sport", "dport", "l4b"):
        out[k] = np.zeros(n, np.uint16)
    for i in np.nonzero(p["status"] == 0)[0]:
        out["sport"][i], out["dport"][i], out["l4b"][i] = ct_fields(f["data"][i].tobytes(), p["family"][i] == 6)
    return out


def compact(p: dict, f: dict, v6: bool):
    """(frame indices, the conntrack call's columns) of one family's status-0
    frames, in frame order"""
    idx = np.nonzero((p["status"] == 0) & (p["family"] == (6 if v6 else 4)))[0]
    t = {k: np.ascontiguousarray(p[k][idx]) for k in ("sport", "dport", "proto", "l4b", "flags")}
    for k in ("saddr", "daddr"):
        a = np.ascontiguousarray(p[k][idx])
        t[k] = a if v6 else np.ascontiguousarray(a[:, :4]).view("<u4")[:, 0].copy()
    t["len"] = np.ascontiguousarray(f["len"][idx], np.uint32)
    t["ep"] = np.ascontiguousarray(f["ep"][idx], np.uint16)
    return idx, t


# --------------------------------------------------------------------------
# the chain
# --------------------------------------------------------------------------
OUT_COLS = ("status", "family", "verdict", "ct_ret", "identity", "stage")
RN_COLS = ("rn_applied", "rn_sport", "rn_saddr", "rn_daddr", "rn_saddr6")


class Chain:
    """the restated cgpu_classify_frames_ct over consecutive batches: `o` holds
    the conntrack maps, counters and the conntrack calls' metrics, `extra` the
    metrics of the frames that ended in the parse"""

    def __init__(self, o=None):
        self.o = o or make_oracle()
        self.extra = np.zeros((256, 4, 2), np.uint64)

    def metrics(self):
        return self.o.metrics() + self.extra

    def run(self, f: dict, now: int = NOW, rev_nat: bool = False) -> dict:
        p = restate_parse_ct(self.o, f)
        n = len(f["len"])
        st = p["status"]
        nc = st == L.FRAME_NOT_CLASSIFIED
        out = {"status": st.copy(), "family": p["family"].copy(),
               "verdict": np.where(nc, 0, st).astype(np.int32),
               "ct_ret": np.full(n, L.CT_NONE, np.uint8), "identity": np.zeros(n, np.uint32),
               "stage": np.where(nc, 7, np.where(st == L.DROP_CT_UNKNOWN_PROTO, 4, 5)).astype(np.uint8)}
        if rev_nat:
            out.update(rn_applied=np.zeros(n, np.uint8), rn_sport=np.zeros(n, np.uint16),
                       rn_saddr=np.zeros(n, np.uint32), rn_daddr=np.zeros(n, np.uint32),
                       rn_saddr6=np.zeros((n, 16), np.uint8))
        for i in np.nonzero((st != 0) & ~nc & (st != L.DROP_SNAPLEN))[0]:
            self.extra[(-int(st[i])) & 0xff, (int(f["flags"][i]) & 1) + 1] += np.array([1, f["len"][i]], np.uint64)
        for v6 in (False, True):
            idx, t = compact(p, f, v6)
            if not len(idx):
                continue
            r = (self.o.classify_v6_ct if v6 else self.o.classify_v4_ct)(t, now, rev_nat=rev_nat)
            for k, x in zip(("verdict", "ct_ret", "identity", "stage"), r[:4]):
                out[k][idx] = x
            if rev_nat:
                rn = r[5]
                out["rn_applied"][idx] = rn["rn_applied"]
                out["rn_sport"][idx] = rn["rn_sport"]
                if v6:
                    out["rn_saddr6"][idx] = rn["rn_saddr"]
                else:
                    out["rn_saddr"][idx] = rn["rn_saddr"]
                    out["rn_daddr"][idx] = rn["rn_daddr"]
        return out


# --------------------------------------------------------------------------
# streams and mixed batches
# --------------------------------------------------------------------------
def _remotes4(rng, k):
    net = rng.choice([0x0A010000, 0x0A010000, 0x0A020000, 0x0B000000], k)   # allowed, ingress only, world
    return np.array([L.ip4_be(int(a)) for a in net + rng.integers(1, 0xFFFF, k)], np.uint32)


def _remotes6(rng, k):
    r = np.zeros((k, 16), np.uint8)
    r[:, 0:4] = [0x20, 0x01, 0x0d, 0xb8]
    r[:, 5] = rng.choice([1, 1, 2, 3], k)
    r[:, 12:16] = rng.integers(0, 256, (k, 4))
    return r


def make_streams(n_conn: int, seed: int = 7):
    """(IPv4 stream, IPv6 stream) of make_ct_stream over the world's endpoint"""
    rng = np.random.Generator(np.random.PCG64(seed))
    s4 = synth.make_ct_stream(rng, n_conn, np.array([synth.LXC_IPV4_RAW], np.uint32), _remotes4(rng, max(4, n_conn // 3)),
                              mean_pkts=6.0, other_frac=0.03, icmp_err_frac=0.08)
    s6 = synth.make_ct_stream(rng, n_conn, np.frombuffer(synth.LXC_IP6, np.uint8)[None, :],
                              _remotes6(rng, max(4, n_conn // 3)), mean_pkts=6.0, other_frac=0.03, icmp_err_frac=0.08)
    return s4, s6


ARP = hx("ff ff ff ff ff ff aa bb cc dd ee ff 08 06 00 01 08 00 06 04 00 01")
JUNK = ("arp", "short", "smac", "gre")


def make_mixed(n: int, stride: int, seed: int = 7, junk: float = 0.12, families=(4, 6)):
    """n frames: an IPv4 and an IPv6 stream merged, each keeping its order, with
    egress ARP frames, frames cut inside the fixed header, frames with a foreign
    source MAC and GRE frames between them (copies of the stream's neighbouring
    frame, so they sit between packets of one connection).  In 64-byte slots the
    IPv6 TCP frames end in DROP_SNAPLEN: their own class.  families: (4,), (6,)
    or both."""
    rng = np.random.Generator(np.random.PCG64(seed * 7919 + n * 31 + stride))
    per = max(2, int(n / (5.0 * len(families))) + 2)
    s4, s6 = make_streams(per, seed=seed + n)
    parts = []
    if 4 in families:
        parts.append(synth.frames_from_ct(s4, stride, v6=False)[0])
    if 6 in families:
        parts.append(synth.frames_from_ct(s6, stride, v6=True)[0])
    # merge: a random choice of the family at every position, each stream in its order
    tot = [len(p["len"]) for p in parts]
    which = np.concatenate([np.full(t, j) for j, t in enumerate(tot)])
    rng.shuffle(which)
    pos = [0] * len(parts)
    rows = []
    for w in which:
        rows.append((w, pos[w]))
        pos[w] += 1
    data, ln, fl = [], [], []
    for w, j in rows:
        p = parts[w]
        d, l_, g = p["data"][j].copy(), int(p["len"][j]), int(p["flags"][j])
        data.append(d)
        ln.append(l_)
        fl.append(g)
        if rng.random() < junk:
            kind = JUNK[int(rng.integers(0, len(JUNK)))]
            d2, l2, g2 = d.copy(), l_, g
            if kind == "arp":
                d2 = np.frombuffer(slot(ARP, stride), np.uint8).copy()
                l2, g2 = 64, 1
            elif kind == "short":
                l2 = 30
            elif kind == "smac":
                d2[6:12] = [0x11, 0x22, 0x33, 0x44, 0x55, 0x66]
                g2 = 1
            else:
                d2[20 if d2[12] == 0x86 else 23] = 47
            data.append(d2)
            ln.append(l2)
            fl.append(g2)
    assert len(data) >= n, (len(data), n)
    return {"data": np.stack(data[:n]), "len": np.array(ln[:n], np.uint32), "flags": np.array(fl[:n], np.uint8),
            "ep": np.zeros(n, np.uint16)}


def classes(out: dict, f: dict) -> set:
    """the classes a chain output holds (the tests assert none is lost)"""
    c = set()
    names = {L.CT_NEW: "new", L.CT_ESTABLISHED: "established", L.CT_REPLY: "reply", L.CT_RELATED: "related"}
    for k, v in names.items():
        if (out["ct_ret"] == k).any():
            c.add(v)
    st = out["status"]
    if (st == L.DROP_CT_UNKNOWN_PROTO).any():
        c.add("gre")
    if ((st != 0) & (st != L.DROP_CT_UNKNOWN_PROTO)).any():
        c.add("ended")
    if ((st == 0) & (out["verdict"] == L.DROP_POLICY)).any():
        c.add("policy drop")
    for fam in (4, 6):
        if ((st == 0) & (out["family"] == fam)).any():
            c.add(f"v{fam}")
    if "rn_applied" in out and (out["rn_applied"] == 1).any():
        c.add("rn applied")
    return c


ALL_CLASSES = {"new", "established", "reply", "related", "gre", "ended", "policy drop", "v4", "v6"}


# --------------------------------------------------------------------------
# the literal frames
# --------------------------------------------------------------------------
E4 = "de ad be ef c0 de aa bb cc dd ee ff 08 00"    # dmac NODE_MAC, smac LXC_MAC
E6 = "de ad be ef c0 de aa bb cc dd ee ff 86 dd"
LX4, RM4 = "40 30 20 10", "0a 01 00 05"             # the endpoint 64.48.32.16, the peer 10.1.0.5
LX6 = "be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc"
RM6 = "20 01 0d b8 00 01 00 00 00 00 00 00 00 00 00 05"
RT6 = "be ef 00 00 00 00 00 00 00 00 00 01 00 01 00 00"   # ROUTER_IP
PAY = "c0 c1 c2 c3 c4 c5 c6 c7 c8 c9 ca cb cc cd ce cf d0 d1 d2 d3 d4 d5 d6 d7 d8 d9"
TCP_SYN = "9c 40 00 50 01 02 03 04 00 00 00 00 51 02 20 00 00 00 00 00"      # doff 5 | NS in byte 12, SYN in 13
TCP_SA = "00 50 9c 40 01 02 03 04 00 00 00 00 50 12 20 00 00 00 00 00"       # SYN | ACK back
UDP_H = "30 39 00 35 00 12 00 00"
IP4_EG = "45 00 00 32 12 34 40 00 40 %s 00 00 " + LX4 + " " + RM4
IP4_IN = "45 00 00 32 12 34 40 00 40 %s 00 00 " + RM4 + " " + LX4
IP6_EG = "60 00 00 00 00 1a %s 40 " + LX6 + " " + RM6
IP6_IN = "60 00 00 00 00 1a %s 40 " + RM6 + " " + LX6
OPT40 = " ".join(["01"] * 40)

# (name, stride, len, flags in, frame bytes, status, then for status 0: family, sport, dport, proto, l4b, flags out)
LITERAL = [
    ("v4 tcp: byte 12 is the low half of l4", 64, 64, 1, (E4, IP4_EG % "06", TCP_SYN, PAY),
     0, 4, 0x409c, 0x5000, 6, 0x0251, 1),
    ("v4 tcp behind 8 bytes of options: l4 = 42", 128, 70, 0,
     (E4, "47 00 00 38 12 34 40 00 40 06 00 00", RM4, LX4, "01 01 01 01 01 01 01 00", TCP_SA, PAY),
     0, 4, 0x5000, 0x409c, 6, 0x1250, 0),
    ("v4 ihl 15 in a 64-byte slot", 64, 100, 0,
     (E4, "4f 00 00 56 12 34 40 00 40 06 00 00", RM4, LX4, OPT40, TCP_SA, PAY),
     L.DROP_SNAPLEN),
    ("v4 ihl 15 in a 128-byte slot", 128, 100, 0,
     (E4, "4f 00 00 56 12 34 40 00 40 06 00 00", RM4, LX4, OPT40, TCP_SA, PAY),
     0, 4, 0x5000, 0x409c, 6, 0x1250, 0),
    ("v4 tcp, len = l4 + 13", 64, 47, 0, (E4, IP4_IN % "06", TCP_SA, PAY), L.DROP_CT_INVALID_HDR),
    ("v4 tcp, len = l4 + 14", 64, 48, 0, (E4, IP4_IN % "06", TCP_SA, PAY), 0, 4, 0x5000, 0x409c, 6, 0x1250, 0),
    ("v4 udp, len = l4 + 3, ingress", 64, 37, 0, (E4, IP4_IN % "11", UDP_H, PAY), L.DROP_CT_INVALID_HDR),
    ("v4 udp, len = l4 + 3, egress under LB_L4", 64, 37, 1, (E4, IP4_EG % "11", UDP_H, PAY), L.EFAULT_LOAD),
    ("v4 udp", 64, 60, 1, (E4, IP4_EG % "11", UDP_H, PAY), 0, 4, 0x3930, 0x3500, 17, 0, 1),
    ("v4 icmp echo request", 64, 60, 1, (E4, IP4_EG % "01", "08 00 00 00 00 07 00 01", PAY), 0, 4, 0, 0, 1, 8, 1),
    ("v4 icmp echo reply", 64, 60, 0, (E4, IP4_IN % "01", "00 00 00 00 00 07 00 01", PAY), 0, 4, 0, 0, 1, 0, 0),
    ("v4 icmp destination unreachable", 64, 60, 0, (E4, IP4_IN % "01", "03 01 00 00 00 00 00 00", PAY),
     0, 4, 0, 0, 1, 3, 0),
    ("v4 ingress fragment", 64, 60, 0,
     (E4, "45 00 00 32 12 34 20 00 40 11 00 00", RM4, LX4, UDP_H, PAY), 0, 4, 0x3930, 0x3500, 17, 0, 2),
    ("v4 gre", 64, 60, 0, (E4, IP4_IN % "2f", "00 00 08 00", PAY), L.DROP_CT_UNKNOWN_PROTO),
    ("egress arp", 64, 60, 1, ("ff ff ff ff ff ff aa bb cc dd ee ff 08 06 00 01 08 00 06 04 00 01",),
     L.FRAME_NOT_CLASSIFIED),
    ("a foreign source mac", 64, 64, 1, ("de ad be ef c0 de 11 22 33 44 55 66 08 00", IP4_EG % "06", TCP_SYN, PAY),
     L.DROP_INVALID_SMAC),
    ("v6 tcp in an 80-byte slot: the flag word at 66", 80, 80, 1, (E6, IP6_EG % "06", TCP_SYN, PAY),
     0, 6, 0x409c, 0x5000, 6, 0x0251, 1),
    ("v6 tcp in a 64-byte slot", 64, 80, 1, (E6, IP6_EG % "06", TCP_SYN, PAY), L.DROP_SNAPLEN),
    ("v6 hop-by-hop, then udp: l4 = 62", 80, 76, 0,
     (E6, IP6_IN % "00", "11 00 01 04 00 00 00 00", UDP_H, PAY), 0, 6, 0x3930, 0x3500, 17, 0, 0),
    ("v6 fragment header", 80, 76, 0, (E6, IP6_IN % "2c", "11 00 00 00 00 00 00 01", UDP_H, PAY),
     L.DROP_FRAG_NOSUPPORT),
    ("egress icmpv6 echo to ROUTER_IP", 80, 70, 1,
     (E6, "60 00 00 00 00 10 3a 40", LX6, RT6, "80 00 00 00 00 07 00 01", PAY), L.FRAME_NOT_CLASSIFIED),
    ("egress icmpv6 echo to a peer", 80, 70, 1,
     (E6, "60 00 00 00 00 10 3a 40", LX6, RM6, "80 00 00 00 00 07 00 01", PAY), 0, 6, 0, 0, 58, 128, 1),
]


def literal_strides():
    return sorted({r[1] for r in LITERAL})


def literal_batch(stride: int):
    """(rows, frames dict) of the table's rows of one stride"""
    rows = [r for r in LITERAL if r[1] == stride]
    n = len(rows)
    f = {"data": np.stack([np.frombuffer(slot(hx(*r[4]), stride), np.uint8) for r in rows]),
         "len": np.array([r[2] for r in rows], np.uint32), "flags": np.array([r[3] for r in rows], np.uint8),
         "ep": np.zeros(n, np.uint16)}
    return rows, f


def literal_expected(rows):
    """{column: expected} over the rows, and the mask of status-0 rows (the
    address columns of those rows come from the bytes: IPv4 26 / 30, IPv6 22 / 38)"""
    n = len(rows)
    exp = {"status": np.array([r[5] for r in rows], np.int32)}
    ok = exp["status"] == 0
    for j, (k, dt) in enumerate((("family", np.uint8), ("sport", np.uint16), ("dport", np.uint16),
                                 ("proto", np.uint8), ("l4b", np.uint16), ("flags", np.uint8))):
        exp[k] = np.array([r[6 + j] if r[5] == 0 else 0 for r in rows], dt)
    exp["saddr"] = np.zeros((n, 16), np.uint8)
    exp["daddr"] = np.zeros((n, 16), np.uint8)
    for i, r in enumerate(rows):
        if r[5] != 0:
            continue
        b = hx(*r[4])
        if r[6] == 4:
            exp["saddr"][i, :4] = list(b[26:30])
            exp["daddr"][i, :4] = list(b[30:34])
        else:
            exp["saddr"][i] = list(b[22:38])
            exp["daddr"][i] = list(b[38:54])
    return exp, ok


def check_parse(got: dict, exp: dict, ended=None):
    """status everywhere; every column where status == 0; sport / dport / l4b 0
    elsewhere; with `ended` (cgpu_frames_parse's own columns of the same frames)
    family, saddr, daddr, proto and flags of the other frames too"""
    np.testing.assert_array_equal(got["status"], exp["status"])
    ok = exp["status"] == 0
    for k in PARSE_COLS[1:]:
        if got.get(k) is None:
            continue
        np.testing.assert_array_equal(got[k][ok], exp[k][ok], err_msg=k)
        if k in ("sport", "dport", "l4b"):
            assert not got[k][~ok].any(), k
        elif ended is not None:
            np.testing.assert_array_equal(got[k][~ok], ended[k][~ok], err_msg=k + " of the ended frames")


# --------------------------------------------------------------------------
# the reverse NAT chain: the service connections of revnat_cases as frames
# with valid checksums, the whole packet inside the slot
# --------------------------------------------------------------------------
RN_STRIDE = 128


def rnat_engine_config() -> dict:
    import revnat_cases as rc
    return dict(ct_max=1 << 14, ct6_max=1 << 14, ipv6_router_ip=rc.ROUTER6)


def rnat_env(t):
    """revnat_cases' environments of both families into an Engine or the
    restatement, and the IPv6 reverse NAT map"""
    import revnat_cases as rc
    rc._env4(t)
    rc._env6(t)
    for ix, (addr, port) in rc._rmap6().items():
        v = np.zeros((), L.LB6_REVERSE_NAT)
        v["address"][:], v["port"] = np.frombuffer(addr, np.uint8), port
        assert t.revnat6_update(ix, v) == 0


def rnat_oracle():
    import revnat_cases as rc
    from oracle import Oracle
    o = Oracle(ct_proto_gate=1, lb_l3=1, lb_l4=1, router_ip=rc.ROUTER6)
    o.ct_set_max(1 << 14)
    o.ct6_set_max(1 << 14)
    rnat_env(o)
    return o


def packet_frame(t: dict, i: int, v6: bool) -> bytes:
    """packet i of a conntrack batch as a whole frame, every checksum valid"""
    import struct
    from lb_frames_cases import build_frame, l4_checksum
    proto, l4b = int(t["proto"][i]), int(t["l4b"][i])
    if v6:
        sa, da = bytes(t["saddr"][i]), bytes(t["daddr"][i])
    else:
        sa, da = struct.pack("<I", int(t["saddr"][i])), struct.pack("<I", int(t["daddr"][i]))
    sp, dp = (int(np.uint16(t[k][i]).byteswap()) for k in ("sport", "dport"))
    fr = bytearray(build_frame(v6, proto, sa, da, sp, dp, bytes(range(0xB0, 0xB8)), icmp_type=l4b & 0xff))
    if proto == TCP:
        l4 = 54 if v6 else 34
        fr[l4 + 12], fr[l4 + 13] = l4b & 0xff, l4b >> 8
        fr[l4 + 16:l4 + 18] = b"\0\0"
        fr[l4 + 16:l4 + 18] = struct.pack(">H", l4_checksum(v6, proto, sa, da, bytes(fr[l4:])))
    return bytes(fr)


def rnat_batch(n: int):
    """about n frames: revnat_cases' IPv4 pure hits and IPv6 hits / ingress
    connections merged (each family in its order) with an egress ARP frame
    after every 16th.  Returns (frames dict, IPv4 entries, IPv6 entries) --
    the entries go into the maps before the batch runs."""
    import revnat_cases as rc
    t4, ents4 = rc.build_v4_hits(max(1, n // 2))[:2]
    t6, ents6 = rc.build_v6(max(1, n // 4), n // 12)[:2]
    n4, n6 = len(t4["proto"]), len(t6["proto"])
    rng = np.random.Generator(np.random.PCG64(n))
    which = np.concatenate([np.zeros(n4, np.int64), np.ones(n6, np.int64)])
    rng.shuffle(which)
    pos = [0, 0]
    data, ln, fl = [], [], []
    for j, w in enumerate(which):
        t = (t4, t6)[w]
        i = pos[w]
        pos[w] += 1
        fr = packet_frame(t, i, bool(w))
        assert len(fr) <= RN_STRIDE
        data.append(np.frombuffer(slot(fr, RN_STRIDE), np.uint8))
        ln.append(len(fr))
        fl.append(int(t["flags"][i]) & 1)
        if j % 16 == 15:
            data.append(np.frombuffer(slot(ARP, RN_STRIDE), np.uint8))
            ln.append(64)
            fl.append(1)
    m = len(data)
    f = {"data": np.stack(data), "len": np.array(ln, np.uint32), "flags": np.array(fl, np.uint8),
         "ep": np.zeros(m, np.uint16)}
    return f, ents4, ents6


def rnat_install(t, ents4, ents6):
    for k, v in ents4:
        assert t.ct4_update(k, v) == 0
    for k, v in ents6:
        assert t.ct6_update(k, v) == 0
