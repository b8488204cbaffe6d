"""Reference for the service step on raw frames (cgpu_classify_frames_lb).

`restate_frame_lb` restates, per frame, what handle_ipv4_from_lxc /
ipv6_l3_from_lxc do between the endpoint checks and ct_lookup:

* bpf_lxc.c:444-460 / :117-139: lb{4,6}_extract_key, lb{4,6}_lookup_service,
  lb{4,6}_local with an empty conntrack table (lib/lb.h:192-216, :604-635,
  :351-380, :700-775, :426-483): the L4 key, then with key.dport = 0 the L3 key;
  the slave by hash % count + 1; the fallback that keeps the slave in the key;
  the loopback source NAT;
* lib/lb.h:653-697 (lb4_xlate) and :398-424 (lb6_xlate) with lib/l4.h:50-60
  (l4_modify_port, from = key.dport as the lookups left it) and lib/csum.h
  (csum_l4_offset_and_flags, csum_l4_replace); the kernel's csum_diff,
  bpf_l3_csum_replace and bpf_l4_csum_replace are written out literally below
  on the words as loaded, BPF_F_MARK_MANGLED_0 included.

Everything before the step (the ethertype dispatch, the ICMPv6 responders, the
MAC / SIP checks, ipv6_hdrlen, extract_l4_port) and everything after it
(ct_lookup's port extraction and protocol gate, the ipcache and policy
decision, counters and metrics) is the frame restatement's, which the
reference's golden vectors pin (tests/test_frames_golden.py): a frame the step
leaves alone is classified as it came, a translated frame as it was rewritten.
A loopback frame, whose tuple keeps the service address, is classified on that
tuple.

`build_frame` makes frames whose checksums are valid from scratch (RFC 1071,
pseudo header included) and `frame_verifies` checks them from scratch: neither
shares a line with the incremental arithmetic.  LITERAL is a hand-written table
of bytes in and bytes out against `literal_world`; its checksums were worked
out from scratch over the translated packet, or for the rows whose input
verifies nothing by one's-complement arithmetic on the 16-bit wire words.
"""
import ipaddress
import struct
from dataclasses import dataclass, field

import numpy as np

from cilium_amd import layouts as L, synth
from forward_frames_cases import M32, _csum_add, csum_rfc1071, hx

TCP, UDP, ICMP, ICMP6 = 6, 17, 1, 58
NONE, XLATED, LOOPBACK = L.LB_NONE, L.LB_XLATED, L.LB_XLATED_LOOPBACK
DROP_NO_SERVICE, DROP_CSUM_L4, DROP_SNAPLEN = L.DROP_NO_SERVICE, L.DROP_CSUM_L4, L.DROP_SNAPLEN
DROP_CT_INVALID_HDR, DROP_CT_UNKNOWN_PROTO = L.DROP_CT_INVALID_HDR, L.DROP_CT_UNKNOWN_PROTO
E = 1  # CGPU_F_EGRESS


def a4(s: str) -> int:
    """an IPv4 address as the u32 a little-endian load of its wire bytes gives"""
    return L.ip4_be(s)


def a6(s: str) -> bytes:
    return ipaddress.ip_address(s).packed


def be16(x: int) -> int:
    """a host-order port as the raw u16 of its wire bytes"""
    return L.htons(x)


# --------------------------------------------------------------------------
# the world: service maps as the datapath's keys and values, an ipcache and
# a policy for the decision afterwards
# --------------------------------------------------------------------------
@dataclass
class LbWorld:
    """svc4: {(address, dport, slave): (target, port, count, rev_nat_index)} with
    every field as stored (raw words); svc6 the same with 16-byte addresses"""
    gate: int = 1
    lb_flags: int = L.LB_L3 | L.LB_L4
    loopback: int = L.IPV4_LOOPBACK
    verify: int = 7
    n_ep: int = 4
    svc4: dict = field(default_factory=dict)
    svc6: dict = field(default_factory=dict)
    ipcache: list = field(default_factory=list)   # (cidr, sec_label)
    policy: list = field(default_factory=list)    # (ep, sec_label, dport host order, proto, egress)
    oracle: object = None                         # the frame restatement, loaded with all of it
    pre: object = None                            # the same endpoints without CONNTRACK: the parse up to the step
    extra: np.ndarray = None                      # metrics of the step's own drops, beside oracle.metrics()

    def service4(self, addr: str, port: int, backends, rev_nat: int, count=None, rows=None):
        """a frontend as lbmap writes it: slave 0 = {count}, slaves 1..n = the
        backends (target, port host order); `rows`: the slaves to install (a
        missing row is a deleted backend); `count` in the backend rows too when
        given (what the fallback's lb4_lookup_service tests)"""
        k = (a4(addr), be16(port))
        self.svc4[k + (0,)] = (0, 0, len(backends), 0)
        for i, (tg, tp) in enumerate(backends, 1):
            if rows is None or i in rows:
                self.svc4[k + (i,)] = (a4(tg), be16(tp), count or 0, be16(rev_nat))

    def service6(self, addr: str, port: int, backends, rev_nat: int, count=None, rows=None):
        k = (a6(addr), be16(port))
        self.svc6[k + (0,)] = (bytes(16), 0, len(backends), 0)
        for i, (tg, tp) in enumerate(backends, 1):
            if rows is None or i in rows:
                self.svc6[k + (i,)] = (a6(tg), be16(tp), count or 0, be16(rev_nat))

    def engine_config(self) -> dict:
        return dict(ct_proto_gate=self.gate, lb_flags=self.lb_flags, ipv4_loopback=self.loopback)

    def metrics(self) -> np.ndarray:
        return self.oracle.metrics() + self.extra


def load_world(t, w: LbWorld):
    """every key of the world through the map calls of an Engine or of the
    restatement"""
    lb4 = t.lb4_update if hasattr(t, "lb4_update") else t.lb_update
    for (addr, dport, slave), (tg, port, count, rn) in w.svc4.items():
        k = np.zeros((), L.LB4_KEY)
        k["address"], k["dport"], k["slave"] = addr, dport, slave
        v = np.zeros((), L.LB4_SERVICE)
        v["target"], v["port"], v["count"], v["rev_nat_index"] = tg, port, count, rn
        assert lb4(k, v) == 0
    for (addr, dport, slave), (tg, port, count, rn) in w.svc6.items():
        k = np.zeros((), L.LB6_KEY)
        k["address"], k["dport"], k["slave"] = np.frombuffer(addr, np.uint8), dport, slave
        v = np.zeros((), L.LB6_SERVICE)
        v["target"], v["port"], v["count"], v["rev_nat_index"] = np.frombuffer(tg, np.uint8), port, count, rn
        assert t.lb6_update(k, v) == 0
    for cidr, label in w.ipcache:
        v = np.zeros((), L.REMOTE_ENDPOINT_INFO)
        v["sec_label"] = label
        assert t.ipcache_update(L.ipcache_key(cidr), v) == 0
    for ep, label, dport, proto, egress in w.policy:
        assert t.policy_update(ep, L.policy_key(label, dport, proto, egress), L.policy_entry(0)) == 0
    info = L.lxc_info(synth.LXC_MAC, synth.LXC_IPV4_RAW, synth.LXC_IP6, w.verify)
    for ep in range(w.n_ep):
        assert t.lxc_update(ep, info) == 0


def attach_oracle(w: LbWorld, **cfg) -> LbWorld:
    """a fresh restatement with the world loaded, and zeroed extra metrics"""
    from oracle import Oracle
    w.oracle = Oracle(ct_proto_gate=w.gate, lb_l3=int(bool(w.lb_flags & L.LB_L3)),
                      lb_l4=int(bool(w.lb_flags & L.LB_L4)), ipv4_loopback=w.loopback, **cfg)
    load_world(w.oracle, w)
    w.pre = Oracle(ct_proto_gate=0, lb_l3=int(bool(w.lb_flags & L.LB_L3)), lb_l4=int(bool(w.lb_flags & L.LB_L4)), **cfg)
    info = L.lxc_info(synth.LXC_MAC, synth.LXC_IPV4_RAW, synth.LXC_IP6, w.verify)
    for ep in range(w.n_ep):
        assert w.pre.lxc_update(ep, info) == 0
    w.extra = np.zeros((256, 4, 2), np.uint64)
    return w


# --------------------------------------------------------------------------
# checksum helpers of the kernel, on the words as loaded
# --------------------------------------------------------------------------
def _fold_not(t: int) -> int:
    """(u16)~csum_fold's two folding rounds"""
    t = (t & 0xFFFF) + (t >> 16)
    t = (t & 0xFFFF) + (t >> 16)
    return ~t & 0xFFFF


def csum_diff(frm: bytes, to: bytes, seed: int = 0) -> int:
    """bpf_csum_diff(from, size, to, size, seed) over 4 or 16 bytes: every
    from-word complemented, then every to-word, added to the seed"""
    d = seed
    for (w,) in struct.iter_unpack("<I", frm):
        d = _csum_add(d, ~w & M32)
    for (w,) in struct.iter_unpack("<I", to):
        d = _csum_add(d, w)
    return d


def csum_replace_diff(c: int, d: int) -> int:
    """l3_csum_replace(off, 0, D, 0) / l4_csum_replace(off, 0, D, BPF_F_PSEUDO_HDR)
    on the field c: csum_replace_by_diff"""
    return _fold_not(_csum_add(d, ~c & M32))


def csum_replace2(c: int, frm: int, to: int) -> int:
    """l4_csum_replace(off, from, to, 2): csum_replace2 as inet_proto_csum_replace2
    reaches it"""
    return _fold_not(_csum_add(_csum_add(~c & M32, ~frm & M32), to))


def _mangled0(c: int, new: int, udp: bool) -> int:
    """BPF_F_MARK_MANGLED_0: a field of 0 is not patched; a patch that gives 0
    stores CSUM_MANGLED_0"""
    if udp and c == 0:
        return 0
    return 0xFFFF if udp and new == 0 else new


# --------------------------------------------------------------------------
# one frame through the call
# --------------------------------------------------------------------------
def _h(fr, off: int) -> int:
    return fr[off] | fr[off + 1] << 8


def l4_of(fr, v6: bool):
    """(l4 offset, protocol) of a frame the parse has passed: ipv4_hdrlen, or
    ipv6_hdrlen's walk (lib/ipv6.h:61-98, the AUTH length rule as written)"""
    if not v6:
        return 14 + 4 * (fr[14] & 15), fr[23]
    nh, off = fr[20], 40
    for _ in range(4):
        if nh not in (0, 43, 51, 60):
            break
        o = 14 + off
        hl = fr[o + 1]
        nh = fr[o]
        off += (hl + 2) << 2 if nh == 51 else (hl + 1) << 3
    return 14 + off, nh


def _lookup_service(svc: dict, lb_flags: int, addr, key: list, slave: int):
    """lb{4,6}_lookup_service on key = [dport]: the L4 key when its count is not
    0, else key.dport = 0 and the L3 key"""
    if (lb_flags & L.LB_L4) and key[0]:
        s = svc.get((addr, key[0], slave))
        if s is not None and s[2]:
            return s
        key[0] = 0
    if lb_flags & L.LB_L3:
        s = svc.get((addr, key[0], slave))
        if s is not None and s[2]:
            return s
    return None


def service_step(w: LbWorld, fr, length: int, hash_, flow_hash):
    """the step on a frame that passed extract_l4_port: None when the frame is
    not load-balanced, else (lb_ret, rev_nat, slave, writes) with writes = the
    stores [(offset, bytes)] in the reference's order (none for a drop)"""
    cap = min(length, len(fr))
    v6 = bytes(fr[12:14]) == b"\x86\xdd"
    l4, proto = l4_of(fr, v6)
    tu = proto in (TCP, UDP)
    key = [0]
    if w.lb_flags & L.LB_L4:
        if tu:
            key[0] = _h(fr, l4 + 2)
        elif proto not in (ICMP, ICMP6):
            return None                                         # DROP_UNKNOWN_L4: skip_service_lookup
    svc = w.svc6 if v6 else w.svc4
    addr = bytes(fr[38:54]) if v6 else struct.unpack_from("<I", fr, 30)[0]
    saddr = bytes(fr[22:38]) if v6 else struct.unpack_from("<I", fr, 26)[0]
    kd0 = key[0]
    s = _lookup_service(svc, w.lb_flags, addr, key, 0)
    if s is None:
        return None
    if w.gate and proto not in (TCP, UDP, ICMP6 if v6 else ICMP):
        return (DROP_NO_SERVICE, 0, 0, [])                      # ct_lookup(CT_SERVICE): DROP_CT_UNKNOWN_PROTO
    if hash_ is None:
        sport = _h(fr, l4) if tu and l4 + 2 <= cap else 0
        hash_ = flow_hash(saddr, addr, sport, kd0, proto)
    slave = hash_ % s[2] + 1
    b = svc.get((addr, key[0], slave))                          # lb{4,6}_lookup_slave
    if b is None:
        b = _lookup_service(svc, w.lb_flags, addr, key, slave)  # the key keeps the slave
        if b is None:
            return (DROP_NO_SERVICE, 0, 0, [])
        slave = hash_ % b[2] + 1
    target, port, _, rev_nat = b
    loop = not v6 and saddr == target
    ret = LOOPBACK if loop else XLATED
    # ---- lb4_xlate / lb6_xlate ----
    coff = {TCP: 16, UDP: 6, ICMP6: 2}.get(proto, 0)            # csum_l4_offset_and_flags
    l4c = v6 or coff != 0                                       # `if (csum_off->offset)` / `if (csum_off)`
    p = l4 + coff
    if l4c and p + 2 > length:
        return (DROP_CSUM_L4, 0, 0, [])
    if l4c and p + 2 > cap:
        return (DROP_SNAPLEN, 0, 0, [])
    udp = proto == UDP
    writes = []
    if v6:
        writes.append((38, target))
        d = csum_diff(addr, target)
    else:
        new_da = struct.pack("<I", target)
        writes.append((30, new_da))
        d = csum_diff(struct.pack("<I", addr), new_da)
        if loop and w.loopback:
            new_sa = struct.pack("<I", w.loopback)
            writes.append((26, new_sa))
            d = csum_diff(struct.pack("<I", saddr), new_sa, d)
        writes.append((24, struct.pack("<H", csum_replace_diff(_h(fr, 24), d))))
    c = _h(fr, p) if l4c else 0
    if l4c:
        c1 = _mangled0(c, csum_replace_diff(c, d), udp)
        writes.append((p, struct.pack("<H", c1)))
        c = c1
    if (w.lb_flags & L.LB_L4) and port and key[0] != port and tu:
        c1 = _mangled0(c, csum_replace2(c, key[0], port), udp)  # l4_modify_port(.., port, key->dport)
        writes.append((p, struct.pack("<H", c1)))
        writes.append((l4 + 2, struct.pack("<H", port)))
    return (ret, rev_nat, slave, writes)


def _one(fr, length, flags, ep):
    return {"data": np.frombuffer(bytes(fr), np.uint8).reshape(1, -1), "len": np.array([length], np.uint32),
            "flags": np.array([flags], np.uint8), "ep": np.array([ep], np.uint16)}


def restate_frame_lb(w: LbWorld, frame: bytearray, length: int, flags: int, ep: int, hash_=None,
                     rewrite: bool = True):
    """(verdict, identity, stage, lb_ret, rev_nat, slave) of one slot; with
    `rewrite` the slot's bytes are translated in place.  Counters and metrics
    accumulate in w.oracle and w.extra."""
    o = w.oracle
    one = _one(frame, length, flags, ep)
    st = int(o.frames_parse(one)["status"][0])
    step = None
    # the parse without CONNTRACK ends behind extract_l4_port: status 0 there = the frame reaches the step
    if (flags & E) and int(w.pre.frames_parse(one)["status"][0]) == 0:
        def fh(sa, da, sp, dp, pr):
            return o.flow_hash6(sa, da, sp, dp, pr) if isinstance(sa, bytes) else o.flow_hash(sa, da, sp, dp, pr)
        step = service_step(w, frame, length, hash_, fh)
    if step is None:
        v, i, s, _ = o.classify_frames(one)
        return (int(v[0]), int(i[0]), int(s[0]), NONE, 0, 0)
    ret, rev_nat, slave, writes = step
    if ret < 0:
        if ret != DROP_SNAPLEN:
            w.extra[-ret & 0xFF, 2] += np.array([1, length], np.uint64)   # {reason, egress}
        return (ret, 0, 6 if ret == DROP_NO_SERVICE else 5, ret, 0, 0)
    new = bytearray(frame)
    for off, b in writes:
        new[off:off + len(b)] = b
    if ret == XLATED or st != 0:
        # the frame as rewritten through the rest of the program (a loopback
        # frame that ends in ct_lookup: as it came, its saddr passes the SIP check)
        v, i, s, _ = o.classify_frames(_one(new if ret == XLATED else frame, length, flags, ep))
    else:
        # loopback: tuple.daddr keeps the service address
        l4, proto = l4_of(new, False)
        # ct_lookup4 reloads the dport from the packet as rewritten (0 without CONNTRACK)
        dport = int(o.frames_parse(one)["dport"][0])
        if w.gate and proto in (TCP, UDP):
            dport = _h(new, l4 + 2)
        t = {"saddr": np.array([w.loopback], np.uint32),
             "daddr": np.array([struct.unpack_from("<I", frame, 30)[0]], np.uint32),
             "dport": np.array([dport], np.uint16), "proto": np.array([proto], np.uint8),
             "flags": np.array([E], np.uint8), "len": np.array([length], np.uint32), "ep": np.array([ep], np.uint16)}
        v, i, s, _ = o.classify_v4(t)
    if rewrite:
        frame[:] = new
    return (int(v[0]), int(i[0]), int(s[0]), ret, rev_nat, slave)


COLS = ("verdict", "identity", "stage", "lb_ret", "rev_nat", "slave")
DTYPES = (np.int32, np.uint32, np.uint8, np.int32, np.uint16, np.uint16)


def restate_frames_lb(w: LbWorld, f: dict, hash_=None, rewrite: bool = True):
    """a batch through restate_frame_lb: the six columns and the data afterwards"""
    n = len(f["len"])
    out = np.zeros((n, 6), np.int64)
    data = f["data"].copy()
    for i in range(n):
        fr = bytearray(data[i].tobytes())
        out[i] = restate_frame_lb(w, fr, int(f["len"][i]), int(f["flags"][i]), int(f["ep"][i]),
                                  None if hash_ is None else int(hash_[i]), rewrite)
        data[i] = np.frombuffer(bytes(fr), np.uint8)
    return {k: out[:, j].astype(dt) for j, (k, dt) in enumerate(zip(COLS, DTYPES))}, data


# --------------------------------------------------------------------------
# frames with checksums valid from scratch, and the check from scratch
# --------------------------------------------------------------------------
def _sum16(b: bytes) -> int:
    """RFC 1071 over b (padded to even), the big-endian u16 for the wire"""
    return csum_rfc1071(b + b"\0" * (len(b) & 1))


def l4_checksum(v6: bool, proto: int, sa: bytes, da: bytes, seg: bytes) -> int:
    """the checksum of the L4 segment whose field is zero: pseudo header for
    TCP / UDP / ICMPv6, none for ICMP; UDP sends 0 as 0xFFFF (RFC 768)"""
    if proto == ICMP and not v6:
        return _sum16(seg)
    ph = sa + da + (struct.pack(">I", len(seg)) + bytes([0, 0, 0, proto]) if v6
                    else bytes([0, proto]) + struct.pack(">H", len(seg)))
    c = _sum16(ph + seg)
    return 0xFFFF if proto == UDP and c == 0 else c


def build_frame(v6: bool, proto: int, sa, da, sport: int = 0x1234, dport: int = 80, payload: bytes = b"",
                opts: bytes = b"", ext: bytes = b"", icmp_type: int = 8, ttl: int = 64, udp_zero: bool = False,
                smac: bytes = synth.LXC_MAC, dmac: bytes = L.NODE_MAC) -> bytes:
    """one Ethernet frame, whole: sa / da as wire bytes, ports in host order;
    opts: IPv4 options (a multiple of 4 bytes); ext: IPv6 extension headers as
    they go on the wire, the first byte of each the next header (the last one's
    is overwritten with proto)"""
    if proto == TCP:
        seg = struct.pack(">HHIIBBHHH", sport, dport, 0x01020304, 0, 0x50, 0x10, 0x2000, 0, 0) + payload
        coff = 16
    elif proto == UDP:
        seg = struct.pack(">HHHH", sport, dport, 8 + len(payload), 0) + payload
        coff = 6
    else:
        seg = bytes([icmp_type, 0, 0, 0, 0x00, 0x07, 0x00, 0x01]) + payload
        coff = 2
    if not (proto == UDP and udp_zero) and proto in (TCP, UDP, ICMP, ICMP6):
        c = l4_checksum(v6, proto, bytes(sa), bytes(da), seg)
        seg = seg[:coff] + struct.pack(">H", c) + seg[coff + 2:]
    if v6:
        first = proto
        if ext:
            ext = bytearray(ext)
            # chain: each header's next-header byte is given, the last one's is proto
            o = 0
            while True:
                ln = (ext[o + 1] + 1) * 8
                if o + ln >= len(ext):
                    ext[o] = proto
                    break
                o += ln
            first = 0
        ip = struct.pack(">IHBB", 0x60000000, len(ext) + len(seg), first, ttl) + bytes(sa) + bytes(da) + bytes(ext)
        eth = dmac + smac + b"\x86\xdd"
    else:
        ihl = 5 + len(opts) // 4
        ip = bytearray(struct.pack(">BBHHHBBH", 0x40 | ihl, 0, 20 + len(opts) + len(seg), 0x1234, 0x4000, ttl, proto, 0)
                       + bytes(sa) + bytes(da) + opts)
        ip[10:12] = struct.pack(">H", csum_rfc1071(bytes(ip)))
        ip = bytes(ip)
        eth = dmac + smac + b"\x08\x00"
    return eth + ip + seg


def frame_verifies(fr, length: int):
    """from scratch: the IPv4 header checksum, and the L4 checksum of TCP /
    UDP / ICMP / ICMPv6 over the whole packet (a UDP checksum of 0 is exempt).
    The packet must lie inside the slot."""
    fr = bytes(fr[:length])
    v6 = fr[12:14] == b"\x86\xdd"
    l4, proto = l4_of(fr, v6)
    if v6:
        sa, da = fr[22:38], fr[38:54]
        end = 54 + struct.unpack_from(">H", fr, 18)[0]
    else:
        hdr = bytearray(fr[14:l4])
        want = struct.unpack_from(">H", hdr, 10)[0]
        hdr[10:12] = b"\0\0"
        if csum_rfc1071(bytes(hdr)) != want:
            return False
        sa, da = fr[26:30], fr[30:34]
        end = 14 + struct.unpack_from(">H", fr, 16)[0]
    assert end <= len(fr), "the packet lies inside the slot"
    coff = {TCP: 16, UDP: 6, ICMP: 2, ICMP6: 2}.get(proto)
    if coff is None or (proto == ICMP and v6) or (proto == ICMP6 and not v6):
        return True
    seg = bytearray(fr[l4:end])
    want = struct.unpack_from(">H", seg, coff)[0]
    if proto == UDP and want == 0:
        return True
    seg[coff:coff + 2] = b"\0\0"
    return l4_checksum(v6, proto, sa, da, bytes(seg)) == want


# --------------------------------------------------------------------------
# the literal world and the literal frames
# --------------------------------------------------------------------------
LXC4 = "64.48.32.16"                       # synth.LXC_IPV4_RAW on the wire
LXC6 = str(ipaddress.ip_address(synth.LXC_IP6))


def literal_world(gate: int = 1) -> LbWorld:
    w = LbWorld(gate=gate)
    w.service4("10.96.0.10", 80, [("10.2.0.5", 8080)], rev_nat=1)          # L4 frontend, the port changes
    w.service4("10.96.0.20", 0, [("10.2.0.6", 0)], rev_nat=2)              # L3 frontend
    w.service4("10.96.0.30", 80, [(LXC4, 80)], rev_nat=3)                  # the backend is the sender: loopback
    w.service4("10.96.0.40", 80, [("10.2.0.7", 80)], rev_nat=4, rows=())   # its only backend row is gone
    w.service4("10.96.0.50", 0, [("10.2.0.8", 8080)], rev_nat=7)             # an L3 frontend whose backend has a port
    w.service6("fd00:96::10", 80, [("fd00:2::5", 8080)], rev_nat=5)
    w.service6("fd00:96::20", 0, [("fd00:2::6", 0)], rev_nat=6)
    w.ipcache = [("10.2.0.0/16", 1234), ("10.96.0.0/16", 5555), ("10.9.0.0/16", 99),
                 ("fd00:2::/32", 4321), ("fd00:96::/32", 6666)]
    w.policy = [(0, 1234, 8080, TCP, 1),   # exact: the translated port
                (0, 1234, 0, 0, 1),        # L3-only
                (0, 5555, 0, 0, 1),        # the service range itself: what a loopback frame is judged on
                (0, 4321, 0, 0, 1)]
    return w


SLOT_FILL = bytes(range(0xA0, 0xA0 + 96))


def slot(head: bytes, stride: int) -> bytes:
    """a frame's bytes in its slot, sentinel bytes behind them"""
    return (head + SLOT_FILL + bytes(stride))[:stride]


ETH4 = "de ad be ef c0 de aa bb cc dd ee ff 08 00"   # dmac NODE_MAC, smac LXC_MAC
ETH6 = "de ad be ef c0 de aa bb cc dd ee ff 86 dd"
RN = be16  # rev_nat_index comes back as stored

# (name, ct_proto_gate, stride, len, flags, bytes in, expected (verdict, identity, stage, lb_ret, rev_nat, slave),
#  bytes out or None = every byte as it was).  The sender is the endpoint, 64.48.32.16 / beef::1:165:82bc; the
#  policy world gives a translated frame verdict 0 with the backend's identity (1234 / 4321; TCP to 8080 hits
#  the exact key, stage 1, everything else the L3 key, stage 2).
LITERAL = [
    ("v4 tcp, port change", 1, 64, 64, E,
     (ETH4, "45 00 00 32 12 34 40 00 40 06 bd e8 40 30 20 10 0a 60 00 0a",
      "12 34 00 50 01 02 03 04 00 00 00 00 50 10 20 00 36 ba 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9"),
     (0, 1234, 1, XLATED, RN(1), 1),
     (ETH4, "45 00 00 32 12 34 40 00 40 06 be 4b 40 30 20 10 0a 02 00 05",
      "12 34 1f 90 01 02 03 04 00 00 00 00 50 10 20 00 17 dd 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9")),
    ("v4 udp, checksum 0: stays 0, the port is stored", 1, 64, 64, E,
     (ETH4, "45 00 00 32 12 34 40 00 40 11 bd dd 40 30 20 10 0a 60 00 0a",
      "12 34 00 50 00 1e 00 00 d0 d1 d2 d3 d4 d5 d6 d7 d8 d9 da db dc dd de df e0 e1 e2 e3 e4 e5"),
     (0, 1234, 2, XLATED, RN(1), 1),
     (ETH4, "45 00 00 32 12 34 40 00 40 11 be 40 40 30 20 10 0a 02 00 05",
      "12 34 1f 90 00 1e 00 00 d0 d1 d2 d3 d4 d5 d6 d7 d8 d9 da db dc dd de df e0 e1 e2 e3 e4 e5")),
    ("v4 udp to the L3 service, the patched checksum is 0: ff ff is stored", 1, 64, 64, E,
     (ETH4, "45 00 00 32 12 34 40 00 40 11 bd d3 40 30 20 10 0a 60 00 14",
      "12 34 00 35 00 1e ff 93 d0 d1 d2 d3 d4 d5 d6 d7 d8 d9 da db dc dd de df e0 e1 e2 e3 00 75"),
     (0, 1234, 2, XLATED, RN(2), 1),
     (ETH4, "45 00 00 32 12 34 40 00 40 11 be 3f 40 30 20 10 0a 02 00 06",
      "12 34 00 35 00 1e ff ff d0 d1 d2 d3 d4 d5 d6 d7 d8 d9 da db dc dd de df e0 e1 e2 e3 00 75")),
    ("v4 icmp echo to the L3 service: daddr and the header checksum alone", 1, 64, 64, E,
     (ETH4, "45 00 00 32 12 34 40 00 40 01 bd e3 40 30 20 10 0a 60 00 14",
      "08 00 f1 e6 00 07 00 01 b0 b1 b2 b3 b4 b5 b6 b7 b8 b9 ba bb bc bd be bf c0 c1 c2 c3 c4 c5"),
     (0, 1234, 2, XLATED, RN(2), 1),
     (ETH4, "45 00 00 32 12 34 40 00 40 01 be 4f 40 30 20 10 0a 02 00 06",
      "08 00 f1 e6 00 07 00 01 b0 b1 b2 b3 b4 b5 b6 b7 b8 b9 ba bb bc bd be bf c0 c1 c2 c3 c4 c5")),
    ("v4 tcp, loopback", 1, 64, 64, E,
     (ETH4, "45 00 00 32 12 34 40 00 40 06 bd d4 40 30 20 10 0a 60 00 1e",
      "12 34 00 50 01 02 03 04 00 00 00 00 50 10 20 00 36 a6 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9"),
     (0, 5555, 2, LOOPBACK, RN(3), 1),
     (ETH4, "45 00 00 32 12 34 40 00 40 06 be 3d 0a f5 ff 1f 40 30 20 10",
      "12 34 00 50 01 02 03 04 00 00 00 00 50 10 20 00 37 0f 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9")),
    ("v4 tcp, ihl 6", 1, 128, 68, E,
     (ETH4, "46 00 00 36 12 34 40 00 40 06 ba e3 40 30 20 10 0a 60 00 0a 01 01 01 00",
      "12 34 00 50 01 02 03 04 00 00 00 00 50 10 20 00 36 ba 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9"),
     (0, 1234, 1, XLATED, RN(1), 1),
     (ETH4, "46 00 00 36 12 34 40 00 40 06 bb 46 40 30 20 10 0a 02 00 05 01 01 01 00",
      "12 34 1f 90 01 02 03 04 00 00 00 00 50 10 20 00 17 dd 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9")),
    ("v6 tcp, port change: the checksum at byte 70", 1, 128, 80, E,
     (ETH6, "60 00 00 00 00 1a 06 40 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc "
      "fd 00 00 96 00 00 00 00 00 00 00 00 00 00 00 10",
      "12 34 00 50 01 02 03 04 00 00 00 00 50 10 20 00 f0 40 00 00 c0 c1 c2 c3 c4 c5"),
     (0, 4321, 2, XLATED, RN(5), 1),
     (ETH6, "60 00 00 00 00 1a 06 40 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc "
      "fd 00 00 02 00 00 00 00 00 00 00 00 00 00 00 05",
      "12 34 1f 90 01 02 03 04 00 00 00 00 50 10 20 00 d1 9f 00 00 c0 c1 c2 c3 c4 c5")),
    ("v6 udp, port change", 1, 64, 64, E,
     (ETH6, "60 00 00 00 00 0a 11 40 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc "
      "fd 00 00 96 00 00 00 00 00 00 00 00 00 00 00 10",
      "12 34 00 50 00 0a db cb d0 d1"),
     (0, 4321, 2, XLATED, RN(5), 1),
     (ETH6, "60 00 00 00 00 0a 11 40 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc "
      "fd 00 00 02 00 00 00 00 00 00 00 00 00 00 00 05",
      "12 34 1f 90 00 0a bd 2a d0 d1")),
    ("icmpv6 echo to the L3 service: the checksum at l4 + 2", 1, 64, 64, E,
     (ETH6, "60 00 00 00 00 0a 3a 40 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc "
      "fd 00 00 96 00 00 00 00 00 00 00 00 00 00 00 20",
      "80 00 8e 38 00 07 00 01 b0 b1"),
     (0, 4321, 2, XLATED, RN(6), 1),
     (ETH6, "60 00 00 00 00 0a 3a 40 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc "
      "fd 00 00 02 00 00 00 00 00 00 00 00 00 00 00 06",
      "80 00 8e e6 00 07 00 01 b0 b1")),
    ("v6 tcp behind a hop-by-hop header", 1, 128, 88, E,
     (ETH6, "60 00 00 00 00 22 00 40 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc "
      "fd 00 00 96 00 00 00 00 00 00 00 00 00 00 00 10 06 00 01 04 00 00 00 00",
      "12 34 00 50 01 02 03 04 00 00 00 00 50 10 20 00 f0 40 00 00 c0 c1 c2 c3 c4 c5"),
     (0, 4321, 2, XLATED, RN(5), 1),
     (ETH6, "60 00 00 00 00 22 00 40 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc "
      "fd 00 00 02 00 00 00 00 00 00 00 00 00 00 00 05 06 00 01 04 00 00 00 00",
      "12 34 1f 90 01 02 03 04 00 00 00 00 50 10 20 00 d1 9f 00 00 c0 c1 c2 c3 c4 c5")),
    ("v6 next header 1, no CONNTRACK: `if (csum_off)` patches the two bytes at l4 + 0", 0, 64, 64, E,
     (ETH6, "60 00 00 00 00 0a 01 40 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc "
      "fd 00 00 96 00 00 00 00 00 00 00 00 00 00 00 20",
      "08 00 06 72 00 07 00 01 b0 b1"),
     (0, 4321, 2, XLATED, RN(6), 1),
     (ETH6, "60 00 00 00 00 0a 01 40 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc "
      "fd 00 00 02 00 00 00 00 00 00 00 00 00 00 00 06",
      "08 ae 06 72 00 07 00 01 b0 b1")),
    ("v4 tcp, the backend row is gone: DROP_NO_SERVICE", 1, 64, 64, E,
     (ETH4, "45 00 00 32 12 34 40 00 40 06 bd ca 40 30 20 10 0a 60 00 28",
      "12 34 00 50 01 02 03 04 00 00 00 00 50 10 20 00 36 9c 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9"),
     (-158, 0, 6, -158, 0, 0),
     None),
    ("v4 tcp cut before its checksum field: DROP_CSUM_L4", 1, 64, 50, E,
     (ETH4, "45 00 00 32 12 34 40 00 40 06 bd e8 40 30 20 10 0a 60 00 0a",
      "12 34 00 50 01 02 03 04 00 00 00 00 50 10 20 00 36 ba 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9"),
     (-154, 0, 5, -154, 0, 0),
     None),
    ("v6 tcp, the checksum at byte 70 past a 64-byte slot: CGPU_DROP_SNAPLEN", 1, 64, 80, E,
     (ETH6, "60 00 00 00 00 1a 06 40 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc "
      "fd 00 00 96 00 00 00 00 00 00 00 00 00 00 00 10",
      "12 34 00 50 01 02 03 04 00 00"),
     (-4096, 0, 5, -4096, 0, 0),
     None),
    ("v4 tcp to no service", 1, 64, 64, E,
     (ETH4, "45 00 00 32 12 34 40 00 40 06 b5 40 40 30 20 10 0a 09 09 09",
      "12 34 00 50 01 02 03 04 00 00 00 00 50 10 20 00 2e 12 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9"),
     (-133, 99, 0, NONE, 0, 0),
     None),
    ("v4 ingress to a service address: no step", 1, 64, 64, 0,
     (ETH4, "45 00 00 32 12 34 40 00 40 06 14 22 0a 02 00 05 0a 60 00 0a",
      "12 34 00 50 01 02 03 04 00 00 00 00 50 10 20 00 8c f3 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9"),
     (-133, 1234, 0, NONE, 0, 0),
     None),
    # lb4_lookup_service sets key.dport = 0 before the L3 key, and l4_modify_port patches the checksum from
    # key.dport: an L3 frontend whose backend carries a port gives 17 8a where from = 80 would give 17 da
    ("v4 tcp, an L3 frontend with a backend port: the port patch starts from key.dport = 0", 1, 64, 64, E,
     (ETH4, "45 00 00 32 12 34 40 00 40 06 bd c0 40 30 20 10 0a 60 00 32",
      "12 34 00 50 01 02 03 04 00 00 00 00 50 10 20 00 36 92 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9"),
     (0, 1234, 1, XLATED, RN(7), 1),
     (ETH4, "45 00 00 32 12 34 40 00 40 06 be 48 40 30 20 10 0a 02 00 08",
      "12 34 1f 90 01 02 03 04 00 00 00 00 50 10 20 00 17 8a 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9")),
    ("egress arp: to the responder, untouched", 1, 64, 64, E,
     ("ff ff ff ff ff ff aa bb cc dd ee ff 08 06", "00 01 08 00 06 04 00 01", ""),
     (0, 0, 7, NONE, 0, 0),
     None),
]


# rows whose output the reference itself leaves with an L4 checksum that does not verify
NOT_VERIFYING = {"v4 tcp, an L3 frontend with a backend port: the port patch starts from key.dport = 0",
                 "v6 next header 1, no CONNTRACK: `if (csum_off)` patches the two bytes at l4 + 0"}


def literal_rows(stride: int, gate: int):
    return [r for r in LITERAL if r[2] == stride and r[1] == gate]


def literal_batch(rows):
    """rows of LITERAL (one stride) as a batch: (frames dict, expected data,
    expected column tuples)"""
    n, stride = len(rows), rows[0][2]
    data = np.zeros((n, stride), np.uint8)
    want = np.zeros((n, stride), np.uint8)
    for i, r in enumerate(rows):
        data[i] = np.frombuffer(slot(hx(*r[5]), stride), np.uint8)
        want[i] = np.frombuffer(slot(hx(*(r[7] if r[7] is not None else r[5])), stride), np.uint8)
    f = {"data": data, "len": np.array([r[3] for r in rows], np.uint32),
         "flags": np.array([r[4] for r in rows], np.uint8), "ep": np.zeros(n, np.uint16)}
    return f, want, [r[6] for r in rows]


# --------------------------------------------------------------------------
# the batch world and mixed batches
# --------------------------------------------------------------------------
def batch_world(gate: int = 1) -> LbWorld:
    """L4 and L3 frontends with several backends (the hash picks), a loopback
    backend, a frontend whose chosen backend row is missing beside an L3
    frontend of the same address that answers the fallback (rows with a
    count, as lb4_lookup_service asks of them), and frontends whose backends
    are all gone -- in both families"""
    w = LbWorld(gate=gate)
    w.service4("10.96.1.1", 80, [("10.2.1.1", 8080), ("10.2.1.2", 80), ("10.2.1.3", 9090)], rev_nat=11)
    w.service4("10.96.1.2", 0, [("10.2.2.1", 0), ("10.2.2.2", 0)], rev_nat=12)
    w.service4("10.96.1.3", 80, [(LXC4, 8080)], rev_nat=13)
    w.service4("10.96.1.4", 80, [("10.2.4.1", 80)], rev_nat=14, rows=())
    w.service4("10.96.1.5", 80, [("10.2.5.1", 80), ("10.2.5.2", 80)], rev_nat=15, rows=())
    w.service4("10.96.1.5", 0, [("10.2.5.3", 0), ("10.2.5.4", 0)], rev_nat=16, count=2)
    w.service6("fd00:96::1:1", 80, [("fd00:2::1:1", 8080), ("fd00:2::1:2", 80)], rev_nat=21)
    w.service6("fd00:96::1:2", 0, [("fd00:2::2:1", 0), ("fd00:2::2:2", 0), ("fd00:2::2:3", 0)], rev_nat=22)
    w.service6("fd00:96::1:4", 80, [("fd00:2::4:1", 80)], rev_nat=24, rows=())
    w.service6("fd00:96::1:5", 80, [("fd00:2::5:1", 80), ("fd00:2::5:2", 80)], rev_nat=25, rows=())
    w.service6("fd00:96::1:5", 0, [("fd00:2::5:3", 0), ("fd00:2::5:4", 0)], rev_nat=26, count=2)
    w.ipcache = [("10.2.0.0/16", 1234), ("10.2.2.0/24", 1235), ("10.96.0.0/16", 5555), ("10.9.0.0/16", 99),
                 ("fd00:2::/32", 4321), ("fd00:96::/32", 6666)]
    w.policy = [(ep, lab, dp, pr, 1) for ep in range(w.n_ep) for lab, dp, pr in
                ((1234, 8080, TCP), (1234, 8080, UDP), (1234, 0, 0), (1235, 0, 0), (5555, 0, 0), (4321, 0, 0),
                 (0, 9090, TCP))]
    w.policy += [(0, 1234, 80, TCP, 0), (1, 4321, 0, 0, 0)]
    return w


HBH = bytes([0, 0, 1, 4, 0, 0, 0, 0])        # a hop-by-hop header of 8 bytes (PadN)
NOP_OPTS = bytes([1, 1, 1, 0])               # IPv4 options: ihl 6

# one frame class per entry: (name, v6, proto, daddr, dport host order, keywords of build_frame, flags, cut)
# cut: the wire length ends before the TCP checksum field
CLASSES = [
    ("v4 tcp L4", False, TCP, "10.96.1.1", 80, {}, E, False),
    ("v4 udp zero L4", False, UDP, "10.96.1.1", 80, {"udp_zero": True}, E, False),
    ("v4 udp L3", False, UDP, "10.96.1.2", 53, {}, E, False),
    ("v4 icmp L3", False, ICMP, "10.96.1.2", 0, {}, E, False),
    ("v4 tcp loopback", False, TCP, "10.96.1.3", 80, {}, E, False),
    ("v4 tcp no backend", False, TCP, "10.96.1.4", 80, {}, E, False),
    ("v4 tcp fallback", False, TCP, "10.96.1.5", 80, {}, E, False),
    ("v4 tcp options", False, TCP, "10.96.1.1", 80, {"opts": NOP_OPTS}, E, False),
    ("v4 tcp no service", False, TCP, "10.2.1.1", 8080, {}, E, False),
    ("v4 ingress", False, TCP, "10.96.1.1", 80, {"sa": "10.2.1.1"}, 0, False),
    ("v6 udp L4", True, UDP, "fd00:96::1:1", 80, {}, E, False),
    ("v6 icmp6 L3", True, ICMP6, "fd00:96::1:2", 0, {"icmp_type": 128}, E, False),
    ("v6 tcp L4", True, TCP, "fd00:96::1:1", 80, {}, E, False),
    ("v6 udp ext", True, UDP, "fd00:96::1:1", 80, {"ext": HBH}, E, False),
    ("v6 udp no service", True, UDP, "fd00:2::1:1", 8080, {}, E, False),
    ("v6 ingress", True, UDP, "fd00:96::1:1", 80, {"sa": "fd00:2::1:1"}, 0, False),
    ("v4 udp L4", False, UDP, "10.96.1.1", 80, {}, E, False),
    ("v4 tcp cut", False, TCP, "10.96.1.1", 80, {}, E, True),
    ("v4 gre L3", False, 47, "10.96.1.2", 0, {}, E, False),
    ("v6 udp no backend", True, UDP, "fd00:96::1:4", 80, {}, E, False),
    ("v6 udp fallback", True, UDP, "fd00:96::1:5", 80, {}, E, False),
    ("arp", None, 0, "", 0, {}, E, False),
]
ARP = hx("ff ff ff ff ff ff aa bb cc dd ee ff 08 06 00 01 08 00 06 04 00 01")


def make_batch(n: int, stride: int, seed: int = 5, cut: bool = True, first: int = 0):
    """n frames, class i % len(CLASSES) (from `first`), random source ports and
    payloads, every checksum valid from scratch (a UDP-zero frame's is 0), the
    whole packet inside a 128-byte slot; a 64-byte slot cuts the IPv6 TCP and
    extension-header frames short of their checksum field, which is their
    class there.  cut=False leaves the truncated-TCP class out (its slot gets
    the plain TCP class).  Returns (frames dict, hash column, class index)."""
    rng = np.random.default_rng(seed * 7919 + n + stride)
    data = np.zeros((n, stride), np.uint8)
    ln = np.zeros(n, np.uint32)
    fl = np.zeros(n, np.uint8)
    cls = np.zeros(n, np.int32)
    for i in range(n):
        k = (first + i) % len(CLASSES)
        name, v6, proto, da, dport, kw, flags, is_cut = CLASSES[k]
        if is_cut and not cut:
            k = 0
            name, v6, proto, da, dport, kw, flags, is_cut = CLASSES[0]
        cls[i] = k
        fl[i] = flags
        if v6 is None:
            fr = ARP
        else:
            kw = dict(kw)
            sa = kw.pop("sa", None)
            sa = ipaddress.ip_address(sa).packed if sa else (synth.LXC_IP6 if v6 else bytes([64, 48, 32, 16]))
            hdr = 14 + (40 if v6 else 20) + len(kw.get("opts", b"")) + len(kw.get("ext", b"")) + \
                {TCP: 20, UDP: 8}.get(proto, 8)
            room = max(0, min(stride, 128) - hdr) if hdr <= stride else 128 - hdr
            pl = bytes(rng.integers(0, 256, int(rng.integers(0, room // 2 + 1)) * 2, dtype=np.uint8))
            if proto == 47:
                kw["icmp_type"] = 0
            fr = build_frame(v6, proto, sa, ipaddress.ip_address(da).packed, int(rng.integers(1024, 65536)), dport,
                             pl, **kw)
        ln[i] = 14 + 20 + 16 if is_cut else len(fr)
        data[i] = np.frombuffer(slot(fr, stride), np.uint8)
    f = {"data": data, "len": ln, "flags": fl, "ep": (np.arange(n) % 4).astype(np.uint16)}
    return f, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), cls


def class_of(name: str) -> int:
    return [c[0] for c in CLASSES].index(name)
