"""Reference for reverse NAT on raw frames (cgpu_rnat_frames_v4 / _v6).

`restate_rnat_frame` restates, per frame, what __lb4_rev_nat / __lb6_rev_nat
write into the packet once lb4_rev_nat / lb6_rev_nat have found the map entry:

* bpf/lib/lb.h:218-252 (reverse_map_l4_port) with lib/l4.h:50-60
  (l4_modify_port: the checksum patch, then the port at l4 + 0);
* lib/lb.h:485-550 (__lb4_rev_nat: the loopback daddr, the saddr, the header
  checksum, the L4 checksum where csum_off->offset is not 0) and :254-294
  (__lb6_rev_nat: the saddr and the L4 checksum, always);
* lib/csum.h (csum_l4_offset_and_flags, csum_l4_replace); the kernel's
  csum_diff, bpf_l3_csum_replace and bpf_l4_csum_replace are the literal ones
  of tests/lb_frames_cases.py, on the words as loaded, BPF_F_MARK_MANGLED_0
  included.

The decision (which packets, which address and port) is the conntrack paths':
the call takes it as the rn columns, and `make_batch` takes those columns from
revnat_cases.restate_v4 / restate_v6 over the frames' own fields, so the
frames and the columns are consistent by construction.

LITERAL is a hand-written table of bytes in and bytes out.  Both sides carry
checksums worked from scratch (RFC 1071 over the packet before and after the
rewrite, pseudo header included), not through the incremental arithmetic; the
UDP rows with a checksum field of 0 by the rule itself.  Most rows are the
reply to a row of lb_frames_cases.LITERAL: the bytes that table has coming in
are the bytes this one has going out.
"""
import ipaddress
import struct

import numpy as np

from cilium_amd import layouts as L, synth
from forward_frames_cases import hx
from lb_frames_cases import (DROP_CSUM_L4, DROP_SNAPLEN, HBH, ICMP, ICMP6, NOP_OPTS, TCP, UDP, _h, _mangled0, a4, a6,
                             be16, build_frame, csum_diff, csum_replace2, csum_replace_diff, frame_verifies, slot)
import revnat_cases as rc


# --------------------------------------------------------------------------
# one frame through the call
# --------------------------------------------------------------------------
def walk6(fr, length: int, cap: int):
    """ipv6_hdrlen as the parse walks it (lib/ipv6.h:61-98): (l4 offset,
    protocol), or None where the parse ends the frame"""
    nh, off, r = fr[20], 40, 1
    for _ in range(4):
        if r != 1:
            break
        if nh in (59, 44):
            r = -1
        elif nh in (0, 43, 51, 60):
            o = 14 + off
            if o + 2 > min(length, cap):
                r = -1
            else:
                hl = fr[o + 1]
                nh = fr[o]
                off += (hl + 2) << 2 if nh == 51 else (hl + 1) << 3
        else:
            r = 0
    return (14 + off, nh) if r == 0 else None


def restate_rnat_frame(frame, length: int, stride: int, applied: int, sa, da, sp: int, v6: bool, loopback=None):
    """(ret, the slot afterwards).  frame: the slot's `stride` bytes; sa: the
    rn_saddr element (the raw u32, or 16 bytes), da: rn_daddr (IPv4), sp:
    rn_sport (raw u16).  loopback None: inferred as the call infers it (da
    differs from the frame's daddr); True / False: ct_state->loopback given, and
    the csum_diff seeded from the daddr words whenever it is set, as
    lb.h:513-535 does."""
    fr = bytearray(frame)
    assert len(fr) == stride
    same = bytes(fr)
    if not applied:
        return 0, same
    cap = min(length, stride)
    if bytes(fr[12:14]) != (b"\x86\xdd" if v6 else b"\x08\x00") or cap < (54 if v6 else 34):
        return 0, same
    if v6:
        w = walk6(fr, length, cap)
        if w is None:
            return 0, same
        l4, proto = w
    else:
        l4, proto = 14 + 4 * (fr[14] & 15), fr[23]
    tu = proto in (TCP, UDP)
    if proto not in (TCP, UDP, ICMP6 if v6 else ICMP):   # ct_lookup's gate
        return 0, same
    if tu and l4 + 2 > cap:                               # ct_lookup's port load
        return 0, same
    coff = {TCP: 16, UDP: 6, ICMP6: 2}.get(proto, 0)      # csum_l4_offset_and_flags
    l4c = v6 or coff != 0
    p = l4 + coff
    if l4c and p + 2 > length:
        return DROP_CSUM_L4, same
    if l4c and p + 2 > cap:
        return DROP_SNAPLEN, same
    udp = proto == UDP
    writes = []
    c = _h(fr, p) if l4c else 0
    if tu and sp != _h(fr, l4):                           # reverse_map_l4_port: port && port != old_port
        c = _mangled0(c, csum_replace2(c, _h(fr, l4), sp), udp)
        writes += [(p, struct.pack("<H", c)), (l4, struct.pack("<H", sp))]
    if v6:
        new = bytes(sa)
        writes.append((22, new))
        d = csum_diff(bytes(fr[22:38]), new)
    else:
        old_sip, old_dip = bytes(fr[26:30]), bytes(fr[30:34])
        d = 0
        if (struct.pack("<I", da) != old_dip) if loopback is None else loopback:
            new_dip = struct.pack("<I", da)
            writes.append((30, new_dip))
            d = csum_diff(old_dip, new_dip, 0)
        new_sip = struct.pack("<I", sa)
        writes.append((26, new_sip))
        d = csum_diff(old_sip, new_sip, d)
        writes.append((24, struct.pack("<H", csum_replace_diff(_h(fr, 24), d))))
    if l4c:
        writes.append((p, struct.pack("<H", _mangled0(c, csum_replace_diff(c, d), udp))))
    for off, b in writes:   # every value from the frame as it came, stored in the reference's order
        fr[off:off + len(b)] = b
    return 0, bytes(fr)


def restate_rnat_frames(f: dict, rn: dict, v6: bool):
    """a batch through restate_rnat_frame: (ret, data afterwards)"""
    n, stride = f["data"].shape
    ret = np.zeros(n, np.int32)
    data = f["data"].copy()
    for i in range(n):
        sa = rn["rn_saddr"][i].tobytes() if v6 else int(rn["rn_saddr"][i])
        da = None if v6 else int(rn["rn_daddr"][i])
        ret[i], b = restate_rnat_frame(data[i].tobytes(), int(f["len"][i]), stride, int(rn["rn_applied"][i]), sa, da,
                                       int(rn["rn_sport"][i]), v6)
        data[i] = np.frombuffer(b, np.uint8)
    return ret, data


# --------------------------------------------------------------------------
# the literal frames
# --------------------------------------------------------------------------
# (name, the call's family is IPv6, stride, len, applied, rn_saddr, rn_daddr, rn_sport, bytes in, ret,
#  bytes out or None = every byte as it was).  The endpoint is 64.48.32.16 / beef::1:165:82bc; the backends
#  10.2.0.5:8080, 10.2.0.6, fd00:2::5 port 8080 and fd00:2::6 answer for the services 10.96.0.10:80, 10.96.0.20,
#  fd00:96::10 port 80 and fd00:96::20; the loopback row is the endpoint's own answer to IPV4_LOOPBACK
#  (10.245.255.31) for 10.96.0.30:80.
LITERAL = [
    ("v4 tcp, the port changes", False, 64, 64, 1, a4("10.96.0.10"), a4("64.48.32.16"), be16(80),
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "45 00 00 32 12 34 40 00 40 06 be 4b 0a 02 00 05 40 30 20 10",
      "1f 90 12 34 01 02 03 04 00 00 00 00 50 10 20 00 17 dd 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9"),
     0,
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "45 00 00 32 12 34 40 00 40 06 bd e8 0a 60 00 0a 40 30 20 10",
      "00 50 12 34 01 02 03 04 00 00 00 00 50 10 20 00 36 ba 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9")),
    ("v4 udp, checksum 0: stays 0, the port is stored", False, 64, 64, 1, a4("10.96.0.10"), a4("64.48.32.16"), be16(80),
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "45 00 00 32 12 34 40 00 40 11 be 40 0a 02 00 05 40 30 20 10",
      "1f 90 12 34 00 1e 00 00 d0 d1 d2 d3 d4 d5 d6 d7 d8 d9 da db dc dd de df e0 e1 e2 e3 e4 e5"),
     0,
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "45 00 00 32 12 34 40 00 40 11 bd dd 0a 60 00 0a 40 30 20 10",
      "00 50 12 34 00 1e 00 00 d0 d1 d2 d3 d4 d5 d6 d7 d8 d9 da db dc dd de df e0 e1 e2 e3 e4 e5")),
    ("v4 udp, the patched checksum is 0: ff ff is stored", False, 64, 64, 1, a4("10.96.0.20"), a4("64.48.32.16"), be16(53),
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "45 00 00 32 12 34 40 00 40 11 be 3f 0a 02 00 06 40 30 20 10",
      "00 35 12 34 00 1e 00 6c d0 d1 d2 d3 d4 d5 d6 d7 d8 d9 da db dc dd de df e0 e1 e2 e3 00 09"),
     0,
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "45 00 00 32 12 34 40 00 40 11 bd d3 0a 60 00 14 40 30 20 10",
      "00 35 12 34 00 1e ff ff d0 d1 d2 d3 d4 d5 d6 d7 d8 d9 da db dc dd de df e0 e1 e2 e3 00 09")),
    ("v4 icmp echo reply: saddr and the header checksum alone", False, 64, 64, 1, a4("10.96.0.20"), a4("64.48.32.16"), be16(0),
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "45 00 00 32 12 34 40 00 40 01 be 4f 0a 02 00 06 40 30 20 10",
      "00 00 f9 e6 00 07 00 01 b0 b1 b2 b3 b4 b5 b6 b7 b8 b9 ba bb bc bd be bf c0 c1 c2 c3 c4 c5"),
     0,
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "45 00 00 32 12 34 40 00 40 01 bd e3 0a 60 00 14 40 30 20 10",
      "00 00 f9 e6 00 07 00 01 b0 b1 b2 b3 b4 b5 b6 b7 b8 b9 ba bb bc bd be bf c0 c1 c2 c3 c4 c5")),
    ("v4 tcp, ihl 6", False, 128, 68, 1, a4("10.96.0.10"), a4("64.48.32.16"), be16(80),
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "46 00 00 36 12 34 40 00 40 06 bb 46 0a 02 00 05 40 30 20 10 01 01 01 00",
      "1f 90 12 34 01 02 03 04 00 00 00 00 50 10 20 00 17 dd 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9"),
     0,
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "46 00 00 36 12 34 40 00 40 06 ba e3 0a 60 00 0a 40 30 20 10 01 01 01 00",
      "00 50 12 34 01 02 03 04 00 00 00 00 50 10 20 00 36 ba 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9")),
    ("v4 tcp, loopback: daddr := the old saddr", False, 64, 64, 1, a4("10.96.0.30"), a4("64.48.32.16"), be16(80),
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "45 00 00 32 12 34 40 00 40 06 be 3d 40 30 20 10 0a f5 ff 1f",
      "00 50 12 34 01 02 03 04 00 00 00 00 50 10 20 00 37 0f 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9"),
     0,
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "45 00 00 32 12 34 40 00 40 06 bd d4 0a 60 00 1e 40 30 20 10",
      "00 50 12 34 01 02 03 04 00 00 00 00 50 10 20 00 36 a6 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9")),
    ("v4 tcp, nat->port 0: the port stays", False, 64, 64, 1, a4("10.96.0.20"), a4("64.48.32.16"), be16(443),
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "45 00 00 32 12 34 40 00 40 06 be 4a 0a 02 00 06 40 30 20 10",
      "01 bb 12 34 01 02 03 04 00 00 00 00 50 10 20 00 35 b1 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9"),
     0,
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "45 00 00 32 12 34 40 00 40 06 bd de 0a 60 00 14 40 30 20 10",
      "01 bb 12 34 01 02 03 04 00 00 00 00 50 10 20 00 35 45 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9")),
    ("v6 tcp, the port changes: the checksum at byte 70", True, 80, 80, 1, a6("fd00:96::10"), None, be16(80),
     ("de ad be ef c0 de aa bb cc dd ee ff 86 dd",
      "60 00 00 00 00 1a 06 40 fd 00 00 02 00 00 00 00 00 00 00 00 00 00 00 05 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc",
      "1f 90 12 34 01 02 03 04 00 00 00 00 50 10 20 00 d1 9f 00 00 c0 c1 c2 c3 c4 c5"),
     0,
     ("de ad be ef c0 de aa bb cc dd ee ff 86 dd",
      "60 00 00 00 00 1a 06 40 fd 00 00 96 00 00 00 00 00 00 00 00 00 00 00 10 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc",
      "00 50 12 34 01 02 03 04 00 00 00 00 50 10 20 00 f0 40 00 00 c0 c1 c2 c3 c4 c5")),
    ("v6 udp, the port changes", True, 80, 72, 1, a6("fd00:96::10"), None, be16(80),
     ("de ad be ef c0 de aa bb cc dd ee ff 86 dd",
      "60 00 00 00 00 12 11 40 fd 00 00 02 00 00 00 00 00 00 00 00 00 00 00 05 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc",
      "1f 90 12 34 00 12 65 bf d0 d1 d2 d3 d4 d5 d6 d7 d8 d9"),
     0,
     ("de ad be ef c0 de aa bb cc dd ee ff 86 dd",
      "60 00 00 00 00 12 11 40 fd 00 00 96 00 00 00 00 00 00 00 00 00 00 00 10 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc",
      "00 50 12 34 00 12 84 60 d0 d1 d2 d3 d4 d5 d6 d7 d8 d9")),
    ("icmpv6 echo reply: the checksum at l4 + 2", True, 80, 72, 1, a6("fd00:96::20"), None, be16(0),
     ("de ad be ef c0 de aa bb cc dd ee ff 86 dd",
      "60 00 00 00 00 12 3a 40 fd 00 00 02 00 00 00 00 00 00 00 00 00 00 00 06 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc",
      "81 00 b7 03 00 07 00 01 b0 b1 b2 b3 b4 b5 b6 b7 b8 b9"),
     0,
     ("de ad be ef c0 de aa bb cc dd ee ff 86 dd",
      "60 00 00 00 00 12 3a 40 fd 00 00 96 00 00 00 00 00 00 00 00 00 00 00 20 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc",
      "81 00 b6 55 00 07 00 01 b0 b1 b2 b3 b4 b5 b6 b7 b8 b9")),
    ("v6 tcp behind a hop-by-hop header", True, 128, 88, 1, a6("fd00:96::10"), None, be16(80),
     ("de ad be ef c0 de aa bb cc dd ee ff 86 dd",
      "60 00 00 00 00 22 00 40 fd 00 00 02 00 00 00 00 00 00 00 00 00 00 00 05 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc 06 00 01 04 00 00 00 00",
      "1f 90 12 34 01 02 03 04 00 00 00 00 50 10 20 00 d1 9f 00 00 c0 c1 c2 c3 c4 c5"),
     0,
     ("de ad be ef c0 de aa bb cc dd ee ff 86 dd",
      "60 00 00 00 00 22 00 40 fd 00 00 96 00 00 00 00 00 00 00 00 00 00 00 10 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc 06 00 01 04 00 00 00 00",
      "00 50 12 34 01 02 03 04 00 00 00 00 50 10 20 00 f0 40 00 00 c0 c1 c2 c3 c4 c5")),
    ("v4 tcp cut before its checksum field: DROP_CSUM_L4", False, 64, 50, 1, a4("10.96.0.10"), a4("64.48.32.16"), be16(80),
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "45 00 00 32 12 34 40 00 40 06 be 4b 0a 02 00 05 40 30 20 10",
      "1f 90 12 34 01 02 03 04 00 00 00 00 50 10 20 00 17 dd 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9"),
     DROP_CSUM_L4, None),
    ("v6 tcp, the checksum at byte 70 past a 64-byte slot: CGPU_DROP_SNAPLEN", True, 64, 80, 1, a6("fd00:96::10"), None, be16(80),
     ("de ad be ef c0 de aa bb cc dd ee ff 86 dd",
      "60 00 00 00 00 1a 06 40 fd 00 00 02 00 00 00 00 00 00 00 00 00 00 00 05 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc",
      "1f 90 12 34 01 02 03 04 00 00 00 00 50 10 20 00 d1 9f 00 00 c0 c1 c2 c3 c4 c5"),
     DROP_SNAPLEN, None),
    ("v4 tcp, applied 0", False, 64, 64, 0, a4("10.96.0.10"), a4("64.48.32.16"), be16(80),
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "45 00 00 32 12 34 40 00 40 06 be 4b 0a 02 00 05 40 30 20 10",
      "1f 90 12 34 01 02 03 04 00 00 00 00 50 10 20 00 17 dd 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9"),
     0, None),
    # a frame of the other family, and one that is not IP, with applied 1: left alone
    ("an IPv6 frame in the IPv4 call", False, 80, 72, 1, a4("10.96.0.10"), a4("64.48.32.16"), be16(80),
     ("de ad be ef c0 de aa bb cc dd ee ff 86 dd",
      "60 00 00 00 00 12 11 40 fd 00 00 02 00 00 00 00 00 00 00 00 00 00 00 05 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc",
      "1f 90 12 34 00 12 65 bf d0 d1 d2 d3 d4 d5 d6 d7 d8 d9"),
     0, None),
    ("an IPv4 frame in the IPv6 call", True, 64, 64, 1, a6("fd00:96::10"), None, be16(80),
     ("de ad be ef c0 de aa bb cc dd ee ff 08 00",
      "45 00 00 32 12 34 40 00 40 06 be 4b 0a 02 00 05 40 30 20 10",
      "1f 90 12 34 01 02 03 04 00 00 00 00 50 10 20 00 17 dd 00 00 c0 c1 c2 c3 c4 c5 c6 c7 c8 c9"),
     0, None),
    ("arp in the IPv4 call", False, 64, 64, 1, a4("10.96.0.10"), a4("64.48.32.16"), be16(80),
     ("ff ff ff ff ff ff aa bb cc dd ee ff 08 06", "00 01 08 00 06 04 00 01", ""),
     0, None),
    ("v6 tcp, applied 0", True, 80, 80, 0, a6("fd00:96::10"), None, be16(80),
     ("de ad be ef c0 de aa bb cc dd ee ff 86 dd",
      "60 00 00 00 00 1a 06 40 fd 00 00 02 00 00 00 00 00 00 00 00 00 00 00 05 be ef 00 00 00 00 00 00 00 00 00 01 01 65 82 bc",
      "1f 90 12 34 01 02 03 04 00 00 00 00 50 10 20 00 d1 9f 00 00 c0 c1 c2 c3 c4 c5"),
     0, None),
]


def literal_groups():
    """[(v6, stride)] of the table, each a batch of its own"""
    return sorted({(r[1], r[2]) for r in LITERAL})


def literal_batch(v6: bool, stride: int):
    """the rows of one family and stride as a batch: (frames dict, rn columns,
    expected data, expected ret)"""
    rows = [r for r in LITERAL if r[1] == v6 and r[2] == stride]
    n = len(rows)
    data = np.zeros((n, stride), np.uint8)
    want = np.zeros((n, stride), np.uint8)
    for i, r in enumerate(rows):
        data[i] = np.frombuffer(slot(hx(*r[8]), stride), np.uint8)
        want[i] = np.frombuffer(slot(hx(*(r[10] if r[10] is not None else r[8])), stride), np.uint8)
    f = {"data": data, "len": np.array([r[3] for r in rows], np.uint32), "flags": np.zeros(n, np.uint8),
         "ep": np.zeros(n, np.uint16)}
    rn = {"rn_applied": np.array([r[4] for r in rows], np.uint8),
          "rn_sport": np.array([r[7] for r in rows], np.uint16)}
    if v6:
        rn["rn_saddr"] = np.stack([np.frombuffer(r[5], np.uint8) for r in rows])
    else:
        rn["rn_saddr"] = np.array([r[5] for r in rows], np.uint32)
        rn["rn_daddr"] = np.array([r[6] for r in rows], np.uint32)
    return f, rn, want, np.array([r[9] for r in rows], np.int32)


# --------------------------------------------------------------------------
# mixed batches
# --------------------------------------------------------------------------
EP4 = bytes([64, 48, 32, 16])
LOOP4 = struct.pack("<I", rc.LOOPBACK)
ARP = hx("ff ff ff ff ff ff aa bb cc dd ee ff 08 06 00 01 08 00 06 04 00 01")
FORCED = "forced"   # applied 1 with columns of no connection: the call must leave the frame alone

# (name, protocol, index kind or FORCED, lb_loopback, egress, keywords of build_frame, special)
# special: "cut" the wire length ends before the TCP checksum field, "same" the frame already carries the
# service's port, "eq" saddr == daddr, "other" a frame of the other family, "arp", "short" the length ends
# inside the fixed header, "frag" a fragment header in front
CLASSES4 = [
    ("tcp port", TCP, rc.K_PORT, 0, 0, {}, None),
    ("udp port", UDP, rc.K_PORT, 0, 0, {}, None),
    ("udp zero", UDP, rc.K_PORT, 0, 0, {"udp_zero": True}, None),
    ("icmp", ICMP, rc.K_PORT, 0, 0, {"icmp_type": 0}, None),
    ("tcp port 0", TCP, rc.K_PORT0, 0, 0, {}, None),
    ("tcp loopback", TCP, rc.K_PORT, 1, 1, {}, None),
    ("udp loopback, saddr == daddr", UDP, rc.K_PORT, 1, 1, {}, "eq"),
    ("tcp options", TCP, rc.K_PORT, 0, 0, {"opts": NOP_OPTS}, None),
    ("tcp cut", TCP, rc.K_PORT, 0, 0, {}, "cut"),
    ("miss", TCP, rc.K_MISS, 0, 0, {}, None),
    ("index 0", UDP, rc.K_ZERO, 0, 0, {}, None),
    ("other family", UDP, FORCED, 0, 0, {}, "other"),
    ("arp", 0, FORCED, 0, 0, {}, "arp"),
    ("gre", 47, FORCED, 0, 0, {"icmp_type": 0}, None),
    ("short", TCP, FORCED, 0, 0, {}, "short"),
    ("tcp same port", TCP, rc.K_PORT, 0, 0, {}, "same"),
]
CLASSES6 = [
    ("tcp port", TCP, rc.K_PORT, 0, 0, {}, None),
    ("udp port", UDP, rc.K_PORT, 0, 0, {}, None),
    ("udp zero", UDP, rc.K_PORT, 0, 1, {"udp_zero": True}, None),
    ("icmp6", ICMP6, rc.K_PORT, 0, 0, {"icmp_type": 129}, None),
    ("tcp port 0", TCP, rc.K_PORT0, 0, 1, {}, None),
    ("udp ext", UDP, rc.K_PORT, 0, 0, {"ext": HBH}, None),
    ("tcp ext", TCP, rc.K_PORT, 0, 0, {"ext": HBH}, None),
    ("tcp cut", TCP, rc.K_PORT, 0, 0, {}, "cut"),
    ("miss", TCP, rc.K_MISS, 0, 0, {}, None),
    ("index 0", UDP, rc.K_ZERO, 0, 0, {}, None),
    ("other family", TCP, FORCED, 0, 0, {}, "other"),
    ("arp", 0, FORCED, 0, 0, {}, "arp"),
    ("frag", UDP, FORCED, 0, 0, {}, "frag"),
    ("short", UDP, FORCED, 0, 0, {}, "short"),
    ("icmp in ipv6", ICMP, FORCED, 0, 0, {}, None),
    ("udp same port", UDP, rc.K_PORT, 0, 0, {}, "same"),
]
# the classes whose frames are rewritten wherever their checksum field lies in the slot
REWRITTEN4 = ("tcp port", "udp port", "udp zero", "icmp", "tcp port 0", "tcp loopback", "udp loopback, saddr == daddr",
              "tcp options", "tcp same port")
REWRITTEN6 = ("tcp port", "udp port", "udp zero", "icmp6", "tcp port 0", "udp ext", "tcp ext", "udp same port")


def classes(v6: bool):
    return CLASSES6 if v6 else CLASSES4


def class_of(v6: bool, name: str) -> int:
    return [c[0] for c in classes(v6)].index(name)


def make_batch(n: int, stride: int, v6: bool, seed: int = 5):
    """n frames of one call: class i % len(classes), random ports and payloads,
    every checksum valid from scratch, the whole packet inside the slot where
    its headers fit (an IPv6 TCP or extension-header frame in a 64-byte slot
    keeps its length and is cut by the slot: that is its class there).  The rn
    columns are revnat_cases.restate_v4 / restate_v6 over the frames' own
    fields and the entry each class names; the FORCED classes get applied 1
    and columns of no connection.  Returns (frames dict, rn columns, class
    index)."""
    rng = np.random.default_rng(seed * 104729 + n * 131 + stride + (7 if v6 else 0))
    cl = classes(v6)
    rmap = rc._rmap6() if v6 else rc._rmap4()
    data = np.zeros((n, stride), np.uint8)
    ln = np.zeros(n, np.uint32)
    cls = np.arange(n, dtype=np.int32) % len(cl)
    idx = np.zeros(n, np.int64)
    loop = np.zeros(n, np.int64)
    egress = np.zeros(n, np.uint8)
    forced = np.zeros(n, bool)
    for i in range(n):
        name, proto, kind, lo, eg, kw, special = cl[cls[i]]
        forced[i] = kind == FORCED
        idx[i] = 0 if forced[i] else rc._idx_of(kind, i // len(cl))
        loop[i], egress[i] = lo, eg
        if special == "arp":
            fr = ARP
        else:
            fv6 = v6 != (special == "other")
            kw = dict(kw)
            rem = (bytes.fromhex("20010db8000100000000000000000000")[:12] + (i + 1).to_bytes(4, "big")) if fv6 \
                else bytes([11, (i >> 16) & 255, (i >> 8) & 255, i & 255])
            ep = synth.LXC_IP6 if fv6 else EP4
            sa, da = (ep, rem) if eg else (rem, ep)
            if lo:
                sa, da = EP4, (EP4 if special == "eq" else LOOP4)
            sport = int(rng.integers(1024, 65536))
            if special == "same":
                sport = int(be16(rmap[int(idx[i])][1]))   # the wire already carries nat->port
            hdr = 14 + (40 if fv6 else 20) + len(kw.get("opts", b"")) + len(kw.get("ext", b"")) + \
                {TCP: 20, UDP: 8}.get(proto, 8)
            room = max(0, stride - hdr)
            pl = bytes(rng.integers(0, 256, int(rng.integers(0, min(room, 40) // 2 + 1)) * 2, dtype=np.uint8))
            fr = bytearray(build_frame(fv6, proto, sa, da, sport, int(rng.integers(1, 65536)), pl, **kw))
            if special == "frag":
                fr[20] = 44
            fr = bytes(fr)
        ln[i] = {"cut": 14 + (40 if v6 else 20) + 16, "short": 50 if v6 else 30}.get(special, len(fr))
        data[i] = np.frombuffer(slot(fr, stride), np.uint8)
    f = {"data": data, "len": ln, "flags": egress.copy(), "ep": np.zeros(n, np.uint16)}
    # the tuple a frames-to-conntrack parse would hand the _rnat call (junk for frames it would not pass)
    t = {"flags": egress, "proto": np.zeros(n, np.uint8), "sport": np.zeros(n, np.uint16)}
    for i in range(n):
        row = data[i].tobytes()
        w = walk6(row, int(ln[i]), stride) if v6 else (14 + 4 * (row[14] & 15), row[23])
        if w is not None and w[0] + 2 <= stride:
            t["proto"][i] = w[1]
            t["sport"][i] = _h(row, w[0])
    ct_ret = np.full(n, L.CT_REPLY, np.uint8)
    if v6:
        t["saddr"] = data[:, 22:38].copy()
        sa, sp, applied = rc.restate_v6(t, ct_ret, idx, rmap)
        rn = {"rn_saddr": sa, "rn_sport": sp, "rn_applied": applied}
        sa[forced] = np.frombuffer(a6("fd00:96::99"), np.uint8)
    else:
        t["saddr"] = data[:, 26:30].copy().view("<u4")[:, 0]
        t["daddr"] = data[:, 30:34].copy().view("<u4")[:, 0]
        sa, da, sp, applied = rc.restate_v4(t, ct_ret, idx, loop, rmap)
        rn = {"rn_saddr": sa, "rn_daddr": da, "rn_sport": sp, "rn_applied": applied}
        sa[forced] = a4("10.96.0.99")
    sp[forced] = int(be16(80))
    applied[forced] = 1
    return f, rn, cls
