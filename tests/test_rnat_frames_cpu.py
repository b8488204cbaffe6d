"""Reverse NAT on raw frames (cgpu_rnat_frames_v4 / _v6) without a GPU: the
restatement against the literal frames, rewritten frames against a
from-scratch checksum, the inferred against the explicit loopback form, and
the calls' argument rules on a host-only context."""
import ctypes as C
import errno
import struct

import numpy as np
import pytest

from cilium_amd import layouts as L
from cilium_amd import _abi
from cilium_amd._abi import Rnf4In, Rnf6In   # noqa: F401  (the mirror of the calls' structs: this file is about them)
from cilium_amd.engine import Engine
from lb_frames_cases import ICMP, TCP, UDP, build_frame, frame_verifies, hx, slot
from rnat_frames_cases import (LITERAL, REWRITTEN4, REWRITTEN6, class_of, classes, literal_batch, literal_groups,
                               make_batch, restate_rnat_frame, restate_rnat_frames)


# ---- the restatement ----------------------------------------------------------
@pytest.mark.parametrize("v6,stride", literal_groups())
def test_restatement_reproduces_the_literal_frames(v6, stride):
    f, rn, want, ret = literal_batch(v6, stride)
    got_ret, data = restate_rnat_frames(f, rn, v6)
    assert got_ret.tolist() == ret.tolist()
    for i in range(len(ret)):
        assert data[i].tobytes() == want[i].tobytes(), i


def test_literal_frames_cover_the_cases():
    names = " | ".join(r[0] for r in LITERAL)
    assert len({r[0] for r in LITERAL}) == len(LITERAL)
    for word in ("v4 tcp, the port changes", "checksum 0", "ff ff is stored", "v4 icmp", "ihl 6", "loopback",
                 "the port stays", "v6 tcp, the port changes", "v6 udp", "icmpv6", "hop-by-hop", "DROP_CSUM_L4",
                 "CGPU_DROP_SNAPLEN", "IPv6 frame in the IPv4 call", "IPv4 frame in the IPv6 call", "applied 0"):
        assert word in names, word
    assert {L.DROP_CSUM_L4, L.DROP_SNAPLEN, 0} == {r[9] for r in LITERAL}
    for r in LITERAL:   # a drop and a frame left alone keep every byte
        assert (r[10] is None) == (r[9] != 0 or r[4] == 0 or "call" in r[0]), r[0]


@pytest.mark.parametrize("row", [r for r in LITERAL if r[10] is not None], ids=lambda r: r[0])
def test_literal_frames_verify_from_scratch(row):
    """both sides of a rewritten row: header and L4 checksum over the whole
    packet, pseudo header included (a UDP checksum of 0 is exempt)"""
    assert frame_verifies(slot(hx(*row[8]), row[2]), row[3])
    assert frame_verifies(slot(hx(*row[10]), row[2]), row[3])
    assert hx(*row[8]) != hx(*row[10])


@pytest.mark.parametrize("v6,stride", [(False, 64), (False, 128), (True, 64), (True, 80), (True, 128)])
def test_rewritten_batch_frames_verify_from_scratch(v6, stride):
    """every frame of make_batch that verified and was rewritten verifies
    afterwards, and in every class that rewrites some frame did both; a frame
    with ret != 0 or applied 0 keeps every byte"""
    rewritten = REWRITTEN6 if v6 else REWRITTEN4
    seen = {k: 0 for k in rewritten}
    for n in (63, 257):
        f, rn, cls = make_batch(n, stride, v6)
        ret, data = restate_rnat_frames(f, rn, v6)
        for i in range(n):
            name = classes(v6)[cls[i]][0]
            changed = data[i].tobytes() != f["data"][i].tobytes()
            if ret[i] != 0 or not rn["rn_applied"][i] or name not in rewritten:
                assert not changed, (name, i)
                continue
            assert changed, (name, i)
            if f["len"][i] <= stride:
                assert frame_verifies(f["data"][i], int(f["len"][i])), (name, i)
                assert frame_verifies(data[i], int(f["len"][i])), (name, i)
                seen[name] += 1
    # a 64-byte slot cuts the IPv6 TCP and extension-header frames short
    cut = {"tcp port", "tcp port 0", "udp ext", "tcp ext"} if v6 and stride == 64 else \
        {"tcp ext"} if v6 and stride == 80 else set()
    for name, k in seen.items():
        assert (k > 0) != (name in cut), (name, k)


def test_batch_generator_meets_the_gpu_tests_needs():
    rets, n_applied = set(), 0
    for v6, stride in ((False, 64), (True, 64), (True, 80)):
        f, rn, cls = make_batch(257, stride, v6)
        ret, data = restate_rnat_frames(f, rn, v6)
        rets |= set(ret.tolist())
        n_applied += int(rn["rn_applied"].sum())
        assert set(cls.tolist()) == set(range(len(classes(v6))))
        for name in ("miss", "index 0"):
            assert not rn["rn_applied"][cls == class_of(v6, name)].any()
        for name in ("other family", "arp", "short"):
            assert rn["rn_applied"][cls == class_of(v6, name)].all()
        same = cls == class_of(v6, "udp same port" if v6 else "tcp same port")
        assert rn["rn_applied"][same].all() and (data[same] != f["data"][same]).any()
    assert rets == {0, L.DROP_CSUM_L4, L.DROP_SNAPLEN} and n_applied


# ---- loopback: inferred from the columns against ct_state->loopback given ------
def _v4(proto, sa, da, csum_field=None, **kw):
    fr = bytearray(build_frame(False, proto, sa, da, 8080, 4660, bytes(range(10)), **kw))
    if csum_field is not None:
        off = 34 + {TCP: 16, UDP: 6}[proto]
        fr[off:off + 2] = struct.pack(">H", csum_field)
    return slot(bytes(fr), 64), len(fr)


def _u32(b):
    return struct.unpack("<I", bytes(b))[0]


LOOP_ADDRS = [(bytes([64, 48, 32, 16]), bytes([10, 245, 255, 31])),      # the usual: the reply goes to IPV4_LOOPBACK
              (bytes([64, 48, 32, 16]), bytes([64, 48, 32, 16])),       # saddr == daddr: nothing to infer
              (bytes([255] * 4), bytes([255] * 4)),                     # and both 255.255.255.255
              (bytes(4), bytes(4)), (bytes([255] * 4), bytes(4)), (bytes(4), bytes([255] * 4))]


@pytest.mark.parametrize("sa,da", LOOP_ADDRS)
@pytest.mark.parametrize("nsa", [bytes([10, 96, 0, 30]), bytes([255] * 4), bytes(4)])
@pytest.mark.parametrize("proto,field", [(TCP, None), (TCP, 0x0000), (TCP, 0xFFFF), (UDP, None), (UDP, 0x0000),
                                         (UDP, 0xFFFF), (ICMP, None)])
def test_inferred_and_explicit_loopback_agree(sa, da, nsa, proto, field):
    """the reference seeds the csum_diff from the daddr words whenever
    ct_state->loopback is set, the call only where the daddr column differs
    from the frame: the stored bytes are the same, shown here and not assumed
    (the header checksum field is tried at 0x0000 and 0xFFFF too)"""
    for hdr_field in (None, 0x0000, 0xFFFF):
        fr, ln = _v4(proto, sa, da, field)
        if hdr_field is not None:
            fr = fr[:24] + struct.pack(">H", hdr_field) + fr[26:]
        for sp in (L.htons(8080), L.htons(80)):
            # loopback: the new daddr is the old saddr
            inferred = restate_rnat_frame(fr, ln, 64, 1, _u32(nsa), _u32(sa), sp, False)
            explicit = restate_rnat_frame(fr, ln, 64, 1, _u32(nsa), _u32(sa), sp, False, loopback=True)
            assert inferred == explicit
            # no loopback: the daddr column is the frame's
            inferred = restate_rnat_frame(fr, ln, 64, 1, _u32(nsa), _u32(da), sp, False)
            explicit = restate_rnat_frame(fr, ln, 64, 1, _u32(nsa), _u32(da), sp, False, loopback=False)
            assert inferred == explicit


def test_explicit_loopback_takes_the_seeded_path():
    """the comparison above is not of a thing with itself: with saddr == daddr
    the explicit form stores the daddr and seeds, the inferred form does not"""
    import rnat_frames_cases as m
    seeds = []
    real = m.csum_diff

    def spy(frm, to, seed=0):
        seeds.append(seed)
        return real(frm, to, seed)
    m.csum_diff = spy
    try:
        ep = bytes([64, 48, 32, 16])
        fr, ln = _v4(TCP, ep, ep)
        restate_rnat_frame(fr, ln, 64, 1, 0x1e00600a, _u32(ep), L.htons(80), False)
        assert seeds == [0]
        del seeds[:]
        restate_rnat_frame(fr, ln, 64, 1, 0x1e00600a, _u32(ep), L.htons(80), False, loopback=True)
        assert seeds == [0, 0xFFFFFFFF]
    finally:
        m.csum_diff = real


# ---- the calls' argument rules -------------------------------------------------
FAMILIES = [False, True]


def _args(v6, n=4, stride=64):
    keep = dict(data=np.zeros(n * stride + 16, np.uint8), len=np.full(n + 1, 64, np.uint32),
                applied=np.ones(n + 1, np.uint8), saddr=np.zeros(16 * (n + 2), np.uint8),
                daddr=np.zeros(n + 1, np.uint32), sport=np.zeros(n + 1, np.uint16), ret=np.zeros(n + 1, np.int32))
    base = (keep["data"].ctypes.data + 15) & ~15
    sa = (keep["saddr"].ctypes.data + 15) & ~15
    if v6:
        iv = _abi.Rnf6In(base, keep["len"].ctypes.data, stride, 0, keep["applied"].ctypes.data, sa,
                         keep["sport"].ctypes.data)
    else:
        iv = _abi.Rnf4In(base, keep["len"].ctypes.data, stride, 0, keep["applied"].ctypes.data, sa,
                         keep["daddr"].ctypes.data, keep["sport"].ctypes.data)
    return keep, iv, {"ret": keep["ret"].ctypes.data}


def _call(e, v6, iv, outs, flags=1, n=4):
    fn = e.L.cgpu_rnat_frames_v6 if v6 else e.L.cgpu_rnat_frames_v4
    return fn(e.h, C.byref(iv) if iv is not None else None, flags, n, outs["ret"], None)


def _rc(v6, change=None, flags=1, n=4):
    e = Engine(device=-1)
    keep, iv, outs = _args(v6)
    if change:
        change(iv, outs)
    rc = _call(e, v6, iv, outs, flags, n)
    e.close()
    return rc


def test_both_symbols_exist_and_the_mirror_matches():
    lib = _abi.lib()
    assert lib.cgpu_rnat_frames_v4 and lib.cgpu_rnat_frames_v6
    # sizeof / offsetof as csrc/host.cpp asserts them at compile time
    assert C.sizeof(_abi.Rnf4In) == 56 and _abi.Rnf4In.stride.offset == 16 and _abi.Rnf4In.reserved.offset == 20
    assert _abi.Rnf4In.applied.offset == 24 and _abi.Rnf4In.sport.offset == 48
    assert C.sizeof(_abi.Rnf6In) == 48 and _abi.Rnf6In.applied.offset == 24 and _abi.Rnf6In.sport.offset == 40
    assert L.RNF_REWRITE == 1


@pytest.mark.parametrize("v6", FAMILIES)
def test_rnat_frames_on_a_host_only_context(v6):
    assert _rc(v6) == -errno.ENODEV
    assert _rc(v6, flags=0) == -errno.ENODEV
    assert _rc(v6, lambda iv, outs: outs.__setitem__("ret", None)) == -errno.ENODEV   # ret is optional
    assert _rc(v6, lambda iv, outs: setattr(iv, "applied", iv.applied + 1)) == -errno.ENODEV
    # n == 0 is a no-op: no device and no column is needed, the shape of the call still is judged
    assert _rc(v6, n=0) == 0
    assert _rc(v6, flags=2, n=0) == -errno.EINVAL


@pytest.mark.parametrize("v6", FAMILIES)
def test_rnat_frames_null_struct_and_context(v6):
    e = Engine(device=-1)
    keep, iv, outs = _args(v6)
    assert _call(e, v6, None, outs) == -errno.EINVAL
    fn = e.L.cgpu_rnat_frames_v6 if v6 else e.L.cgpu_rnat_frames_v4
    assert fn(None, C.byref(iv), 1, 4, outs["ret"], None) == -errno.EINVAL
    e.close()


@pytest.mark.parametrize("v6,field", [(v6, f) for v6 in FAMILIES for f in
                                      ("data", "len", "applied", "saddr", "sport") + (() if v6 else ("daddr",))])
def test_rnat_frames_null_required_column(v6, field):
    assert _rc(v6, lambda iv, outs: setattr(iv, field, None)) == -errno.EINVAL
    assert _rc(v6, lambda iv, outs: setattr(iv, field, None), n=0) == 0   # with n == 0 nothing is required


@pytest.mark.parametrize("v6", FAMILIES)
def test_rnat_frames_flags_and_reserved(v6):
    for flags in (2, 3, 0x80000000):
        assert _rc(v6, flags=flags) == -errno.EINVAL
    assert _rc(v6, lambda iv, outs: setattr(iv, "reserved", 1)) == -errno.EINVAL


@pytest.mark.parametrize("v6", FAMILIES)
@pytest.mark.parametrize("stride", [0, 16, 48, 63, 72, 100])
def test_rnat_frames_bad_stride(v6, stride):
    assert _rc(v6, lambda iv, outs: setattr(iv, "stride", stride)) == -errno.EINVAL


@pytest.mark.parametrize("v6", FAMILIES)
def test_rnat_frames_alignment(v6):
    for off in (1, 4, 8):
        assert _rc(v6, lambda iv, outs: setattr(iv, "data", iv.data + off)) == -errno.EINVAL
    for off in (1, 2):
        assert _rc(v6, lambda iv, outs: setattr(iv, "len", iv.len + off)) == -errno.EINVAL
        assert _rc(v6, lambda iv, outs: outs.__setitem__("ret", outs["ret"] + off)) == -errno.EINVAL
        if not v6:
            assert _rc(v6, lambda iv, outs: setattr(iv, "daddr", iv.daddr + off)) == -errno.EINVAL
    assert _rc(v6, lambda iv, outs: setattr(iv, "sport", iv.sport + 1)) == -errno.EINVAL
    for off in (1, 2, 4, 8) if v6 else (1, 2):
        assert _rc(v6, lambda iv, outs: setattr(iv, "saddr", iv.saddr + off)) == -errno.EINVAL
    if not v6:
        assert _rc(v6, lambda iv, outs: setattr(iv, "saddr", iv.saddr + 4)) == -errno.ENODEV


# ---- Engine.rnat_frames --------------------------------------------------------
class _Recorder:
    """stands in for the library: records which entry points a call reaches"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append(name)
            return 0
        return f


class _T:
    """just enough of a tensor for the engine's argument marshalling"""

    def __init__(self, n, shape=None):
        self.n, self.shape, self.device = n, shape or (n,), "cpu"

    def numel(self):
        return self.n

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return 4096


class _Stream:
    cuda_stream = 0


@pytest.mark.parametrize("v6", FAMILIES)
def test_engine_rnat_frames_routes_by_family_and_wants_its_columns(v6):
    e = object.__new__(Engine)
    e.L, e.h = _Recorder(), None
    f = {"data": _T(4 * 64, (4, 64)), "len": _T(4)}
    rn = {k: _T(4) for k in ("rn_applied", "rn_saddr", "rn_sport", "rn_daddr", "verdict")}
    if v6:
        rn["rn_saddr"] = _T(64, (4, 16))
    with pytest.raises(ValueError):   # columns of another batch
        e.rnat_frames(f, dict(rn, rn_sport=_T(5)), v6=v6, out={"ret": _T(4)}, stream=_Stream())
    out = e.rnat_frames(f, rn, v6=v6, out={"ret": _T(4)}, stream=_Stream())
    assert set(out) == {"ret"} and e.L.calls == ["cgpu_rnat_frames_v6" if v6 else "cgpu_rnat_frames_v4"]
    for k in ("rn_applied", "rn_saddr", "rn_sport") + (() if v6 else ("rn_daddr",)):
        del e.L.calls[:]
        with pytest.raises(ValueError):
            e.rnat_frames(f, {j: v for j, v in rn.items() if j != k}, v6=v6, out={"ret": _T(4)}, stream=_Stream())
        assert e.L.calls == []   # before any launch
    if v6:   # IPv6 has no rn_daddr
        e.rnat_frames(f, {j: v for j, v in rn.items() if j != "rn_daddr"}, v6=True, out={"ret": _T(4)},
                      stream=_Stream())


def test_header_says_the_rules_and_what_is_out_of_scope():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cgpu.h")).read()
    body = hdr[hdr.index("Reverse NAT on raw frames"):hdr.index("int cgpu_rnat_frames_v6")]
    for word in ("A dropped frame keeps every", "inferred from the columns", "index\n * bits cleared", "_ctlb",
                 "_host form", "skb->csum", "#define CGPU_RNF_REWRITE 1u", "CGPU_DROP_WRITE_ERROR is never returned"):
        assert word in body, word
