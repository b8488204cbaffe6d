"""The forwarding step on raw frames without a device: the per-frame
restatement against the literal frames (tests/forward_frames_cases.py), the
incremental checksum against a from-scratch RFC 1071 sum, and
cgpu_forward_frames' argument checks and struct sizes on a host-only context."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from cilium_amd import build
from cilium_amd._abi import FwdOut, FwdfIn, FwdfParams
from cilium_amd.engine import Engine
from forward_cases import DROP, HOST, LOCAL, LXC, NETDEV, NONE, OVERLAY, PROXY, STACK, TIME_EXCEEDED
from forward_frames_cases import (FRAMES, batch_frame_world, csum_dec_ttl, csum_rfc1071, family_batch,
                                  header_verifies, literal_frame, literal_frame_world, mixed_batch,
                                  restate_frame, restate_frames)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


# --------------------------------------------------------------------------
# the literal frames pin the restatement
# --------------------------------------------------------------------------
@pytest.mark.parametrize("row", FRAMES, ids=[r[0] for r in FRAMES])
@pytest.mark.parametrize("stride", [64, 128])
def test_restatement_matches_the_literal_frames(row, stride):
    name, mode, encap, verdict, stage, flags, tunnel, length, head, want, after = row
    fr = bytearray(literal_frame(head, stride))
    got = restate_frame(literal_frame_world(encap), mode, fr, length, flags, verdict, stage, tunnel, True)
    assert tuple(got) == want, name
    assert bytes(fr) == literal_frame(after if after is not None else head, stride), name
    # without the rewrite flag: the same decision, every byte kept
    fr = bytearray(literal_frame(head, stride))
    assert tuple(restate_frame(literal_frame_world(encap), mode, fr, length, flags, verdict, stage, tunnel,
                               False)) == want
    assert bytes(fr) == literal_frame(head, stride)


def test_literal_frames_cover_the_rewrite_table():
    seen = {(r[1], r[8][0].endswith("86 dd"), r[9][0], r[10] is not None) for r in FRAMES}
    for v6 in (False, True):
        for act in (PROXY, HOST, LOCAL, STACK):
            assert (LXC, v6, act, True) in seen, (v6, act)
        assert (NETDEV, v6, LOCAL, True) in seen and (NETDEV, v6, STACK, False) in seen
        assert (LXC, v6, OVERLAY, False) in seen and (LXC, v6, DROP, False) in seen
    assert (LXC, True, TIME_EXCEEDED, False) in seen and (LXC, False, NONE, False) in seen
    assert not any(r[2] and r[9][0] in (NONE, DROP, OVERLAY, TIME_EXCEEDED) and r[10] is not None for r in FRAMES)
    by_name = {r[0]: r for r in FRAMES}
    for name in ("lxc4 local, checksum ff ff", "lxc4 local, checksum fe ff", "lxc4 local, checksum 00 00",
                 "lxc4 local, ihl 6", "lxc4 local, ttl 2", "lxc4 local, ttl 1: dropped as it came"):
        assert name in by_name


# --------------------------------------------------------------------------
# the incremental checksum against a from-scratch sum
# --------------------------------------------------------------------------
def test_rewritten_literal_headers_verify():
    """every literal IPv4 frame whose header verifies on input verifies after
    the rewrite, over ihl * 4 bytes -- by a sum that knows nothing of the
    incremental formula; the hand-written outputs themselves included"""
    n = 0
    for r in FRAMES:
        head = literal_frame(r[8])
        if head[12:14] != b"\x08\x00" or not header_verifies(head):
            continue
        fr = bytearray(head)
        restate_frame(literal_frame_world(r[2]), r[1], fr, r[7], r[5], r[3], r[4], r[6], True)
        assert header_verifies(fr), r[0]
        if r[10] is not None:
            assert header_verifies(literal_frame(r[10])), r[0]
            n += 1
    assert n >= 8


def test_rfc1071_on_a_known_header():
    # the worked example of RFC 1071 style sums: 45 00 00 73 00 00 40 00 40 11 [b8 61] c0 a8 00 01 c0 a8 00 c7
    h = bytes.fromhex("450000730000400040110000c0a80001c0a800c7")
    assert csum_rfc1071(h) == 0xB861


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
@pytest.mark.parametrize("mode", [LXC, NETDEV], ids=["lxc", "netdev"])
def test_rewritten_batch_headers_verify(mode, v6):
    w = batch_frame_world()
    b, f = family_batch(w, v6, 257)
    if not v6:
        assert all(header_verifies(f["data"][i]) for i in range(257))
    exp, data = restate_frames(w, mode, f, b["verdict"], b["stage"], b["tunnel"], True)
    changed = (data != f["data"]).any(axis=1)
    moved = np.isin(exp["action"], (PROXY, HOST, LOCAL)) | ((exp["action"] == STACK) & (mode == LXC))
    np.testing.assert_array_equal(changed, moved)  # (random MACs never equal the written ones)
    assert changed.any() and (~changed).any()
    assert (data[:, 32:] == f["data"][:, 32:]).all()
    if not v6:
        assert all(header_verifies(data[i]) for i in range(257))
        assert (data[changed, 22] == f["data"][changed, 22] - 1).all()
    else:
        assert (data[changed, 21] == f["data"][changed, 21] - 1).all()
        assert (data[:, 22:32] == f["data"][:, 22:32]).all() and (data[:, 12:21] == f["data"][:, 12:21]).all()


def test_incremental_checksum_over_every_input():
    """every checksum field and every ttl that is decremented: the result is
    the field plus one with an end-around carry, and never 0xFFFF"""
    c = np.arange(65536, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)

    def add(a, b):  # csum_dec_ttl's steps on a whole column, in u64 masked to 32 bits
        r = (a + b) & m
        return (r + (r < b)) & m
    want = np.where(c == 0xFFFF, 1, np.where(c == 0xFFFE, 0, c + np.uint64(1)))
    for ttl in range(2, 256):
        t = add(add(~c & m, np.uint64(~ttl & 0xFFFFFFFF)), np.uint64(ttl - 1))
        t = (t & np.uint64(0xFFFF)) + (t >> np.uint64(16))
        t = (t & np.uint64(0xFFFF)) + (t >> np.uint64(16))
        got = ~t & np.uint64(0xFFFF)
        np.testing.assert_array_equal(got, want, err_msg=f"ttl {ttl}")
        assert (got != 0xFFFF).all()
        # the column form is the scalar function
        for x in (0, 1, 0x1234, 0xFEFF, 0xFFFE, 0xFFFF):
            assert csum_dec_ttl(x, ttl) == int(got[x])


def test_mixed_batch_interleaves_the_families():
    w = batch_frame_world()
    b4, b6, f, is6 = mixed_batch(w, 5)
    assert f["data"].shape == (10, 64) and is6.tolist() == [False, True] * 5
    assert (f["data"][~is6, 12:14] == (0x08, 0x00)).all() and (f["data"][is6, 12:14] == (0x86, 0xDD)).all()


# --------------------------------------------------------------------------
# the C ABI on a host-only context
# --------------------------------------------------------------------------
def _args(n=4, stride=64, mode=LXC):
    """a well-formed call's structs over host arrays (never dereferenced: the
    context has no device)"""
    keep = dict(data=np.zeros(n * stride + 64, np.uint8), len=np.zeros(n, np.uint32), flags=np.zeros(n, np.uint8),
                verdict=np.zeros(n, np.int32), stage=np.zeros(n, np.uint8), tunnel=np.zeros(n, np.uint32),
                action=np.zeros(n, np.uint8), ret=np.zeros(n + 1, np.int32), ifindex=np.zeros(n + 1, np.uint32),
                arg=np.zeros(n + 1, np.uint32))
    base = (keep["data"].ctypes.data + 15) & ~15
    p = FwdfParams()
    p.fwd.mode, p.fwd.flags, p.fwd.ipv4_mask, p.fwd.host_ifindex, p.fwd.encap_ifindex = mode, 1, 0xFFFF, 1, 1
    p.flags = 1
    iv = FwdfIn(base, keep["len"].ctypes.data, keep["flags"].ctypes.data, stride, 0, keep["verdict"].ctypes.data,
                keep["stage"].ctypes.data, keep["tunnel"].ctypes.data)
    ov = FwdOut(*[keep[k].ctypes.data for k in ("action", "ret", "ifindex", "arg")])
    return keep, p, iv, ov


def _call(e, p, iv, ov, n=4):
    return e.L.cgpu_forward_frames(e.h, C.byref(p) if p is not None else None, C.byref(iv) if iv is not None else None,
                                   n, C.byref(ov) if ov is not None else None, None)


def test_forward_frames_on_a_host_only_context():
    e = Engine(device=-1)
    keep, p, iv, ov = _args()
    assert _call(e, p, iv, ov) == -errno.ENODEV
    assert _call(e, p, iv, ov, n=0) == -errno.ENODEV
    keep, p, iv, ov = _args(mode=NETDEV)
    iv.flags = iv.verdict = iv.stage = iv.tunnel = None   # NETDEV reads none of them
    ov.ret = ov.ifindex = ov.arg = None
    p.flags = p.fwd.flags = 0
    assert _call(e, p, iv, ov) == -errno.ENODEV
    e.close()


def test_forward_frames_null_structs():
    e = Engine(device=-1)
    keep, p, iv, ov = _args()
    assert _call(e, None, iv, ov) == -errno.EINVAL
    assert _call(e, p, None, ov) == -errno.EINVAL
    assert _call(e, p, iv, None) == -errno.EINVAL
    assert e.L.cgpu_forward_frames(None, C.byref(p), C.byref(iv), 4, C.byref(ov), None) == -errno.EINVAL
    e.close()


def _bad(change, mode=LXC, n=4):
    e = Engine(device=-1)
    keep, p, iv, ov = _args(mode=mode)
    change(p, iv, ov)
    rc = _call(e, p, iv, ov, n)
    e.close()
    return rc


@pytest.mark.parametrize("field", ["data", "len", "flags", "verdict", "stage"])
def test_forward_frames_null_required_column(field):
    assert _bad(lambda p, iv, ov: setattr(iv, field, None)) == -errno.EINVAL


def test_forward_frames_null_action_and_netdev_columns():
    assert _bad(lambda p, iv, ov: setattr(ov, "action", None)) == -errno.EINVAL
    for field in ("data", "len"):   # NETDEV needs these two only
        assert _bad(lambda p, iv, ov: setattr(iv, field, None), mode=NETDEV) == -errno.EINVAL
    assert _bad(lambda p, iv, ov: setattr(iv, "tunnel", None)) == -errno.ENODEV  # optional everywhere


def test_forward_frames_mode_flags_reserved_pad():
    assert _bad(lambda p, iv, ov: setattr(p.fwd, "mode", 2)) == -errno.EINVAL
    assert _bad(lambda p, iv, ov: setattr(p.fwd, "flags", 2)) == -errno.EINVAL
    assert _bad(lambda p, iv, ov: setattr(p, "flags", 2)) == -errno.EINVAL
    assert _bad(lambda p, iv, ov: setattr(p, "flags", 3)) == -errno.EINVAL
    for i in range(3):
        def fwd_res(p, iv, ov, i=i):
            p.fwd.reserved[i] = 1

        def res(p, iv, ov, i=i):
            p.reserved[i] = 1
        assert _bad(fwd_res) == -errno.EINVAL and _bad(res) == -errno.EINVAL
    for i in range(2):
        def pad(p, iv, ov, i=i):
            p.pad[i] = 1
        assert _bad(pad) == -errno.EINVAL
    assert _bad(lambda p, iv, ov: setattr(iv, "reserved", 1)) == -errno.EINVAL
    # all of it is judged before the batch size is
    assert _bad(lambda p, iv, ov: setattr(p.fwd, "mode", 2), n=0) == -errno.EINVAL
    assert _bad(lambda p, iv, ov: setattr(iv, "stride", 48), n=0) == -errno.EINVAL


@pytest.mark.parametrize("stride", [0, 16, 48, 63, 72, 100])
def test_forward_frames_bad_stride(stride):
    assert _bad(lambda p, iv, ov: setattr(iv, "stride", stride)) == -errno.EINVAL


def test_forward_frames_alignment():
    for off in (1, 4, 8):
        assert _bad(lambda p, iv, ov: setattr(iv, "data", iv.data + off)) == -errno.EINVAL
    for field in ("len", "verdict", "tunnel"):
        for off in (1, 2):
            assert _bad(lambda p, iv, ov: setattr(iv, field, getattr(iv, field) + off)) == -errno.EINVAL
    for field in ("ret", "ifindex", "arg"):
        assert _bad(lambda p, iv, ov: setattr(ov, field, getattr(ov, field) + 2)) == -errno.EINVAL
    # one-byte columns sit anywhere
    assert _bad(lambda p, iv, ov: setattr(iv, "flags", iv.flags + 1)) == -errno.ENODEV
    assert _bad(lambda p, iv, ov: setattr(iv, "stage", iv.stage + 1)) == -errno.ENODEV
    assert _bad(lambda p, iv, ov: setattr(ov, "action", ov.action + 1)) == -errno.ENODEV


def test_struct_sizes_match_the_header(tmp_path):
    """sizeof and the field offsets of the two new structs, as a C compiler
    sees include/cgpu.h, against the ctypes mirror"""
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cgpu.h"\n'
                   "int main(void){printf(\"%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n\","
                   "sizeof(cgpu_fwdf_params), sizeof(cgpu_fwdf_in), offsetof(cgpu_fwdf_params, host_mac),"
                   "offsetof(cgpu_fwdf_params, pad), offsetof(cgpu_fwdf_params, flags),"
                   "offsetof(cgpu_fwdf_params, reserved), offsetof(cgpu_fwdf_in, stride),"
                   "offsetof(cgpu_fwdf_in, verdict), offsetof(cgpu_fwdf_in, stage), offsetof(cgpu_fwdf_in, tunnel));"
                   "return 0;}\n")
    exe = tmp_path / "sz"
    # a host C compiler: the system's, or the clang that hipcc drives
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(build.hipcc()) or ""))),
                              "llvm", "bin", "clang")
    cc = next(c for c in (shutil.which(os.environ.get("CC", "cc")), shutil.which("gcc"), shutil.which("clang"),
                          rocm_clang, "/opt/rocm/llvm/bin/clang") if c and os.path.exists(c))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P, I = FwdfParams, FwdfIn
    assert got == [C.sizeof(P), C.sizeof(I), P.host_mac.offset, P.pad.offset, P.flags.offset, P.reserved.offset,
                   I.stride.offset, I.verdict.offset, I.stage.offset, I.tunnel.offset]
    assert got[:2] == [56, 56]
    # the header says what the call does not model
    hdr = open(os.path.join(ROOT, "include", "cgpu.h")).read()
    body = hdr[hdr.index("The forwarding step on raw frames"):hdr.index("int cgpu_forward_frames")]
    for word in ("ipv4_redirect_to_host_port", "ipv6_store_flowlabel", "rewrite_dmac_to_host", "DROP_WRITE_ERROR",
                 "LXC_NAT46", "tunnel header"):
        assert re.search(word, body), word
    assert sys.byteorder == "little"
