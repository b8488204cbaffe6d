"""The stateful path on raw frames, without a GPU: the reference of
tests/frames_ct_cases.py against its hand-written table, the round trip of
make_ct_stream streams through synth.frames_from_ct, the class coverage of
the batches the GPU tests use, and the argument rules of cgpu_frames_parse_ct
/ cgpu_classify_frames_ct on a host-only context."""
import ctypes as C
import errno
import os

import numpy as np
import pytest

from cilium_amd import _abi, layouts as L, synth
from cilium_amd.engine import Engine
import frames_ct_cases as fc


# ---- the literal table ---------------------------------------------------------
@pytest.fixture(scope="module")
def oracle():
    return fc.make_oracle()


@pytest.mark.parametrize("stride", fc.literal_strides())
def test_restatement_reproduces_the_literal_table(oracle, stride):
    rows, f = fc.literal_batch(stride)
    exp, ok = fc.literal_expected(rows)
    got = fc.restate_parse_ct(oracle, f)
    for i, r in enumerate(rows):
        assert got["status"][i] == exp["status"][i], r[0]
    fc.check_parse(got, exp)


def test_literal_table_covers_the_cases():
    names = " | ".join(r[0] for r in fc.LITERAL)
    for word in ("byte 12", "l4 = 42", "ihl 15 in a 64", "ihl 15 in a 128", "l4 + 13", "l4 + 14", "ingress",
                 "LB_L4", "echo request", "echo reply", "unreachable", "fragment", "gre", "arp", "source mac",
                 "80-byte", "v6 tcp in a 64", "l4 = 62", "fragment header", "ROUTER_IP", "to a peer"):
        assert word in names, word
    st = {r[5] for r in fc.LITERAL}
    assert {0, L.DROP_SNAPLEN, L.DROP_CT_INVALID_HDR, L.EFAULT_LOAD, L.DROP_CT_UNKNOWN_PROTO, L.FRAME_NOT_CLASSIFIED,
            L.DROP_INVALID_SMAC, L.DROP_FRAG_NOSUPPORT} <= st
    # the byte order of l4: doff / NS (byte 12) in the low half, the flags (byte 13) in the high half
    r = fc.LITERAL[0]
    b = fc.hx(*r[4])
    assert b[46] == 0x51 and b[47] == 0x02 and r[10] == 0x0251


# ---- round trip ----------------------------------------------------------------
@pytest.mark.parametrize("v6,stride", [(False, 64), (False, 128), (True, 80), (True, 128)])
def test_streams_round_trip_through_frames(oracle, v6, stride):
    """every frame of a make_ct_stream stream has status 0 and the stream's own
    columns, but the packets of the untracked protocol (-137)"""
    s = fc.make_streams(600, seed=3)[1 if v6 else 0]
    f, s = synth.frames_from_ct(s, stride, v6=v6)
    n = len(s["proto"])
    assert n > 2000 and f["data"].shape == (n, stride)
    got = fc.restate_parse_ct(oracle, f)
    gre = s["proto"] == 47
    assert 20 < gre.sum() < n // 10
    np.testing.assert_array_equal(got["status"], np.where(gre, L.DROP_CT_UNKNOWN_PROTO, 0))
    ok = ~gre
    assert (got["family"] == (6 if v6 else 4)).all()
    for k in ("proto", "l4b", "flags"):
        np.testing.assert_array_equal(got[k][ok], s[k][ok], err_msg=k)
    tu = (s["proto"] == 6) | (s["proto"] == 17)   # the stream's ICMP packets carry their connection's ports: not on the wire
    for k in ("sport", "dport"):
        np.testing.assert_array_equal(got[k][tu], s[k][tu], err_msg=k)
        assert not got[k][~tu].any()
    w = 16 if v6 else 4
    for k in ("saddr", "daddr"):
        np.testing.assert_array_equal(got[k][ok][:, :w], np.ascontiguousarray(s[k]).view(np.uint8).reshape(n, w)[ok],
                                      err_msg=k)
    np.testing.assert_array_equal(f["len"], s["len"])
    assert (s["len"][s["proto"] == 6] >= (74 if v6 else 54)).all()


def test_v6_tcp_in_64_byte_slots_is_its_own_class(oracle):
    s = fc.make_streams(100, seed=3)[1]
    f, s = synth.frames_from_ct(s, 64, v6=True)
    got = fc.restate_parse_ct(oracle, f)
    tcp = s["proto"] == 6
    assert tcp.sum() > 50 and (got["status"][tcp] == L.DROP_SNAPLEN).all()
    assert (got["status"][s["proto"] == 17] == 0).all()


# ---- class coverage of the GPU tests' batches ----------------------------------
def test_the_gpu_batch_holds_every_class():
    f = fc.make_mixed(4099, 80)
    out = fc.Chain().run(f)
    assert fc.classes(out, f) == fc.ALL_CLASSES
    st = out["status"]
    for code in (L.FRAME_NOT_CLASSIFIED, L.DROP_INVALID, L.DROP_INVALID_SMAC, L.DROP_CT_UNKNOWN_PROTO):
        assert (st == code).sum() > 10, code
    # the ended frames sit between packets of connections: both neighbours of some are conntrack packets
    mid = (st[1:-1] != 0) & (st[:-2] == 0) & (st[2:] == 0)
    assert mid.sum() > 50
    f64 = fc.make_mixed(4099, 64)
    assert (fc.Chain().run(f64)["status"] == L.DROP_SNAPLEN).sum() > 100


def test_all_sizes_together_lose_no_class():
    seen = set()
    for n in fc.SIZES:
        f = fc.make_mixed(n, 128)
        seen |= fc.classes(fc.Chain().run(f), f)
    assert seen == fc.ALL_CLASSES


def test_the_reverse_nat_batch_applies():
    f, e4, e6 = fc.rnat_batch(200)
    o = fc.rnat_oracle()
    fc.rnat_install(o, e4, e6)
    out = fc.Chain(o).run(f, rev_nat=True)
    assert "rn applied" in fc.classes(out, f)
    ap = out["rn_applied"] == 1
    assert (ap & (out["family"] == 4)).sum() > 10 and (ap & (out["family"] == 6)).sum() > 10
    assert (out["status"] != 0).sum() > 5
    assert not out["rn_saddr6"][out["family"] != 6].any() and not out["rn_saddr"][out["family"] != 4].any()
    # every frame carries valid checksums and lies inside its slot
    from lb_frames_cases import frame_verifies
    for i in np.nonzero(out["status"] == 0)[0]:
        assert frame_verifies(f["data"][i], int(f["len"][i])), i


# ---- the calls' argument rules -------------------------------------------------
N = 4


def _args(stride=64):
    keep = dict(data=np.zeros(N * stride + 16, np.uint8), len=np.full(N + 1, 64, np.uint32),
                flags=np.zeros(N, np.uint8), ep=np.zeros(N + 1, np.uint16),
                status=np.zeros(N + 1, np.int32), family=np.zeros(N, np.uint8), a16=np.zeros(16 * (3 * N + 4), np.uint8),
                u16=np.zeros(4 * N + 4, np.uint16), u8=np.zeros(4 * N, np.uint8), u32=np.zeros(4 * N + 4, np.uint32))
    base = (keep["data"].ctypes.data + 15) & ~15
    a16 = (keep["a16"].ctypes.data + 15) & ~15
    u16, u8, u32 = keep["u16"].ctypes.data, keep["u8"].ctypes.data, keep["u32"].ctypes.data
    fr = _abi.Frames(base, keep["len"].ctypes.data, keep["flags"].ctypes.data, keep["ep"].ctypes.data, stride, 0)
    cols = _abi.FrameCtCols(keep["status"].ctypes.data, keep["family"].ctypes.data, a16, a16 + 16 * N, u16, u16 + 2 * N,
                            u8, u16 + 4 * N, u8 + N)
    out = _abi.FctOut(keep["status"].ctypes.data, keep["family"].ctypes.data, u32, u8, u32 + 4 * N, u8 + N,
                      u8 + 2 * N, u16, u32 + 8 * N, u32 + 12 * N, a16 + 32 * N)
    return keep, fr, cols, out


def _rc(call, change=None, n=N, ctx=True, **cfg):
    """the return code of cgpu_frames_parse_ct ("parse") or cgpu_classify_frames_ct
    ("classify") on a host-only context after `change(frames, columns)`"""
    e = Engine(device=-1, **cfg)
    keep, fr, cols, out = _args()
    o = cols if call == "parse" else out
    if change:
        change(fr, o)
    h = e.h if ctx else None
    if call == "parse":
        rc = e.L.cgpu_frames_parse_ct(h, C.byref(fr), n, C.byref(o), None)
    else:
        rc = e.L.cgpu_classify_frames_ct(h, C.byref(fr), n, fc.NOW, C.byref(o), None)
    e.close()
    return rc


CALLS = ["parse", "classify"]


def test_both_symbols_exist_and_the_mirror_matches():
    lib = _abi.lib()
    assert lib.cgpu_frames_parse_ct and lib.cgpu_classify_frames_ct
    # sizeof / offsetof as csrc/host.cpp asserts them at compile time
    assert C.sizeof(_abi.FrameCtCols) == 72 and _abi.FrameCtCols.l4.offset == 56
    assert C.sizeof(_abi.FctOut) == 88 and _abi.FctOut.rn_applied.offset == 48
    assert _abi.CGPU_ABI_VERSION == 2


@pytest.mark.parametrize("call", CALLS)
def test_host_only_context(call):
    assert _rc(call) == -errno.ENODEV
    assert _rc(call, n=0) == -errno.ENODEV          # the context is judged before n
    # the optional columns may be NULL
    opt = ("family", "saddr", "daddr", "sport", "dport", "proto", "l4", "flags") if call == "parse" else \
        ("status", "family", "stage")
    for k in opt:
        assert _rc(call, lambda fr, o: setattr(o, k, None)) == -errno.ENODEV, k
    # ENODEV comes before the ct_proto_gate rule
    assert _rc(call, ct_proto_gate=0) == -errno.ENODEV


@pytest.mark.parametrize("call", CALLS)
def test_null_struct_context_and_required_columns(call):
    e = Engine(device=-1)
    keep, fr, cols, out = _args()
    o = cols if call == "parse" else out
    if call == "parse":
        fn = lambda h, f, x: e.L.cgpu_frames_parse_ct(h, f, N, x, None)          # noqa: E731
    else:
        fn = lambda h, f, x: e.L.cgpu_classify_frames_ct(h, f, N, fc.NOW, x, None)  # noqa: E731
    assert fn(None, C.byref(fr), C.byref(o)) == -errno.EINVAL
    assert fn(e.h, None, C.byref(o)) == -errno.EINVAL
    assert fn(e.h, C.byref(fr), None) == -errno.EINVAL
    e.close()
    for k in ("data", "len", "flags", "ep"):
        assert _rc(call, lambda fr, o: setattr(fr, k, None)) == -errno.EINVAL, k
    for k in (("status",) if call == "parse" else ("verdict", "ct_ret", "identity")):
        assert _rc(call, lambda fr, o: setattr(o, k, None)) == -errno.EINVAL, k
        # with n == 0 no column is needed (an empty tensor has no address): the context is judged next
        assert _rc(call, lambda fr, o: setattr(o, k, None), n=0) == -errno.ENODEV, k


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("stride", [0, 16, 48, 63, 72, 100])
def test_bad_stride(call, stride):
    assert _rc(call, lambda fr, o: setattr(fr, "stride", stride)) == -errno.EINVAL


@pytest.mark.parametrize("call", CALLS)
def test_reserved_and_alignment(call):
    assert _rc(call, lambda fr, o: setattr(fr, "reserved", 1)) == -errno.EINVAL
    for off in (1, 4, 8):
        assert _rc(call, lambda fr, o: setattr(fr, "data", fr.data + off)) == -errno.EINVAL
    for off in (1, 2):
        assert _rc(call, lambda fr, o: setattr(fr, "len", fr.len + off)) == -errno.EINVAL
        assert _rc(call, lambda fr, o: setattr(o, "status", o.status + off)) == -errno.EINVAL
    assert _rc(call, lambda fr, o: setattr(fr, "ep", fr.ep + 1)) == -errno.EINVAL
    if call == "parse":
        for k in ("sport", "dport", "l4"):
            assert _rc(call, lambda fr, o: setattr(o, k, getattr(o, k) + 1)) == -errno.EINVAL, k
        for k in ("saddr", "daddr"):
            for off in (1, 2, 4, 8):
                assert _rc(call, lambda fr, o: setattr(o, k, getattr(o, k) + off)) == -errno.EINVAL, k
    else:
        for k in ("verdict", "identity", "rn_saddr4", "rn_daddr4"):
            for off in (1, 2):
                assert _rc(call, lambda fr, o: setattr(o, k, getattr(o, k) + off)) == -errno.EINVAL, k
        assert _rc(call, lambda fr, o: setattr(o, "rn_sport", o.rn_sport + 1)) == -errno.EINVAL
        for off in (1, 2, 4, 8):
            assert _rc(call, lambda fr, o: setattr(o, "rn_saddr6", o.rn_saddr6 + off)) == -errno.EINVAL


def test_classify_rn_group_and_batch_size():
    rn = ("rn_applied", "rn_sport", "rn_saddr4", "rn_daddr4", "rn_saddr6")
    for k in rn:   # given in part
        assert _rc("classify", lambda fr, o: setattr(o, k, None)) == -errno.EINVAL, k
    for k in rn:   # one alone
        assert _rc("classify", lambda fr, o: [setattr(o, j, None) for j in rn if j != k]) == -errno.EINVAL, k
    assert _rc("classify", lambda fr, o: [setattr(o, j, None) for j in rn]) == -errno.ENODEV
    assert _rc("classify", n=(1 << 31)) == -errno.EINVAL
    assert _rc("classify", n=(1 << 31) - 1) == -errno.ENODEV


# ---- Engine, synth, documents ---------------------------------------------------
def test_engine_has_the_methods_and_synth_the_builder():
    import inspect
    sig = inspect.signature(Engine.classify_frames_ct)
    assert list(sig.parameters)[1:] == ["f", "now", "out", "stage", "rev_nat", "stream"]
    assert list(inspect.signature(Engine.frames_parse_ct).parameters)[1:] == ["f", "out", "stream"]
    assert list(inspect.signature(synth.frames_from_ct).parameters) == ["t", "stride", "v6"]


def test_header_and_design_say_the_rules():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = " ".join(open(os.path.join(root, "include", "cgpu.h")).read().replace("\n * ", " ").split())
    for s in ("cgpu_frames_parse_ct", "cgpu_classify_frames_ct", "pins ONE snapshot", "in frame order",
              "125 bytes per frame", "cannot be captured into a graph", "ct_proto_gate == 0"):
        assert s in h, s
    d = " ".join(open(os.path.join(root, "DESIGN.md")).read().split())
    for s in ("cgpu_classify_frames_ct", "125 bytes per frame", "`_ctlb` form on frames"):
        assert s in d, s
