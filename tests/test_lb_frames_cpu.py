"""The service step on raw frames (cgpu_classify_frames_lb) without a GPU: the
restatement against the literal frames, the literal frames against a
from-scratch checksum, and the call's argument rules on a host-only context."""
import ctypes as C
import errno

import numpy as np
import pytest

from cilium_amd import layouts as L
from cilium_amd._abi import FlbIn, FlbOut
from cilium_amd.engine import Engine
from lb_frames_cases import (COLS, LITERAL, LOOPBACK, NONE, NOT_VERIFYING, XLATED, attach_oracle, batch_world,
                             build_frame, frame_verifies, hx, literal_batch, literal_rows, literal_world,
                             make_batch, restate_frames_lb, slot)

GROUPS = [(64, 1), (128, 1), (64, 0)]   # (stride, ct_proto_gate) of the literal rows


def test_literal_rows_are_all_in_a_group():
    assert sum(len(literal_rows(s, g)) for s, g in GROUPS) == len(LITERAL)
    assert len({r[0] for r in LITERAL}) == len(LITERAL)


@pytest.mark.parametrize("stride,gate", GROUPS)
@pytest.mark.parametrize("rewrite", [True, False])
def test_restatement_reproduces_the_literal_frames(stride, gate, rewrite):
    rows = literal_rows(stride, gate)
    f, want, exp = literal_batch(rows)
    w = attach_oracle(literal_world(gate))
    out, data = restate_frames_lb(w, f, None, rewrite)
    for i, r in enumerate(rows):
        assert tuple(int(out[k][i]) for k in COLS) == r[6], r[0]
        assert data[i].tobytes() == (want if rewrite else f["data"])[i].tobytes(), r[0]


def test_literal_frames_cover_the_cases():
    rets = {r[6][3] for r in LITERAL}
    assert {NONE, XLATED, LOOPBACK, L.DROP_NO_SERVICE, L.DROP_CSUM_L4, L.DROP_SNAPLEN} <= rets
    assert any(r[7] is None and r[4] == 0 for r in LITERAL)              # an ingress frame
    assert any(hx(*r[5])[12:14] == b"\x08\x06" for r in LITERAL)         # ARP


@pytest.mark.parametrize("row", [r for r in LITERAL if r[7] is not None], ids=lambda r: r[0])
def test_literal_outputs_verify_from_scratch(row):
    """the input's checksums are valid, so the output's must be: header and
    L4, pseudo header included (UDP checksum 0 is exempt inside frame_verifies).
    The two rows of NOT_VERIFYING are the reference's own: it patches from a
    port the packet does not carry, or two bytes that are no checksum."""
    name, _, stride, length = row[:4]
    assert frame_verifies(slot(hx(*row[5]), stride), length), "input"
    if name in NOT_VERIFYING:
        assert not frame_verifies(slot(hx(*row[7]), stride), length) or "next header 1" in name
    else:
        assert frame_verifies(slot(hx(*row[7]), stride), length), "output"


def test_frame_builder_and_verifier_disagree_on_a_flipped_bit():
    for v6, proto in ((False, 6), (False, 17), (False, 1), (True, 6), (True, 17), (True, 58)):
        sa = bytes(16) if v6 else bytes(4)
        fr = bytearray(build_frame(v6, proto, sa, sa, payload=b"\x01\x02\x03\x04", icmp_type=128 if v6 else 8))
        assert frame_verifies(fr, len(fr))
        fr[-1] ^= 0x10
        assert not frame_verifies(fr, len(fr))


@pytest.mark.parametrize("stride", [64, 128])
def test_batch_generator_meets_the_gpu_tests_needs(stride):
    """what tests/test_gpu_lb_frames.py asks of its batches, shown here on the
    restatement alone: every lb_ret value, a port rewrite, a UDP-zero frame
    and an option frame among the translated ones, three quarters of the
    frames reaching policy in the parse, and every translated frame still
    verifying from scratch"""
    w = attach_oracle(batch_world())
    f, h, cls = make_batch(257, stride, cut=False)
    out, data = restate_frames_lb(w, f, h)
    assert {NONE, XLATED, LOOPBACK, L.DROP_NO_SERVICE} <= set(out["lb_ret"].tolist())
    assert (w.oracle.frames_parse(f)["status"] == 0).mean() >= 0.75
    x = out["lb_ret"] > 0
    assert x.sum() > 100
    for i in np.flatnonzero(x):
        assert frame_verifies(data[i], int(f["len"][i])), i
    for i in np.flatnonzero(~x):
        assert data[i].tobytes() == f["data"][i].tobytes()


# ---- the call's argument rules ------------------------------------------------
def _args(n=4, stride=64):
    keep = dict(data=np.zeros(n * stride + 16, np.uint8), len=np.full(n + 1, 64, np.uint32),
                flags=np.ones(n + 1, np.uint8), ep=np.zeros(n + 1, np.uint16), hash=np.zeros(n + 1, np.uint32),
                verdict=np.zeros(n + 1, np.int32), identity=np.zeros(n + 1, np.uint32), stage=np.zeros(n + 1, np.uint8),
                lb_ret=np.zeros(n + 1, np.int32), rev_nat=np.zeros(n + 1, np.uint16), slave=np.zeros(n + 1, np.uint16))
    base = (keep["data"].ctypes.data + 15) & ~15
    iv = FlbIn(base, keep["len"].ctypes.data, keep["flags"].ctypes.data, keep["ep"].ctypes.data, stride, 0,
               keep["hash"].ctypes.data)
    ov = FlbOut(keep["lb_ret"].ctypes.data, keep["rev_nat"].ctypes.data, keep["slave"].ctypes.data)
    outs = {k: keep[k].ctypes.data for k in ("verdict", "identity", "stage")}
    return keep, iv, ov, outs


def _call(e, iv, ov, outs, flags=1, n=4):
    return e.L.cgpu_classify_frames_lb(e.h, C.byref(iv) if iv is not None else None, flags, n, outs["verdict"],
                                       outs["identity"], outs["stage"], C.byref(ov) if ov is not None else None, None)


def _rc(change=None, flags=1, n=4):
    e = Engine(device=-1)
    keep, iv, ov, outs = _args()
    if change:
        change(iv, ov, outs)
    rc = _call(e, iv, ov, outs, flags, n)
    e.close()
    return rc


def test_frames_lb_on_a_host_only_context():
    assert _rc() == -errno.ENODEV
    assert _rc(n=0) == -errno.ENODEV
    assert _rc(flags=0) == -errno.ENODEV
    e = Engine(device=-1)
    keep, iv, ov, outs = _args()
    iv.hash = None
    outs["stage"] = None
    assert _call(e, iv, None, outs) == -errno.ENODEV      # hash, stage and the lb struct are optional
    ov.lb_ret = ov.rev_nat = ov.slave = None
    assert _call(e, iv, ov, outs) == -errno.ENODEV
    e.close()


def test_frames_lb_null_struct_and_context():
    e = Engine(device=-1)
    keep, iv, ov, outs = _args()
    assert _call(e, None, ov, outs) == -errno.EINVAL
    assert e.L.cgpu_classify_frames_lb(None, C.byref(iv), 1, 4, outs["verdict"], outs["identity"], outs["stage"],
                                       C.byref(ov), None) == -errno.EINVAL
    e.close()


@pytest.mark.parametrize("field", ["data", "len", "flags", "ep"])
def test_frames_lb_null_required_column(field):
    assert _rc(lambda iv, ov, outs: setattr(iv, field, None)) == -errno.EINVAL


@pytest.mark.parametrize("field", ["verdict", "identity"])
def test_frames_lb_null_required_output(field):
    assert _rc(lambda iv, ov, outs: outs.__setitem__(field, None)) == -errno.EINVAL


def test_frames_lb_flags_and_reserved():
    for flags in (2, 3, 0x80000000):
        assert _rc(flags=flags) == -errno.EINVAL
    assert _rc(lambda iv, ov, outs: setattr(iv, "reserved", 1)) == -errno.EINVAL
    # judged before the batch size is
    assert _rc(flags=2, n=0) == -errno.EINVAL
    assert _rc(lambda iv, ov, outs: setattr(iv, "stride", 48), n=0) == -errno.EINVAL


@pytest.mark.parametrize("stride", [0, 16, 48, 63, 72, 100])
def test_frames_lb_bad_stride(stride):
    assert _rc(lambda iv, ov, outs: setattr(iv, "stride", stride)) == -errno.EINVAL


def test_frames_lb_alignment():
    for off in (1, 4, 8):
        assert _rc(lambda iv, ov, outs: setattr(iv, "data", iv.data + off)) == -errno.EINVAL
    for field in ("len", "hash"):
        for off in (1, 2):
            assert _rc(lambda iv, ov, outs: setattr(iv, field, getattr(iv, field) + off)) == -errno.EINVAL
    for field in ("verdict", "identity"):
        assert _rc(lambda iv, ov, outs: outs.__setitem__(field, outs[field] + 2)) == -errno.EINVAL
    assert _rc(lambda iv, ov, outs: setattr(ov, "lb_ret", ov.lb_ret + 2)) == -errno.EINVAL
    for field in ("rev_nat", "slave"):
        assert _rc(lambda iv, ov, outs: setattr(ov, field, getattr(ov, field) + 1)) == -errno.EINVAL
    assert _rc(lambda iv, ov, outs: setattr(iv, "ep", iv.ep + 1)) == -errno.EINVAL
    # one-byte columns sit anywhere
    assert _rc(lambda iv, ov, outs: setattr(iv, "flags", iv.flags + 1)) == -errno.ENODEV
    assert _rc(lambda iv, ov, outs: outs.__setitem__("stage", outs["stage"] + 1)) == -errno.ENODEV


def test_struct_layout_of_the_mirror():
    assert C.sizeof(FlbIn) == 48 and FlbIn.stride.offset == 32 and FlbIn.reserved.offset == 36
    assert FlbIn.hash.offset == 40 and C.sizeof(FlbOut) == 24


def test_header_says_what_is_out_of_scope():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cgpu.h")).read()
    body = hdr[hdr.index("cgpu_classify_frames with the egress service step"):hdr.index("int cgpu_classify_frames_lb")]
    for word in ("_ctlb", "NAT on frames", "_host form", "netdev mode", "CHECKSUM_COMPLETE"):
        assert word in body, word
    for define in ("#define CGPU_FLB_REWRITE 1u", "#define CGPU_DROP_WRITE_ERROR (-141)",
                   "#define CGPU_DROP_CSUM_L4 (-154)"):
        assert define in body, define


# ---- classify_frames(lb=...) routing ------------------------------------------
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


def _stub_engine():
    e = object.__new__(Engine)
    e.L, e.h = _Recorder(), None
    return e


class _Stream:
    cuda_stream = 0


def test_classify_frames_without_lb_takes_the_old_path():
    f = {"data": _T(4 * 64, (4, 64)), "len": _T(4), "flags": _T(4), "ep": _T(4)}
    out = {k: _T(4) for k in ("verdict", "identity", "stage", "lb_ret", "rev_nat", "slave")}
    e = _stub_engine()
    e.classify_frames(f, out=dict(out), stream=_Stream())
    assert e.L.calls == ["cgpu_classify_frames"]
    e = _stub_engine()
    e.classify_frames(f, out=dict(out), stream=_Stream(), lb=None)
    assert e.L.calls == ["cgpu_classify_frames"]
    e = _stub_engine()
    e.classify_frames(f, out=dict(out), stream=_Stream(), lb={})
    assert e.L.calls == ["cgpu_classify_frames_lb"]
    e = _stub_engine()
    e.classify_frames(f, out=dict(out), stream=_Stream(), lb=dict(rewrite=False, hash=_T(4)))
    assert e.L.calls == ["cgpu_classify_frames_lb"]
    with pytest.raises(TypeError):
        _stub_engine().classify_frames(f, out=dict(out), stream=_Stream(), lb=dict(rewrite=False, sport=1))
    e.h = None
