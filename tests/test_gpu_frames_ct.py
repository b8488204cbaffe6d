"""GPU tests of the stateful path on raw frames (cgpu_frames_parse_ct,
cgpu_classify_frames_ct) against tests/frames_ct_cases.py: the literal table,
mixed batches against the restated parse and the restated chain (outputs,
metrics, policy counters, conntrack maps), the composition of the two calls
with classify_v4_ct / classify_v6_ct on a second engine, the edges of the
inner calls, and the reverse NAT chain into the frames.  Bit-exact throughout.

Batches hold n in {1, 63, 257, 4099} frames (one lane, a partial wave, a
partial workgroup, several workgroups) in 64-byte slots (IPv6 TCP ends in
CGPU_DROP_SNAPLEN there: its own class), 80- and 128-byte slots."""
import errno

import numpy as np
import pytest

from cilium_amd import build, layouts as L, synth
from lb_frames_cases import frame_verifies
from rnat_frames_cases import restate_rnat_frames
import frames_ct_cases as fc

pytestmark = pytest.mark.gpu
STRIDES = (64, 80, 128)
GUARD = 256
FILL = 0x5A
VIEW = {"sport": np.uint16, "dport": np.uint16, "l4b": np.uint16, "identity": np.uint32, "rn_sport": np.uint16,
        "rn_saddr": np.uint32, "rn_daddr": np.uint32}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a device"
    build.build()
    return torch


def _engine(world=True, **kw):
    from cilium_amd.engine import Engine
    e = Engine(device=0, **{**fc.engine_config(), **kw})
    if world:
        fc.load_world(e)
    e.commit()
    return e


@pytest.fixture(scope="module")
def engine(torch_cuda):
    e = _engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def oracle():
    return fc.make_oracle()


@pytest.fixture(scope="module")
def mixed():
    """(n, stride, families) -> the batch, built once and left unchanged"""
    cache = {}

    def get(n, stride, families=(4, 6)):
        k = (n, stride, families)
        if k not in cache:
            cache[k] = fc.make_mixed(n, stride, families=families)
        return cache[k]
    return get


def _host(out):
    """the tensors of an engine call as the arrays the restatement holds"""
    r = {}
    for k, v in out.items():
        if v is None:
            continue
        a = v.cpu().numpy()
        r[k] = a.view(VIEW[k]) if k in VIEW else a
    return r


def _same(got, exp, keys, msg=""):
    for k in keys:
        np.testing.assert_array_equal(got[k], exp[k], err_msg=f"{k} {msg}")


# ---- 1. frames_parse_ct -----------------------------------------------------------
@pytest.mark.parametrize("stride", fc.literal_strides())
def test_parse_literal_table(torch_cuda, engine, stride):
    rows, f = fc.literal_batch(stride)
    exp, ok = fc.literal_expected(rows)
    d = synth.frames_to_device(f)
    got = _host(engine.frames_parse_ct(d))
    ended = _host(engine.frames_parse(d))
    for i, r in enumerate(rows):
        assert got["status"][i] == exp["status"][i], r[0]
    fc.check_parse(got, exp, ended)


@pytest.mark.parametrize("stride", STRIDES)
def test_parse_mixed_batches(torch_cuda, engine, oracle, mixed, stride):
    seen = set()
    for n in fc.SIZES:
        f = mixed(n, stride)
        d = synth.frames_to_device(f)
        got = _host(engine.frames_parse_ct(d))
        exp = fc.restate_parse_ct(oracle, f)
        fc.check_parse(got, exp, _host(engine.frames_parse(d)))
        seen |= set(np.unique(got["status"]).tolist())
        seen |= {f"v{int(x)}" for x in np.unique(got["family"][got["status"] == 0])}
    want = {0, 1, L.DROP_INVALID, L.DROP_INVALID_SMAC, L.DROP_CT_UNKNOWN_PROTO, "v4", "v6"}
    assert want <= seen and ((L.DROP_SNAPLEN in seen) == (stride == 64))


class Guarded:
    """a device column between two guard regions"""

    def __init__(self, torch, a):
        a = np.ascontiguousarray(a)
        self.shape, self.dtype, self.nbytes = a.shape, a.dtype, a.nbytes
        self.buf = torch.full((GUARD + a.nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.buf[GUARD:GUARD + a.nbytes] = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).cuda()
        self.t = self.buf[GUARD:GUARD + a.nbytes].view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.itemsize])
        if a.ndim == 2:
            self.t = self.t.view(a.shape[0], a.shape[1])
        assert self.t.numel() == a.size and self.t.data_ptr() % 16 == 0

    def host(self):
        return self.buf[GUARD:GUARD + self.nbytes].cpu().numpy().view(self.dtype).reshape(self.shape)

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return (b[:GUARD] == FILL).all() and (b[GUARD + self.nbytes:] == FILL).all()


PARSE_DT = {"status": np.int32, "family": np.uint8, "saddr": np.uint8, "daddr": np.uint8, "sport": np.uint16,
            "dport": np.uint16, "proto": np.uint8, "l4b": np.uint16, "flags": np.uint8}


def _guarded_frames(torch, f):
    return {k: Guarded(torch, f[k]) for k in ("data", "len", "flags", "ep")}


def _inputs_kept(g, f):
    for k, x in g.items():
        assert x.guards_intact(), k
        np.testing.assert_array_equal(x.host(), np.ascontiguousarray(f[k]), err_msg=k)


@pytest.mark.parametrize("absent", [None] + [k for k in fc.PARSE_COLS if k != "status"])
def test_parse_optional_columns_guards_and_stream(torch_cuda, engine, oracle, mixed, absent):
    """every optional column NULL in turn, on a non-default stream, every
    buffer between guard regions, the inputs unchanged"""
    torch = torch_cuda
    n = 257
    f = mixed(n, 80)
    exp = fc.restate_parse_ct(oracle, f)
    gi = _guarded_frames(torch, f)
    go = {k: Guarded(torch, np.full((n, 16) if k in ("saddr", "daddr") else n, 0x7E, PARSE_DT[k]))
          for k in fc.PARSE_COLS if k != absent}
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    out = engine.frames_parse_ct({k: x.t for k, x in gi.items()},
                                 out={k: (go[k].t if k in go else None) for k in fc.PARSE_COLS}, stream=s)
    s.synchronize()
    assert absent is None or out[absent] is None
    _inputs_kept(gi, f)
    got = {k: x.host() for k, x in go.items()}
    for k, x in go.items():
        assert x.guards_intact(), k
    fc.check_parse(got, exp)


# ---- 2. classify_frames_ct against the restated chain ---------------------------------
def _counters(t):
    out = []
    for k in fc.POLICY_KEYS:
        r = t.policy_lookup(0, k)
        e = r[1] if not isinstance(r[1], (bytes, bytearray)) else np.frombuffer(r[1], L.POLICY_ENTRY)[0]
        out.append((int(e["packets"]), int(e["bytes"])))
    return out


def _maps_equal(e, o):
    for dump in ("ct4_dump", "ct6_dump"):
        ek, ev = getattr(e, dump)()
        ok, ov = getattr(o, dump)()
        np.testing.assert_array_equal(ek, ok, err_msg=dump)
        np.testing.assert_array_equal(ev, ov, err_msg=dump)


@pytest.mark.parametrize("stride", STRIDES)
def test_classify_against_the_chain(torch_cuda, mixed, stride):
    """the four sizes one after the other on one engine and one chain (the
    conntrack maps carry over, the scratch grows): every output, the metrics,
    the policy counters, the maps' sizes; no class lost over the sizes"""
    e = _engine()
    ch = fc.Chain()
    seen = set()
    for j, n in enumerate(fc.SIZES):
        f = mixed(n, stride)
        got = _host(e.classify_frames_ct(synth.frames_to_device(f), fc.NOW + j))
        torch_cuda.cuda.synchronize()
        exp = ch.run(f, fc.NOW + j)
        _same(got, exp, fc.OUT_COLS, f"n={n}")
        seen |= fc.classes(exp, f)
        np.testing.assert_array_equal(e.metrics(), ch.metrics(), err_msg=f"n={n}")
        assert _counters(e) == _counters(ch.o), n
        assert (e.ct4_count(), e.ct6_count()) == (ch.o.ct4_count(), ch.o.ct6_count())
        assert e.ct_stats()["live"] == ch.o.ct4_count() and e.ct_stats(v6=True)["live"] == ch.o.ct6_count()
    assert seen == fc.ALL_CLASSES
    _maps_equal(e, ch.o)
    e.close()


def test_two_batches_of_one_stream_leave_the_same_maps(torch_cuda, mixed):
    f = mixed(4099, 128)
    e = _engine()
    ch = fc.Chain()
    for j, sl in enumerate((slice(0, 2000), slice(2000, 4099))):
        fb = {k: np.ascontiguousarray(v[sl]) for k, v in f.items()}
        got = _host(e.classify_frames_ct(synth.frames_to_device(fb), fc.NOW + 3 * j))
        exp = ch.run(fb, fc.NOW + 3 * j)
        _same(got, exp, fc.OUT_COLS, f"batch {j}")
        # a reordered or dropped packet shows in the sequence of ct_ret
        assert (got["ct_ret"] == L.CT_ESTABLISHED).sum() > 100 and (got["ct_ret"] == L.CT_REPLY).sum() > 100
    _maps_equal(e, ch.o)
    np.testing.assert_array_equal(e.metrics(), ch.metrics())
    e.close()


def test_classify_guards_stream_and_optional_outputs(torch_cuda, mixed):
    """status / family / stage NULL, the rn group given, a non-default stream,
    every buffer between guard regions, the inputs unchanged"""
    torch = torch_cuda
    n = 257
    f = mixed(n, 80)
    exp = fc.Chain().run(f, rev_nat=True)
    e = _engine()
    gi = _guarded_frames(torch, f)
    dt = {"verdict": np.int32, "ct_ret": np.uint8, "identity": np.uint32, "rn_applied": np.uint8,
          "rn_sport": np.uint16, "rn_saddr": np.uint32, "rn_daddr": np.uint32, "rn_saddr6": np.uint8}
    go = {k: Guarded(torch, np.full((n, 16) if k == "rn_saddr6" else n, 0x7E, t)) for k, t in dt.items()}
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    out = {k: x.t for k, x in go.items()}
    out.update(status=None, family=None, stage=None)
    fr = e._frames({k: x.t for k, x in gi.items()})
    from cilium_amd._abi import FctOut, check
    import ctypes as C
    ov = FctOut(None, None, out["verdict"].data_ptr(), out["ct_ret"].data_ptr(), out["identity"].data_ptr(), None,
                out["rn_applied"].data_ptr(), out["rn_sport"].data_ptr(), out["rn_saddr"].data_ptr(),
                out["rn_daddr"].data_ptr(), out["rn_saddr6"].data_ptr())
    check(e.L.cgpu_classify_frames_ct(e.h, C.byref(fr), n, fc.NOW, C.byref(ov), C.c_void_p(s.cuda_stream)), "call")
    s.synchronize()
    _inputs_kept(gi, f)
    for k, x in go.items():
        assert x.guards_intact(), k
        np.testing.assert_array_equal(x.host(), exp[k], err_msg=k)
    e.close()


# ---- 3. composition without the restatement --------------------------------------------
@pytest.mark.parametrize("stride", (80,))
def test_classify_is_parse_then_the_conntrack_calls(torch_cuda, mixed, stride):
    torch = torch_cuda
    f = mixed(4099, stride)
    d = synth.frames_to_device(f)
    e1, e2 = _engine(), _engine()
    got = _host(e1.classify_frames_ct(d, fc.NOW))
    p = e2.frames_parse_ct(d)
    torch.cuda.synchronize()
    for v6, call in ((False, e2.classify_v4_ct), (True, e2.classify_v6_ct)):
        idx = torch.nonzero((p["status"] == 0) & (p["family"] == (6 if v6 else 4)))[:, 0]
        assert idx.numel() > 500
        t = {k: p[k][idx].contiguous() for k in ("sport", "dport", "proto", "l4b", "flags")}
        for k in ("saddr", "daddr"):
            a = p[k][idx].contiguous()
            t[k] = a if v6 else a[:, :4].contiguous().view(torch.int32)[:, 0].contiguous()
        t["len"], t["ep"] = d["len"][idx].contiguous(), d["ep"][idx].contiguous()
        r = _host(call(t, fc.NOW))
        i = idx.cpu().numpy()
        for k in ("verdict", "ct_ret", "identity", "stage"):
            np.testing.assert_array_equal(got[k][i], r[k], err_msg=f"{k} v6={v6}")
    ended = got["status"] != 0
    assert ended.sum() > 100 and (got["ct_ret"][ended] == L.CT_NONE).all() and not got["identity"][ended].any()
    np.testing.assert_array_equal(e1.ct4_dump()[0], e2.ct4_dump()[0])
    np.testing.assert_array_equal(e1.ct6_dump()[1], e2.ct6_dump()[1])
    e1.close()
    e2.close()


# ---- 4. edges of the inner calls ---------------------------------------------------------
def _one(f, i):
    return {k: np.ascontiguousarray(v[i:i + 1]) for k, v in f.items()}


def test_edges_of_the_inner_calls(torch_cuda, mixed):
    f = mixed(4099, 128)
    ref = fc.Chain().run(f)
    st, fam = ref["status"], ref["family"]
    ended = np.nonzero(st != 0)[0]
    cases = {
        "no frame reaches conntrack": {k: np.ascontiguousarray(v[ended]) for k, v in f.items()},
        "IPv4 only": mixed(257, 128, (4,)),
        "IPv6 only": mixed(257, 128, (6,)),
        "one IPv4 packet": _one(f, int(np.nonzero((st == 0) & (fam == 4))[0][0])),
        "one IPv6 packet": _one(f, int(np.nonzero((st == 0) & (fam == 6))[0][0])),
        "one ended frame": _one(f, int(ended[0])),
        "one unknown protocol": _one(f, int(np.nonzero(st == L.DROP_CT_UNKNOWN_PROTO)[0][0])),
    }
    for name, fb in cases.items():
        e = _engine()
        ch = fc.Chain()
        exp = ch.run(fb)
        got = _host(e.classify_frames_ct(synth.frames_to_device(fb), fc.NOW))
        _same(got, exp, fc.OUT_COLS, name)
        np.testing.assert_array_equal(e.metrics(), ch.metrics(), err_msg=name)
        assert (e.ct4_count(), e.ct6_count()) == (ch.o.ct4_count(), ch.o.ct6_count()), name
        if name == "no frame reaches conntrack":
            assert len(fb["len"]) > 100 and e.ct4_count() == 0 and e.ct6_count() == 0
        if name == "IPv4 only":
            assert e.ct4_count() > 0 and e.ct6_count() == 0
        if name == "IPv6 only":
            assert e.ct6_count() > 0 and e.ct4_count() == 0
        e.close()


def test_errors_on_a_device_context(torch_cuda, mixed):
    from cilium_amd._abi import CgpuError
    d = synth.frames_to_device(mixed(63, 64))
    e = _engine(world=False, ct_proto_gate=0)
    for call in (lambda: e.frames_parse_ct(d), lambda: e.classify_frames_ct(d, fc.NOW)):
        with pytest.raises(CgpuError) as x:
            call()
        assert x.value.errno == errno.EINVAL
    e.close()
    e = _engine()
    empty = {k: v[:0] for k, v in d.items()}
    assert e.classify_frames_ct(empty, fc.NOW)["verdict"].numel() == 0
    assert e.frames_parse_ct(empty)["status"].numel() == 0
    with pytest.raises(TypeError):
        e.classify_frames_ct(d, fc.NOW, rev_nat=dict(rewrit=True))
    e.close()


# ---- 5. the reverse NAT chain -----------------------------------------------------------
@pytest.mark.parametrize("n", (63, 600))
def test_reverse_nat_chain_into_the_frames(torch_cuda, n):
    torch = torch_cuda
    f, e4, e6 = fc.rnat_batch(n)
    o = fc.rnat_oracle()
    fc.rnat_install(o, e4, e6)
    exp = fc.Chain(o).run(f, rev_nat=True)
    e = _engine(world=False, **fc.rnat_engine_config())
    fc.rnat_env(e)
    e.commit()
    fc.rnat_install(e, e4, e6)
    d = synth.frames_to_device(f)
    got = _host(e.classify_frames_ct(d, fc.NOW, rev_nat=dict(rewrite=True)))
    torch.cuda.synchronize()
    _same(got, exp, fc.OUT_COLS + fc.RN_COLS)
    ap, fam = exp["rn_applied"] == 1, exp["family"]
    assert (ap & (fam == 4)).sum() >= 5 and (ap & (fam == 6)).sum() >= 5
    # the frames afterwards: the restated rewrite, one family after the other
    r4, data = restate_rnat_frames(f, exp, v6=False)
    r6, data = restate_rnat_frames(dict(f, data=data), dict(exp, rn_saddr=exp["rn_saddr6"]), v6=True)
    after = d["data"].cpu().numpy()
    np.testing.assert_array_equal(after, data)
    np.testing.assert_array_equal(got["rn_ret"], np.where(fam == 4, r4, np.where(fam == 6, r6, 0)))
    assert not got["rn_ret"].any()
    changed = (after != f["data"]).any(axis=1)
    assert changed.sum() >= 10 and not changed[~ap].any()       # ended frames and the rest keep every byte
    for i in np.nonzero(changed)[0]:
        assert frame_verifies(after[i], int(f["len"][i])), i
    # rewrite=False: the columns and rn_ret alone
    e2 = _engine(world=False, **fc.rnat_engine_config())
    fc.rnat_env(e2)
    e2.commit()
    fc.rnat_install(e2, e4, e6)
    d2 = synth.frames_to_device(f)
    got2 = _host(e2.classify_frames_ct(d2, fc.NOW, rev_nat=dict(rewrite=False)))
    _same(got2, exp, fc.OUT_COLS + fc.RN_COLS)
    np.testing.assert_array_equal(d2["data"].cpu().numpy(), f["data"])
    e.close()
    e2.close()
