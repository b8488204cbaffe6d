"""GPU tests of the service step on raw frames (cgpu_classify_frames_lb):
the literal frames, mixed batches against the restatement
(tests/lb_frames_cases.py), the rewrite flag, an independent from-scratch
checksum check, the golden-pinned tuple path, the default hash, and the chain
into cgpu_forward_frames.  Bit-exact throughout.

Batches hold n in {1, 63, 257, 4099} frames (one lane, a partial wave, a
partial workgroup, a grid tail) in 64- and 128-byte slots.  A test runs all
four sizes and asserts over them together that no class of frame was lost:
every lb_ret value, a port rewrite, a UDP-zero frame and an option or
extension-header frame among the translated ones."""
import struct

import numpy as np
import pytest

from cilium_amd import build, layouts as L, synth
from forward_cases import LXC, World, key4, key6
from forward_frames_cases import frame_world, fwdf_kwargs, load_frame_world, restate_frames
from lb_frames_cases import (CLASSES, COLS, DTYPES, LOOPBACK, NONE, TCP, UDP, XLATED, a4, a6,
                             attach_oracle, batch_world, class_of, frame_verifies, l4_of, literal_batch, literal_rows,
                             literal_world, load_world, make_batch, restate_frames_lb)

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 257, 4099)
STRIDES = (64, 128)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a device"
    build.build()
    return torch


def _engine(w, **kw):
    from cilium_amd.engine import Engine
    e = Engine(device=0, **w.engine_config(), **kw)
    load_world(e, w)
    e.commit()
    return e


def _dev(torch, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32)).cuda()


def _run(torch, e, f, h=None, rewrite=True, **kw):
    """the call on a fresh device copy of f: (columns, data afterwards)"""
    d = synth.frames_to_device(f)
    out = e.classify_frames_lb(d, hash=_dev(torch, h), rewrite=rewrite, **kw)
    torch.cuda.synchronize()
    cols = {k: out[k].cpu().numpy().view(dt) for k, dt in zip(COLS, DTYPES)}
    return cols, d["data"].cpu().numpy()


def _same(got, want, what=""):
    for k in COLS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")


class Seen:
    """what a test's batches held, over all its sizes"""

    def __init__(self):
        self.ret, self.cls = set(), set()

    def add(self, cols, cls):
        self.ret |= set(cols["lb_ret"].tolist())
        self.cls |= {int(c) for c, r in zip(cls, cols["lb_ret"]) if r > 0}

    def check(self, stride, cut=True):
        assert {NONE, XLATED, LOOPBACK, L.DROP_NO_SERVICE} <= self.ret, self.ret
        if cut:
            assert L.DROP_CSUM_L4 in self.ret
        for name in ("v4 tcp L4", "v4 udp zero L4", "v4 tcp options", "v4 tcp fallback", "v6 udp fallback",
                     "v4 icmp L3", "v6 icmp6 L3") + (("v6 tcp L4", "v6 udp ext") if stride >= 128 else ()):
            assert class_of(name) in self.cls, f"no translated frame of class {name!r}"


# ---- 1. the literal frames ----------------------------------------------------
@pytest.mark.parametrize("stride,gate", [(64, 1), (128, 1), (64, 0)])
def test_literal_frames(torch_cuda, stride, gate):
    rows = literal_rows(stride, gate)
    f, want, exp = literal_batch(rows)
    e = _engine(literal_world(gate))
    cols, data = _run(torch_cuda, e, f)
    for i, r in enumerate(rows):
        assert tuple(int(cols[k][i]) for k in COLS) == r[6], r[0]
        assert data[i].tobytes() == want[i].tobytes(), r[0]
    e.close()


# ---- 2. mixed batches against the restatement -----------------------------------
@pytest.mark.parametrize("stride", STRIDES)
def test_batches_against_the_restatement(torch_cuda, stride):
    seen = Seen()
    for n in SIZES:
        w = attach_oracle(batch_world())
        f, h, cls = make_batch(n, stride)
        want, wdata = restate_frames_lb(w, f, h)
        e = _engine(w)
        cols, data = _run(torch_cuda, e, f, h)
        _same(cols, want, f"n={n}")
        np.testing.assert_array_equal(data, wdata)
        np.testing.assert_array_equal(e.metrics(), w.metrics())
        seen.add(cols, cls)
        e.close()
    seen.check(stride)


def test_batch_without_conntrack_and_with_l3_only(torch_cuda):
    """ct_proto_gate = 0 (ports 0, no gate) and the LB_L3-only / LB_L4-only
    builds: without LB_L4 there is no key dport and protocol 47 reaches the
    L3 frontend (DROP_NO_SERVICE behind the gate, translated without it)"""
    for gate, flags in ((0, L.LB_L3 | L.LB_L4), (1, L.LB_L3), (0, L.LB_L3), (1, L.LB_L4)):
        w = batch_world(gate)
        w.lb_flags = flags
        attach_oracle(w)
        f, h, cls = make_batch(257, 128)
        want, wdata = restate_frames_lb(w, f, h)
        e = _engine(w)
        cols, data = _run(torch_cuda, e, f, h)
        _same(cols, want, f"gate={gate} flags={flags}")
        np.testing.assert_array_equal(data, wdata)
        np.testing.assert_array_equal(e.metrics(), w.metrics())
        assert (cols["lb_ret"] > 0).sum() > 20
        e.close()


# ---- 3. rewrite off -------------------------------------------------------------
@pytest.mark.parametrize("stride", STRIDES)
def test_rewrite_off_changes_no_byte_and_no_column(torch_cuda, stride):
    seen = Seen()
    for n in SIZES:
        f, h, cls = make_batch(n, stride, seed=6)
        e1, e2 = _engine(batch_world()), _engine(batch_world())
        on, data_on = _run(torch_cuda, e1, f, h, rewrite=True)
        off, data_off = _run(torch_cuda, e2, f, h, rewrite=False)
        np.testing.assert_array_equal(data_off, f["data"])
        _same(off, on, f"n={n}")
        np.testing.assert_array_equal(e1.metrics(), e2.metrics())
        if n > 1:
            assert (data_on != f["data"]).any()
        seen.add(on, cls)
        e1.close()
        e2.close()
    seen.check(stride)


# ---- 4. the checksums from scratch ------------------------------------------------
@pytest.mark.parametrize("stride", STRIDES)
def test_translated_frames_verify_from_scratch(torch_cuda, stride):
    """valid checksums in: every translated frame's IPv4 header and L4
    checksum (pseudo header included) verify from scratch afterwards, every
    other frame is byte for byte its input.  The restatement is not asked."""
    seen = Seen()
    for n in SIZES:
        f, h, cls = make_batch(n, stride, seed=7)
        for i in range(n):
            c = CLASSES[cls[i]]   # not ARP, not the truncated frame, not the protocol without a checksum
            if c[1] is not None and not c[7] and c[2] != 47 and f["len"][i] <= stride:
                assert frame_verifies(f["data"][i], int(f["len"][i])), ("input", i)
        e = _engine(batch_world())
        cols, data = _run(torch_cuda, e, f, h)
        for i in range(n):
            if cols["lb_ret"][i] > 0:
                assert frame_verifies(data[i], int(f["len"][i])), (n, i, CLASSES[cls[i]][0])
                assert data[i].tobytes() != f["data"][i].tobytes()
            else:
                assert data[i].tobytes() == f["data"][i].tobytes(), (n, i, CLASSES[cls[i]][0])
        seen.add(cols, cls)
        e.close()
    seen.check(stride)


# ---- 5. the golden-pinned tuple path ----------------------------------------------
@pytest.mark.parametrize("stride", STRIDES)
def test_equals_the_tuple_path(torch_cuda, stride):
    """ct_proto_gate = 1, LB_L3 | LB_L4, one explicit hash column for both:
    the frames whose parse reaches policy get the verdict, identity and stage
    of classify_v4_lb / classify_v6_lb on the parsed columns and (IPv4 egress)
    the lb_ret, rev_nat and slave of lb4_select(LB_LXC); run on those frames
    alone, two fresh engines end with the same metrics and policy counters.
    The truncated-TCP class is left out: the tuple path has no frame to run
    short of."""
    torch = torch_cuda
    seen = Seen()
    for n in SIZES:
        w = batch_world()
        f, h, cls = make_batch(n, stride, seed=8, cut=False)
        ea, eb = _engine(w), _engine(w)
        p = {k: v.cpu().numpy() for k, v in ea.frames_parse(synth.frames_to_device(f)).items()}
        keep = p["status"] == 0
        assert keep.mean() >= 0.75
        fs = {k: np.ascontiguousarray(v[keep]) for k, v in f.items()}
        hs, cs = h[keep], cls[keep]
        ps = {k: v[keep] for k, v in p.items()}
        cols, _ = _run(torch, ea, fs, hs)
        seen.add(cols, cs)
        for v6 in (False, True):
            m = ps["family"] == (6 if v6 else 4)
            if not m.any():
                continue
            t = {"saddr": ps["saddr"][m] if v6 else np.ascontiguousarray(ps["saddr"][m][:, :4]).view(np.uint32)[:, 0],
                 "daddr": ps["daddr"][m] if v6 else np.ascontiguousarray(ps["daddr"][m][:, :4]).view(np.uint32)[:, 0],
                 "dport": ps["dport"][m].view(np.uint16), "proto": ps["proto"][m], "flags": ps["flags"][m],
                 "len": fs["len"][m], "ep": fs["ep"][m], "hash": hs[m], "sport": np.zeros(m.sum(), np.uint16)}
            d = synth.to_device(t)
            out = (eb.classify_v6_lb if v6 else eb.classify_v4_lb)(d)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(cols["verdict"][m], out["verdict"].cpu().numpy())
            np.testing.assert_array_equal(cols["identity"][m], out["identity"].cpu().numpy().view(np.uint32))
            np.testing.assert_array_equal(cols["stage"][m], out["stage"].cpu().numpy())
            if not v6:
                eg = (t["flags"] & 1) == 1
                sel = eb.lb4_select(d, L.LB_LXC)
                torch.cuda.synchronize()
                np.testing.assert_array_equal(cols["lb_ret"][m][eg], sel["ret"].cpu().numpy()[eg])
                np.testing.assert_array_equal(cols["rev_nat"][m][eg], sel["rev_nat"].cpu().numpy().view(np.uint16)[eg])
                np.testing.assert_array_equal(cols["slave"][m][eg], sel["slave"].cpu().numpy().view(np.uint16)[eg])
                assert not cols["lb_ret"][m][~eg].any()
        np.testing.assert_array_equal(ea.metrics(), eb.metrics())
        for ep, lab, dport, proto, egress in w.policy:
            k = L.policy_key(lab, dport, proto, egress)
            (ra, ga), (rb, gb) = ea.policy_lookup(ep, k), eb.policy_lookup(ep, k)
            assert ra == 0 and rb == 0
            assert (int(ga["packets"]), int(ga["bytes"])) == (int(gb["packets"]), int(gb["bytes"]))
        ea.close()
        eb.close()
    seen.check(stride, cut=False)


# ---- 6. the default hash -----------------------------------------------------------
def _own_hash(e, f):
    """cgpu_flow_hash / _hash6 of (saddr, daddr, sport, key dport, proto) as the
    frame carries them: sport the u16 at l4 for TCP / UDP inside min(len,
    stride), the key dport the u16 at l4 + 2 under LB_L4"""
    n, stride = f["data"].shape
    h = np.zeros(n, np.uint32)
    for i in range(n):
        fr = f["data"][i].tobytes()
        et = fr[12:14]
        v6 = et == b"\x86\xdd"
        if et not in (b"\x08\x00", b"\x86\xdd") or f["len"][i] < (54 if v6 else 34):
            continue
        l4, proto = l4_of(fr, v6)
        cap = min(int(f["len"][i]), stride)
        tu = proto in (TCP, UDP)
        if tu and l4 + 4 > cap:   # extract_l4_port ends the frame: no hash is taken
            continue
        sport = struct.unpack_from("<H", fr, l4)[0] if tu else 0
        kd = struct.unpack_from("<H", fr, l4 + 2)[0] if tu else 0
        h[i] = e.flow_hash6(fr[22:38], fr[38:54], sport, kd, proto) if v6 else \
            e.flow_hash(*struct.unpack_from("<II", fr, 26), sport, kd, proto)
    return h


@pytest.mark.parametrize("stride", STRIDES)
def test_default_hash_is_the_flow_hash_of_the_frames_fields(torch_cuda, stride):
    seen = Seen()
    for n in SIZES:
        f, _, cls = make_batch(n, stride, seed=9)
        e1, e2 = _engine(batch_world()), _engine(batch_world())
        own, data_own = _run(torch_cuda, e1, f, None)
        given, data_given = _run(torch_cuda, e2, f, _own_hash(e2, f))
        _same(own, given, f"n={n}")
        np.testing.assert_array_equal(data_own, data_given)
        seen.add(own, cls)
        if n >= 257:   # the hash picks: more than one slave of the three-backend frontend
            assert len(set(own["slave"][cls == class_of("v4 tcp L4")].tolist())) > 1
        e1.close()
        e2.close()
    seen.check(stride)


# ---- 7. the chain into forward_frames ------------------------------------------------
@pytest.mark.parametrize("stride", STRIDES)
def test_chain_into_forward_frames(torch_cuda, stride):
    """classify_frames(f, lb=..., forward=...) = forward_frames' restatement on
    the service restatement's rewritten frames, verdicts and stages: a
    translated frame is forwarded on the backend's address"""
    torch = torch_cuda
    fw = frame_world(World(eps={key4(a4("10.2.1.1")): (7, 100, 0), key4(a4("10.2.2.1")): (1, 0, L.ENDPOINT_F_HOST),
                                key6(a6("fd00:2::1:1")): (9, 101, 0), key6(a6("fd00:2::2:2")): (8, 102, 0)},
                           host_ifindex=11, encap_ifindex=22))
    seen = Seen()
    for n in SIZES:
        w = attach_oracle(batch_world())
        f, h, cls = make_batch(n, stride, seed=10)
        want, wdata = restate_frames_lb(w, f, h)
        fexp, fdata = restate_frames(fw, LXC, {"data": wdata, "len": f["len"], "flags": f["flags"]},
                                     verdict=want["verdict"], stage=want["stage"])
        e = _engine(w)
        load_frame_world(e, fw)
        e.commit()
        d = synth.frames_to_device(f)
        out = e.classify_frames(d, lb=dict(hash=_dev(torch, h)), forward=fwdf_kwargs(fw, LXC))
        torch.cuda.synchronize()
        cols = {k: out[k].cpu().numpy().view(dt) for k, dt in zip(COLS, DTYPES)}
        _same(cols, want, f"n={n}")
        np.testing.assert_array_equal(d["data"].cpu().numpy(), fdata)
        for k, dt in (("action", np.uint8), ("ret", np.int32), ("ifindex", np.uint32), ("arg", np.uint32)):
            np.testing.assert_array_equal(out["fwd_" + k].cpu().numpy().view(dt), fexp[k], err_msg=k)
        if n >= 63:   # a translated frame reaches a local endpoint: forwarded on the backend's address
            x = (cols["lb_ret"] > 0) & (fexp["action"] == 3)
            assert x.any()
        seen.add(cols, cls)
        e.close()
    seen.check(stride)
