"""GPU tests of reverse NAT on raw frames (cgpu_rnat_frames_v4 / _v6): the
literal frames, mixed batches against the restatement
(tests/rnat_frames_cases.py) with guard regions round every buffer, the
rewrite flag, the optional ret column, frames left alone, mixed-family
batches, the chain behind classify_v4_ct / classify_v6_ct(rev_nat=True) with a
from-scratch checksum check, and a non-default stream.  Bit-exact throughout.

Batches hold n in {1, 63, 257, 4099} frames (one lane, a partial wave, a
partial workgroup, more than one workgroup) in 64- and 128-byte slots for
IPv4 and 64-, 80- and 128-byte slots for IPv6 (64 cuts the IPv6 TCP checksum
off: CGPU_DROP_SNAPLEN).  A test runs all four sizes and asserts over them
together that no class of frame was lost."""
import struct

import numpy as np
import pytest

from cilium_amd import build, layouts as L, synth
from lb_frames_cases import ICMP, ICMP6, TCP, UDP, build_frame, frame_verifies, l4_of, slot
from revnat_cases import (ROUTER6, _a6, _env4, _env6, _rmap4, _rmap6, build_v4_hits, build_v6, restate_v4,
                          restate_v6)
from rnat_frames_cases import (REWRITTEN4, REWRITTEN6, class_of, classes, literal_batch, literal_groups, make_batch,
                               restate_rnat_frames)

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 257, 4099)
SHAPES = [(False, 64), (False, 128), (True, 64), (True, 80), (True, 128)]   # (IPv6, stride)
GUARD = 256
FILL = 0x5A


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a device"
    build.build()
    return torch


@pytest.fixture(scope="module")
def engine(torch_cuda):
    """the step reads no table: one engine without a committed snapshot serves"""
    from cilium_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batches():
    """(IPv6, stride, n) -> (frames, rn columns, class index, expected ret,
    expected data): built and restated once, shared and left unchanged"""
    cache = {}

    def get(v6, stride, n):
        k = (v6, stride, n)
        if k not in cache:
            f, rn, cls = make_batch(n, stride, v6)
            ret, data = restate_rnat_frames(f, rn, v6)
            for a in list(f.values()) + list(rn.values()) + [cls, ret, data]:
                a.setflags(write=False)
            cache[k] = (f, rn, cls, ret, data)
        return cache[k]
    return get


class Guarded:
    """a device column between two guard regions"""

    def __init__(self, torch, a):
        a = np.ascontiguousarray(a)
        self.shape, self.dtype, self.nbytes = a.shape, a.dtype, a.nbytes
        self.buf = torch.full((GUARD + a.nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.buf[GUARD:GUARD + a.nbytes] = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).cuda()
        # the column itself, in the torch type of its width (numel is the element count)
        self.t = self.buf[GUARD:GUARD + a.nbytes].view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.itemsize])
        if a.ndim == 2:
            self.t = self.t.view(a.shape[0], a.shape[1])
        assert self.t.numel() == a.size and self.t.data_ptr() % 16 == 0

    def host(self):
        return self.buf[GUARD:GUARD + self.nbytes].cpu().numpy().view(self.dtype).reshape(self.shape)

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return (b[:GUARD] == FILL).all() and (b[GUARD + self.nbytes:] == FILL).all()


def _run(torch, e, f, rn, v6, rewrite=True, want_ret=True, stream=None):
    """the call on fresh guarded device copies: (ret or None, data afterwards);
    the guards and the input columns are checked here"""
    n = len(f["len"])
    g = {"data": Guarded(torch, f["data"]), "len": Guarded(torch, f["len"].astype(np.uint32)),
         "ret": Guarded(torch, np.full(n, 0x7E7E7E7E, np.int32))}
    for k in ("rn_applied", "rn_saddr", "rn_sport") + (() if v6 else ("rn_daddr",)):
        g[k] = Guarded(torch, rn[k])
    d = {"data": g["data"].t, "len": g["len"].t}
    out = e.rnat_frames(d, {k: g[k].t for k in g if k.startswith("rn_")}, v6=v6, rewrite=rewrite,
                        out={"ret": g["ret"].t if want_ret else None}, stream=stream)
    torch.cuda.synchronize()
    assert set(out) == {"ret"}
    for k, x in g.items():
        assert x.guards_intact(), k
        if k not in ("data", "ret"):
            np.testing.assert_array_equal(x.host(), np.ascontiguousarray(rn[k] if k != "len" else f["len"]), err_msg=k)
    ret = g["ret"].host()
    if not want_ret:
        assert (ret == 0x7E7E7E7E).all()
    return (ret if want_ret else None), g["data"].host()


# ---- 1. the literal frames ----------------------------------------------------
@pytest.mark.parametrize("v6,stride", literal_groups())
def test_literal_frames(torch_cuda, engine, v6, stride):
    f, rn, want, ret = literal_batch(v6, stride)
    got, data = _run(torch_cuda, engine, f, rn, v6)
    assert got.tolist() == ret.tolist()
    for i in range(len(ret)):
        assert data[i].tobytes() == want[i].tobytes(), i


# ---- 2. mixed batches against the restatement -----------------------------------
def _check_classes(v6, stride, seen):
    """every class occurred, and every rewriting class rewrote a frame, over
    the sizes together (a 64- / 80-byte slot cuts some IPv6 classes short)"""
    cut = {"tcp port", "tcp port 0", "udp ext", "tcp ext"} if v6 and stride == 64 else set()
    assert seen["cls"] == set(range(len(classes(v6))))
    for name in (REWRITTEN6 if v6 else REWRITTEN4):
        assert (class_of(v6, name) in seen["rewritten"]) != (name in cut), name
    assert {0, L.DROP_CSUM_L4} <= seen["ret"]
    assert (L.DROP_SNAPLEN in seen["ret"]) == (v6 and stride == 64)


def _note(seen, cls, ret, before, after):
    seen["cls"] |= set(cls.tolist())
    seen["ret"] |= set(ret.tolist())
    seen["rewritten"] |= {int(c) for c, a, b in zip(cls, before, after) if a.tobytes() != b.tobytes()}


@pytest.mark.parametrize("v6,stride", SHAPES)
def test_batches_against_the_restatement(torch_cuda, engine, batches, v6, stride):
    seen = {"cls": set(), "ret": set(), "rewritten": set()}
    for n in SIZES:
        f, rn, cls, ret, data = batches(v6, stride, n)
        got, gdata = _run(torch_cuda, engine, f, rn, v6)
        np.testing.assert_array_equal(got, ret, err_msg=f"n={n}")
        np.testing.assert_array_equal(gdata, data, err_msg=f"n={n}")   # every slot byte, behind len included
        _note(seen, cls, got, f["data"], gdata)
    _check_classes(v6, stride, seen)


# ---- 3. rewrite off, and no ret column -------------------------------------------
@pytest.mark.parametrize("v6,stride", SHAPES)
def test_rewrite_off_changes_no_byte_and_gives_the_same_ret(torch_cuda, engine, batches, v6, stride):
    for n in SIZES:
        f, rn, cls, ret, data = batches(v6, stride, n)
        off, data_off = _run(torch_cuda, engine, f, rn, v6, rewrite=False)
        np.testing.assert_array_equal(data_off, f["data"])
        np.testing.assert_array_equal(off, ret)
        none, data_none = _run(torch_cuda, engine, f, rn, v6, rewrite=False, want_ret=False)
        np.testing.assert_array_equal(data_none, f["data"])


@pytest.mark.parametrize("v6,stride", SHAPES)
def test_without_a_ret_column_the_bytes_are_the_same(torch_cuda, engine, batches, v6, stride):
    for n in SIZES:
        f, rn, cls, ret, data = batches(v6, stride, n)
        none, gdata = _run(torch_cuda, engine, f, rn, v6, want_ret=False)
        assert none is None
        np.testing.assert_array_equal(gdata, data)


# ---- 4. frames that are left alone ------------------------------------------------
@pytest.mark.parametrize("v6,stride", [(False, 64), (True, 80)])
def test_unapplied_and_foreign_frames_keep_every_byte(torch_cuda, engine, batches, v6, stride):
    """applied 0 everywhere: nothing changes whatever the other columns hold;
    and in the batch as it is, the frames of the other family, ARP, short
    frames and ungated protocols keep every byte with applied 1"""
    for n in SIZES:
        f, rn, cls, ret, data = batches(v6, stride, n)
        rn0 = dict(rn, rn_applied=np.zeros(n, np.uint8))
        got, gdata = _run(torch_cuda, engine, f, rn0, v6)
        assert not got.any()
        np.testing.assert_array_equal(gdata, f["data"])
        got, gdata = _run(torch_cuda, engine, f, rn, v6)
        for name in ("other family", "arp", "short", "miss", "index 0") + (("frag", "icmp in ipv6") if v6 else ("gre",)):
            m = cls == class_of(v6, name)
            assert not got[m].any(), name
            np.testing.assert_array_equal(gdata[m], f["data"][m], err_msg=name)


def test_mixed_family_batch_through_both_calls(torch_cuda, engine, batches):
    """IPv4 and IPv6 frames interleaved in one buffer of 128-byte slots, every
    one applied: the IPv4 call rewrites the IPv4 frames alone, the IPv6 call
    on the result the IPv6 frames alone, and the end is each family's own
    restatement"""
    torch = torch_cuda
    for n in (63, 257):
        f4, rn4, _, _, d4 = batches(False, 128, n)
        f6, rn6, _, _, d6 = batches(True, 128, n)
        data = np.empty((2 * n, 128), np.uint8)
        data[0::2], data[1::2] = f4["data"], f6["data"]
        ln = np.empty(2 * n, np.uint32)
        ln[0::2], ln[1::2] = f4["len"], f6["len"]
        f = {"data": data, "len": ln}

        def spread(a, other, at):
            x = np.zeros((2 * n,) + a.shape[1:], a.dtype)
            x[at::2] = a
            x[1 - at::2] = other
            return x
        # the other family's slots carry applied 1 and columns that would change them
        m4 = {"rn_applied": spread(rn4["rn_applied"], 1, 0), "rn_saddr": spread(rn4["rn_saddr"], 0x0a0a0a0a, 0),
              "rn_daddr": spread(rn4["rn_daddr"], 0x0b0b0b0b, 0), "rn_sport": spread(rn4["rn_sport"], 0x5000, 0)}
        m6 = {"rn_applied": spread(rn6["rn_applied"], 1, 1), "rn_saddr": spread(rn6["rn_saddr"], 0xfd, 1),
              "rn_sport": spread(rn6["rn_sport"], 0x5000, 1)}
        is4 = (data[:, 12] == 0x08) & (data[:, 13] == 0x00)
        is6 = (data[:, 12] == 0x86) & (data[:, 13] == 0xDD)
        assert is4[0::2].sum() > n // 2 and is6[1::2].sum() > n // 2 and is4[1::2].any() and is6[0::2].any()
        want_r4, want4 = restate_rnat_frames(f, m4, False)
        r4, after4 = _run(torch, engine, f, m4, False)
        np.testing.assert_array_equal(r4, want_r4)
        np.testing.assert_array_equal(after4, want4)
        np.testing.assert_array_equal(after4[0::2], d4)            # the IPv4 batch's own slots: as on their own
        np.testing.assert_array_equal(after4[~is4], data[~is4])    # nothing but IPv4 frames was touched
        assert not r4[~is4].any() and (after4[is4] != data[is4]).any()
        f2 = {"data": after4, "len": ln}
        want_r6, want6 = restate_rnat_frames(f2, m6, True)
        r6, after6 = _run(torch, engine, f2, m6, True)
        np.testing.assert_array_equal(r6, want_r6)
        np.testing.assert_array_equal(after6, want6)
        np.testing.assert_array_equal(after6[~is6], after4[~is6])
        assert not r6[~is6].any() and (after6[is6] != after4[is6]).any()
        own6 = is6[1::2]                                            # the IPv6 batch's own IPv6 frames: as on their own
        np.testing.assert_array_equal(after6[1::2][own6], d6[own6])


# ---- 5. behind the conntrack calls --------------------------------------------------
def _frames_of(t, v6, stride=128):
    """the tuples of a conntrack stream as frames with valid checksums: TCP /
    UDP with the tuple's ports, ICMP errors by their type (the l4b column)"""
    n = len(t["proto"])
    data = np.zeros((n, stride), np.uint8)
    ln = np.zeros(n, np.uint32)
    for i in range(n):
        proto = int(t["proto"][i])
        sa = t["saddr"][i].tobytes() if v6 else struct.pack("<I", int(t["saddr"][i]))
        da = t["daddr"][i].tobytes() if v6 else struct.pack("<I", int(t["daddr"][i]))
        fr = build_frame(v6, proto, sa, da, L.htons(int(t["sport"][i])), L.htons(int(t["dport"][i])),
                         bytes([i & 255, (i >> 8) & 255] * (1 + i % 5)),
                         icmp_type=int(t["l4b"][i]) & 255 if proto in (ICMP, ICMP6) else 0)
        ln[i] = len(fr)
        data[i] = np.frombuffer(slot(fr, stride), np.uint8)
    return {"data": data, "len": ln, "flags": t["flags"].astype(np.uint8), "ep": np.zeros(n, np.uint16)}


def _chain(torch, e, t, v6, classify):
    f = _frames_of(t, v6)
    for i in range(len(f["len"])):
        assert frame_verifies(f["data"][i], int(f["len"][i])), ("input", i)
    out = classify(synth.to_device(t), 1000, rev_nat=True)
    d = synth.frames_to_device(f)
    r = e.rnat_frames(d, out, v6=v6)          # the out of the classify call goes in as it is
    p = e.frames_parse(d)
    torch.cuda.synchronize()
    data = d["data"].cpu().numpy()
    applied = out["rn_applied"].cpu().numpy()
    assert not r["ret"].cpu().numpy().any()
    assert (p["family"].cpu().numpy() == (6 if v6 else 4)).all()
    psa, pda = p["saddr"].cpu().numpy(), p["daddr"].cpu().numpy()
    sport = out["rn_sport"].cpu().numpy().view(np.uint16)
    if v6:
        np.testing.assert_array_equal(psa, out["rn_saddr"].cpu().numpy())
        np.testing.assert_array_equal(pda, t["daddr"])
    else:
        np.testing.assert_array_equal(np.ascontiguousarray(psa[:, :4]).view(np.uint32)[:, 0],
                                      out["rn_saddr"].cpu().numpy().view(np.uint32))
        np.testing.assert_array_equal(np.ascontiguousarray(pda[:, :4]).view(np.uint32)[:, 0],
                                      out["rn_daddr"].cpu().numpy().view(np.uint32))
    for i in range(len(applied)):
        l4, proto = l4_of(data[i].tobytes(), v6)
        if proto in (TCP, UDP):
            assert struct.unpack_from("<H", data[i].tobytes(), l4)[0] == sport[i], i
        assert frame_verifies(data[i], int(f["len"][i])), ("output", i)
        assert (data[i].tobytes() != f["data"][i].tobytes()) == bool(applied[i]), i
    return applied


@pytest.mark.parametrize("n", [1, 257, 4099])
def test_behind_classify_v4_ct(torch_cuda, n):
    from cilium_amd.engine import Engine
    t, ents, cr, idx, loop, case = build_v4_hits(n)
    exp = restate_v4(t, cr, idx, loop, _rmap4())
    e = Engine(device=0, ct_max=1 << 14)
    _env4(e)
    e.commit()
    for k, v in ents:
        assert e.ct4_update(k, v) == 0
    applied = _chain(torch_cuda, e, t, False, e.classify_v4_ct)
    np.testing.assert_array_equal(applied, exp[3])
    if n >= 257:   # replies with a port change, with loopback, ICMP errors, and packets left alone
        assert (applied == 1).any() and (applied == 0).any()
        assert ((exp[1] != t["daddr"]) & (applied == 1)).any()
        assert ((exp[2] != t["sport"]) & (applied == 1)).any()
        assert ((t["proto"] == ICMP) & (applied == 1)).any()
    e.close()


@pytest.mark.parametrize("n_eg,n_in", [(1, 0), (200, 19), (3800, 100)], ids=["1", "257", "4100"])
def test_behind_classify_v6_ct(torch_cuda, n_eg, n_in):
    from cilium_amd.engine import Engine
    t, ents, cr, idx = build_v6(n_eg, n_in)
    exp = restate_v6(t, cr, idx, _rmap6())
    e = Engine(device=0, ct_max=1 << 14, ct6_max=1 << 14, ipv6_router_ip=ROUTER6)
    _env6(e)
    for ix, (addr, port) in _rmap6().items():
        v = np.zeros((), L.LB6_REVERSE_NAT)
        v["address"][:], v["port"] = _a6(addr), port
        assert e.revnat6_update(ix, v) == 0
    e.commit()
    for k, v in ents:
        assert e.ct6_update(k, v) == 0
    applied = _chain(torch_cuda, e, t, True, e.classify_v6_ct)
    np.testing.assert_array_equal(applied, exp[2])
    if n_in:
        assert (applied == 1).any() and (applied == 0).any()
        assert ((t["proto"] == ICMP6) & (applied == 1)).any()
        assert ((exp[1] != t["sport"]) & (applied == 1)).any()
    e.close()


# ---- 6. a stream of the caller's ----------------------------------------------------
@pytest.mark.parametrize("v6,stride", [(False, 64), (True, 80)])
def test_on_a_non_default_stream(torch_cuda, engine, batches, v6, stride):
    torch = torch_cuda
    f, rn, cls, ret, data = batches(v6, stride, 4099)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got, gdata = _run(torch, engine, f, rn, v6, stream=s)
    null, ndata = _run(torch, engine, f, rn, v6)
    np.testing.assert_array_equal(got, null)
    np.testing.assert_array_equal(gdata, ndata)
    np.testing.assert_array_equal(gdata, data)
