"""The forwarding step on raw frames on the device (cgpu_forward_frames,
Engine.forward_frames, forward= on classify_frames).

The decision is compared with cgpu_forward_v4 / _v6 on the columns cut out of
the frames and with the restatement of tests/forward_cases.py; the rewritten
buffer with the per-frame restatement of tests/forward_frames_cases.py, which
the literal frames there pin (tests/test_forward_frames_cpu.py).  Everything
is integer work: every comparison is bit for bit."""
import numpy as np
import pytest

from cilium_amd import build, layouts as L, synth
from forward_cases import (ENDPOINT_F_HOST, LXC, NETDEV, World, categories, engine_cfg, ip4, ip6, key4, key6, restate)
from forward_frames_cases import (FRAMES, STAGE_NOT_CLASSIFIED, batch_frame_world, build_frames, family_batch,
                                  frame_world, fwdf_kwargs, interleave, literal_batch, literal_frame_world, load_frame_world,
                                  mixed_batch, restate_frames)

pytestmark = pytest.mark.gpu
COLS = ("action", "ret", "ifindex", "arg")
GUARD = 256  # bytes behind the last slot that no launch may touch


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a device"
    build.build()
    return torch


def _engine(**kw):
    from cilium_amd.engine import Engine
    return Engine(device=0, **kw)


@pytest.fixture(scope="module")
def batch_engine(torch_cuda):
    w = batch_frame_world()
    e = _engine(**engine_cfg(w))
    load_frame_world(e, w)
    e.commit()
    yield e
    e.close()


@pytest.fixture(scope="module")
def literal_engine(torch_cuda):
    w = literal_frame_world()
    e = _engine(**engine_cfg(w))
    load_frame_world(e, w)
    e.commit()
    yield e
    e.close()


def _i32(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda() if x is not None else None


def _u8(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.uint8)).cuda() if x is not None else None


def _frames_dev(torch, f, offset=0):
    """the frames on the device, the slots `offset` bytes into an allocation
    that goes on for GUARD bytes behind the last one; (dict, whole buffer)"""
    n, stride = f["data"].shape
    raw = torch.full((offset + n * stride + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    raw[offset:offset + n * stride] = torch.from_numpy(np.ascontiguousarray(f["data"]).reshape(-1)).cuda()
    d = {"data": raw[offset:offset + n * stride].view(n, stride), "len": _i32(torch, f["len"]),
         "flags": _u8(torch, f.get("flags"))}
    return d, raw


def _whole(f, data, offset=0):
    """what the whole allocation must hold when the slots hold `data`"""
    n, stride = f["data"].shape
    x = np.full(offset + n * stride + GUARD, 0xEE, np.uint8)
    x[offset:offset + n * stride] = data.reshape(-1)
    return x


def _np(out):
    r = {"action": out["action"].cpu().numpy(), "ret": out["ret"].cpu().numpy()}
    for k in ("ifindex", "arg"):
        r[k] = out[k].cpu().numpy().view(np.uint32)
    return r


def _run(torch, e, w, mode, f, verdict=None, stage=None, tunnel=None, rewrite=True, offset=0):
    """(output columns, the whole allocation afterwards)"""
    d, raw = _frames_dev(torch, f, offset)
    o = e.forward_frames(d, verdict=_i32(torch, verdict), stage=_u8(torch, stage), tunnel=_i32(torch, tunnel),
                         rewrite=rewrite, **fwdf_kwargs(w, mode))
    torch.cuda.synchronize()
    return _np(o), raw.cpu().numpy()


def _same(got, exp, msg):
    for k in COLS:
        np.testing.assert_array_equal(got[k], exp[k], err_msg=f"{msg}: {k}")


def _columns_call(torch, e, w, mode, v6, f, b):
    """cgpu_forward_v4 / _v6 on the columns cut out of the frames of one
    family; a NOT_CLASSIFIED frame is the egress bit cleared there"""
    data = f["data"]
    if v6:
        daddr = torch.from_numpy(np.ascontiguousarray(data[:, 38:54])).cuda()
        ttl = data[:, 21]
    else:
        daddr = _i32(torch, np.ascontiguousarray(data[:, 30:34]).view(np.uint32).reshape(-1))
        ttl = data[:, 22]
    flags = np.where(b["stage"] == STAGE_NOT_CLASSIFIED, 0, f["flags"]).astype(np.uint8)
    kw = {k: v for k, v in fwdf_kwargs(w, mode).items() if k != "host_mac"}
    o = (e.forward_v6 if v6 else e.forward_v4)(daddr, verdict=_i32(torch, b["verdict"]),
                                               tunnel=_i32(torch, b["tunnel"]), flags=_u8(torch, flags),
                                               ttl=_u8(torch, ttl), **kw)
    torch.cuda.synchronize()
    return _np(o)


def _batch(w, kind, n):
    """frames and their columns: (frames, verdict, stage, tunnel, [(is this
    family's, v6, its columns, its frames)])"""
    if kind == "mix":
        b4, b6, f, is6 = mixed_batch(w, n)
        col = {k: interleave(b4[k], b6[k], is6) for k in ("verdict", "stage", "tunnel")}
        parts = [(~is6, False, b4), (is6, True, b6)]
    else:
        v6 = kind == "v6"
        b, f = family_batch(w, v6, n)
        col = b
        parts = [(np.ones(n, bool), v6, b)]
    return f, col["verdict"], col["stage"], col["tunnel"], parts


# --------------------------------------------------------------------------
# 1. the decision, and the rewrite, on batches that hold every row
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 5000])
@pytest.mark.parametrize("kind", ["v4", "v6", "mix"])
@pytest.mark.parametrize("encap", [True, False], ids=["encap", "noencap"])
@pytest.mark.parametrize("mode", [LXC, NETDEV], ids=["lxc", "netdev"])
def test_decision_matches_the_column_calls(torch_cuda, batch_engine, mode, encap, kind, n):
    """a mix holds n frames of each family"""
    w = batch_frame_world(encap)
    f, verdict, stage, tunnel, parts = _batch(w, kind, n)
    got, _ = _run(torch_cuda, batch_engine, w, mode, f, verdict, stage, tunnel, rewrite=False)
    for m, v6, b in parts:
        sub = {"data": f["data"][m], "len": f["len"][m], "flags": f["flags"][m]}
        cols = {k: b[k] for k in ("daddr", "verdict", "tunnel", "flags", "ttl")}
        live = np.ones(m.sum(), bool) if mode == NETDEV else b["stage"] != STAGE_NOT_CLASSIFIED
        if n >= 257:  # every row of the decision lists is in the batch, on a frame that is classified
            for name, c in categories(w, mode, v6, cols).items():
                assert (c & live).any(), name
            assert mode == NETDEV or (~live).any()
        exp = restate(w, mode, v6, **{**cols, "flags": np.where(live, b["flags"], 0).astype(np.uint8)})
        mine = {k: got[k][m] for k in COLS}
        _same(mine, exp, f"restatement, v6 {v6}")
        _same(mine, _columns_call(torch_cuda, batch_engine, w, mode, v6, sub, b), f"column call, v6 {v6}")


@pytest.mark.parametrize("n", [1, 257, 5000])
@pytest.mark.parametrize("kind", ["v4", "v6", "mix"])
@pytest.mark.parametrize("encap", [True, False], ids=["encap", "noencap"])
@pytest.mark.parametrize("mode", [LXC, NETDEV], ids=["lxc", "netdev"])
def test_rewrite_matches_the_restatement(torch_cuda, batch_engine, mode, encap, kind, n):
    w = batch_frame_world(encap)
    f, verdict, stage, tunnel, _ = _batch(w, kind, n)
    exp, data = restate_frames(w, mode, f, verdict, stage, tunnel, True)
    if n >= 257:
        assert (data != f["data"]).any() and (data[:, :32] == f["data"][:, :32]).all(axis=1).any()
    got, raw = _run(torch_cuda, batch_engine, w, mode, f, verdict, stage, tunnel, rewrite=True)
    _same(got, exp, "rewrite")
    np.testing.assert_array_equal(raw, _whole(f, data))  # untouched slots, bytes past 32, the guard
    got, raw = _run(torch_cuda, batch_engine, w, mode, f, verdict, stage, tunnel, rewrite=False)
    _same(got, exp, "no rewrite")
    np.testing.assert_array_equal(raw, _whole(f, f["data"]))


# --------------------------------------------------------------------------
# 2. the literal frames through the engine
# --------------------------------------------------------------------------
@pytest.mark.parametrize("stride,offset", [(64, 0), (128, 0), (64, 16), (128, 16)])
def test_literal_frames(torch_cuda, literal_engine, stride, offset):
    groups = sorted({(r[1], r[2]) for r in FRAMES})
    assert len(groups) == 3
    for mode, encap in groups:
        rows = [r for r in FRAMES if (r[1], r[2]) == (mode, encap)]
        w = literal_frame_world(encap)
        f, verdict, stage, tunnel, want, outs = literal_batch(rows, stride)
        got, raw = _run(torch_cuda, literal_engine, w, mode, f, verdict, stage, tunnel, True, offset)
        for i, r in enumerate(rows):
            assert tuple(int(got[k][i]) for k in COLS) == tuple(x & 0xFFFFFFFF if j > 1 else x
                                                                for j, x in enumerate(outs[i])), r[0]
            at = offset + i * stride
            assert raw[at:at + stride].tobytes() == want[i].tobytes(), r[0]
        np.testing.assert_array_equal(raw, _whole(f, want, offset))


# --------------------------------------------------------------------------
# 3. table shapes
# --------------------------------------------------------------------------
def _mix32(a, b):
    """tables.h mix32 / fmix32 / fwd_hash4 / fold6, restated to craft keys of one home slot"""
    m = (1 << 64) - 1
    h = (((b << 32) | a) * 0x9E3779B97F4A7C15) & m
    h ^= h >> 29
    h = (h * 0xbf58476d1ce4e5b9) & m
    h ^= h >> 32
    return h & 0xFFFFFFFF


def _fmix32(h):
    h ^= h >> 16
    h = (h * 0x85ebca6b) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def _home4(a):
    return _mix32(a, 0x46574434)


def _home6(addr16):
    w = np.frombuffer(addr16, "<u4")
    return _fmix32(int(w[0]) ^ _fmix32(int(w[1]) ^ _fmix32(int(w[2]) ^ _fmix32(int(w[3]) ^ 0x6B43A9B5))))


def test_keys_of_one_home_slot_get_their_own_macs(torch_cuda):
    """six endpoints per family whose keys share a home slot of the 64-slot
    tables (hop bits 0..5 of that slot): each frame gets its own endpoint's
    MACs, not the home key's"""
    a4, a6 = [], []
    i = 0
    while len(a4) < 6 or len(a6) < 6:
        i += 1
        x4, x6 = ip4(f"10.7.{i // 250}.{i % 250 + 1}"), ip6(f"fd07::{i:x}")
        if len(a4) < 6 and _home4(x4) & 63 == 5:
            a4.append(x4)
        if len(a6) < 6 and _home6(x6) & 63 == 9:
            a6.append(x6)
    w = World(host_ifindex=3, encap_ifindex=4)
    for j, a in enumerate(a4):
        w.eps[key4(a)] = (10 + j, 100 + j, 0)
    for j, a in enumerate(a6):
        w.eps[key6(a)] = (20 + j, 200 + j, 0)
    w = frame_world(w)
    assert len({m for m, _ in w.macs.values()}) == 12
    e = _engine(**engine_cfg(w))
    load_frame_world(e, w)
    e.commit()
    assert e.forward_table_bytes()["endpoints4"] == 64 * 16 and e.forward_table_bytes()["endpoints6"] == 64 * 32
    n = 6
    b4 = dict(daddr=np.array(a4, np.uint32), ttl=np.full(n, 9, np.uint8), flags=np.ones(n, np.uint8))
    b6 = dict(daddr=np.frombuffer(b"".join(a6), np.uint8).reshape(n, 16), ttl=np.full(n, 9, np.uint8),
              flags=np.ones(n, np.uint8))
    for v6, b in ((False, b4), (True, b6)):
        f = build_frames(b, v6)
        exp, data = restate_frames(w, NETDEV, f)
        assert (exp["action"] == 3).all() and len({data[i, :12].tobytes() for i in range(n)}) == n
        got, raw = _run(torch_cuda, e, w, NETDEV, f)
        _same(got, exp, f"v6 {v6}")
        np.testing.assert_array_equal(raw, _whole(f, data))
    e.close()


def test_local_without_forwarding_tables_writes_zero_macs(torch_cuda):
    w = frame_world(World(host_ifindex=3, encap_ifindex=4), macs=False)
    e = _engine(**engine_cfg(w))
    for i in range(40):
        assert e.endpoint_update(L.endpoint_key(f"10.1.0.{i + 1}")) == 0
        assert e.endpoint_update(L.endpoint_key(f"fd00::{i + 1:x}")) == 0
        w.eps[key4(ip4(f"10.1.0.{i + 1}"))] = (0, 0, 0)
        w.eps[key6(ip6(f"fd00::{i + 1:x}"))] = (0, 0, 0)
    e.commit()
    assert sum(e.forward_table_bytes().values()) == 0
    n = 80
    d4 = np.array([ip4(f"10.1.0.{i + 1}") for i in range(n)], np.uint32)       # the second half: no endpoints
    d6 = np.frombuffer(b"".join(ip6(f"fd00::{i + 1:x}") for i in range(n)), np.uint8).reshape(n, 16)
    ttl = np.where(np.arange(n) % 7 == 0, 1, 64).astype(np.uint8)
    for mode in (LXC, NETDEV):
        for v6, d in ((False, d4), (True, d6)):
            f = build_frames(dict(daddr=d, ttl=ttl, flags=np.ones(n, np.uint8)), v6)
            z = np.zeros(n, np.int32)
            exp, data = restate_frames(w, mode, f, z, z.astype(np.uint8))
            loc = exp["action"] == 3
            assert loc.sum() > 30 and (data[loc, :12] == 0).all() and (f["data"][loc, :12] != 0).any()
            got, raw = _run(torch_cuda, e, w, mode, f, z, z.astype(np.uint8))
            _same(got, exp, f"mode {mode} v6 {v6}")
            np.testing.assert_array_equal(raw, _whole(f, data))
    e.close()


def test_changed_macs_are_written_after_the_commit(torch_cuda):
    w = frame_world(World(host_ifindex=3, encap_ifindex=4), macs=False)
    k4, k6 = key4(ip4("10.1.0.5")), key6(ip6("fd00::5"))
    w.eps[k4], w.eps[k6] = (7, 70, 0), (8, 80, 0)
    w.macs[k4], w.macs[k6] = (0x0000_0605_0403_0201, 0x0000_1615_1413_1211), (0x0000_2625_2423_2221, 0)
    e = _engine(**engine_cfg(w))
    load_frame_world(e, w)
    e.commit()
    f4 = build_frames(dict(daddr=np.array([ip4("10.1.0.5")], np.uint32), ttl=np.array([3], np.uint8)), False)
    f6 = build_frames(dict(daddr=np.frombuffer(ip6("fd00::5"), np.uint8).reshape(1, 16), ttl=np.array([3], np.uint8)),
                      True)
    f = {k: np.concatenate([f4[k], f6[k]]) for k in f4}

    def check(msg):
        exp, data = restate_frames(w, NETDEV, f)
        got, raw = _run(torch_cuda, e, w, NETDEV, f)
        _same(got, exp, msg)
        np.testing.assert_array_equal(raw, _whole(f, data), err_msg=msg)
        return data
    first = check("first")
    assert first[0, :12].tobytes() == bytes([1, 2, 3, 4, 5, 6, 0x11, 0x12, 0x13, 0x14, 0x15, 0x16])
    assert first[1, :12].tobytes() == bytes([0x21, 0x22, 0x23, 0x24, 0x25, 0x26, 0, 0, 0, 0, 0, 0])
    # only the MACs change: the same ifindex and lxc_id
    new = {k4: (0x0000_aaaa_aaaa_aa02, 0x0000_bbbb_bbbb_bb02), k6: (0, 0x0000_cccc_cccc_cc02)}
    for k, ip in ((k4, "10.1.0.5"), (k6, "fd00::5")):
        ifx, lid, fl = w.eps[k]
        assert e.endpoint_update(L.endpoint_key(ip), 0, L.endpoint_info(ifx, lid, fl, *new[k])) == 0
    assert check("before the commit").tobytes() == first.tobytes()
    e.commit()
    w.macs.update(new)
    second = check("after the commit")
    assert second[0, :12].tobytes() == bytes.fromhex("02aaaaaaaaaa02bbbbbbbbbb")
    assert second[1, :12].tobytes() == bytes.fromhex("00000000000002cccccccccc")
    e.close()


# --------------------------------------------------------------------------
# 4. forward= on classify_frames
# --------------------------------------------------------------------------
def test_classify_frames_forward_chain(torch_cuda):
    """classify_frames(forward=) on the frames of a small config-1 batch: the
    fwd_* of classify_v4 of the tuples followed by the forwarding step with no
    tunnel column and ttl 64 (classify_v4's own forward= takes the tunnel word
    from the ipcache, which the frames call does not return).  Behind them
    frames of every other kind, in 64-byte slots: a NOT_CLASSIFIED IPv6 frame
    and a SNAPLEN frame come back NONE / DROP and untouched."""
    torch = torch_cuda
    T = synth.make_tables(n_prefixes=2000, n_identities=100, n_endpoints=5, keys_per_ep=500)
    tn = synth.make_tuples(T, 3000)
    ft = synth.frames_from_tuples(tn, stride=64)
    rng = np.random.Generator(np.random.PCG64(0xF7A))
    g = synth.make_frames(rng, 1500, width=128, addr4=T.pfx_addr.astype(np.uint32).byteswap())
    f = {k: np.concatenate([ft[k], np.ascontiguousarray(g[k][:, :64] if k == "data" else g[k]).astype(ft[k].dtype)])
         for k in ft}
    nt, n = len(tn["flags"]), len(f["len"])
    e = _engine(ct_proto_gate=1, **T.engine_config())
    synth.load_engine(e, T)
    e.commit()
    t = synth.to_device(tn)
    cls = e.classify_v4(t)
    # a third of the allowed egress destinations as endpoints with MACs (some the host's), another third's /16 mapped
    m = ((tn["flags"] & 1) == 1) & (cls["verdict"].cpu().numpy() == 0)
    u = np.unique(tn["daddr"][m])
    assert len(u) >= 30
    w = World(host_ifindex=5, encap_ifindex=6)
    k = len(u) // 3
    for i, a in enumerate(u[:k]):
        w.eps[key4(int(a))] = (i + 1, i + 100, ENDPOINT_F_HOST if i % 9 == 0 else 0)
    for i, a in enumerate(u[k:2 * k]):
        w.tun[key4(int(a) & 0xFFFF)] = key4(ip4(f"192.168.4.{i % 250 + 1}"))
    w = frame_world(w)
    load_frame_world(e, w)
    e.commit()
    cls = e.classify_v4(t)
    fwd = fwdf_kwargs(w, LXC)
    cols = {k2: v for k2, v in fwd.items() if k2 != "host_mac"}
    ref = e.forward_v4(t["daddr"], verdict=cls["verdict"], flags=t["flags"],
                       ttl=torch.full((nt,), 64, dtype=torch.uint8, device="cuda"), **cols)
    d, raw = _frames_dev(torch, f)
    d["ep"] = torch.from_numpy(f["ep"].view(np.int16)).cuda()
    out = e.classify_frames(d, forward=dict(fwd, rewrite=True))
    torch.cuda.synchronize()
    verdict, stage = out["verdict"].cpu().numpy(), out["stage"].cpu().numpy()
    np.testing.assert_array_equal(verdict[:nt], cls["verdict"].cpu().numpy())
    got = _np({c: out["fwd_" + c] for c in COLS})
    want = _np(ref)
    for c in COLS:
        np.testing.assert_array_equal(got[c][:nt], want[c], err_msg=c)
    assert {0, 1, 3, 4, 5, 6} <= set(want["action"].tolist())
    # the whole batch: the call on its own, and the restatement
    exp, data = restate_frames(w, LXC, f, verdict, stage)
    _same(got, exp, "chain")
    np.testing.assert_array_equal(raw.cpu().numpy(), _whole(f, data))
    is6 = (f["data"][:, 12] == 0x86) & (f["data"][:, 13] == 0xDD)
    is4 = (f["data"][:, 12] == 0x08) & (f["data"][:, 13] == 0x00)
    egress = (f["flags"] & 1) == 1
    resp = (stage == STAGE_NOT_CLASSIFIED) & is6 & (f["len"] >= 54) & egress
    snap = (verdict == L.DROP_SNAPLEN) & egress & ((is4 & (f["len"] >= 34)) | (is6 & (f["len"] >= 54)))
    assert resp.any() and snap.any()
    assert (got["action"][resp] == 0).all() and (got["action"][snap] == 1).all()
    assert (got["ret"][snap] == L.DROP_SNAPLEN).all()
    assert (data[resp | snap] == f["data"][resp | snap]).all()
    d2, raw2 = _frames_dev(torch, f)
    alone = e.forward_frames(d2, verdict=out["verdict"], stage=out["stage"], **fwd)
    torch.cuda.synchronize()
    _same(_np(alone), exp, "alone")
    np.testing.assert_array_equal(raw2.cpu().numpy(), raw.cpu().numpy())
    with pytest.raises(TypeError):
        e.classify_frames(d2, forward=dict(ttl=1))
    e.close()


# --------------------------------------------------------------------------
# 5. frames that are not IP, or shorter than their IP header
# --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [LXC, NETDEV], ids=["lxc", "netdev"])
def test_short_and_non_ip_frames(torch_cuda, batch_engine, mode):
    w = batch_frame_world()
    b4, b6, f, is6 = mixed_batch(w, 64)
    n = 128
    live = (interleave(b4["stage"], b6["stage"], is6) != STAGE_NOT_CLASSIFIED) if mode == LXC else np.ones(n, bool)
    f["data"][0:n:8, 12:14] = (0x08, 0x06)            # ARP where an IPv4 header was
    f["data"][1:n:8, 12:14] = (0x88, 0x47)            # MPLS where an IPv6 header was
    f["len"][2:n:8] = 33                              # IPv4, one byte short of its header
    f["len"][3:n:8] = 53                              # IPv6, one byte short
    f["len"][4:n:8] = 34                              # IPv4, exactly its header
    f["len"][5:n:8] = 54
    f["len"][6:n:8] = 13                              # not even an ethertype's worth
    f["len"][7:n:8] = 1500                            # longer than the slot: the slot bounds it, 64 >= 54
    col = {k: interleave(b4[k], b6[k], is6) for k in ("verdict", "stage", "tunnel")}
    exp, data = restate_frames(w, mode, f, col["verdict"], col["stage"], col["tunnel"])
    out = np.arange(n) % 8
    gone = np.isin(out, (0, 1, 2, 3, 6))
    assert (exp["action"][gone] == 0).all() and (data[gone] == f["data"][gone]).all()
    assert (exp["action"][~gone & live] != 0).any() and (data[~gone] != f["data"][~gone]).any()
    got, raw = _run(torch_cuda, batch_engine, w, mode, f, col["verdict"], col["stage"], col["tunnel"])
    _same(got, exp, "short")
    for k in COLS:
        assert (got[k][gone] == 0).all(), k
    np.testing.assert_array_equal(raw, _whole(f, data))


def test_column_rules(torch_cuda, batch_engine):
    """LXC mode needs verdict, stage and flags; NETDEV mode none of them; an
    empty batch is a no-op"""
    from cilium_amd._abi import CgpuError
    torch = torch_cuda
    w = batch_frame_world()
    b, f = family_batch(w, False, 33)
    for drop in ("verdict", "stage"):
        with pytest.raises(CgpuError):
            _run(torch, batch_engine, w, LXC, f, **{k: b[k] for k in ("verdict", "stage") if k != drop})
    with pytest.raises(CgpuError):
        _run(torch, batch_engine, w, LXC, {**f, "flags": None}, b["verdict"], b["stage"])
    exp, data = restate_frames(w, NETDEV, f, tunnel=b["tunnel"])
    got, raw = _run(torch, batch_engine, w, NETDEV, {**f, "flags": None}, tunnel=b["tunnel"])
    _same(got, exp, "netdev nulls")
    np.testing.assert_array_equal(raw, _whole(f, data))
    d, raw = _frames_dev(torch, f)
    empty = {"data": d["data"][:0], "len": d["len"][:0], "flags": d["flags"][:0]}
    assert batch_engine.forward_frames(empty, mode=NETDEV)["action"].numel() == 0
