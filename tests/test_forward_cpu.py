"""The forwarding step without a device: the restatement against the literal
table (tests/forward_cases.py), and the two maps' semantics on a host-only
context (cilium_lxc with values, cilium_tunnel_map), their checkpoint, and the
call's argument checks."""
import ctypes as C
import errno
import struct

import numpy as np
import pytest

from cilium_amd import layouts as L
from cilium_amd._abi import CgpuError, FwdIn, FwdOut, FwdParams
from cilium_amd.engine import BPF_ANY, BPF_EXIST, BPF_NOEXIST, Engine, LXCMap, TunnelMap
from forward_cases import (CASES, FUNCS, LXC, NETDEV, World, batch_world, build_batch, case_columns, ip4, ip6,
                           key4, key6, literal_world, load_world, restate)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_matches_the_literal_table(case):
    name, mode, v6, encap, *_, want = case
    got = restate(literal_world(encap), mode, v6, **case_columns(case))
    assert (int(got["action"][0]), int(got["ret"][0]), int(got["ifindex"][0]), int(got["arg"][0])) == want, name


def test_table_covers_every_action_of_every_program():
    seen = {(c[1], c[2], c[9][0]) for c in CASES}
    for v6 in (False, True):
        for a in range(1, 7):  # DROP .. STACK
            assert (LXC, v6, a) in seen, (v6, a)
        assert (LXC, v6, 0) in seen
        for a in (3, 5, 6):
            assert (NETDEV, v6, a) in seen
    assert (LXC, True, 7) in seen and (NETDEV, True, 7) in seen and (NETDEV, False, 1) in seen
    assert set(FUNCS) == {(m, f) for m in (LXC, NETDEV) for f in (False, True)}


def test_null_columns_of_the_restatement():
    w = literal_world()
    d = np.array([ip4("10.1.0.5"), ip4("10.2.3.4"), ip4("10.9.9.9")], np.uint32)
    got = restate(w, NETDEV, False, d)
    assert got["action"].tolist() == [3, 5, 6] and got["arg"].tolist() == [1234, ip4("192.168.0.2"), 0]


def test_batches_hold_their_categories():
    for v6 in (False, True):
        b = build_batch(batch_world(), v6, 257)
        acts = set(restate(batch_world(), LXC, v6, **b)["action"].tolist())
        assert acts == ({0, 1, 2, 3, 4, 5, 6, 7} if v6 else {0, 1, 2, 3, 4, 5, 6})


# --------------------------------------------------------------------------
# maps on a host-only context
# --------------------------------------------------------------------------
def _ek(raw: bytes):
    return np.frombuffer(raw, L.ENDPOINT_KEY)[0]


def test_endpoint_info_layout_and_flags():
    assert L.ENDPOINT_INFO.itemsize == 48
    assert [L.ENDPOINT_INFO.fields[f][1] for f in ("ifindex", "unused", "lxc_id", "flags", "mac", "node_mac",
                                                   "pad")] == [0, 4, 6, 8, 16, 24, 32]
    e = Engine(device=-1)
    k = L.endpoint_key("10.1.0.5")
    info = L.endpoint_info(7, 1234, 0, bytes([2, 0, 0, 0, 0, 5]), bytes([2, 0, 0, 0, 0, 1]))
    assert e.endpoint_update(k, BPF_EXIST, info) == -errno.ENOENT
    assert e.endpoint_lookup_info(k)[0] == -errno.ENOENT
    assert e.endpoint_update(k, BPF_NOEXIST, info) == 0
    assert e.endpoint_update(k, BPF_NOEXIST, info) == -errno.EEXIST
    assert e.endpoint_update(k, 7, info) == -errno.EINVAL
    assert e.endpoint_lookup(k) == 0
    rc, got = e.endpoint_lookup_info(k)
    assert rc == 0 and got.tobytes() == info.tobytes()
    assert int(got["mac"]) == 0x050000000002
    # the old call is a zero-info update: over an info it zeroes it
    assert e.endpoint_update(k, BPF_EXIST) == 0
    rc, got = e.endpoint_lookup_info(k)
    assert rc == 0 and got.tobytes() == bytes(48)
    assert e.endpoint_update(k, BPF_ANY, info) == 0
    # the whole 20-byte key is compared: a pad byte makes another key
    padded = _ek(key4(ip4("10.1.0.5"), pad4=1))
    assert e.endpoint_lookup_info(padded)[0] == -errno.ENOENT
    assert e.endpoint_update(padded, BPF_ANY, L.endpoint_info(1, 1)) == 0
    assert e.endpoint_lookup_info(k)[1]["lxc_id"] == 1234
    # delete removes key and value
    assert e.endpoint_delete(k) == 0
    assert e.endpoint_lookup(k) == -errno.ENOENT and e.endpoint_lookup_info(k)[0] == -errno.ENOENT
    assert e.endpoint_delete(k) == -errno.ENOENT
    assert e.endpoint_update(k) == 0
    assert e.endpoint_lookup_info(k)[1].tobytes() == bytes(48)  # not the value of before the delete
    e.close()


def test_endpoints_max_holds_for_both_calls():
    e = Engine(device=-1, endpoints_max=3)
    for i in range(3):
        assert e.endpoint_update(L.endpoint_key(f"10.0.0.{i + 1}"), BPF_ANY, L.endpoint_info(i, i)) == 0
    assert e.endpoint_update(L.endpoint_key("10.0.0.9"), BPF_ANY, L.endpoint_info(1, 1)) == -errno.E2BIG
    assert e.endpoint_update(L.endpoint_key("10.0.0.9")) == -errno.E2BIG
    assert e.endpoint_update(L.endpoint_key("10.0.0.1"), BPF_ANY, L.endpoint_info(9, 9)) == 0  # overwrite
    e.close()


def test_lxcmap_wrapper():
    e = Engine(device=-1)
    m = LXCMap(e)
    m.WriteEndpoint(["10.1.0.5", "fd00::5"], ifindex=7, lxc_id=1234, mac=bytes(range(6)))
    m.AddHostEntry("10.1.0.1")
    for ip in ("10.1.0.5", "fd00::5"):
        rc, v = e.endpoint_lookup_info(L.endpoint_key(ip))
        assert rc == 0 and (int(v["ifindex"]), int(v["lxc_id"]), int(v["flags"])) == (7, 1234, 0)
    assert int(e.endpoint_lookup_info(L.endpoint_key("10.1.0.1"))[1]["flags"]) == L.ENDPOINT_F_HOST
    m.DeleteEntry("10.1.0.5")
    with pytest.raises(CgpuError):
        m.DeleteEntry("10.1.0.5")
    e.close()


def test_tunnel_map_semantics():
    e = Engine(device=-1)
    k, v = L.endpoint_key("10.2.0.0"), L.endpoint_key("192.168.0.2")
    assert e.tunnel_count() == 0 and e.tunnel_keys() == []
    assert e.tunnel_lookup(k)[0] == -errno.ENOENT and e.tunnel_delete(k) == -errno.ENOENT
    assert e.tunnel_update(k, v, BPF_EXIST) == -errno.ENOENT
    assert e.tunnel_update(k, v, BPF_NOEXIST) == 0
    assert e.tunnel_update(k, v, BPF_NOEXIST) == -errno.EEXIST
    assert e.tunnel_update(k, v, 5) == -errno.EINVAL
    v2 = L.endpoint_key("fd00::2")  # a value is 20 raw bytes, whatever its family
    assert e.tunnel_update(k, v2, BPF_EXIST) == 0
    assert e.tunnel_lookup(k)[1].tobytes() == v2.tobytes()
    padded = _ek(key4(ip4("10.2.0.0"), pad5=1))
    assert e.tunnel_lookup(padded)[0] == -errno.ENOENT  # whole-key compare
    assert e.tunnel_update(padded, v) == 0 and e.tunnel_count() == 2
    assert e.tunnel_lookup(k)[1].tobytes() == v2.tobytes()
    t = TunnelMap(e)
    t.SetTunnelEndpoint("fd01::", "192.168.0.3")
    assert e.tunnel_lookup(L.endpoint_key("fd01::"))[1].tobytes() == L.endpoint_key("192.168.0.3").tobytes()
    t.DeleteTunnelEndpoint("fd01::")
    with pytest.raises(CgpuError):
        t.DeleteTunnelEndpoint("fd01::")
    assert e.tunnel_delete(k) == 0 and e.tunnel_count() == 1
    e.close()


def test_tunnel_map_full_and_walk():
    e = Engine(device=-1)
    n = L.TUNNEL_ENDPOINT_MAP_SIZE
    keys = np.zeros(n, L.ENDPOINT_KEY)
    keys["ip"][:, :4] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)
    keys["ip"][:, 3] = 10
    keys["family"] = 1
    val = L.endpoint_key("192.168.0.2")
    up = e.L.cgpu_tunnel_update
    vb = val.tobytes()
    for i in range(n):
        assert up(e.h, keys[i].tobytes(), vb, BPF_NOEXIST) == 0
    assert e.tunnel_count() == n
    assert e.tunnel_update(L.endpoint_key("11.0.0.0"), val) == -errno.E2BIG
    assert e.tunnel_update(_ek(keys[5].tobytes()), L.endpoint_key("192.168.0.9"), BPF_EXIST) == 0  # overwrite fits
    walked = e.tunnel_keys()
    assert len(walked) == n and {k.tobytes() for k in walked} == {k.tobytes() for k in keys}
    assert e.tunnel_delete(_ek(keys[0].tobytes())) == 0
    assert e.tunnel_update(L.endpoint_key("11.0.0.0"), val) == 0
    e.close()


def _dump(e, ep_keys):
    """cilium_lxc has no get_next_key: ep_keys are the keys the test wrote"""
    eps = sorted((k, e.endpoint_lookup_info(_ek(k))[1].tobytes()) for k in ep_keys)
    tun = sorted((k.tobytes(), e.tunnel_lookup(k)[1].tobytes()) for k in e.tunnel_keys())
    return eps, tun


def test_checkpoint_round_trips_both_maps(tmp_path):
    w = literal_world()
    e = Engine(device=-1)
    load_world(e, w)
    want = _dump(e, list(w.eps))
    assert len(want[0]) == len(w.eps) and len(want[1]) == len(w.tun)
    assert any(v != bytes(48) for _, v in want[0]) and any(v == bytes(48) for _, v in want[0])
    p = str(tmp_path / "m.bin")
    e.mirror_save(p)
    r = Engine(device=-1)
    r.mirror_restore(p)
    assert _dump(r, list(w.eps)) == want
    # a context whose tunnel map holds something is not empty
    only = Engine(device=-1)
    assert only.tunnel_update(L.endpoint_key("10.2.0.0"), L.endpoint_key("192.168.0.2")) == 0
    with pytest.raises(CgpuError) as ex:
        only.mirror_restore(p)
    assert ex.value.errno == errno.EEXIST
    for x in (e, r, only):
        x.close()


def test_checkpoint_without_the_sections_leaves_the_maps_empty(tmp_path):
    e = Engine(device=-1)
    assert e.endpoint_update(L.endpoint_key("10.1.0.5")) == 0
    p = str(tmp_path / "plain.bin")
    e.mirror_save(p)
    buf = open(p, "rb").read()
    assert struct.unpack_from("<I", buf, 12)[0] == 12  # the file of a mirror that never used the new calls
    r = Engine(device=-1)
    r.mirror_restore(p)
    assert r.tunnel_count() == 0 and r.endpoint_lookup_info(L.endpoint_key("10.1.0.5"))[1].tobytes() == bytes(48)
    for x in (e, r):
        x.close()


# --------------------------------------------------------------------------
# the call's argument checks (no device)
# --------------------------------------------------------------------------
def _call(e, v6=False, **pk):
    p = FwdParams(pk.get("mode", 0), pk.get("flags", 1), 0xFFFF, 1, 1)
    for i, x in enumerate(pk.get("reserved", (0, 0, 0))):
        p.reserved[i] = x
    iv, ov = FwdIn(), FwdOut()
    fn = e.L.cgpu_forward_v6 if v6 else e.L.cgpu_forward_v4
    return fn(e.h, C.byref(p), C.byref(iv), 0, C.byref(ov), None)


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_forward_on_a_host_only_context(v6):
    e = Engine(device=-1)
    assert _call(e, v6) == -errno.ENODEV
    assert _call(e, v6, mode=1, flags=0) == -errno.ENODEV
    for r in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        assert _call(e, v6, reserved=r) == -errno.EINVAL
    assert _call(e, v6, mode=2) == -errno.EINVAL
    assert _call(e, v6, flags=2) == -errno.EINVAL
    fn = e.L.cgpu_forward_v6 if v6 else e.L.cgpu_forward_v4
    assert fn(e.h, None, C.byref(FwdIn()), 0, C.byref(FwdOut()), None) == -errno.EINVAL
    e.close()
