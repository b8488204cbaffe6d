"""Checkpoint / resume of the host mirror: cgpu_mirror_save and
cgpu_mirror_restore on host-only contexts (device = -1).  A context holding
every map kind (ipcache incl. IPv6 and tombstones, 3 endpoints' policy maps,
the four prefilter CIDR maps and the PreFilter revision, cilium_lxc, lb4 /
lb6 services, per-endpoint lxc info, both conntrack maps) is saved and
restored into a fresh context; every dump, lookup and count is identical.
Corrupted, truncated and foreign files are -EINVAL, a non-empty target is
-EEXIST, and nothing is applied from a file that fails validation."""
import errno
import os

import numpy as np
import pytest

from cilium_amd import layouts as L, synth
from cilium_amd._abi import CgpuError
from cilium_amd.engine import (CIDR_V4_DYN, CIDR_V4_FIX, CIDR_V6_DYN, CIDR_V6_FIX, Engine,
                               PreFilter)


def _populated():
    e = Engine(device=-1, ct_max=4096, lb_max_entries=1 << 16)
    T = synth.make_tables(n_prefixes=500, n_identities=50, n_endpoints=3, keys_per_ep=300)
    synth.load_engine(e, T)
    assert e.ipcache_update(L.ipcache_key("f00d::/64"), L.remote_info(777)) == 0
    assert e.ipcache_update(L.ipcache_key("f00d::1/128"), L.remote_info(0)) == 0  # tombstone
    # counters supplied with an entry travel with it
    assert e.policy_update(1, L.policy_key(4242, 80, 6, 1), L.policy_entry(8080, 12, 3456)) == 0
    pf = PreFilter(e)
    pf.Insert(0, ["10.1.0.0/16", "10.2.3.4/32", "2001:db8::/48", "2001:db8::5/128"])
    assert pf.Revision() == 2
    for ip in ("10.200.0.1", "10.200.0.2", "f00d::10"):
        assert e.endpoint_update(L.endpoint_key(ip)) == 0
    S = synth.make_services(T, 40)
    assert e.lb4_update_batch(S.keys, S.vals) == 0
    k6 = np.zeros((), L.LB6_KEY)
    k6["address"][:] = np.frombuffer(bytes.fromhex("20010db8000000000000000000000099"), np.uint8)
    k6["dport"] = L.htons(443)
    v6 = np.zeros((), L.LB6_SERVICE)
    v6["count"] = 1
    assert e.lb6_update(k6, v6) == 0
    k6["slave"] = 1
    v6["count"] = 0
    v6["target"][:] = np.frombuffer(bytes.fromhex("20010db8000000000000000000000001"), np.uint8)
    assert e.lb6_update(k6, v6) == 0
    synth.load_lxc(e, [5000, 5007, 5014])
    rng = np.random.default_rng(3)
    for i in range(50):
        k = np.zeros((), L.CT4_TUPLE)
        k["daddr"], k["saddr"], k["dport"], k["nexthdr"] = 0x0A000001 + i, 0x0B000001, 80, 6
        v = np.zeros((), L.CT_ENTRY)
        v["lifetime"], v["rx_packets"], v["src_sec_id"] = 100 + i, i, 5000
        assert e.ct4_update(k, v) == 0
        k6t = np.zeros((), L.CT6_TUPLE)
        k6t["daddr"][:] = rng.integers(0, 256, 16, dtype=np.uint8)
        k6t["saddr"][:] = rng.integers(0, 256, 16, dtype=np.uint8)
        k6t["nexthdr"], k6t["flags"] = 58, 2
        v["rev_nat_index"] = i
        assert e.ct6_update(k6t, v) == 0
    return e


def _state(e):
    st = {"ipc": sorted(bytes(k) for k in e.ipcache_keys())}
    st["ipc_vals"] = sorted(bytes(e.ipcache_lookup(np.frombuffer(k, L.IPCACHE_KEY)[0])[1])
                            for k in st["ipc"])
    for ep in range(4):
        k, v = e.policy_dump(ep)
        st[f"pol{ep}"] = (k.tobytes(), v.tobytes())
    for w in (CIDR_V4_DYN, CIDR_V4_FIX, CIDR_V6_DYN, CIDR_V6_FIX):
        st[f"cidr{w}"] = sorted(bytes(k) for k in e.cidr_keys(w))
    st["ep"] = [e.endpoint_lookup(L.endpoint_key(ip)) for ip in ("10.200.0.1", "10.200.0.2", "f00d::10",
                                                                   "10.200.0.3")]
    st["lb4"] = [(bytes(k), bytes(e.lb4_lookup(k)[1])) for k in e.lb4_keys()]
    st["lb6"] = [(bytes(k), bytes(e.lb6_lookup(k)[1])) for k in e.lb6_keys()]
    st["lxc"] = [None if v is None else v.tobytes() for v in (e.lxc_lookup(ep) for ep in range(3))]
    st["rev"] = PreFilter(e).Revision()
    st["ct4"] = [a.tobytes() for a in e.ct4_dump()]
    st["ct6"] = [a.tobytes() for a in e.ct6_dump()]
    st["rn4"] = [(i, bytes(e.revnat4_lookup(i)[1])) for i in e.revnat4_keys()]
    st["rn6"] = [(i, bytes(e.revnat6_lookup(i)[1])) for i in e.revnat6_keys()]
    st["epi"] = []
    for ip in ("10.200.0.1", "10.200.0.2", "f00d::10", "10.200.0.3"):
        rc, v = e.endpoint_lookup_info(L.endpoint_key(ip))
        st["epi"].append((rc, None if v is None else v.tobytes()))
    st["tun"] = [(bytes(k), bytes(e.tunnel_lookup(k)[1])) for k in e.tunnel_keys()]
    return st


FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mirror_v1_all_sections.bin")
SMALL = {"ct_max": 64, "ct6_max": 64}
_A6 = bytes.fromhex("20010db8000000000000000000000099")


def _all_sections():
    """Two or three records in every one of the file's 14 section kinds,
    written by literal calls only: what tests/golden/mirror_v1_all_sections.bin
    was saved from."""
    e = Engine(device=-1, **SMALL)
    for cidr, ident, tun in (("10.1.0.0/16", 300, 0), ("f00d::/64", 777, 0x0100000A), ("f00d::1/128", 0, 0)):
        assert e.ipcache_update(L.ipcache_key(cidr), L.remote_info(ident, tun)) == 0
    assert e.policy_update(0, L.policy_key(300, 80, 6, 0), L.policy_entry(4000)) == 0
    assert e.policy_update(1, L.policy_key(4242, 80, 6, 1), L.policy_entry(8080, 12, 3456)) == 0
    assert e.policy_update(1, L.policy_key(777, 0, 0, 0), L.policy_entry()) == 0
    PreFilter(e).Insert(0, ["10.1.0.0/16", "10.2.3.4/32", "2001:db8::/48", "2001:db8::5/128"])
    PreFilter(e).Insert(2, ["10.9.0.0/16"])
    assert e.endpoint_update(L.endpoint_key("10.200.0.1"),
                             info=L.endpoint_info(7, 3, 0, bytes.fromhex("0a1b2c3d4e5f"),
                                                  bytes.fromhex("020000000001"))) == 0
    assert e.endpoint_update(L.endpoint_key("10.200.0.2")) == 0  # the all-zero value: no MIR_EPI record
    assert e.endpoint_update(L.endpoint_key("f00d::10"),
                             info=L.endpoint_info(9, 4, L.ENDPOINT_F_HOST, bytes.fromhex("0a1b2c3d4e60"))) == 0
    assert e.lb4_update(L.lb4_key("10.96.0.10", 80, 0), L.lb4_service(0, 0, 1, rev_nat=3)) == 0
    assert e.lb4_update(L.lb4_key("10.96.0.10", 80, 1), L.lb4_service("10.1.0.1", 8080, 0, rev_nat=3)) == 0
    for slave, count, target in ((0, 2, bytes(16)), (1, 0, _A6[:15] + b"\x01"), (2, 0, _A6[:15] + b"\x02")):
        k6, v6 = np.zeros((), L.LB6_KEY), np.zeros((), L.LB6_SERVICE)
        k6["address"][:] = np.frombuffer(_A6, np.uint8)
        k6["dport"], k6["slave"] = L.htons(443), slave
        v6["count"], v6["rev_nat_index"] = count, L.htons(5)
        v6["target"][:] = np.frombuffer(target, np.uint8)
        assert e.lb6_update(k6, v6) == 0
    assert e.lxc_update(0, L.lxc_info(bytes.fromhex("0a1b2c3d4e5f"), 0x0100C80A, _A6, 7, 5000)) == 0
    assert e.lxc_update(2, L.lxc_info(bytes(6), 0, bytes(16), 0, 5014)) == 0
    v = np.zeros((), L.CT_ENTRY)
    for i in range(3):
        k = np.zeros((), L.CT4_TUPLE)
        k["daddr"], k["saddr"], k["dport"], k["sport"], k["nexthdr"] = 0x0A000001 + i, 0x0B000001, 80, 1000 + i, 6
        v["lifetime"], v["rx_packets"], v["src_sec_id"], v["rev_nat_index"] = 100 + i, i, 5000, i
        assert e.ct4_update(k, v) == 0
    for i in range(2):
        k = np.zeros((), L.CT6_TUPLE)
        k["daddr"][:] = np.frombuffer(_A6[:15] + bytes([i]), np.uint8)
        k["saddr"][:] = np.frombuffer(_A6, np.uint8)
        k["nexthdr"], k["flags"] = 58, 2
        v["tx_bytes"] = 64 * i
        assert e.ct6_update(k, v) == 0
    assert e.revnat4_update(L.revnat_index(3), L.lb4_reverse_nat("10.96.0.10", 80)) == 0
    assert e.revnat4_update(L.revnat_index(4), L.lb4_reverse_nat("10.96.0.11", 53)) == 0
    assert e.revnat6_update(L.revnat_index(5), L.lb6_reverse_nat(_A6, 443)) == 0
    assert e.revnat6_update(L.revnat_index(600), L.lb6_reverse_nat("fd00::1", 0)) == 0
    for ip, node in (("10.7.0.0", "192.168.0.7"), ("10.8.0.0", "192.168.0.8"), ("f00d:8::", "fd00::8")):
        assert e.tunnel_update(L.endpoint_key(ip), L.endpoint_key(node)) == 0
    return e


def test_mirror_all_sections_match_the_fixture(tmp_path):
    """The file format, byte for byte: a context with records in all 14
    section kinds saves exactly tests/golden/mirror_v1_all_sections.bin, the
    fixture restores into an equal context, and that one saves it again."""
    want = open(FIXTURE, "rb").read()
    e = _all_sections()
    path = str(tmp_path / "a.bin")
    e.mirror_save(path)
    assert open(path, "rb").read() == want
    # every section kind is in it, in the format's order, none of them empty
    tags, off = [], 16
    while off < len(want) - 8:
        tag, rec, n = np.frombuffer(want, "<u4", 2, off).tolist() + [int(np.frombuffer(want, "<u8", 1, off + 8)[0])]
        assert n >= 1
        tags.append(tag)
        off += 16 + rec * n
    assert tags == list(range(1, 15)) and int(np.frombuffer(want, "<u4", 1, 12)[0]) == 14
    f = Engine(device=-1, **SMALL)
    f.mirror_restore(FIXTURE)
    a, b = _state(e), _state(f)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], k
    assert a["rn4"] and a["rn6"] and a["tun"] and a["epi"][0][1] != a["epi"][1][1]
    path2 = str(tmp_path / "b.bin")
    f.mirror_save(path2)
    assert open(path2, "rb").read() == want
    e.close()
    f.close()


def _fnv1a(raw: bytes) -> int:
    h = 1469598103934665603
    for b in raw:
        h = ((h ^ b) * 0x100000001B3) & (2 ** 64 - 1)
    return h


def test_mirror_restore_rolls_back_from_the_last_section(tmp_path):
    """The failing record is the file's very last one (a tunnel key written
    twice): every section before it, the reverse-NAT maps, the endpoint
    values and the tunnel records already applied included, is rolled back
    to an empty context, which then takes the intact fixture."""
    raw = bytearray(open(FIXTURE, "rb").read())
    body = len(raw) - 8
    raw[body - 40:body - 20] = raw[body - 120:body - 100]  # last tunnel key := first tunnel key
    raw[body:] = np.uint64(_fnv1a(bytes(raw[:body]))).tobytes()
    path = str(tmp_path / "dup.bin")
    open(path, "wb").write(raw)
    f = Engine(device=-1, **SMALL)
    fresh = _state(f)
    for _ in range(2):
        with pytest.raises(CgpuError) as ex:
            f.mirror_restore(path)
        assert ex.value.errno == errno.EEXIST and "tunnel key exists" in str(ex.value)
        assert _empty(f) and _state(f) == fresh
        assert f.revnat4_count() == 0 and f.revnat6_count() == 0 and f.tunnel_count() == 0
        assert f.lb6_count() == 0 and f.lxc_lookup(0) is None
    f.mirror_restore(FIXTURE)
    e = _all_sections()
    assert _state(f) == _state(e)
    e.close()
    f.close()


def test_mirror_roundtrip(tmp_path):
    e = _populated()
    path = str(tmp_path / "mirror.bin")
    e.mirror_save(path)
    assert not os.path.exists(path + ".tmp")
    f = Engine(device=-1, ct_max=4096, lb_max_entries=1 << 16)
    f.mirror_restore(path)
    a, b = _state(e), _state(f)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], k
    assert len(a["ct4"][0]) and len(a["ct6"][0]) and a["rev"] == 2
    # the entry's supplied counters travel with it
    k, v = f.policy_dump(1)
    hit = v[(k["sec_label"] == 4242)]
    assert int(hit["packets"][0]) == 12 and int(hit["bytes"][0]) == 3456
    # restore into a non-empty context is refused
    with pytest.raises(CgpuError) as ex:
        f.mirror_restore(path)
    assert ex.value.errno == errno.EEXIST
    e.close()
    f.close()


@pytest.mark.parametrize("damage", ["flip", "truncate", "foreign", "missing"])
def test_mirror_rejects_bad_files(tmp_path, damage):
    e = _populated()
    path = str(tmp_path / "mirror.bin")
    e.mirror_save(path)
    raw = bytearray(open(path, "rb").read())
    if damage == "flip":
        raw[len(raw) // 2] ^= 0x40
    elif damage == "truncate":
        raw = raw[: len(raw) - 100]
    elif damage == "foreign":
        raw[:8] = b"NOTAMIRR"
    if damage == "missing":
        path = str(tmp_path / "absent.bin")
    else:
        open(path, "wb").write(raw)
    f = Engine(device=-1, ct_max=4096, lb_max_entries=1 << 16)
    with pytest.raises(CgpuError) as ex:
        f.mirror_restore(path)
    assert ex.value.errno == (errno.ENOENT if damage == "missing" else errno.EINVAL)
    assert f.ipcache_keys() == [] and f.ct4_count() == 0  # nothing applied
    e.close()
    f.close()


def _empty(f):
    return (f.ipcache_keys() == [] and f.ct4_count() == 0 and f.ct6_count() == 0 and
            all(len(f.policy_dump(ep)[0]) == 0 for ep in range(4)) and f.lb4_keys() == [] and
            PreFilter(f).Revision() == 1)


@pytest.mark.parametrize("cap", [{"ct_max": 16}, {"ct6_max": 16}, {"ipcache_max": 100},
                                 {"policy_max_per_ep": 64}, {"lb_max_entries": 8}])
def test_mirror_restore_refuses_smaller_context(tmp_path, cap):
    """a target configured smaller than the saver is refused with
    -E2BIG before any record is applied."""
    e = _populated()
    path = str(tmp_path / "mirror.bin")
    e.mirror_save(path)
    kw = {"ct_max": 4096, "lb_max_entries": 1 << 16}
    kw.update(cap)
    f = Engine(device=-1, **kw)
    with pytest.raises(CgpuError) as ex:
        f.mirror_restore(path)
    assert ex.value.errno == errno.E2BIG
    assert _empty(f)
    e.close()
    f.close()


def test_mirror_restore_rolls_back_partial_replay(tmp_path):
    """A record that fails during the replay itself (here the total policy
    capacity, which the per-section precheck does not cover) rolls back
    every record already applied: the context is empty again, and a retry
    fails the same way rather than with -EEXIST."""
    e = _populated()
    path = str(tmp_path / "mirror.bin")
    e.mirror_save(path)
    f = Engine(device=-1, ct_max=4096, lb_max_entries=1 << 16, policy_max_total=400)
    for _ in range(2):
        with pytest.raises(CgpuError) as ex:
            f.mirror_restore(path)
        assert ex.value.errno in (errno.E2BIG, errno.ENOSPC)
        assert _empty(f)
    # a context of the saver's size takes the same file
    g = Engine(device=-1, ct_max=4096, lb_max_entries=1 << 16)
    g.mirror_restore(path)
    assert _state(g) == _state(e)
    for x in (e, f, g):
        x.close()
