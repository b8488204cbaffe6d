"""The reverse-NAT maps cilium_lb4_reverse_nat / cilium_lb6_reverse_nat on a
host-only context (device = -1): bpf(2) map semantics of the cgpu_revnat4_* /
cgpu_revnat6_* calls (as the cgpu_lb4_* calls), the raw-index byte order, and
their two sections in a checkpoint."""
import errno
import struct

import numpy as np
import pytest

from cilium_amd import layouts as L
from cilium_amd._abi import CgpuError
from cilium_amd.engine import BPF_ANY, BPF_EXIST, BPF_NOEXIST, Engine

V6A = "2001:db8::a"
V6B = "2001:db8::b"


def _fam(e, v6):
    """(update, delete, lookup, keys, count, value constructor, two addresses)"""
    if v6:
        return (e.revnat6_update, e.revnat6_delete, e.revnat6_lookup, e.revnat6_keys, e.revnat6_count,
                L.lb6_reverse_nat, (V6A, V6B))
    return (e.revnat4_update, e.revnat4_delete, e.revnat4_lookup, e.revnat4_keys, e.revnat4_count,
            L.lb4_reverse_nat, ("10.96.0.1", "10.96.0.2"))


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_update_flags_lookup_delete(v6):
    e = Engine(device=-1)
    upd, dele, look, keys, count, val, (a, b) = _fam(e, v6)
    assert count() == 0 and keys() == []
    # absent keys
    assert look(7) == (-errno.ENOENT, None)
    assert dele(7) == -errno.ENOENT
    assert upd(7, val(a, 80), BPF_EXIST) == -errno.ENOENT
    # NOEXIST creates once, ANY overwrites, EXIST overwrites
    assert upd(7, val(a, 80), BPF_NOEXIST) == 0
    assert upd(7, val(b, 81), BPF_NOEXIST) == -errno.EEXIST
    rc, got = look(7)
    assert rc == 0 and bytes(got) == bytes(val(a, 80))
    assert upd(7, val(b, 81), BPF_ANY) == 0
    assert bytes(look(7)[1]) == bytes(val(b, 81))
    assert upd(7, val(a, 0), BPF_EXIST) == 0
    assert bytes(look(7)[1]) == bytes(val(a, 0)) and int(look(7)[1]["port"]) == 0
    assert upd(7, val(a, 80), 3) == -errno.EINVAL
    assert count() == 1
    # the other family's map is another map
    other = _fam(e, not v6)
    assert other[4]() == 0 and other[2](7)[0] == -errno.ENOENT
    assert dele(7) == 0 and count() == 0 and look(7)[0] == -errno.ENOENT
    e.close()


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_get_next_key_walks_every_key_once(v6):
    e = Engine(device=-1)
    upd, dele, look, keys, count, val, (a, b) = _fam(e, v6)
    rng = np.random.default_rng(5)
    want = sorted({0, 1, 0xFFFF, 0x0100, 0x00FF, *(int(x) for x in rng.integers(0, 1 << 16, 300))})
    for i in rng.permutation(want):
        assert upd(int(i), val(a, int(i) & 0xFFF)) == 0
    got = keys()
    assert len(got) == len(set(got)) == len(want) == count()
    assert sorted(got) == want
    for i in want[::3]:
        assert dele(i) == 0
    assert sorted(keys()) == sorted(set(want) - set(want[::3]))
    e.close()


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_e2big_at_lb_max_entries(v6):
    e = Engine(device=-1, lb_max_entries=4)
    upd, dele, look, keys, count, val, (a, b) = _fam(e, v6)
    for i in range(4):
        assert upd(100 + i, val(a, 1)) == 0
    assert upd(200, val(a, 1)) == -errno.E2BIG
    assert upd(200, val(a, 1), BPF_NOEXIST) == -errno.E2BIG
    assert upd(101, val(b, 2)) == 0  # an existing key still updates
    assert count() == 4
    assert dele(100) == 0 and upd(200, val(a, 1)) == 0
    # the capacity is per map: the other family and the service map are untouched
    other = _fam(e, not v6)
    for i in range(4):
        assert other[0](i, other[5](other[6][0], 1)) == 0
    assert e.lb4_update(L.lb4_key("10.96.0.1", 80, 0), L.lb4_service(0, 0, 1)) == 0
    e.close()


def test_raw_index_is_the_service_entrys_word():
    """The __u16 key is looked up as stored (lb.h:570): UpdateRevNat(i, ...)
    must land on the 16 raw bits lb4_service(...)["rev_nat_index"] holds."""
    e = Engine(device=-1)
    for i in (1, 2, 255, 0x0300, 0x1234, 0xFFFF):  # no index is another one byte-swapped
        raw = int(L.lb4_service("10.0.0.1", 80, 0, rev_nat=i)["rev_nat_index"])
        assert raw == L.revnat_index(i) == (((i & 0xFF) << 8) | (i >> 8))
        e.UpdateRevNat(i, "10.96.0.9", 8000 + (i & 0xFF))
        rc, v = e.revnat4_lookup(raw)
        assert rc == 0
        assert bytes(v) == bytes(L.lb4_reverse_nat("10.96.0.9", 8000 + (i & 0xFF)))
        assert struct.pack("<I", int(v["address"])) == bytes([10, 96, 0, 9])  # network order
        assert struct.pack("<H", int(v["port"])) == struct.pack(">H", 8000 + (i & 0xFF))
        if raw != i:
            assert e.revnat4_lookup(i)[0] == -errno.ENOENT
        e.UpdateRevNat(i, V6A, 443)
        rc, v6 = e.revnat6_lookup(raw)
        assert rc == 0 and bytes(v6) == bytes(L.lb6_reverse_nat(V6A, 443))
    assert e.revnat4_count() == 6 and e.revnat6_count() == 6
    e.DeleteRevNat(0x1234)
    assert e.revnat4_lookup(L.revnat_index(0x1234))[0] == -errno.ENOENT
    e.DeleteRevNat(0x1234, v6=True)
    assert e.revnat6_count() == 5
    with pytest.raises(CgpuError):
        e.DeleteRevNat(0x1234)
    e.close()


def _dump(e):
    return ([(k, bytes(e.revnat4_lookup(k)[1])) for k in e.revnat4_keys()],
            [(k, bytes(e.revnat6_lookup(k)[1])) for k in e.revnat6_keys()])


def test_checkpoint_round_trips_both_maps(tmp_path):
    e = Engine(device=-1)
    for i in range(1, 40):
        e.UpdateRevNat(i, f"10.96.{i}.1", 80 + i if i % 3 else 0)
    for i in range(1, 20):
        e.UpdateRevNat(i * 7, f"2001:db8::{i:x}", 443)
    assert e.lb4_update(L.lb4_key("10.96.1.1", 80, 0), L.lb4_service(0, 0, 1)) == 0
    want = _dump(e)
    assert len(want[0]) == 39 and len(want[1]) == 19
    p = str(tmp_path / "m.bin")
    e.mirror_save(p)
    r = Engine(device=-1)
    r.mirror_restore(p)
    assert _dump(r) == want
    assert r.lb4_count() == 1
    # a context whose reverse-NAT maps hold something is not empty
    with pytest.raises(CgpuError) as ex:
        r.mirror_restore(p)
    assert ex.value.errno == errno.EEXIST
    only_rn = Engine(device=-1)
    only_rn.UpdateRevNat(1, "10.96.0.1", 80)
    with pytest.raises(CgpuError) as ex:
        only_rn.mirror_restore(p)
    assert ex.value.errno == errno.EEXIST
    # a context too small for the file's reverse-NAT section refuses it whole
    small = Engine(device=-1, lb_max_entries=8)
    with pytest.raises(CgpuError) as ex:
        small.mirror_restore(p)
    assert ex.value.errno == errno.E2BIG
    assert small.revnat4_count() == 0 and small.revnat6_count() == 0 and small.lb4_count() == 0
    for x in (e, r, only_rn, small):
        x.close()


def _fnv(b: bytes) -> int:
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _sections(buf: bytes):
    """[(tag, record bytes, count, start, end)] of a checkpoint file."""
    nsec = struct.unpack_from("<I", buf, 12)[0]
    off, out = 16, []
    for _ in range(nsec):
        tag, rec, n = struct.unpack_from("<IIQ", buf, off)
        out.append((tag, rec, n, off, off + 16 + rec * n))
        off = out[-1][4]
    assert off == len(buf) - 8
    return out


def test_checkpoint_with_empty_maps_and_without_their_sections(tmp_path):
    e = Engine(device=-1)
    assert e.ipcache_update(L.ipcache_key("10.1.0.0/16"), L.remote_info(300)) == 0
    assert e.lb4_update(L.lb4_key("10.96.1.1", 80, 0), L.lb4_service(0, 0, 1)) == 0
    p = str(tmp_path / "empty.bin")
    e.mirror_save(p)
    r = Engine(device=-1)
    r.mirror_restore(p)
    assert r.revnat4_count() == 0 and r.revnat6_count() == 0
    assert r.lb4_count() == 1 and len(r.ipcache_keys()) == 1
    # the file as it was written before the two sections existed: the first
    # ten sections, the section count 10, the checksum over that
    buf = open(p, "rb").read()
    secs = _sections(buf)
    assert len(secs) == 12 and [s[0] for s in secs[10:]] == [11, 12]
    assert [(s[1], s[2]) for s in secs[10:]] == [(8, 0), (20, 0)]
    old = bytearray(buf[:secs[10][3]])
    struct.pack_into("<I", old, 12, 10)
    old += struct.pack("<Q", _fnv(bytes(old)))
    p2 = str(tmp_path / "old.bin")
    open(p2, "wb").write(bytes(old))
    r2 = Engine(device=-1)
    r2.mirror_restore(p2)
    assert r2.revnat4_count() == 0 and r2.revnat6_count() == 0
    assert r2.lb4_count() == 1 and len(r2.ipcache_keys()) == 1
    for x in (e, r, r2):
        x.close()
