"""The bpf(2) hash-map contract of the host mirror's htab families, through the
C ABI on host-only contexts (device = -1): cilium_lb4_services,
cilium_lb6_services, cilium_tunnel_map, cilium_lb4_reverse_nat,
cilium_lb6_reverse_nat, and the part of it that cilium_lxc has.

One matrix for all of them: BPF_ANY / BPF_NOEXIST / BPF_EXIST, -E2BIG at the
capacity, delete / lookup of a missing key (-ENOENT, the last error left
alone), get_next_key as an ordered walk, the count after every step, and the
bytes of cgpu_last_error() after every failing call.  The walk orders and the
message texts are literals: they are the library's behaviour as recorded, and
a change to either is a change of the ABI."""
import ctypes as C
import errno
import struct

import pytest

from cilium_amd import build
from cilium_amd._abi import lib
from cilium_amd.engine import BPF_ANY, BPF_EXIST, BPF_NOEXIST, Engine


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


def _ep_key(ip: bytes, family: int) -> bytes:
    return ip + bytes(16 - len(ip)) + bytes([family, 0, 0, 0])


_A6 = bytes.fromhex("20010db8000000000000000000000099")


class Htab:
    """One family: how its calls take a key, and what it was recorded to do."""

    def __init__(self, name, klen, vlen, keys, order, noun, full, cap_cfg=None):
        self.name, self.klen, self.vlen, self.keys, self.order = name, klen, vlen, keys, order
        self.missing = f"{noun} not present".encode()
        self.exists = f"{noun} exists".encode()
        self.full = full.encode()
        self.cap_cfg = cap_cfg  # config that bounds the map at 4 entries; None: fixed size

    def val(self, i: int) -> bytes:
        return bytes((7 * i + j + 1) & 0xFF for j in range(self.vlen))

    def _k(self, key):
        return key

    def fn(self, op):
        return getattr(lib(), f"cgpu_{self.name}_{op}")

    def update(self, e, key, val, flags=BPF_ANY):
        return self.fn("update")(e.h, self._k(key), val, flags)

    def delete(self, e, key):
        return self.fn("delete")(e.h, self._k(key))

    def lookup(self, e, key):
        out = C.create_string_buffer(self.vlen)
        rc = self.fn("lookup")(e.h, self._k(key), out)
        return rc, out.raw

    def next(self, e, key):
        out = C.create_string_buffer(self.klen)
        rc = self.fn("get_next_key")(e.h, key, out)
        return rc, out.raw

    def count(self, e):
        return self.fn("count")(e.h)


class Revnat(Htab):
    """The reverse-NAT calls take the u16 index by value."""

    def _k(self, key):
        return struct.unpack("<H", key)[0]

    def next(self, e, key):
        out = C.c_uint16()
        prev = None if key is None else C.byref(C.c_uint16(self._k(key)))
        rc = self.fn("get_next_key")(e.h, prev, C.byref(out))
        return rc, struct.pack("<H", out.value)


def _lb4(address, dport, slave):
    return struct.pack("<IHH", address, dport, slave)


def _lb6(addr, dport, slave):
    return addr + struct.pack("<HH", dport, slave)


_RN_KEYS = [struct.pack("<H", i) for i in (0x0100, 0x0001, 0x0002, 0xFFFF, 0x0000, 0x0101)]

FAMILIES = [
    # keys 0 and 1 differ only in the slave, keys 0 and 2 only in the last
    # address byte; key 5's slave (256) sorts after 1 numerically but before
    # it as little-endian bytes
    Htab("lb4", 8, 12,
         [_lb4(0x0A00600A, 0x5000, 0), _lb4(0x0A00600A, 0x5000, 1), _lb4(0x0B00600A, 0x5000, 0),
          _lb4(0x0A00600A, 0xBB01, 0), _lb4(0x0100000A, 0x5000, 2), _lb4(0x0A00600A, 0x5000, 256)],
         [4, 0, 1, 5, 3, 2], "lb4 key", "lb4 service map full (4)", {"lb_max_entries": 4}),
    Htab("lb6", 20, 24,
         [_lb6(_A6, 0xBB01, 0), _lb6(_A6, 0xBB01, 1), _lb6(_A6[:15] + b"\x9a", 0xBB01, 0),
          _lb6(_A6, 0x5000, 0), _lb6(bytes.fromhex("fd00" + "00" * 13 + "01"), 0xBB01, 2),
          _lb6(_A6, 0xBB01, 256)],
         [3, 0, 1, 5, 2, 4], "lb6 key", "lb6 service map full (4)", {"lb_max_entries": 4}),
    # keys 0 and 5 differ only in the family byte, keys 0 and 1 in the last address byte
    Htab("tunnel", 20, 20,
         [_ep_key(bytes([10, 0, 1, 0]), 1), _ep_key(bytes([10, 0, 1, 1]), 1),
          _ep_key(bytes([10, 0, 2, 0]), 1), _ep_key(bytes.fromhex("f00d" + "00" * 13 + "01"), 2),
          _ep_key(bytes([9, 255, 255, 255]), 1), _ep_key(bytes([10, 0, 1, 0]), 2)],
         [4, 0, 5, 1, 2, 3], "tunnel key", "tunnel map full (65536)"),
    Revnat("revnat4", 2, 6, _RN_KEYS, [4, 1, 2, 0, 5, 3], "lb4 reverse NAT index",
           "lb4 reverse NAT map full (4)", {"lb_max_entries": 4}),
    Revnat("revnat6", 2, 18, _RN_KEYS, [4, 1, 2, 0, 5, 3], "lb6 reverse NAT index",
           "lb6 reverse NAT map full (4)", {"lb_max_entries": 4}),
]
IDS = [f.name for f in FAMILIES]


def _err():
    return lib().cgpu_last_error()


@pytest.mark.parametrize("f", FAMILIES, ids=IDS)
def test_flags_capacity_and_messages(f):
    e = Engine(device=-1, **(f.cap_cfg or {}))
    K = f.keys
    assert f.count(e) == 0
    # ANY on a missing key inserts, on a present key replaces
    assert f.update(e, K[0], f.val(0), BPF_ANY) == 0
    assert f.count(e) == 1 and f.lookup(e, K[0]) == (0, f.val(0))
    assert f.update(e, K[0], f.val(10), BPF_ANY) == 0
    assert f.count(e) == 1 and f.lookup(e, K[0]) == (0, f.val(10))
    assert f.update(e, K[0], f.val(11), BPF_NOEXIST) == -errno.EEXIST
    assert _err() == f.exists
    assert f.update(e, K[1], f.val(1), BPF_EXIST) == -errno.ENOENT
    assert _err() == f.missing
    assert f.count(e) == 1 and f.lookup(e, K[0]) == (0, f.val(10))
    # flags above EXIST: refused before the map is looked at
    assert f.update(e, K[0], f.val(0), 3) == -errno.EINVAL
    assert _err() == b"bad update flags 3"
    assert f.update(e, K[1], f.val(0), 1 << 40) == -errno.EINVAL
    assert _err() == b"bad update flags 1099511627776"
    assert f.count(e) == 1
    # delete / lookup of a missing key: a bare -ENOENT, the last error untouched
    assert f.delete(e, K[5]) == -errno.ENOENT
    assert _err() == b"bad update flags 1099511627776"
    assert f.lookup(e, K[5])[0] == -errno.ENOENT
    assert _err() == b"bad update flags 1099511627776"
    for i in (1, 2, 3):
        assert f.update(e, K[i], f.val(i), BPF_NOEXIST) == 0
        assert f.count(e) == i + 1
    if f.cap_cfg:
        # the fifth distinct key, whatever the flag that may insert
        for flags in (BPF_ANY, BPF_NOEXIST):
            assert f.update(e, K[4], f.val(4), flags) == -errno.E2BIG
            assert _err() == f.full
        assert f.update(e, K[4], f.val(4), BPF_EXIST) == -errno.ENOENT
        assert _err() == f.missing
        assert f.count(e) == 4 and f.lookup(e, K[4])[0] == -errno.ENOENT
    # replacing a present key in the full map succeeds
    assert f.update(e, K[2], f.val(12), BPF_ANY) == 0
    assert f.update(e, K[3], f.val(13), BPF_EXIST) == 0
    assert f.count(e) == 4
    assert [f.lookup(e, K[i]) for i in range(4)] == [(0, f.val(v)) for v in (10, 1, 12, 13)]
    # a delete makes room again
    assert f.delete(e, K[1]) == 0 and f.count(e) == 3
    assert f.delete(e, K[1]) == -errno.ENOENT and f.count(e) == 3
    assert f.update(e, K[4], f.val(4), BPF_NOEXIST) == 0 and f.count(e) == 4
    assert f.lookup(e, K[4]) == (0, f.val(4)) and f.lookup(e, K[1])[0] == -errno.ENOENT
    e.close()


@pytest.mark.parametrize("f", FAMILIES, ids=IDS)
def test_get_next_key_walk(f):
    e = Engine(device=-1)
    K = f.keys
    assert f.next(e, None)[0] == -errno.ENOENT and f.next(e, K[0])[0] == -errno.ENOENT
    for i, k in enumerate(K):
        assert f.update(e, k, f.val(i), BPF_NOEXIST) == 0
        assert f.count(e) == i + 1
    walk, prev = [], None
    while True:
        rc, nxt = f.next(e, prev)
        if rc:
            assert rc == -errno.ENOENT
            break
        walk.append(K.index(nxt))
        prev = nxt
        assert len(walk) <= len(K)
    assert walk == f.order
    # from a key that is not in the map: the next larger key
    gone = f.order[2]
    assert f.delete(e, K[gone]) == 0 and f.count(e) == 5
    assert f.next(e, K[gone]) == (0, K[f.order[3]])
    assert f.next(e, K[f.order[1]]) == (0, K[f.order[3]])
    assert f.next(e, None) == (0, K[f.order[0]])
    assert f.next(e, K[f.order[5]])[0] == -errno.ENOENT
    for i in range(6):
        assert f.lookup(e, K[i]) == ((-errno.ENOENT, bytes(f.vlen)) if i == gone else (0, f.val(i)))
    e.close()


@pytest.mark.parametrize("f", FAMILIES, ids=IDS)
def test_null_arguments(f):
    """A null context, key, value or output is -EINVAL "null argument"; a
    null value is reported before bad flags; the count of no context is 0."""
    e = Engine(device=-1)
    out = C.create_string_buffer(24)
    k0 = f._k(f.keys[0])
    nxt = C.byref(C.c_uint16()) if f.klen == 2 else out
    calls = [("update", (None, k0, bytes(f.vlen), 0)), ("update", (e.h, k0, None, 0)),
             ("update", (e.h, k0, None, 9)), ("delete", (None, k0)), ("lookup", (None, k0, out)),
             ("lookup", (e.h, k0, None)), ("get_next_key", (None, None, nxt)),
             ("get_next_key", (e.h, None, None))]
    if f.klen != 2:  # a key passed by pointer may be null too
        calls += [("update", (e.h, None, bytes(f.vlen), 0)), ("delete", (e.h, None)),
                  ("lookup", (e.h, None, out))]
    for op, args in calls:
        assert f.update(e, f.keys[0], bytes(f.vlen), 9) == -errno.EINVAL and _err() == b"bad update flags 9"
        assert f.fn(op)(*args) == -errno.EINVAL, (op, args)
        assert _err() == b"null argument", (op, args)
    assert f.fn("count")(None) == 0 and f.count(e) == 0
    e.close()


def test_tunnel_map_capacity():
    """cilium_tunnel_map has the reference's fixed size, 65,536 entries."""
    f = FAMILIES[2]
    e = Engine(device=-1)
    upd = f.fn("update")
    for i in range(65536):
        assert upd(e.h, _ep_key(struct.pack(">I", 0x0B000000 + i), 1), f.keys[0], BPF_NOEXIST) == 0
    assert f.count(e) == 65536
    for flags in (BPF_ANY, BPF_NOEXIST):
        assert f.update(e, f.keys[0], f.val(0), flags) == -errno.E2BIG
        assert _err() == f.full
    assert f.update(e, _ep_key(struct.pack(">I", 0x0B000007), 1), f.val(3), BPF_EXIST) == 0
    assert f.delete(e, _ep_key(struct.pack(">I", 0x0B000008), 1)) == 0
    assert f.update(e, f.keys[0], f.val(0), BPF_NOEXIST) == 0 and f.count(e) == 65536
    e.close()


@pytest.mark.parametrize("batch", ["lb4", "lb6"])
def test_update_batch_stops_at_the_first_failure(batch):
    f = FAMILIES[IDS.index(batch)]
    e = Engine(device=-1, lb_max_entries=4)
    keys = b"".join(f.keys)
    vals = b"".join(f.val(i) for i in range(6))
    fn = f.fn("update_batch")
    assert fn(e.h, keys, vals, 6, BPF_EXIST) == -errno.ENOENT and _err() == f.missing
    assert f.count(e) == 0
    assert fn(e.h, keys, vals, 6, BPF_ANY) == -errno.E2BIG and _err() == f.full
    assert f.count(e) == 4 and [f.lookup(e, k)[0] for k in f.keys] == [0, 0, 0, 0, -errno.ENOENT, -errno.ENOENT]
    assert fn(e.h, keys, vals, 4, BPF_NOEXIST) == -errno.EEXIST and _err() == f.exists
    assert fn(e.h, keys, b"".join(f.val(9) for _ in range(4)), 4, BPF_EXIST) == 0
    assert f.lookup(e, f.keys[3]) == (0, f.val(9))
    assert fn(e.h, None, None, 0, BPF_ANY) == 0
    assert fn(e.h, None, vals, 1, BPF_ANY) == -errno.EINVAL and _err() == b"null argument"
    assert fn(e.h, keys, vals, 1, 3) == -errno.EINVAL and _err() == b"bad update flags 3"
    e.close()


def test_endpoint_map_row():
    """cilium_lxc: a set of keys plus the values that are not all-zero.  It
    has the flag and capacity rules, and the bare -ENOENT of delete / lookup;
    it has no get_next_key and no count."""
    import numpy as np
    from cilium_amd import layouts as L
    e = Engine(device=-1, endpoints_max=4)
    K = [L.endpoint_key(ip) for ip in ("10.0.1.0", "10.0.1.1", "10.0.2.0", "f00d::1", "9.255.255.255", "f00d::2")]
    info = L.endpoint_info(ifindex=7, lxc_id=3, mac=bytes.fromhex("0a1b2c3d4e5f"))
    info2 = L.endpoint_info(ifindex=8, lxc_id=4, mac=bytes.fromhex("0a1b2c3d4e60"))
    zero = np.zeros((), L.ENDPOINT_INFO)

    def got(k):
        rc, v = e.endpoint_lookup_info(k)
        return rc, (None if v is None else v.tobytes())

    assert e.endpoint_update(K[0], BPF_ANY) == 0 and e.endpoint_lookup(K[0]) == 0
    assert got(K[0]) == (0, zero.tobytes())
    assert e.endpoint_update(K[0], BPF_ANY, info=info) == 0 and got(K[0]) == (0, info.tobytes())
    assert e.endpoint_update(K[0], BPF_ANY, info=info2) == 0 and got(K[0]) == (0, info2.tobytes())
    for upd in (lambda k, fl: e.endpoint_update(k, fl), lambda k, fl: e.endpoint_update(k, fl, info=info)):
        assert upd(K[0], BPF_NOEXIST) == -errno.EEXIST and _err() == b"exists"
        assert upd(K[1], BPF_EXIST) == -errno.ENOENT and _err() == b"missing"
        assert upd(K[0], 3) == -errno.EINVAL and _err() == b"bad update flags 3"
    assert got(K[0]) == (0, info2.tobytes())
    assert e.endpoint_delete(K[5]) == -errno.ENOENT and _err() == b"bad update flags 3"
    assert e.endpoint_lookup(K[5]) == -errno.ENOENT and _err() == b"bad update flags 3"
    assert got(K[5]) == (-errno.ENOENT, None) and _err() == b"bad update flags 3"
    assert e.endpoint_update(K[1], BPF_NOEXIST, info=info) == 0
    assert e.endpoint_update(K[2], BPF_NOEXIST) == 0
    assert e.endpoint_update(K[3], BPF_ANY, info=zero) == 0  # the all-zero value is no value
    assert got(K[3]) == (0, zero.tobytes())
    for upd in (lambda k, fl: e.endpoint_update(k, fl), lambda k, fl: e.endpoint_update(k, fl, info=info)):
        assert upd(K[4], BPF_ANY) == -errno.E2BIG and _err() == b"endpoint map full"
        assert upd(K[4], BPF_NOEXIST) == -errno.E2BIG and _err() == b"endpoint map full"
    assert e.endpoint_lookup(K[4]) == -errno.ENOENT
    # replacing in the full map; the plain update writes the all-zero value
    assert e.endpoint_update(K[2], BPF_EXIST, info=info2) == 0 and got(K[2]) == (0, info2.tobytes())
    assert e.endpoint_update(K[1], BPF_ANY) == 0 and got(K[1]) == (0, zero.tobytes())
    assert e.endpoint_delete(K[2]) == 0 and e.endpoint_delete(K[2]) == -errno.ENOENT
    assert e.endpoint_update(K[4], BPF_NOEXIST) == 0 and got(K[4]) == (0, zero.tobytes())
    assert e.endpoint_update(K[2], BPF_ANY) == -errno.E2BIG
    assert [e.endpoint_lookup(k) for k in K] == [0, 0, -errno.ENOENT, 0, 0, -errno.ENOENT]
    e.close()
