"""Python face of the engine: a thin wrapper over the C ABI (include/cgpu.h).

The map objects mirror the method sets of the reference's Go map wrappers so
that tests read like the reference's own callers:

* :class:`PolicyMap`  — pkg/maps/policymap/policymap.go (Allow/AllowKey/Exists/
  Delete/DeleteKey/DumpToSlice/Flush)
* :class:`IPCacheMap` — pkg/maps/ipcache/ipcache.go (Update/Delete with the
  tombstone-on-ENOSYS variant, NewKey) and the IPIdentityMappingListener hook
  (pkg/ipcache/listener.go:36-48, pkg/datapath/ipcache/listener.go:78-127)
* :class:`CIDRMap`    — pkg/maps/cidrmap/cidrmap.go (InsertCIDR/DeleteCIDR/
  CIDRExists/CIDRDump, checkPrefixlen)
* :class:`LBMap`      — pkg/maps/lbmap/lbmap.go (UpdateService/DeleteService/
  LookupService/DumpServiceMapsToUserspace over cilium_lb4_services)

Batch entry points take torch CUDA tensors (device memory) and launch on the
caller's current HIP stream.  Nothing here computes a verdict on the CPU.
"""
from __future__ import annotations

import ctypes as C
import errno
import ipaddress

import numpy as np

from . import layouts as L
from ._abi import (CgpuConfig, CgpuError, CtlbOut, DlvIn, DlvOut, FctOut, FlbIn, FlbOut, FrameCtCols, FrameTuples, Frames, FwdIn, FwdOut,
                   FwdParams,
                   FwdfIn, FwdfParams, Lb4Out, Lb4Tuples, Rnat4Out, Rnat6Out, Rnf4In, Rnf6In, TuplesV4, TuplesV4Ct, TuplesV6Ct,
                   TuplesV6, check, lib)

CIDR_V4_DYN, CIDR_V4_FIX, CIDR_V6_DYN, CIDR_V6_FIX = 0, 1, 2, 3
BPF_ANY, BPF_NOEXIST, BPF_EXIST = 0, 1, 2


def _buf(x) -> bytes:
    return np.ascontiguousarray(x).tobytes()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    return C.c_void_p(stream.cuda_stream)


class Engine:
    """One cgpu context bound to one GPU (device=-1: host-only, table ops)."""

    def __init__(self, device: int = 0, **cfg):
        self.L = lib()
        self.cfg = CgpuConfig()
        self.L.cgpu_config_default(C.byref(self.cfg))
        for k, v in cfg.items():
            if not hasattr(self.cfg, k):
                raise TypeError(f"unknown config field {k}")
            if k in ("ipv6_router_ip", "node_mac"):
                getattr(self.cfg, k)[:] = bytes(v)
                continue
            setattr(self.cfg, k, v)
        h = C.c_void_p()
        check(self.L.cgpu_ctx_create(C.byref(self.cfg), device, C.byref(h)), "cgpu_ctx_create")
        self.h = h
        self.device = device
        self._bound = None

    def close(self):
        if getattr(self, "h", None):
            self.L.cgpu_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------- raw map ops
    def ipcache_update(self, key, val, flags=BPF_ANY) -> int:
        return self.L.cgpu_ipcache_update(self.h, _buf(key), _buf(val), flags)

    def ipcache_delete(self, key) -> int:
        return self.L.cgpu_ipcache_delete(self.h, _buf(key))

    def ipcache_lookup(self, key):
        out = C.create_string_buffer(8)
        rc = self.L.cgpu_ipcache_lookup(self.h, _buf(key), out)
        return rc, (np.frombuffer(out.raw, L.REMOTE_ENDPOINT_INFO)[0] if rc == 0 else None)

    def ipcache_update_batch(self, keys, vals, flags=BPF_ANY) -> int:
        k = np.ascontiguousarray(keys, L.IPCACHE_KEY)
        v = np.ascontiguousarray(vals, L.REMOTE_ENDPOINT_INFO)
        assert len(k) == len(v)
        return self.L.cgpu_ipcache_update_batch(self.h, k.ctypes.data, v.ctypes.data, len(k), flags)

    def ipcache_keys(self):
        keys, prev = [], None
        out = C.create_string_buffer(24)
        while self.L.cgpu_ipcache_get_next_key(self.h, prev, out) == 0:
            prev = out.raw
            keys.append(np.frombuffer(prev, L.IPCACHE_KEY)[0])
        return keys

    def policy_update(self, ep, key, entry, flags=BPF_ANY) -> int:
        return self.L.cgpu_policy_update(self.h, ep, _buf(key), _buf(entry), flags)

    def policy_delete(self, ep, key) -> int:
        return self.L.cgpu_policy_delete(self.h, ep, _buf(key))

    def policy_lookup(self, ep, key):
        out = C.create_string_buffer(24)
        rc = self.L.cgpu_policy_lookup(self.h, ep, _buf(key), out)
        return rc, (np.frombuffer(out.raw, L.POLICY_ENTRY)[0] if rc == 0 else None)

    def policy_keys(self, ep):
        keys, prev = [], None
        out = C.create_string_buffer(8)
        while self.L.cgpu_policy_get_next_key(self.h, ep, prev, out) == 0:
            prev = out.raw
            keys.append(np.frombuffer(prev, L.POLICY_KEY)[0])
        return keys

    def policy_flush(self, ep) -> int:
        return self.L.cgpu_policy_flush(self.h, ep)

    def policy_update_batch(self, eps, keys, entries, flags=BPF_ANY) -> int:
        e = np.ascontiguousarray(eps, np.uint32)
        k = np.ascontiguousarray(keys, L.POLICY_KEY)
        v = np.ascontiguousarray(entries, L.POLICY_ENTRY)
        assert len(e) == len(k) == len(v)
        return self.L.cgpu_policy_update_batch(self.h, e.ctypes.data, k.ctypes.data, v.ctypes.data,
                                               len(k), flags)

    def policy_lookup_batch(self, eps, keys):
        """(rc[n], entries[n]) of cgpu_policy_lookup_batch (one device read)."""
        e = np.ascontiguousarray(eps, np.uint32)
        k = np.ascontiguousarray(keys, L.POLICY_KEY)
        out = np.zeros(len(k), L.POLICY_ENTRY)
        rc = np.zeros(len(k), np.int32)
        check(self.L.cgpu_policy_lookup_batch(self.h, e.ctypes.data, k.ctypes.data, len(k),
                                              out.ctypes.data, rc.ctypes.data),
              "cgpu_policy_lookup_batch")
        return rc, out

    def policy_counters(self, eps, keys) -> np.ndarray:
        """(n, 2) uint64 {packets, bytes} of present keys (raises if any is absent)."""
        rc, out = self.policy_lookup_batch(eps, keys)
        assert (rc == 0).all(), "policy key absent"
        return np.stack([out["packets"], out["bytes"]], 1).astype(np.uint64)

    def policy_dump(self, ep):
        """DumpToSlice of one endpoint's map: (keys, entries)."""
        n = C.c_size_t()
        rc = self.L.cgpu_policy_dump(self.h, ep, None, None, 0, C.byref(n))
        keys = np.zeros(n.value, L.POLICY_KEY)
        ents = np.zeros(n.value, L.POLICY_ENTRY)
        if n.value:
            check(self.L.cgpu_policy_dump(self.h, ep, keys.ctypes.data, ents.ctypes.data, n.value,
                                          C.byref(n)), "cgpu_policy_dump")
        elif rc < 0:
            check(rc, "cgpu_policy_dump")
        return keys, ents

    @staticmethod
    def _cidr_buf(key) -> bytes:
        raw = _buf(key)
        return raw + bytes(20 - len(raw))

    def cidr_update(self, which, key, flags=BPF_ANY) -> int:
        return self.L.cgpu_cidr_update(self.h, which, self._cidr_buf(key), flags)

    def cidr_update_batch(self, which, keys, flags=BPF_ANY) -> int:
        """keys: LPM_V4_KEY / LPM_V6_KEY records (padded to 20-byte keys)."""
        k = np.ascontiguousarray(keys)
        buf = np.zeros((len(k), 20), np.uint8)
        buf[:, :k.dtype.itemsize] = k.view(np.uint8).reshape(len(k), k.dtype.itemsize)
        return self.L.cgpu_cidr_update_batch(self.h, which, buf.ctypes.data, len(k), flags)

    def cidr_delete(self, which, key) -> int:
        return self.L.cgpu_cidr_delete(self.h, which, self._cidr_buf(key))

    def cidr_lookup(self, which, key) -> int:
        return self.L.cgpu_cidr_lookup(self.h, which, self._cidr_buf(key))

    def cidr_keys(self, which):
        keys, prev = [], None
        out = C.create_string_buffer(20)
        dt = L.LPM_V4_KEY if which in (CIDR_V4_DYN, CIDR_V4_FIX) else L.LPM_V6_KEY
        while self.L.cgpu_cidr_get_next_key(self.h, which, prev, out) == 0:
            prev = out.raw
            keys.append(np.frombuffer(prev[:dt.itemsize], dt)[0])
        return keys

    def endpoint_update(self, key, flags=BPF_ANY, info=None) -> int:
        """info: an L.ENDPOINT_INFO value (cgpu_endpoint_update_info); None
        writes the all-zero value."""
        if info is not None:
            return self.L.cgpu_endpoint_update_info(self.h, _buf(key), _buf(np.asarray(info, L.ENDPOINT_INFO)),
                                                    flags)
        return self.L.cgpu_endpoint_update(self.h, _buf(key), flags)

    def endpoint_lookup_info(self, key):
        out = C.create_string_buffer(48)
        rc = self.L.cgpu_endpoint_lookup_info(self.h, _buf(key), out)
        return rc, (np.frombuffer(out.raw, L.ENDPOINT_INFO)[0] if rc == 0 else None)

    # --- cilium_tunnel_map (key and value: raw 20-byte endpoint keys) ---
    def tunnel_update(self, key, val, flags=BPF_ANY) -> int:
        return self.L.cgpu_tunnel_update(self.h, _buf(key), _buf(val), flags)

    def tunnel_delete(self, key) -> int:
        return self.L.cgpu_tunnel_delete(self.h, _buf(key))

    def tunnel_lookup(self, key):
        out = C.create_string_buffer(20)
        rc = self.L.cgpu_tunnel_lookup(self.h, _buf(key), out)
        return rc, (np.frombuffer(out.raw, L.ENDPOINT_KEY)[0] if rc == 0 else None)

    def tunnel_keys(self):
        keys, prev = [], None
        out = C.create_string_buffer(20)
        while self.L.cgpu_tunnel_get_next_key(self.h, prev, out) == 0:
            prev = out.raw
            keys.append(np.frombuffer(prev, L.ENDPOINT_KEY)[0])
        return keys

    def tunnel_count(self) -> int:
        return self.L.cgpu_tunnel_count(self.h)

    def endpoint_delete(self, key) -> int:
        return self.L.cgpu_endpoint_delete(self.h, _buf(key))

    def endpoint_lookup(self, key) -> int:
        return self.L.cgpu_endpoint_lookup(self.h, _buf(key))

    def lb4_update(self, key, val, flags=BPF_ANY) -> int:
        return self.L.cgpu_lb4_update(self.h, _buf(key), _buf(val), flags)

    def lb4_update_batch(self, keys, vals, flags=BPF_ANY) -> int:
        k = np.ascontiguousarray(keys, L.LB4_KEY)
        v = np.ascontiguousarray(vals, L.LB4_SERVICE)
        assert len(k) == len(v)
        return self.L.cgpu_lb4_update_batch(self.h, k.ctypes.data, v.ctypes.data, len(k), flags)

    def lb4_delete(self, key) -> int:
        return self.L.cgpu_lb4_delete(self.h, _buf(key))

    def lb4_lookup(self, key):
        out = C.create_string_buffer(12)
        rc = self.L.cgpu_lb4_lookup(self.h, _buf(key), out)
        return rc, (np.frombuffer(out.raw, L.LB4_SERVICE)[0] if rc == 0 else None)

    def lb4_keys(self):
        keys, prev = [], None
        out = C.create_string_buffer(8)
        while self.L.cgpu_lb4_get_next_key(self.h, prev, out) == 0:
            prev = out.raw
            keys.append(np.frombuffer(prev, L.LB4_KEY)[0])
        return keys

    def lb4_count(self) -> int:
        return self.L.cgpu_lb4_count(self.h)

    # --- cilium_lb6_services ---
    def lb6_update(self, key, val, flags=BPF_ANY) -> int:
        return self.L.cgpu_lb6_update(self.h, _buf(key), _buf(val), flags)

    def lb6_update_batch(self, keys, vals, flags=BPF_ANY) -> int:
        k = np.ascontiguousarray(keys, L.LB6_KEY)
        v = np.ascontiguousarray(vals, L.LB6_SERVICE)
        assert len(k) == len(v)
        return self.L.cgpu_lb6_update_batch(self.h, k.ctypes.data, v.ctypes.data, len(k), flags)

    def lb6_delete(self, key) -> int:
        return self.L.cgpu_lb6_delete(self.h, _buf(key))

    def lb6_lookup(self, key):
        out = C.create_string_buffer(24)
        rc = self.L.cgpu_lb6_lookup(self.h, _buf(key), out)
        return rc, (np.frombuffer(out.raw, L.LB6_SERVICE)[0] if rc == 0 else None)

    def lb6_keys(self):
        keys, prev = [], None
        out = C.create_string_buffer(20)
        while self.L.cgpu_lb6_get_next_key(self.h, prev, out) == 0:
            prev = out.raw
            keys.append(np.frombuffer(prev, L.LB6_KEY)[0])
        return keys

    def lb6_count(self) -> int:
        return self.L.cgpu_lb6_count(self.h)

    # --- cilium_lb4_reverse_nat / cilium_lb6_reverse_nat (index: the raw u16 key) ---
    def _revnat_keys(self, fn):
        keys, prev = [], None
        out = C.c_uint16()
        while fn(self.h, prev, C.byref(out)) == 0:
            keys.append(int(out.value))
            prev = C.byref(C.c_uint16(out.value))
        return keys

    def revnat4_update(self, index: int, val, flags=BPF_ANY) -> int:
        return self.L.cgpu_revnat4_update(self.h, index, _buf(val), flags)

    def revnat4_delete(self, index: int) -> int:
        return self.L.cgpu_revnat4_delete(self.h, index)

    def revnat4_lookup(self, index: int):
        out = C.create_string_buffer(6)
        rc = self.L.cgpu_revnat4_lookup(self.h, index, out)
        return rc, (np.frombuffer(out.raw, L.LB4_REVERSE_NAT)[0] if rc == 0 else None)

    def revnat4_keys(self):
        return self._revnat_keys(self.L.cgpu_revnat4_get_next_key)

    def revnat4_count(self) -> int:
        return self.L.cgpu_revnat4_count(self.h)

    def revnat6_update(self, index: int, val, flags=BPF_ANY) -> int:
        return self.L.cgpu_revnat6_update(self.h, index, _buf(val), flags)

    def revnat6_delete(self, index: int) -> int:
        return self.L.cgpu_revnat6_delete(self.h, index)

    def revnat6_lookup(self, index: int):
        out = C.create_string_buffer(18)
        rc = self.L.cgpu_revnat6_lookup(self.h, index, out)
        return rc, (np.frombuffer(out.raw, L.LB6_REVERSE_NAT)[0] if rc == 0 else None)

    def revnat6_keys(self):
        return self._revnat_keys(self.L.cgpu_revnat6_get_next_key)

    def revnat6_count(self) -> int:
        return self.L.cgpu_revnat6_count(self.h)

    def UpdateRevNat(self, index: int, vip: str, port: int):  # noqa: N802
        """lbmap.UpdateRevNat (lbmap.go:229-244): reverse-NAT entry `index`
        (host order, as UpdateService's rev_nat) -> {vip, port}; the family
        follows the address."""
        if ipaddress.ip_address(vip).version == 4:
            check(self.revnat4_update(L.revnat_index(index), L.lb4_reverse_nat(vip, port)), "UpdateRevNat")
        else:
            check(self.revnat6_update(L.revnat_index(index), L.lb6_reverse_nat(vip, port)), "UpdateRevNat")

    def DeleteRevNat(self, index: int, v6: bool = False):  # noqa: N802
        """lbmap.DeleteRevNat (lbmap.go:246-260)."""
        fn = self.revnat6_delete if v6 else self.revnat4_delete
        rc = fn(L.revnat_index(index))
        if rc != 0:
            raise CgpuError(errno.ENOENT, f"reverse NAT index {index} not found")

    def flow_hash6(self, saddr16, daddr16, sport, dport, proto) -> int:
        return self.L.cgpu_flow_hash6(bytes(saddr16), bytes(daddr16), sport, dport, proto)

    # --- conntrack map cilium_ct4_global ---
    def ct4_update(self, key, val, flags=BPF_ANY) -> int:
        return self.L.cgpu_ct4_update(self.h, _buf(key), _buf(val), flags)

    def ct4_delete(self, key) -> int:
        return self.L.cgpu_ct4_delete(self.h, _buf(key))

    def ct4_lookup(self, key):
        out = C.create_string_buffer(56)
        rc = self.L.cgpu_ct4_lookup(self.h, _buf(key), out)
        return rc, (np.frombuffer(out.raw, L.CT_ENTRY)[0] if rc == 0 else None)

    def ct4_count(self) -> int:
        return self.L.cgpu_ct4_count(self.h)

    def ct4_gc(self, time: int) -> int:
        d = C.c_uint64()
        check(self.L.cgpu_ct4_gc(self.h, time, C.byref(d)), "cgpu_ct4_gc")
        return d.value

    def ct_stats(self, v6: bool = False) -> dict:
        """cgpu_ct_stats: live entries, tombstones and compactions of the map."""
        out = np.zeros(3, np.uint64)
        check(self.L.cgpu_ct_stats(self.h, int(v6), out.ctypes.data_as(C.c_void_p)), "cgpu_ct_stats")
        return {"live": int(out[0]), "tombstones": int(out[1]), "compactions": int(out[2])}

    def ct_lru_stats(self, v6: bool = False) -> dict:
        """cgpu_ct_lru_stats: LRU mode's evictions and creates that found no victim."""
        out = np.zeros(2, np.uint64)
        check(self.L.cgpu_ct_lru_stats(self.h, int(v6), out.ctypes.data_as(C.c_void_p)), "cgpu_ct_lru_stats")
        return {"evictions": int(out[0]), "no_victim": int(out[1])}

    def ct4_flush(self) -> None:
        check(self.L.cgpu_ct4_flush(self.h), "cgpu_ct4_flush")

    def ct4_dump(self):
        """(keys, vals) of the whole map via get_next_key + lookup, sorted
        canonically (layouts.ct_sorted)."""
        keys, vals, prev = [], [], None
        out = C.create_string_buffer(14)
        cap = self.ct4_count()
        while self.L.cgpu_ct4_get_next_key(self.h, prev, out) == 0:
            # a key stored twice would restart the walk forever
            if len(keys) > cap:
                raise AssertionError("cilium_ct4_global holds a key twice")
            prev = out.raw
            rc, v = self.ct4_lookup(np.frombuffer(prev, L.CT4_TUPLE)[0])
            assert rc == 0
            keys.append(np.frombuffer(prev, L.CT4_TUPLE)[0])
            vals.append(v)
        return L.ct_sorted(np.array(keys, L.CT4_TUPLE), np.array(vals, L.CT_ENTRY))

    # --- cilium_ct6_global (IPv6 conntrack) ---
    def ct6_update(self, key, val, flags=BPF_ANY) -> int:
        return self.L.cgpu_ct6_update(self.h, _buf(key), _buf(val), flags)

    def ct6_delete(self, key) -> int:
        return self.L.cgpu_ct6_delete(self.h, _buf(key))

    def ct6_lookup(self, key):
        out = C.create_string_buffer(56)
        rc = self.L.cgpu_ct6_lookup(self.h, _buf(key), out)
        return rc, (np.frombuffer(out.raw, L.CT_ENTRY)[0] if rc == 0 else None)

    def ct6_count(self) -> int:
        return self.L.cgpu_ct6_count(self.h)

    def ct6_gc(self, time: int) -> int:
        d = C.c_uint64()
        check(self.L.cgpu_ct6_gc(self.h, time, C.byref(d)), "cgpu_ct6_gc")
        return d.value

    def ct6_flush(self) -> None:
        check(self.L.cgpu_ct6_flush(self.h), "cgpu_ct6_flush")

    def ct6_dump(self):
        keys, vals, prev = [], [], None
        out = C.create_string_buffer(38)
        cap = self.ct6_count()
        while self.L.cgpu_ct6_get_next_key(self.h, prev, out) == 0:
            # a key stored twice would restart the walk forever
            if len(keys) > cap:
                raise AssertionError("cilium_ct6_global holds a key twice")
            prev = out.raw
            rc, v = self.ct6_lookup(np.frombuffer(prev, L.CT6_TUPLE)[0])
            assert rc == 0
            keys.append(np.frombuffer(prev, L.CT6_TUPLE)[0])
            vals.append(v)
        return L.ct_sorted(np.array(keys, L.CT6_TUPLE), np.array(vals, L.CT_ENTRY))

    # --- L3 MapState compilation ---
    def l3_compile(self, prog, ep_sets, id_sets, flags: int = 3) -> np.ndarray:
        """cgpu_l3_compile: prog = cilium_amd.policy.L3Program, *_sets =
        [[Label]] (endpoint / identity label arrays) or their interned form
        prog.label_sets(...) (offsets, LABEL records).  -> (n_ep, n_id) uint8,
        bit 0 ingress Allowed, bit 1 egress Allowed."""
        from . import policy as P
        eo, el = ep_sets if isinstance(ep_sets, tuple) else prog.label_sets(ep_sets)
        io, il = id_sets if isinstance(id_sets, tuple) else prog.label_sets(id_sets)
        allow = np.zeros((len(eo) - 1, len(io) - 1), np.uint8)
        cp, ce, ci = P.c_program(prog), P.c_label_sets(eo, el), P.c_label_sets(io, il)
        check(self.L.cgpu_l3_compile(self.h, C.byref(cp), C.byref(ce), C.byref(ci), flags,
                                     allow.ctypes.data), "cgpu_l3_compile")
        return allow

    def mapstate_sync(self, msp) -> dict:
        """cgpu_mapstate_sync: msp = cilium_amd.policy.compile_mapstate(...).
        Computes every endpoint's desired MapState on the device and syncs
        it into the host mirror's policy maps (visible after commit()).
        -> the sync counts {desired, added, updated, deleted, unchanged,
        failed}; raises on the first failing key like syncPolicyMap's error."""
        from . import policy as P
        m = msp
        cp, ce, ci = P.c_program(m.prog), P.c_label_sets(*m.ep_sets), P.c_label_sets(*m.id_sets)
        spec, stats = P.c_mapstate_spec(m), P.CMapStateStats()
        rc = self.L.cgpu_mapstate_sync(self.h, C.byref(cp), C.byref(ce), C.byref(ci),
                                       C.byref(spec), C.byref(stats))
        out = {n: getattr(stats, n) for n, _ in P.CMapStateStats._fields_}
        check(rc, "cgpu_mapstate_sync")
        return out

    def flow_hash(self, saddr, daddr, sport, dport, proto) -> int:
        return self.L.cgpu_flow_hash(saddr, daddr, sport, dport, proto)

    def commit(self) -> int:
        ep = C.c_uint64()
        check(self.L.cgpu_commit(self.h, C.byref(ep)), "cgpu_commit")
        return ep.value

    def checksum(self) -> int:
        s = C.c_uint64()
        check(self.L.cgpu_table_checksum(self.h, C.byref(s)), "cgpu_table_checksum")
        return s.value

    def mirror_save(self, path: str) -> None:
        """cgpu_mirror_save: checkpoint the host mirror (+ counters, CT maps)."""
        check(self.L.cgpu_mirror_save(self.h, str(path).encode()), "cgpu_mirror_save")

    def mirror_restore(self, path: str) -> None:
        """cgpu_mirror_restore into this (empty) context; commit afterwards."""
        check(self.L.cgpu_mirror_restore(self.h, str(path).encode()), "cgpu_mirror_restore")

    def verify(self) -> None:
        """cgpu_table_verify: the device tables still equal the host images
        (raises CgpuError EIO naming the group otherwise)."""
        check(self.L.cgpu_table_verify(self.h), "cgpu_table_verify")

    TABLES = ("ipcache", "policy", "prefilter", "endpoint", "lb4", "lxc", "lb6", "ct4", "ct6")

    def table_bytes(self) -> dict:
        """cgpu_table_bytes: device bytes of each table group of the published
        snapshot and of the conntrack maps."""
        out = np.zeros(len(self.TABLES), np.uint64)
        check(self.L.cgpu_table_bytes(self.h, out.ctypes.data_as(C.c_void_p)), "cgpu_table_bytes")
        return {k: int(v) for k, v in zip(self.TABLES, out)}

    def counter_layout_checksum(self) -> int:
        s = C.c_uint64()
        check(self.L.cgpu_counter_layout_checksum(self.h, C.byref(s)), "cgpu_counter_layout_checksum")
        return s.value

    # -------------------------------------------------------------- batches
    PATH_PLAIN, PATH_LB, PATH_CASCADE = 0, 1, 2

    def _classify_tun(self, v6: bool, path: int, t: dict, out, stage, stream):
        """cgpu_classify_v4_tun / _v6_tun: the stateless call `path` names
        with out["tunnel"] (int32 holding the raw u32) as one more output:
        the tunnel_endpoint of the ipcache entry an egress tuple's identity
        came from, 0 elsewhere (include/cgpu.h).  Needs
        Engine(ipcache_tunnel=1)."""
        import torch
        n = t["flags"].numel()
        dev = t["flags"].device
        if out is None:
            out = {"verdict": torch.empty(n, dtype=torch.int32, device=dev),
                   "identity": torch.empty(n, dtype=torch.int32, device=dev),
                   "stage": torch.empty(n, dtype=torch.uint8, device=dev) if stage else None}
        if out.get("tunnel") is None:
            out["tunnel"] = torch.empty(n, dtype=torch.int32, device=dev)
        tv = (TuplesV6 if v6 else TuplesV4)(*[t[k].data_ptr() for k in
                                              ("saddr", "daddr", "dport", "proto", "flags", "len", "ep")])
        fn = "cgpu_classify_v6_tun" if v6 else "cgpu_classify_v4_tun"
        check(getattr(self.L, fn)(self.h, C.byref(tv), _ptr(t.get("sport")), _ptr(t.get("hash")), path, n,
                                  _ptr(out["verdict"]), _ptr(out["identity"]), _ptr(out.get("stage")),
                                  _ptr(out["tunnel"]), _stream(stream)), fn)
        return out

    def classify_v4(self, t: dict, out: dict | None = None, stage: bool = True, stream=None,
                    tunnel: bool = False, forward: dict | None = None, deliver: bool = False):
        """t: dict of CUDA tensors saddr/daddr (int32 view of network-order
        u32), dport (int16), proto/flags (uint8), len (int32), ep (int16).
        tunnel=True: out["tunnel"] too (_classify_tun).  forward=<dict of
        forward_v4's mode / encap / ipv4_mask / host_ifindex / encap_ifindex>:
        the tunnel form, then the forwarding step on its outputs into
        out["fwd_action"], ["fwd_ret"], ["fwd_ifindex"], ["fwd_arg"]
        (_forward_into; t may hold "ttl").  deliver=True (only with forward=
        in FWD_LXC mode): then the destination endpoint's ingress policy for
        the LOCAL packets, with t["ep"] as the sender, into out["dlv_verdict"],
        ["dlv_identity"], ["dlv_stage"] (_deliver_into)."""
        self._check_deliver(deliver, forward)
        if forward is not None:
            out = self._classify_tun(False, self.PATH_PLAIN, t, out, stage, stream)
            out = self._forward_into(False, t, out, forward, stream)
            return self._deliver_into(False, t, out, stream) if deliver else out
        if tunnel:
            return self._classify_tun(False, self.PATH_PLAIN, t, out, stage, stream)
        import torch
        n = t["saddr"].numel()
        dev = t["saddr"].device
        if out is None:
            out = {"verdict": torch.empty(n, dtype=torch.int32, device=dev),
                   "identity": torch.empty(n, dtype=torch.int32, device=dev),
                   "stage": torch.empty(n, dtype=torch.uint8, device=dev) if stage else None}
        tv = TuplesV4(*[t[k].data_ptr() for k in
                        ("saddr", "daddr", "dport", "proto", "flags", "len", "ep")])
        check(self.L.cgpu_classify_v4(self.h, C.byref(tv), n, _ptr(out["verdict"]),
                                      _ptr(out["identity"]), _ptr(out.get("stage")),
                                      _stream(stream)), "cgpu_classify_v4")
        return out

    @staticmethod
    def _hptr(x):
        if x is None:
            return None
        return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data)

    def _host_call(self, fn, tv_cls, t, n, out, stage, stream, lb):
        """The host-resident classify entry points: t holds HOST arrays
        (numpy, or CPU tensors -- page-locked ones overlap the copies with
        the classify) with the dtypes of the device call; outputs are host
        numpy arrays, complete when `stream` is (the call synchronizes it
        before returning unless out is given)."""
        p = self._hptr
        given = out is not None
        if out is None:
            out = {"verdict": np.empty(n, np.int32), "identity": np.empty(n, np.uint32),
                   "stage": np.empty(n, np.uint8) if stage else None}
        tv = tv_cls(*[p(t[k]).value for k in ("saddr", "daddr", "dport", "proto", "flags", "len", "ep")])
        lbargs = (p(t.get("sport")), p(t.get("hash"))) if lb else ()
        check(getattr(self.L, fn)(self.h, C.byref(tv), *lbargs, n, p(out["verdict"]),
                                  p(out["identity"]), p(out.get("stage")), _stream(stream)), fn)
        if not given:
            import torch
            (stream or torch.cuda.current_stream()).synchronize()
        return out

    def classify_v4_host(self, t: dict, out: dict | None = None, stage: bool = True, stream=None):
        """cgpu_classify_v4_host: classify_v4 over host arrays (_host_call)."""
        return self._host_call("cgpu_classify_v4_host", TuplesV4, t, len(t["saddr"]), out, stage,
                               stream, False)

    def classify_v4_lb_host(self, t: dict, out: dict | None = None, stage: bool = True, stream=None,
                            xdp: bool = False):
        """cgpu_classify_v4_lb_host / cgpu_classify_v4_cascade_host (xdp):
        classify_v4_lb over host arrays; t holds "hash" or "sport" too."""
        fn = "cgpu_classify_v4_cascade_host" if xdp else "cgpu_classify_v4_lb_host"
        return self._host_call(fn, TuplesV4, t, len(t["saddr"]), out, stage, stream, True)

    def classify_v6_host(self, t: dict, out: dict | None = None, stage: bool = True, stream=None,
                         lb: bool = False):
        """cgpu_classify_v6_host / cgpu_classify_v6_lb_host (lb): classify_v6
        over host arrays (saddr / daddr (n, 16) uint8, any alignment)."""
        fn = "cgpu_classify_v6_lb_host" if lb else "cgpu_classify_v6_host"
        return self._host_call(fn, TuplesV6, t, len(t["flags"]), out, stage, stream, lb)

    def prefilter_host(self, saddr, daddr, flags, v6: bool = False, out=None, stream=None):
        """cgpu_prefilter_v4_host / _v6_host over host arrays; returns the
        verdict bytes (synchronizes `stream` unless out is given)."""
        p = self._hptr
        given = out is not None
        if out is None:
            out = np.empty(len(flags), np.uint8)
        fn = "cgpu_prefilter_v6_host" if v6 else "cgpu_prefilter_v4_host"
        check(getattr(self.L, fn)(self.h, p(saddr), p(daddr), p(flags), len(flags), p(out),
                                  _stream(stream)), fn)
        if not given:
            import torch
            (stream or torch.cuda.current_stream()).synchronize()
        return out

    def _ct_tun(self, v6: bool, t: dict, now: int, out, stage, stream):
        """cgpu_classify_v4_ct_tun / _v6_ct_tun: the plain stateful call with
        out["tunnel"] (int32 holding the raw u32), the forward tuple's tunnel
        endpoint (include/cgpu.h).  Needs Engine(ipcache_tunnel=1)."""
        import torch
        n = t["flags"].numel()
        dev = t["flags"].device
        if out is None:
            out = {"verdict": torch.empty(n, dtype=torch.int32, device=dev),
                   "ct_ret": torch.empty(n, dtype=torch.uint8, device=dev),
                   "identity": torch.empty(n, dtype=torch.int32, device=dev),
                   "stage": torch.empty(n, dtype=torch.uint8, device=dev) if stage else None}
        if out.get("tunnel") is None:
            out["tunnel"] = torch.empty(n, dtype=torch.int32, device=dev)
        tv = (TuplesV6Ct if v6 else TuplesV4Ct)(*[t[k].data_ptr() for k in (
            "saddr", "daddr", "sport", "dport", "proto", "l4b", "flags", "len", "ep")])
        fn = "cgpu_classify_v6_ct_tun" if v6 else "cgpu_classify_v4_ct_tun"
        check(getattr(self.L, fn)(self.h, C.byref(tv), n, now, _ptr(out["verdict"]), _ptr(out["ct_ret"]),
                                  _ptr(out["identity"]), _ptr(out.get("stage")), _ptr(out["tunnel"]),
                                  _stream(stream)), fn)
        return out

    def classify_v4_ct(self, t: dict, now: int, out: dict | None = None, stage: bool = True,
                       stream=None, tunnel: bool = False, rev_nat: bool = False,
                       forward: dict | None = None, deliver: bool = False):
        """Stateful classification (cgpu_classify_v4_ct): t holds CUDA tensors
        saddr/daddr (int32), sport/dport (int16, network order), proto/flags
        (uint8), l4b (int16: TCP header bytes 12-13 / ICMP type), len (int32),
        ep (int16); now = bpf_ktime_get_sec() of the batch.
        tunnel=True: out["tunnel"] too (_ct_tun).  rev_nat=True
        (cgpu_classify_v4_ct_rnat): out["rn_saddr"], ["rn_daddr"] (int32),
        ["rn_sport"] (int16), ["rn_applied"] (uint8), the frame after the
        replies' reverse NAT.  forward=: as classify_v4, on the tunnel form;
        deliver=True raises (the conntrack form of the delivery step is not
        built)."""
        self._no_deliver_ct(deliver, "classify_v4_ct")
        if (tunnel or forward is not None) and rev_nat:
            raise ValueError("tunnel / forward and rev_nat cannot be combined")
        if forward is not None:
            out = self._ct_tun(False, t, now, out, stage, stream)
            return self._forward_into(False, t, out, forward, stream)
        if tunnel:
            return self._ct_tun(False, t, now, out, stage, stream)
        import torch
        n = t["saddr"].numel()
        dev = t["saddr"].device
        if out is None:
            out = {"verdict": torch.empty(n, dtype=torch.int32, device=dev),
                   "ct_ret": torch.empty(n, dtype=torch.uint8, device=dev),
                   "identity": torch.empty(n, dtype=torch.int32, device=dev),
                   "stage": torch.empty(n, dtype=torch.uint8, device=dev) if stage else None}
        tv = TuplesV4Ct(*[t[k].data_ptr() for k in
                          ("saddr", "daddr", "sport", "dport", "proto", "l4b", "flags", "len", "ep")])
        if rev_nat:
            rn = self._rnat_out(False, out, n, dev)
            check(self.L.cgpu_classify_v4_ct_rnat(self.h, C.byref(tv), n, now, _ptr(out["verdict"]),
                                                  _ptr(out["ct_ret"]), _ptr(out["identity"]),
                                                  _ptr(out.get("stage")), C.byref(rn), _stream(stream)),
                  "cgpu_classify_v4_ct_rnat")
            return out
        check(self.L.cgpu_classify_v4_ct(self.h, C.byref(tv), n, now, _ptr(out["verdict"]),
                                         _ptr(out["ct_ret"]), _ptr(out["identity"]),
                                         _ptr(out.get("stage")), _stream(stream)),
              "cgpu_classify_v4_ct")
        return out

    @staticmethod
    def _rnat_out(v6: bool, out: dict, n: int, dev):
        """The rev_nat=True outputs into `out` (allocated unless given) and
        their cgpu_rnat4_out / cgpu_rnat6_out."""
        import torch
        if out.get("rn_saddr") is None:
            out["rn_saddr"] = torch.empty((n, 16), dtype=torch.uint8, device=dev) if v6 else \
                torch.empty(n, dtype=torch.int32, device=dev)
        if not v6 and out.get("rn_daddr") is None:
            out["rn_daddr"] = torch.empty(n, dtype=torch.int32, device=dev)
        if out.get("rn_sport") is None:
            out["rn_sport"] = torch.empty(n, dtype=torch.int16, device=dev)
        if out.get("rn_applied") is None:
            out["rn_applied"] = torch.empty(n, dtype=torch.uint8, device=dev)
        if v6:
            return Rnat6Out(*[out[k].data_ptr() for k in ("rn_saddr", "rn_sport", "rn_applied")])
        return Rnat4Out(*[out[k].data_ptr() for k in ("rn_saddr", "rn_daddr", "rn_sport", "rn_applied")])

    def classify_v4_ctlb(self, t: dict, now: int, out: dict | None = None, stage: bool = True,
                         xlate: bool = True, stream=None, rev_nat: bool = False, forward=None):
        """cgpu_classify_v4_ctlb: classify_v4_ct with the stateful service
        step (lb4_local with CONNTRACK) in front; t may carry a "hash" column
        (skb->hash, int32).  out adds "daddr" / "dport": the frame after the
        service step (xlate=False: not written)."""
        self._no_forward(forward, "classify_v4_ctlb")
        import torch
        n = t["saddr"].numel()
        dev = t["saddr"].device
        if out is None:
            out = {"verdict": torch.empty(n, dtype=torch.int32, device=dev),
                   "ct_ret": torch.empty(n, dtype=torch.uint8, device=dev),
                   "identity": torch.empty(n, dtype=torch.int32, device=dev),
                   "stage": torch.empty(n, dtype=torch.uint8, device=dev) if stage else None,
                   "daddr": torch.empty(n, dtype=torch.int32, device=dev) if xlate else None,
                   "dport": torch.empty(n, dtype=torch.int16, device=dev) if xlate else None}
        tv = TuplesV4Ct(*[t[k].data_ptr() for k in
                          ("saddr", "daddr", "sport", "dport", "proto", "l4b", "flags", "len", "ep")])
        ov = CtlbOut(*[_ptr(out.get(k)) for k in ("verdict", "ct_ret", "identity", "stage", "daddr",
                                                   "dport")])
        if rev_nat:  # cgpu_classify_v4_ctlb_rnat: out["rn_*"] as classify_v4_ct
            rn = self._rnat_out(False, out, n, dev)
            check(self.L.cgpu_classify_v4_ctlb_rnat(self.h, C.byref(tv), _ptr(t.get("hash")), n, now,
                                                    C.byref(ov), C.byref(rn), _stream(stream)),
                  "cgpu_classify_v4_ctlb_rnat")
            return out
        check(self.L.cgpu_classify_v4_ctlb(self.h, C.byref(tv), _ptr(t.get("hash")), n, now,
                                           C.byref(ov), _stream(stream)), "cgpu_classify_v4_ctlb")
        return out

    def classify_v6_ct(self, t: dict, now: int, out: dict | None = None, stage: bool = True,
                       stream=None, tunnel: bool = False, rev_nat: bool = False,
                       forward: dict | None = None, deliver: bool = False):
        """cgpu_classify_v6_ct: as classify_v4_ct with saddr / daddr (n, 16)
        uint8 tensors (16-byte aligned rows).  rev_nat=True: out["rn_saddr"]
        (n, 16) uint8, ["rn_sport"], ["rn_applied"] (IPv6 has no rn_daddr)."""
        self._no_deliver_ct(deliver, "classify_v6_ct")
        if (tunnel or forward is not None) and rev_nat:
            raise ValueError("tunnel / forward and rev_nat cannot be combined")
        if forward is not None:
            out = self._ct_tun(True, t, now, out, stage, stream)
            return self._forward_into(True, t, out, forward, stream)
        if tunnel:
            return self._ct_tun(True, t, now, out, stage, stream)
        import torch
        n = t["saddr"].shape[0]
        dev = t["saddr"].device
        if out is None:
            out = {"verdict": torch.empty(n, dtype=torch.int32, device=dev),
                   "ct_ret": torch.empty(n, dtype=torch.uint8, device=dev),
                   "identity": torch.empty(n, dtype=torch.int32, device=dev),
                   "stage": torch.empty(n, dtype=torch.uint8, device=dev) if stage else None}
        tv = TuplesV6Ct(*[t[k].data_ptr() for k in
                          ("saddr", "daddr", "sport", "dport", "proto", "l4b", "flags", "len", "ep")])
        if rev_nat:
            rn = self._rnat_out(True, out, n, dev)
            check(self.L.cgpu_classify_v6_ct_rnat(self.h, C.byref(tv), n, now, _ptr(out["verdict"]),
                                                  _ptr(out["ct_ret"]), _ptr(out["identity"]),
                                                  _ptr(out.get("stage")), C.byref(rn), _stream(stream)),
                  "cgpu_classify_v6_ct_rnat")
            return out
        check(self.L.cgpu_classify_v6_ct(self.h, C.byref(tv), n, now, _ptr(out["verdict"]),
                                         _ptr(out["ct_ret"]), _ptr(out["identity"]),
                                         _ptr(out.get("stage")), _stream(stream)),
              "cgpu_classify_v6_ct")
        return out

    def classify_v6_ctlb(self, t: dict, now: int, out: dict | None = None, stage: bool = True,
                         xlate: bool = True, stream=None, rev_nat: bool = False, forward=None):
        """cgpu_classify_v6_ctlb: classify_v6_ct with the stateful service
        step (lb6_local with CONNTRACK) in front; out "daddr" is (n, 16)
        uint8."""
        self._no_forward(forward, "classify_v6_ctlb")
        import torch
        n = t["saddr"].shape[0]
        dev = t["saddr"].device
        if out is None:
            out = {"verdict": torch.empty(n, dtype=torch.int32, device=dev),
                   "ct_ret": torch.empty(n, dtype=torch.uint8, device=dev),
                   "identity": torch.empty(n, dtype=torch.int32, device=dev),
                   "stage": torch.empty(n, dtype=torch.uint8, device=dev) if stage else None,
                   "daddr": torch.empty((n, 16), dtype=torch.uint8, device=dev) if xlate else None,
                   "dport": torch.empty(n, dtype=torch.int16, device=dev) if xlate else None}
        tv = TuplesV6Ct(*[t[k].data_ptr() for k in
                          ("saddr", "daddr", "sport", "dport", "proto", "l4b", "flags", "len", "ep")])
        ov = CtlbOut(*[_ptr(out.get(k)) for k in ("verdict", "ct_ret", "identity", "stage", "daddr",
                                                   "dport")])
        if rev_nat:  # cgpu_classify_v6_ctlb_rnat: out["rn_*"] as classify_v6_ct
            rn = self._rnat_out(True, out, n, dev)
            check(self.L.cgpu_classify_v6_ctlb_rnat(self.h, C.byref(tv), _ptr(t.get("hash")), n, now,
                                                    C.byref(ov), C.byref(rn), _stream(stream)),
                  "cgpu_classify_v6_ctlb_rnat")
            return out
        check(self.L.cgpu_classify_v6_ctlb(self.h, C.byref(tv), _ptr(t.get("hash")), n, now,
                                           C.byref(ov), _stream(stream)), "cgpu_classify_v6_ctlb")
        return out

    def classify_v4_lb(self, t: dict, out: dict | None = None, stage: bool = True, stream=None,
                       xdp: bool = False, tunnel: bool = False, forward=None):
        """classify_v4 with the egress service step first (BASELINE config 5).
        t additionally holds "hash" (int32 view of skb->hash) or "sport".
        xdp=True: cgpu_classify_v4_cascade, the netdev's XDP prefilter before
        every ingress tuple too (the full config-5 cascade).
        tunnel=True: out["tunnel"] too (_classify_tun)."""
        self._no_forward(forward, "classify_v4_cascade" if xdp else "classify_v4_lb")
        if tunnel:
            return self._classify_tun(False, self.PATH_CASCADE if xdp else self.PATH_LB, t, out, stage,
                                      stream)
        import torch
        n = t["saddr"].numel()
        dev = t["saddr"].device
        if out is None:
            out = {"verdict": torch.empty(n, dtype=torch.int32, device=dev),
                   "identity": torch.empty(n, dtype=torch.int32, device=dev),
                   "stage": torch.empty(n, dtype=torch.uint8, device=dev) if stage else None}
        tv = TuplesV4(*[t[k].data_ptr() for k in
                        ("saddr", "daddr", "dport", "proto", "flags", "len", "ep")])
        fn = "cgpu_classify_v4_cascade" if xdp else "cgpu_classify_v4_lb"
        check(getattr(self.L, fn)(self.h, C.byref(tv), _ptr(t.get("sport")), _ptr(t.get("hash")), n,
                                  _ptr(out["verdict"]), _ptr(out["identity"]), _ptr(out.get("stage")),
                                  _stream(stream)), fn)
        return out

    def classify_v4_cascade(self, t: dict, out: dict | None = None, stage: bool = True, stream=None,
                            tunnel: bool = False, forward=None):
        """BASELINE config 5 whole (cgpu_classify_v4_cascade): XDP prefilter
        -> ipcache -> policy for ingress tuples, service step -> ipcache ->
        policy for egress ones."""
        return self.classify_v4_lb(t, out=out, stage=stage, stream=stream, xdp=True, tunnel=tunnel,
                                   forward=forward)

    def lb4_select(self, t: dict, mode: int, out: dict | None = None, stream=None):
        """Service translation alone: t holds saddr/daddr (int32 views),
        dport/sport (int16 views), proto (uint8), optional hash (int32)."""
        import torch
        n = t["daddr"].numel()
        dev = t["daddr"].device
        if out is None:
            out = {"ret": torch.empty(n, dtype=torch.int32, device=dev),
                   "saddr": torch.empty(n, dtype=torch.int32, device=dev),
                   "daddr": torch.empty(n, dtype=torch.int32, device=dev),
                   "dport": torch.empty(n, dtype=torch.int16, device=dev),
                   "rev_nat": torch.empty(n, dtype=torch.int16, device=dev),
                   "slave": torch.empty(n, dtype=torch.int16, device=dev)}
        tv = Lb4Tuples(*[_ptr(t.get(k)) for k in ("saddr", "daddr", "sport", "dport", "proto",
                                                  "hash")])
        ov = Lb4Out(*[_ptr(out.get(k)) for k in ("ret", "saddr", "daddr", "dport", "rev_nat",
                                                 "slave")])
        check(self.L.cgpu_lb4_select(self.h, mode, C.byref(tv), n, C.byref(ov), _stream(stream)),
              "cgpu_lb4_select")
        return out

    def classify_v6(self, t: dict, out: dict | None = None, stage: bool = True, stream=None,
                    tunnel: bool = False, forward: dict | None = None, deliver: bool = False):
        """t: saddr/daddr uint8 CUDA tensors of shape (n, 16) (16-byte
        aligned), the other columns as classify_v4 (forward= and deliver=
        too)."""
        self._check_deliver(deliver, forward)
        if forward is not None:
            out = self._classify_tun(True, self.PATH_PLAIN, t, out, stage, stream)
            out = self._forward_into(True, t, out, forward, stream)
            return self._deliver_into(True, t, out, stream) if deliver else out
        if tunnel:
            return self._classify_tun(True, self.PATH_PLAIN, t, out, stage, stream)
        import torch
        n = t["flags"].numel()
        dev = t["flags"].device
        if out is None:
            out = {"verdict": torch.empty(n, dtype=torch.int32, device=dev),
                   "identity": torch.empty(n, dtype=torch.int32, device=dev),
                   "stage": torch.empty(n, dtype=torch.uint8, device=dev) if stage else None}
        tv = TuplesV6(*[t[k].data_ptr() for k in
                        ("saddr", "daddr", "dport", "proto", "flags", "len", "ep")])
        check(self.L.cgpu_classify_v6(self.h, C.byref(tv), n, _ptr(out["verdict"]),
                                      _ptr(out["identity"]), _ptr(out.get("stage")),
                                      _stream(stream)), "cgpu_classify_v6")
        return out

    def classify_v6_lb(self, t: dict, out: dict | None = None, stage: bool = True, stream=None,
                       tunnel: bool = False, forward=None):
        """classify_v6 with the egress service step of ipv6_l3_from_lxc first;
        t additionally holds "hash" (int32 view of skb->hash) or "sport"."""
        self._no_forward(forward, "classify_v6_lb")
        if tunnel:
            return self._classify_tun(True, self.PATH_LB, t, out, stage, stream)
        import torch
        n = t["flags"].numel()
        dev = t["flags"].device
        if out is None:
            out = {"verdict": torch.empty(n, dtype=torch.int32, device=dev),
                   "identity": torch.empty(n, dtype=torch.int32, device=dev),
                   "stage": torch.empty(n, dtype=torch.uint8, device=dev) if stage else None}
        tv = TuplesV6(*[t[k].data_ptr() for k in
                        ("saddr", "daddr", "dport", "proto", "flags", "len", "ep")])
        check(self.L.cgpu_classify_v6_lb(self.h, C.byref(tv), _ptr(t.get("sport")),
                                         _ptr(t.get("hash")), n, _ptr(out["verdict"]),
                                         _ptr(out["identity"]), _ptr(out.get("stage")),
                                         _stream(stream)), "cgpu_classify_v6_lb")
        return out

    def ipcache_lookup_batch(self, addr, tunnel: bool | None = None, stream=None):
        """cgpu_ipcache_lookup_v4 / _v6: ipcache_lookup4 / 6 (eps.h:56-80) of a
        batch of addresses on the device.  addr: a uint32 / int32 CUDA tensor
        (network-order IPv4) or an (n, 16) uint8 one (IPv6, any alignment).
        Returns {"found" (uint8; a tombstone is found), "sec_label",
        "tunnel"} -- int32 tensors holding the raw u32 words; "tunnel" is
        None without Engine(ipcache_tunnel=1) (tunnel=True asks for it
        regardless: -EINVAL there)."""
        import torch
        v6 = addr.dtype == torch.uint8
        if v6:
            assert addr.dim() == 2 and addr.shape[1] == 16 and addr.stride(1) == 1 and \
                (addr.shape[0] < 2 or addr.stride(0) == 16), "IPv6 addresses: dense (n, 16) uint8"
        else:
            assert addr.dtype in (torch.int32, torch.uint32) and addr.is_contiguous(), \
                "IPv4 addresses: a contiguous 32-bit tensor"
        n = addr.shape[0]
        if tunnel is None:
            tunnel = bool(self.cfg.ipcache_tunnel)
        out = {"found": torch.empty(n, dtype=torch.uint8, device=addr.device),
               "sec_label": torch.empty(n, dtype=torch.int32, device=addr.device),
               "tunnel": torch.empty(n, dtype=torch.int32, device=addr.device) if tunnel else None}
        fn = "cgpu_ipcache_lookup_v6" if v6 else "cgpu_ipcache_lookup_v4"
        check(getattr(self.L, fn)(self.h, _ptr(addr), n, _ptr(out["found"]), _ptr(out["sec_label"]),
                                  _ptr(out["tunnel"]), _stream(stream)), fn)
        return out

    FWD_LXC, FWD_NETDEV = L.FWD_LXC, L.FWD_NETDEV
    _FWD_KEYS = ("mode", "encap", "ipv4_mask", "host_ifindex", "encap_ifindex")

    def _forward(self, v6: bool, daddr, verdict, tunnel, flags, ttl, mode, encap, ipv4_mask, host_ifindex,
                 encap_ifindex, out, stream):
        import torch
        n = daddr.shape[0]
        dev = daddr.device
        if out is None:
            out = {"action": torch.empty(n, dtype=torch.uint8, device=dev),
                   "ret": torch.empty(n, dtype=torch.int32, device=dev),
                   "ifindex": torch.empty(n, dtype=torch.int32, device=dev),
                   "arg": torch.empty(n, dtype=torch.int32, device=dev)}
        p = FwdParams(mode, L.FWD_ENCAP if encap else 0, ipv4_mask, host_ifindex, encap_ifindex)
        iv = FwdIn(*[x.data_ptr() if x is not None else None for x in (daddr, verdict, tunnel, flags, ttl)])
        ov = FwdOut(*[out[k].data_ptr() if out.get(k) is not None else None
                      for k in ("action", "ret", "ifindex", "arg")])
        fn = "cgpu_forward_v6" if v6 else "cgpu_forward_v4"
        check(getattr(self.L, fn)(self.h, C.byref(p), C.byref(iv), n, C.byref(ov), _stream(stream)), fn)
        return out

    def forward_v4(self, daddr, verdict=None, tunnel=None, flags=None, ttl=None, mode=L.FWD_LXC,
                   encap=True, ipv4_mask=0xffff, host_ifindex=1, encap_ifindex=1, out=None, stream=None):
        """cgpu_forward_v4: where each packet of an allowed batch goes
        (include/cgpu.h has the decision lists).  daddr: int32 / uint32 CUDA
        tensor as it leaves the classify step; verdict (int32) and flags
        (uint8) of that step (FWD_NETDEV reads neither); tunnel: the raw
        tunnel_endpoint words (int32 / uint32; None = all 0); ttl (uint8; None
        = never expired).  Returns {"action" (uint8, L.FWD_*), "ret",
        "ifindex", "arg"} (int32 tensors holding the raw words); a given `out`
        may leave any of the last three None."""
        return self._forward(False, daddr, verdict, tunnel, flags, ttl, mode, encap, ipv4_mask,
                             host_ifindex, encap_ifindex, out, stream)

    def forward_v6(self, daddr, verdict=None, tunnel=None, flags=None, ttl=None, mode=L.FWD_LXC,
                   encap=True, ipv4_mask=0xffff, host_ifindex=1, encap_ifindex=1, out=None, stream=None):
        """cgpu_forward_v6: forward_v4 with daddr an (n, 16) uint8 tensor at
        any alignment and ttl the hop limit."""
        return self._forward(True, daddr, verdict, tunnel, flags, ttl, mode, encap, ipv4_mask,
                             host_ifindex, encap_ifindex, out, stream)

    def forward_table_bytes(self) -> dict:
        """cgpu_forward_table_bytes: device bytes of the forwarding tables (all
        0 while they are not built)."""
        b = (C.c_uint64 * 4)()
        check(self.L.cgpu_forward_table_bytes(self.h, b), "cgpu_forward_table_bytes")
        return dict(zip(("endpoints4", "endpoints6", "tunnel4", "tunnel6"), (int(x) for x in b)))

    def _forward_into(self, v6: bool, t: dict, out: dict, forward: dict, stream):
        """forward=<forward_v4's keyword parameters> of a classify call: the
        forwarding step on the call's own daddr, verdict, tunnel and flags
        (and t["ttl"] when present), into out["fwd_*"]."""
        bad = set(forward) - set(self._FWD_KEYS)
        if bad:
            raise TypeError(f"unknown forward parameter(s) {sorted(bad)}")
        given = {k: out.get("fwd_" + k) for k in ("action", "ret", "ifindex", "arg")}
        f = (self.forward_v6 if v6 else self.forward_v4)(
            t["daddr"], verdict=out["verdict"], tunnel=out["tunnel"], flags=t["flags"], ttl=t.get("ttl"),
            out=given if given["action"] is not None else None, stream=stream, **forward)
        for k, v in f.items():
            out["fwd_" + k] = v
        return out

    def _deliver(self, v6: bool, action, arg, dport, proto, flags, len, src_label, src_ep, out, stream):
        import torch
        if (src_label is None) == (src_ep is None):
            raise ValueError("exactly one of src_label and src_ep is needed")
        n = action.numel()
        dev = action.device
        if out is None:
            out = {"verdict": torch.empty(n, dtype=torch.int32, device=dev),
                   "identity": torch.empty(n, dtype=torch.int32, device=dev),
                   "stage": torch.empty(n, dtype=torch.uint8, device=dev)}
        iv = DlvIn(*[x.data_ptr() if x is not None else None
                     for x in (action, arg, src_label, src_ep, dport, proto, flags, len)])
        ov = DlvOut(*[out[k].data_ptr() if out.get(k) is not None else None
                      for k in ("verdict", "identity", "stage")])
        fn = "cgpu_deliver_v6" if v6 else "cgpu_deliver_v4"
        check(getattr(self.L, fn)(self.h, C.byref(iv), n, C.byref(ov), _stream(stream)), fn)
        return out

    def deliver_v4(self, action, arg, dport, proto, flags, len, src_label=None, src_ep=None, out=None,
                   stream=None):
        """cgpu_deliver_v4: the destination endpoint's ingress policy for the
        packets a forwarding step marked FWD_LOCAL (include/cgpu.h).  action
        (uint8) and arg (int32 / uint32) are that step's outputs; dport
        (int16), proto / flags (uint8) and len (int32) the classify call's
        columns; the label per packet is src_label (int32 / uint32) or the
        SECLABEL of the endpoint id src_ep (int16) -- exactly one of the two.
        Returns {"verdict", "identity" (int32), "stage" (uint8)}; packets that
        are not LOCAL read (0, 0, L.STAGE_NOT_LOCAL).  A given `out` may
        leave identity and stage None."""
        return self._deliver(False, action, arg, dport, proto, flags, len, src_label, src_ep, out, stream)

    def deliver_v6(self, action, arg, dport, proto, flags, len, src_label=None, src_ep=None, out=None,
                   stream=None):
        """cgpu_deliver_v6: deliver_v4 for IPv6 packets (ICMPv6 passes the
        protocol gate, the fragment bit is not read)."""
        return self._deliver(True, action, arg, dport, proto, flags, len, src_label, src_ep, out, stream)

    def _deliver_into(self, v6: bool, t: dict, out: dict, stream):
        """deliver=True of a classify call: the delivery step on the call's
        own fwd_action / fwd_arg and dport, proto, flags, len, with t["ep"] as
        the sending endpoint, into out["dlv_*"]."""
        if out.get("fwd_arg") is None:
            raise ValueError("deliver=True needs the forwarding step's arg output (out['fwd_arg'])")
        given = {k: out.get("dlv_" + k) for k in ("verdict", "identity", "stage")}
        d = (self.deliver_v6 if v6 else self.deliver_v4)(
            out["fwd_action"], out["fwd_arg"], t["dport"], t["proto"], t["flags"], t["len"], src_ep=t["ep"],
            out=given if given["verdict"] is not None else None, stream=stream)
        for k, v in d.items():
            out["dlv_" + k] = v
        return out

    @staticmethod
    def _check_deliver(deliver, forward):
        if deliver and (forward is None or forward.get("mode", L.FWD_LXC) != L.FWD_LXC):
            raise ValueError("deliver=True needs forward= in FWD_LXC mode: the delivery step runs on that "
                             "step's LOCAL packets with the sending endpoint's label")

    @staticmethod
    def _no_deliver_ct(deliver, what: str):
        if deliver:
            raise ValueError(f"{what} has no deliver= form: the conntrack form of the delivery step "
                             "(its CT_INGRESS lookups and creates) is not built")

    @staticmethod
    def _no_forward(forward, what: str):
        if forward is not None:
            raise ValueError(f"{what} has no forward= form: the translated daddr and the tunnel endpoint "
                             "are not outputs of the service paths")

    def prefilter_v4(self, saddr, daddr, flags, out=None, stream=None):
        import torch
        n = flags.numel()
        if out is None:
            out = torch.empty(n, dtype=torch.uint8, device=flags.device)
        check(self.L.cgpu_prefilter_v4(self.h, _ptr(saddr), _ptr(daddr), _ptr(flags), n,
                                       _ptr(out), _stream(stream)), "cgpu_prefilter_v4")
        return out

    def prefilter_v6(self, saddr16, daddr16, flags, out=None, stream=None):
        import torch
        n = flags.numel()
        if out is None:
            out = torch.empty(n, dtype=torch.uint8, device=flags.device)
        check(self.L.cgpu_prefilter_v6(self.h, _ptr(saddr16), _ptr(daddr16), _ptr(flags), n,
                                       _ptr(out), _stream(stream)), "cgpu_prefilter_v6")
        return out

    # ---------------------------------------------------------- raw frames
    def lxc_update(self, ep: int, info) -> int:
        """info: a layouts.LXC_INFO record (lxc_config.h of endpoint ep)."""
        return check(self.L.cgpu_lxc_update(self.h, ep, _buf(info)), "cgpu_lxc_update")

    def lxc_delete(self, ep: int) -> int:
        return self.L.cgpu_lxc_delete(self.h, ep)

    def lxc_lookup(self, ep: int):
        out = np.zeros((), L.LXC_INFO)
        rc = self.L.cgpu_lxc_lookup(self.h, ep, out.ctypes.data_as(C.c_void_p))
        return None if rc == -errno.ENOENT else (check(rc, "cgpu_lxc_lookup"), out)[1]

    @staticmethod
    def _frames(f: dict) -> Frames:
        data = f["data"]
        assert data.dim() == 2 and data.is_contiguous()
        return Frames(data.data_ptr(), f["len"].data_ptr(), f["flags"].data_ptr(),
                      f["ep"].data_ptr(), data.shape[1], 0)

    def frames_parse(self, f: dict, out: dict | None = None, stream=None):
        """f: CUDA tensors data (n, stride) uint8, len int32, flags uint8,
        ep int16.  Returns the policy tuple columns (cgpu_frames_parse)."""
        import torch
        n = f["len"].numel()
        dev = f["len"].device
        if out is None:
            out = {"status": torch.empty(n, dtype=torch.int32, device=dev),
                   "family": torch.empty(n, dtype=torch.uint8, device=dev),
                   "saddr": torch.empty((n, 16), dtype=torch.uint8, device=dev),
                   "daddr": torch.empty((n, 16), dtype=torch.uint8, device=dev),
                   "dport": torch.empty(n, dtype=torch.int16, device=dev),
                   "proto": torch.empty(n, dtype=torch.uint8, device=dev),
                   "flags": torch.empty(n, dtype=torch.uint8, device=dev)}
        fr = self._frames(f)
        ot = FrameTuples(*[_ptr(out.get(k)) for k in ("status", "family", "saddr", "daddr",
                                                      "dport", "proto", "flags")])
        check(self.L.cgpu_frames_parse(self.h, C.byref(fr), n, C.byref(ot), _stream(stream)),
              "cgpu_frames_parse")
        return out

    def frames_parse_ct(self, f: dict, out: dict | None = None, stream=None):
        """cgpu_frames_parse_ct: the frames' columns for the stateful path.
        f as frames_parse.  Returns status, family, saddr / daddr ((n, 16)
        uint8), sport / dport (int16: the wire ports as loaded), proto, l4b
        (int16: TCP header bytes 12-13 / the ICMP type, the conntrack dicts'
        name for cgpu_tuples_v4_ct.l4) and flags; a frame with status != 0 has
        sport, dport and l4b of 0.  In a given `out` every key but status may
        be None or missing (that column is not written)."""
        import torch
        n = f["len"].numel()
        dev = f["len"].device
        if out is None:
            out = {"status": torch.empty(n, dtype=torch.int32, device=dev),
                   "family": torch.empty(n, dtype=torch.uint8, device=dev),
                   "saddr": torch.empty((n, 16), dtype=torch.uint8, device=dev),
                   "daddr": torch.empty((n, 16), dtype=torch.uint8, device=dev),
                   "sport": torch.empty(n, dtype=torch.int16, device=dev),
                   "dport": torch.empty(n, dtype=torch.int16, device=dev),
                   "proto": torch.empty(n, dtype=torch.uint8, device=dev),
                   "l4b": torch.empty(n, dtype=torch.int16, device=dev),
                   "flags": torch.empty(n, dtype=torch.uint8, device=dev)}
        fr = self._frames(f)
        ot = FrameCtCols(*[_ptr(out.get(k)) for k in ("status", "family", "saddr", "daddr", "sport", "dport",
                                                      "proto", "l4b", "flags")])
        check(self.L.cgpu_frames_parse_ct(self.h, C.byref(fr), n, C.byref(ot), _stream(stream)),
              "cgpu_frames_parse_ct")
        return out

    def classify_frames_ct(self, f: dict, now: int, out: dict | None = None, stage: bool = True,
                           rev_nat: dict | None = None, stream=None):
        """cgpu_classify_frames_ct: the stateful decision on a mixed batch of
        raw frames, in frame order (include/cgpu.h has the rules).  Returns
        status, family, verdict, ct_ret, identity, stage.  The call waits on
        the host and cannot be captured into a graph.
        rev_nat=dict(rewrite=True | False): the _rnat conntrack calls run, and
        out gains rn_applied, rn_sport, rn_saddr / rn_daddr (int32, the IPv4
        frames') and rn_saddr6 ((n, 16) uint8, the IPv6 frames'); then
        rnat_frames runs once per family on the same frames (with rewrite, the
        default, f["data"] is modified in place; each call leaves the other
        family's frames alone) and out["rn_ret"] holds each frame's ret of its
        family's call, 0 for a frame that is not IP."""
        import torch
        n = f["len"].numel()
        dev = f["len"].device
        if rev_nat is not None:
            bad = set(rev_nat) - {"rewrite"}
            if bad:
                raise TypeError(f"unknown rev_nat parameter(s) {sorted(bad)}")
        if out is None:
            out = {}
        for k, dt in (("status", torch.int32), ("family", torch.uint8), ("verdict", torch.int32),
                      ("ct_ret", torch.uint8), ("identity", torch.int32), ("stage", torch.uint8)):
            if k not in out:
                out[k] = torch.empty(n, dtype=dt, device=dev) if (stage or k != "stage") else None
        if rev_nat is not None:
            for k, dt in (("rn_applied", torch.uint8), ("rn_sport", torch.int16), ("rn_saddr", torch.int32),
                          ("rn_daddr", torch.int32)):
                if out.get(k) is None:
                    out[k] = torch.empty(n, dtype=dt, device=dev)
            if out.get("rn_saddr6") is None:
                out["rn_saddr6"] = torch.empty((n, 16), dtype=torch.uint8, device=dev)
            if out.get("family") is None:  # rn_ret is picked by it
                out["family"] = torch.empty(n, dtype=torch.uint8, device=dev)
        rnk = ("rn_applied", "rn_sport", "rn_saddr", "rn_daddr", "rn_saddr6")
        fr = self._frames(f)
        ov = FctOut(*[_ptr(out.get(k)) for k in ("status", "family", "verdict", "ct_ret", "identity", "stage")],
                    *[_ptr(out.get(k)) if rev_nat is not None else None for k in rnk])
        check(self.L.cgpu_classify_frames_ct(self.h, C.byref(fr), n, now, C.byref(ov), _stream(stream)),
              "cgpu_classify_frames_ct")
        if rev_nat is not None:
            rw = bool(rev_nat.get("rewrite", True))
            r4 = self.rnat_frames(f, out, v6=False, rewrite=rw, stream=stream)["ret"]
            r6 = self.rnat_frames(f, {"rn_applied": out["rn_applied"], "rn_sport": out["rn_sport"],
                                      "rn_saddr": out["rn_saddr6"]}, v6=True, rewrite=rw, stream=stream)["ret"]
            fam = out["family"]
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
                out["rn_ret"] = torch.where(fam == 4, r4, torch.where(fam == 6, r6, torch.zeros_like(r4)))
        return out

    _FWDF_KEYS = _FWD_KEYS + ("host_mac", "rewrite")

    def classify_frames(self, f: dict, out: dict | None = None, stage: bool = True, stream=None,
                        forward: dict | None = None, lb: dict | None = None):
        """Raw frames to verdicts in one pass (cgpu_classify_frames).
        lb=<dict of classify_frames_lb's hash / rewrite>: the egress service
        step first (cgpu_classify_frames_lb; out["lb_ret" / "rev_nat" /
        "slave"] too), which with rewrite (the default) translates f["data"]
        in place; None is the call without the step.
        forward=<forward_frames' keyword parameters mode, encap, ipv4_mask,
        host_ifindex, encap_ifindex, host_mac, rewrite>: then the forwarding
        step on the frames (as translated) with the call's own verdict and
        stage and no tunnel column, into out["fwd_action" / "fwd_ret" /
        "fwd_ifindex" / "fwd_arg"]; with rewrite (the default) f["data"] is
        modified in place."""
        import torch
        n = f["len"].numel()
        dev = f["len"].device
        if forward is not None:
            bad = set(forward) - set(self._FWDF_KEYS)
            if bad:
                raise TypeError(f"unknown forward parameter(s) {sorted(bad)}")
            if not stage and forward.get("mode", L.FWD_LXC) == L.FWD_LXC:
                raise ValueError("forward= in FWD_LXC mode reads the stage output")
        if lb is not None:
            bad = set(lb) - {"hash", "rewrite"}
            if bad:
                raise TypeError(f"unknown lb parameter(s) {sorted(bad)}")
            out = self.classify_frames_lb(f, out=out, stage=stage, stream=stream, **lb)
        else:
            if out is None:
                out = {"verdict": torch.empty(n, dtype=torch.int32, device=dev),
                       "identity": torch.empty(n, dtype=torch.int32, device=dev),
                       "stage": torch.empty(n, dtype=torch.uint8, device=dev) if stage else None}
            fr = self._frames(f)
            check(self.L.cgpu_classify_frames(self.h, C.byref(fr), n, _ptr(out["verdict"]),
                                              _ptr(out["identity"]), _ptr(out.get("stage")),
                                              _stream(stream)), "cgpu_classify_frames")
        if forward is not None:
            given = {k: out.get("fwd_" + k) for k in ("action", "ret", "ifindex", "arg")}
            r = self.forward_frames(f, verdict=out["verdict"], stage=out.get("stage"),
                                    out=given if given["action"] is not None else None, stream=stream, **forward)
            for k, v in r.items():
                out["fwd_" + k] = v
        return out

    def classify_frames_lb(self, f: dict, hash=None, rewrite: bool = True, out: dict | None = None,
                           stage: bool = True, stream=None):
        """cgpu_classify_frames_lb: classify_frames with the stateless egress
        service step on the frame's own fields and, with `rewrite`, the bytes
        lb4_xlate / lb6_xlate store (daddr, the loopback saddr, dport, the
        IPv4 header checksum and the L4 checksum) in f["data"] itself
        (include/cgpu.h has the rules).  hash: the int32 view of skb->hash per
        frame, or None for flow_hash / flow_hash6 of the frame's fields.
        Returns verdict, identity, stage, lb_ret, rev_nat, slave."""
        import torch
        data = f["data"]
        assert data.dim() == 2 and data.is_contiguous()
        n = f["len"].numel()
        dev = data.device
        if out is None:
            out = {}
        for k, dt in (("verdict", torch.int32), ("identity", torch.int32), ("stage", torch.uint8),
                      ("lb_ret", torch.int32), ("rev_nat", torch.int16), ("slave", torch.int16)):
            if k not in out:
                out[k] = torch.empty(n, dtype=dt, device=dev) if (stage or k != "stage") else None
        iv = FlbIn(data.data_ptr(), f["len"].data_ptr(), f["flags"].data_ptr(), f["ep"].data_ptr(),
                   data.shape[1], 0, _ptr(hash))
        ov = FlbOut(_ptr(out.get("lb_ret")), _ptr(out.get("rev_nat")), _ptr(out.get("slave")))
        check(self.L.cgpu_classify_frames_lb(self.h, C.byref(iv), L.FLB_REWRITE if rewrite else 0, n,
                                             _ptr(out["verdict"]), _ptr(out["identity"]), _ptr(out.get("stage")),
                                             C.byref(ov), _stream(stream)), "cgpu_classify_frames_lb")
        return out

    def forward_frames(self, f: dict, verdict=None, stage=None, tunnel=None, mode=L.FWD_LXC, encap=True,
                       ipv4_mask=0xffff, host_ifindex=1, encap_ifindex=1, host_mac=bytes(6), rewrite=True,
                       out=None, stream=None):
        """cgpu_forward_frames: the decision of forward_v4 / _v6 per frame of
        a mixed batch, on the frame's own daddr and ttl / hop limit, and with
        `rewrite` that branch's MAC, ttl / hop limit and IPv4 checksum rewrite
        in f["data"] itself (include/cgpu.h has the table).  f: the dict of
        synth.frames_to_device (data (n, stride) uint8, len, flags; ep is not
        read); verdict (int32) and stage (uint8) are classify_frames' outputs
        (FWD_NETDEV reads neither, nor flags); tunnel: the raw tunnel_endpoint
        words (None = all 0); host_mac: six bytes, the dmac of PROXY / HOST
        frames.  Returns {"action", "ret", "ifindex", "arg"} as forward_v4."""
        import torch
        data = f["data"]
        assert data.dim() == 2 and data.is_contiguous()
        n = f["len"].numel()
        dev = data.device
        if out is None:
            out = {"action": torch.empty(n, dtype=torch.uint8, device=dev),
                   "ret": torch.empty(n, dtype=torch.int32, device=dev),
                   "ifindex": torch.empty(n, dtype=torch.int32, device=dev),
                   "arg": torch.empty(n, dtype=torch.int32, device=dev)}
        host_mac = bytes(host_mac)
        if len(host_mac) != 6:
            raise ValueError("host_mac is six bytes")
        p = FwdfParams(FwdParams(mode, L.FWD_ENCAP if encap else 0, ipv4_mask, host_ifindex, encap_ifindex),
                       (C.c_uint8 * 6)(*host_mac), (C.c_uint8 * 2)(), L.FWDF_REWRITE if rewrite else 0)
        iv = FwdfIn(data.data_ptr(), f["len"].data_ptr(), _ptr(f.get("flags")), data.shape[1], 0,
                    _ptr(verdict), _ptr(stage), _ptr(tunnel))
        ov = FwdOut(*[out[k].data_ptr() if out.get(k) is not None else None
                      for k in ("action", "ret", "ifindex", "arg")])
        check(self.L.cgpu_forward_frames(self.h, C.byref(p), C.byref(iv), n, C.byref(ov), _stream(stream)),
              "cgpu_forward_frames")
        return out

    def rnat_frames(self, f: dict, rn: dict, v6: bool = False, rewrite: bool = True, out: dict | None = None,
                    stream=None):
        """cgpu_rnat_frames_v4 / _v6: the reverse NAT a classify_v4_ct /
        classify_v6_ct(..., rev_nat=True) call decided, written into the
        frames of the same packets: with `rewrite` the sport, saddr (IPv4
        loopback: daddr), the IPv4 header checksum and the L4 checksum in
        f["data"] itself (include/cgpu.h has the rules).  f: the dict of
        synth.frames_to_device (data, len; flags and ep are not read); rn: any
        dict holding rn_applied, rn_saddr, rn_sport and for IPv4 rn_daddr (the
        `out` of those calls goes in as it is).  Returns {"ret"}: 0, or
        DROP_CSUM_L4 / DROP_SNAPLEN for a frame whose L4 checksum field is out
        of reach (out={"ret": None}: no ret column)."""
        import torch
        need = ("rn_applied", "rn_saddr", "rn_sport") + (() if v6 else ("rn_daddr",))
        missing = [k for k in need if rn.get(k) is None]
        if missing:
            raise ValueError(f"rnat_frames needs the column(s) {missing}")
        data = f["data"]
        assert data.dim() == 2 and data.is_contiguous()
        n = f["len"].numel()
        if data.shape[0] != n or any(rn[k].numel() != n * (16 if v6 and k == "rn_saddr" else 1) for k in need):
            raise ValueError("rnat_frames: the frames and the rn columns are not of one batch")
        if out is None:
            out = {"ret": torch.empty(n, dtype=torch.int32, device=data.device)}
        fl = L.RNF_REWRITE if rewrite else 0
        if v6:
            iv = Rnf6In(data.data_ptr(), f["len"].data_ptr(), data.shape[1], 0, rn["rn_applied"].data_ptr(),
                        rn["rn_saddr"].data_ptr(), rn["rn_sport"].data_ptr())
            check(self.L.cgpu_rnat_frames_v6(self.h, C.byref(iv), fl, n, _ptr(out.get("ret")), _stream(stream)),
                  "cgpu_rnat_frames_v6")
        else:
            iv = Rnf4In(data.data_ptr(), f["len"].data_ptr(), data.shape[1], 0, rn["rn_applied"].data_ptr(),
                        rn["rn_saddr"].data_ptr(), rn["rn_daddr"].data_ptr(), rn["rn_sport"].data_ptr())
            check(self.L.cgpu_rnat_frames_v4(self.h, C.byref(iv), fl, n, _ptr(out.get("ret")), _stream(stream)),
                  "cgpu_rnat_frames_v4")
        return out

    def classify_frames_host(self, f: dict, out: dict | None = None, stage: bool = True, stream=None):
        """cgpu_classify_frames_host: f holds HOST arrays (numpy, or CPU
        tensors -- page-locked ones are read by the CUs) data (n, stride)
        uint8, len, flags, ep; outputs are host arrays, complete when
        `stream` is (synchronized here unless out is given)."""
        import numpy as np
        n = len(f["len"])

        def ptr(x):
            if x is None:
                return None
            return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data
        data = f["data"]
        assert data.ndim == 2 if hasattr(data, "ndim") else data.dim() == 2
        given = out is not None
        if out is None:
            out = {"verdict": np.empty(n, np.int32), "identity": np.empty(n, np.uint32),
                   "stage": np.empty(n, np.uint8) if stage else None}
        fr = Frames(ptr(data), ptr(f["len"]), ptr(f["flags"]), ptr(f["ep"]), data.shape[1], 0)
        check(self.L.cgpu_classify_frames_host(self.h, C.byref(fr), n, C.c_void_p(ptr(out["verdict"])),
                                               C.c_void_p(ptr(out["identity"])),
                                               C.c_void_p(ptr(out.get("stage"))), _stream(stream)),
              "cgpu_classify_frames_host")
        if not given:
            import torch
            (stream or torch.cuda.current_stream()).synchronize()
        return out

    def host_stage_release(self) -> None:
        """cgpu_host_stage_release: free the host-batch device staging."""
        check(self.L.cgpu_host_stage_release(self.h), "cgpu_host_stage_release")

    def host_stage_bytes(self) -> int:
        """cgpu_host_stage_bytes: device bytes the host-batch staging holds."""
        return int(self.L.cgpu_host_stage_bytes(self.h))

    # ------------------------------------------------------------- counters
    def counter_delta_bytes(self) -> int:
        return self.L.cgpu_counter_delta_bytes(self.h)

    def counter_bind(self, tensor) -> None:
        """Accumulate launches into `tensor` (CUDA int64, >= delta bytes)."""
        if tensor is None:
            check(self.L.cgpu_counter_bind(self.h, None, 0), "cgpu_counter_bind")
        else:
            check(self.L.cgpu_counter_bind(self.h, _ptr(tensor),
                                           tensor.numel() * tensor.element_size()),
                  "cgpu_counter_bind")
        self._bound = tensor

    def counter_fold(self, stream=None) -> None:
        check(self.L.cgpu_counter_fold(self.h, _stream(stream)), "cgpu_counter_fold")

    def metrics(self) -> np.ndarray:
        out = np.zeros((256, 4, 2), np.uint64)
        check(self.L.cgpu_metrics_read(self.h, out.ctypes.data_as(C.c_void_p)),
              "cgpu_metrics_read")
        return out

    def counters_rebalance(self) -> int:
        """cgpu_counters_rebalance: hot (LDS) counter slots to the most-hit
        keys; returns how many keys moved."""
        m = C.c_uint64()
        check(self.L.cgpu_counters_rebalance(self.h, C.byref(m)), "cgpu_counters_rebalance")
        return m.value

    def stream_release(self, stream) -> None:
        """cgpu_stream_release: free the stream's packed counter buffer."""
        check(self.L.cgpu_stream_release(self.h, _stream(stream)), "cgpu_stream_release")

    def counters_reset(self) -> None:
        check(self.L.cgpu_counters_reset(self.h), "cgpu_counters_reset")

    # ------------------------------------------- multi-GPU
    @staticmethod
    def comm_id() -> bytes:
        """A fresh communicator id (rank 0 creates it and shares it)."""
        buf = C.create_string_buffer(128)
        check(lib().cgpu_comm_id_create(buf), "cgpu_comm_id_create")
        return buf.raw

    def comm_init(self, comm_id: bytes, nranks: int, rank: int) -> None:
        assert len(comm_id) == 128
        check(self.L.cgpu_comm_init(self.h, comm_id, nranks, rank), "cgpu_comm_init")

    def counters_allreduce(self, stream=None) -> None:
        """RCCL SUM of the delta buffer over the communicator's ranks."""
        check(self.L.cgpu_counters_allreduce(self.h, _stream(stream)), "cgpu_counters_allreduce")


# ---------------------------------------------------------------------------
# Go-API mirrors
# ---------------------------------------------------------------------------
class PolicyMap:
    """pkg/maps/policymap.PolicyMap over one endpoint's map (ports host order)."""

    def __init__(self, engine: Engine, ep: int):
        self.e, self.ep = engine, ep

    def Allow(self, identity, dport, proto, direction, proxy_port=0):  # noqa: N802
        rc = self.e.policy_update(self.ep, L.policy_key(identity, dport, proto, direction),
                                  L.policy_entry(proxy_port))
        check(rc, "PolicyMap.Allow")

    def AllowKey(self, key, proxy_port=0):  # noqa: N802 (key: host-order fields)
        self.Allow(int(key["sec_label"]), int(key["dport"]), int(key["protocol"]),
                   int(key["egress"]) & 1, proxy_port)

    def Exists(self, identity, dport, proto, direction) -> bool:  # noqa: N802
        rc, _ = self.e.policy_lookup(self.ep, L.policy_key(identity, dport, proto, direction))
        return rc == 0

    def Delete(self, identity, dport, proto, direction):  # noqa: N802
        check(self.e.policy_delete(self.ep, L.policy_key(identity, dport, proto, direction)),
              "PolicyMap.Delete")

    def DeleteKey(self, key):  # noqa: N802
        self.Delete(int(key["sec_label"]), int(key["dport"]), int(key["protocol"]),
                    int(key["egress"]) & 1)

    def DumpToSlice(self):  # noqa: N802
        out = []
        for k in self.e.policy_keys(self.ep):
            rc, ent = self.e.policy_lookup(self.ep, k)
            if rc == 0:
                out.append((k, ent))
        return out

    def Flush(self):  # noqa: N802
        check(self.e.policy_flush(self.ep), "PolicyMap.Flush")


class IPCacheMap:
    """pkg/maps/ipcache.Map + the ipcache listener hook."""

    def __init__(self, engine: Engine, supports_delete: bool = True):
        self.e = engine
        self.supports_delete = supports_delete

    def Update(self, cidr: str, identity: int, tunnel: int = 0):  # noqa: N802
        check(self.e.ipcache_update(L.ipcache_key(cidr), L.remote_info(identity, tunnel)),
              "ipcache.Update")

    def Delete(self, cidr: str):  # noqa: N802
        # pkg/maps/ipcache/ipcache.go:182-200: without delete support the
        # entry is overwritten with zeroes (a tombstone that still matches)
        if not self.supports_delete:
            return self.Update(cidr, 0, 0)
        check(self.e.ipcache_delete(L.ipcache_key(cidr)), "ipcache.Delete")

    # IPIdentityMappingListener.OnIPIdentityCacheChange (listener.go:78-127)
    def OnIPIdentityCacheChange(self, modType: str, cidr: str, identity: int,  # noqa: N802
                                hostIP: int = 0):
        if modType == "upsert":
            self.Update(cidr, identity, hostIP)
        elif modType == "delete":
            try:
                self.Delete(cidr)
            except CgpuError as ex:
                if ex.errno != errno.ENOENT:
                    raise


class CIDRMap:
    """pkg/maps/cidrmap.CIDRMap (prefilter maps)."""

    def __init__(self, engine: Engine, which: int):
        self.e, self.which = engine, which
        self.v6 = which in (CIDR_V6_DYN, CIDR_V6_FIX)
        self.prefixlen = 0 if which in (CIDR_V4_DYN, CIDR_V6_DYN) else (128 if self.v6 else 32)
        self.dynamic = which in (CIDR_V4_DYN, CIDR_V6_DYN)

    def _check(self, plen, op):
        # checkPrefixlen (cidrmap.go:75-83)
        if self.prefixlen != 0 and ((self.dynamic and self.prefixlen < plen) or
                                    (not self.dynamic and self.prefixlen != plen)):
            raise ValueError(f"Unable to {op} element with dynamic prefix length "
                             f"cm.Prefixlen={self.prefixlen} key.Prefixlen={plen}")

    def InsertCIDR(self, cidr: str):  # noqa: N802
        k = L.lpm_key(cidr)
        self._check(int(k["prefixlen"]), "update")
        check(self.e.cidr_update(self.which, k), "InsertCIDR")

    def DeleteCIDR(self, cidr: str):  # noqa: N802
        k = L.lpm_key(cidr)
        self._check(int(k["prefixlen"]), "delete")
        check(self.e.cidr_delete(self.which, k), "DeleteCIDR")

    def CIDRExists(self, cidr: str) -> bool:  # noqa: N802
        return self.e.cidr_lookup(self.which, L.lpm_key(cidr)) == 0

    def CIDRDump(self):  # noqa: N802
        out = []
        for k in self.e.cidr_keys(self.which):
            raw = bytes(k["addr"])
            addr = ipaddress.ip_address(raw)
            out.append(f"{addr}/{int(k['prefixlen'])}")
        return out


class PreFilter:
    """pkg/policy/prefilter.go PreFilter (Insert / Delete / Dump with the
    revision check, selectMap routing and undo), over cgpu_prefilter_*.
    CIDRs are strings; IPv4 ones go to the v4 maps (net.IPNet mask of 32
    bits), IPv6 ones to the v6 maps."""

    PREFIX = np.dtype([("bits", "<u4"), ("prefixlen", "<u4"), ("addr", "u1", (16,))])

    def __init__(self, engine: Engine):
        self.e = engine

    @classmethod
    def _prefixes(cls, cidrs):
        out = np.zeros(len(cidrs), cls.PREFIX)
        for i, c in enumerate(cidrs):
            net = ipaddress.ip_network(c, strict=False)
            raw = net.network_address.packed
            out[i]["bits"] = net.max_prefixlen
            out[i]["prefixlen"] = net.prefixlen
            out[i]["addr"][:len(raw)] = np.frombuffer(raw, np.uint8)
        return out

    def Insert(self, revision: int, cidrs):  # noqa: N802
        p = self._prefixes(cidrs)
        check(self.e.L.cgpu_prefilter_insert(self.e.h, revision, p.ctypes.data, len(p)),
              "PreFilter.Insert")

    def Delete(self, revision: int, cidrs):  # noqa: N802
        p = self._prefixes(cidrs)
        check(self.e.L.cgpu_prefilter_delete(self.e.h, revision, p.ctypes.data, len(p)),
              "PreFilter.Delete")

    def Revision(self) -> int:  # noqa: N802
        r = C.c_int64()
        check(self.e.L.cgpu_prefilter_revision(self.e.h, C.byref(r)), "PreFilter.Revision")
        return r.value

    def Dump(self):  # noqa: N802
        """(CIDR strings of the maps in prefilter.go order v4 dyn, v4 fix,
        v6 dyn, v6 fix; revision)"""
        out = []
        for which in (CIDR_V4_DYN, CIDR_V4_FIX, CIDR_V6_DYN, CIDR_V6_FIX):
            out += CIDRMap(self.e, which).CIDRDump()
        return out, self.Revision()


class LBMap:
    """pkg/maps/lbmap over cilium_lb4_services (IPv4): the frontend/backend
    writes of UpdateService (lbmap.go:350-428: backends at slaves 1..n, then
    the master slot 0 {count, weight}, then stale slaves removed) and
    DeleteService."""

    def __init__(self, engine: Engine):
        self.e = engine

    def UpdateService(self, vip: str, port: int, backends, rev_nat: int = 0):  # noqa: N802
        """backends: [(target, port, weight), ...] (ports host order)."""
        rc, old = self.e.lb4_lookup(L.lb4_key(vip, port, 0))
        existing = int(old["count"]) if rc == 0 else 0
        for i, (tgt, bport, w) in enumerate(backends):
            check(self.e.lb4_update(L.lb4_key(vip, port, i + 1),
                                    L.lb4_service(tgt, bport, 0, rev_nat, w)), "UpdateService")
        nonzero = sum(1 for b in backends if b[2])
        check(self.e.lb4_update(L.lb4_key(vip, port, 0),
                                L.lb4_service(0, 0, len(backends), 0, nonzero)), "UpdateService")
        for s in range(len(backends) + 1, existing + 1):
            self.e.lb4_delete(L.lb4_key(vip, port, s))

    def UpdateRevNat(self, index: int, vip: str, port: int):  # noqa: N802
        self.e.UpdateRevNat(index, vip, port)

    def DeleteRevNat(self, index: int, v6: bool = False):  # noqa: N802
        self.e.DeleteRevNat(index, v6)

    def DeleteService(self, vip: str, port: int):  # noqa: N802
        rc, old = self.e.lb4_lookup(L.lb4_key(vip, port, 0))
        if rc != 0:
            raise CgpuError(errno.ENOENT, f"service {vip}:{port} not found")
        for s in range(int(old["count"]), -1, -1):
            self.e.lb4_delete(L.lb4_key(vip, port, s))

    def LookupService(self, vip: str, port: int):  # noqa: N802
        rc, master = self.e.lb4_lookup(L.lb4_key(vip, port, 0))
        if rc != 0:
            return None
        out = []
        for s in range(1, int(master["count"]) + 1):
            rc, be = self.e.lb4_lookup(L.lb4_key(vip, port, s))
            if rc == 0:
                out.append(be)
        return out

    def DumpServiceMapsToUserspace(self):  # noqa: N802
        return [(k, self.e.lb4_lookup(k)[1]) for k in self.e.lb4_keys()]


class LXCMap:
    """pkg/maps/lxcmap/lxcmap.go:154-198 over cilium_lxc with its values."""

    def __init__(self, engine: Engine):
        self.e = engine

    def WriteEndpoint(self, ips, ifindex: int, lxc_id: int, mac=0, node_mac=0):  # noqa: N802
        """One endpoint_info under every key of the endpoint (GetBPFKeys:
        its IPv4 and IPv6 address)."""
        info = L.endpoint_info(ifindex, lxc_id, 0, mac, node_mac)
        for ip in ([ips] if isinstance(ips, str) else ips):
            check(self.e.endpoint_update(L.endpoint_key(ip), BPF_ANY, info), "WriteEndpoint")

    def AddHostEntry(self, ip: str):  # noqa: N802
        check(self.e.endpoint_update(L.endpoint_key(ip), BPF_ANY, L.endpoint_info(flags=L.ENDPOINT_F_HOST)),
              "AddHostEntry")

    def DeleteEntry(self, ip: str):  # noqa: N802
        if self.e.endpoint_delete(L.endpoint_key(ip)) != 0:
            raise CgpuError(errno.ENOENT, f"endpoint {ip} not found")


class TunnelMap:
    """pkg/maps/tunnel/tunnel.go:83-99 over cilium_tunnel_map."""

    def __init__(self, engine: Engine):
        self.e = engine

    def SetTunnelEndpoint(self, prefix: str, endpoint: str):  # noqa: N802
        check(self.e.tunnel_update(L.endpoint_key(prefix), L.endpoint_key(endpoint)), "SetTunnelEndpoint")

    def DeleteTunnelEndpoint(self, prefix: str):  # noqa: N802
        if self.e.tunnel_delete(L.endpoint_key(prefix)) != 0:
            raise CgpuError(errno.ENOENT, f"tunnel prefix {prefix} not found")
