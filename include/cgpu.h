/*
 * cgpu.h — C ABI of the MI355X flow-classification engine.
 *
 * Drop-in for the kernel-map boundary the reference's Go agent programs
 * through bpf(2) (pkg/bpf/bpf.go:153-245 UpdateElement / LookupElement /
 * DeleteElement / GetNextKey) and for the per-packet BPF datapath functions
 * that read those maps (bpf/lib/policy.h, bpf/lib/eps.h, bpf/bpf_xdp.c).
 * A Go package pkg/datapath/gpu binds this header through cgo (see
 * INTEGRATION.md); keys and values are the reference byte layouts so the Go
 * side passes unsafe.Pointer through unchanged, exactly as it does today.
 *
 * Conventions (mirroring bpf(2) as wrapped by pkg/bpf):
 *   - every function returns 0 or a negative errno:
 *       -ENOENT missing key, -EEXIST / -ENOENT for BPF_NOEXIST / BPF_EXIST,
 *       -E2BIG hash map full, -ENOSPC LPM map full, -EINVAL bad argument
 *       (prefixlen, family, flags), -ENODEV no GPU bound to the context,
 *       -EIO device error (details: cgpu_last_error()).
 *   - the caller owns every key/value/tuple buffer; the library copies.
 *   - table updates are thread-safe (one mutex on the host mirror) and become
 *     visible to classification only at cgpu_commit(), which publishes a new
 *     immutable device snapshot (epoch).  Classification launches read the
 *     latest published snapshot and never take the mirror lock: they run
 *     concurrently with updates and with commits (a launch pins the snapshot
 *     it started on; its buffers are freed only after its kernels finish).
 *     Like the reference (pkg/endpoint/bpf.go:459-465), a set of updates is
 *     not atomic unless it is committed at once.
 *   - batch entry points take DEVICE pointers (HBM-resident SoA columns) and
 *     a hipStream_t (passed as void*; NULL = the null stream).  They enqueue
 *     and return; results are ready when the stream reaches that point.
 *     There is no CPU execution path: without a device they fail -ENODEV.
 */
#ifndef CGPU_H
#define CGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGPU_ABI_VERSION 2u

/* bpf(2) update flags (include/uapi/linux/bpf.h) */
#define CGPU_ANY 0u
#define CGPU_NOEXIST 1u
#define CGPU_EXIST 2u

/* ------------------------------------------------------------------ */
/* Reference byte layouts                                              */
/* ------------------------------------------------------------------ */

/* struct policy_key, bpf/lib/common.h:180-186; Go PolicyKey
 * (pkg/maps/policymap/policymap.go:63-68).  dport in network order.
 * egress_pad holds the bitfield byte {egress:1, pad:7}: bit 0 = egress. */
typedef struct cgpu_policy_key {
	uint32_t sec_label;
	uint16_t dport;
	uint8_t protocol;
	uint8_t egress_pad;
} cgpu_policy_key;

/* struct policy_entry, bpf/lib/common.h:188-193 (proxy_port network order) */
typedef struct cgpu_policy_entry {
	uint16_t proxy_port;
	uint16_t pad[3];
	uint64_t packets;
	uint64_t bytes;
} cgpu_policy_entry;

/* struct ipcache_key, bpf/lib/maps.h:135-148 (24 B, packed).  prefixlen
 * counts the 32 static bits {pad[3], family} plus the IP bits
 * (bpf/lib/eps.h:48-52; Go pkg/maps/ipcache/ipcache.go:72-98). */
typedef struct cgpu_ipcache_key {
	uint32_t prefixlen;
	uint8_t pad[3];
	uint8_t family; /* ENDPOINT_KEY_IPV4 = 1, ENDPOINT_KEY_IPV6 = 2 */
	uint8_t ip[16];
} cgpu_ipcache_key;

/* struct remote_endpoint_info, bpf/lib/common.h:175-178 */
typedef struct cgpu_remote_endpoint_info {
	uint32_t sec_label;
	uint32_t tunnel_endpoint;
} cgpu_remote_endpoint_info;

/* struct lpm_v4_key / lpm_v6_key, bpf/lib/xdp.h:23-31 (Go cidrKey,
 * pkg/maps/cidrmap/cidrmap.go:49-52, truncated to 4 + AddrSize bytes).
 * Only the first 4 (v4) or 16 (v6) bytes of addr are used. */
typedef struct cgpu_cidr_key {
	uint32_t prefixlen;
	uint8_t addr[16];
} cgpu_cidr_key;

/* struct endpoint_key, bpf/lib/common.h:147-160 (20 B, packed) */
typedef struct cgpu_endpoint_key {
	uint8_t ip[16];
	uint8_t family;
	uint8_t pad4;
	uint16_t pad5;
} cgpu_endpoint_key;

/* prefilter maps: pkg/policy/prefilter.go:33-39 preFilterMapType */
enum cgpu_cidr_map {
	CGPU_CIDR_V4_DYN = 0, /* LPM, bpf_xdp.c CIDR4_LMAP_NAME */
	CGPU_CIDR_V4_FIX = 1, /* exact hash, CIDR4_HMAP_NAME */
	CGPU_CIDR_V6_DYN = 2,
	CGPU_CIDR_V6_FIX = 3,
};

/* ------------------------------------------------------------------ */
/* Configuration: the compile-time #defines the agent writes into      */
/* node_config.h / lxc_config.h / filter_config.h become runtime fields */
/* ------------------------------------------------------------------ */
typedef struct cgpu_config {
	uint32_t abi_version;       /* = CGPU_ABI_VERSION */
	/* capacities (max_elem of the reference maps; device sizing) */
	uint32_t ipcache_max;       /* IPCACHE_MAP_SIZE 512000 (node_config.h:63) */
	uint32_t policy_max_per_ep; /* POLICY_MAP_SIZE 16384 (policymap.go:37) */
	uint32_t policy_max_total;  /* device slots across all endpoints */
	uint32_t max_endpoints;     /* policy maps = endpoint ids [0, max) */
	uint32_t cidr_dyn_max;      /* maxLKeys 64k (prefilter.go:43) */
	uint32_t cidr_fix_max;      /* maxHKeys 20M (prefilter.go:44) */
	uint32_t endpoints_max;     /* ENDPOINTS_MAP_SIZE 65536 */
	/* reserved identities (node_config.h:34-37) */
	uint32_t host_id, world_id, cluster_id, health_id;
	/* IPV4_CLUSTER_MASK / IPV4_CLUSTER_RANGE, network-order u32 as the
	 * agent writes them (daemon/daemon.go:919-920) */
	uint32_t ipv4_cluster_mask, ipv4_cluster_range;
	uint8_t ipv6_router_ip[16]; /* ROUTER_IP, ipv6_match_prefix_64 */
	/* CONNTRACK protocol gate: non ICMP/TCP/UDP -> DROP_CT_UNKNOWN_PROTO
	 * before policy (bpf/lib/conntrack.h:526-528) */
	uint8_t ct_proto_gate;
	/* ingress label: 0 -> secctx = resolved source identity (FROM_HOST
	 * form, bpf_netdev.c:403); 1 -> WORLD_ID (derive_ipv4_sec_ctx,
	 * bpf_netdev.c:278-290) */
	uint8_t ingress_secctx_world;
	/* prefilter: CIDR4_FILTER/CIDR4_LPM_PREFILTER/... (prefilter.go:65-89) */
	uint8_t prefilter_fix4, prefilter_dyn4, prefilter_fix6, prefilter_dyn6;
	uint8_t reserved0[2];
	/* identity handed to handle_ipv4 on ingress (from_netdev: 0) */
	uint32_t ingress_src_identity;
	/* counter slots [0, hot_counter_slots) are reserved for L3-only and
	 * identity-wildcard policy keys (the entries most tuples hit) and are
	 * accumulated in LDS per workgroup before one flush to HBM */
	uint32_t hot_counter_slots;
	/* service map cilium_lb4_services: max_elem (CILIUM_LB_MAP_MAX_ENTRIES,
	 * bpf/node_config.h:60; raise it for the 1M-service config) */
	uint32_t lb_max_entries;
	/* IPV4_LOOPBACK (bpf/node_config.h:45), network-order u32 as written */
	uint32_t ipv4_loopback;
	/* CGPU_LB_L3 | CGPU_LB_L4: the LB_L3 / LB_L4 build switches of lib/lb.h
	 * (bpf/lxc_config.h:44-45 and bpf/init.sh:352 set both) */
	uint32_t lb_flags;
	/* NODE_MAC (bpf/node_config.h:51): the gateway MAC an endpoint's egress
	 * frames must be addressed to (is_valid_gw_dst_mac, lib/lxc.h:77-90) */
	uint8_t node_mac[6];
	uint8_t reserved1[2];
	/* CT_MAP_SIZE of cilium_ct4_global: live conntrack entries the map
	 * holds (MapNumEntriesGlobal 1000000, pkg/maps/ctmap/ctmap.go:101);
	 * device slots are 2x this, rounded up to a power of two */
	uint32_t ct_max;
	/* schedule overrides, CGPU_SCHED_* (0 = the tuned default).  Every
	 * schedule computes the same results; they exist for the parity tests of
	 * the fallback kernels and for A/B timing, and are fixed per context (no
	 * behaviour is read from the environment). */
	uint32_t schedule;
	/* CT_MAP_SIZE of cilium_ct6_global (0 = ct_max) */
	uint32_t ct6_max;
	/* 1: the conntrack maps behave as BPF_MAP_TYPE_LRU_HASH, which the
	 * reference builds CT_MAP4 / CT_MAP6 as on every kernel with LRU maps
	 * (bpf/bpf_lxc.c:53-75, probe bpf/probes/raw_lru_map.t): a create that
	 * finds the map full evicts an entry instead of failing.  All four
	 * conntrack calls, cgpu_classify_v{4,6}_ct and cgpu_classify_v{4,6}_ctlb
	 * (the service walk's CT_SERVICE creates included), and their _tun /
	 * _rnat forms.
	 * The victim is the engine's own choice, not the kernel's per-CPU LRU
	 * list: before any walk of a batch, every key a packet of the batch can
	 * look up or create is marked in a filter (on the service paths a
	 * superset, from every backend a service packet can be sent to); a create
	 * that finds the map full scans CT_EVICT_SCAN = 4096 slots from a hashed
	 * start and evicts the first live entry whose key is outside the filter.
	 * So every packet of a batch gets the result the map the batch found
	 * gives it, and no key the batch touches is evicted; across batches an
	 * entry idle in one batch may be gone in the next.
	 * The one remaining failure: a create still fails (DROP_CT_CREATE_FAILED,
	 * on the service step DROP_NO_SERVICE) when no entry outside the batch's
	 * keys lies within those 4096 slots, which is the case when one batch
	 * needs more entries than the map holds (or marks so many keys that the
	 * filter, capped at 256 MiB, saturates).  cgpu_ct_lru_stats counts both.
	 * 0 (default): the non-LRU build, CT_MAP_SIZE enforced as -E2BIG. */
	uint32_t ct_lru;
	/* 1: cgpu_commit also compiles the second word of every ipcache value,
	 * struct remote_endpoint_info.tunnel_endpoint (bpf/lib/common.h:175-178),
	 * into device tables, and the calls with a `tunnel` output may be given
	 * one.  0 (default): the device holds identities only, exactly the tables
	 * and bytes of a build without this field, and every such call given a
	 * non-NULL tunnel pointer returns -EINVAL.  (Was reserved[0]; the struct
	 * size and CGPU_ABI_VERSION stay.) */
	uint32_t ipcache_tunnel;
} cgpu_config;

#define CGPU_SCHED_PER_LANE 1u   /* classify: one tuple per lane (k_classify) instead of x4 */
#define CGPU_SCHED_GLOBAL_CTR 2u /* classify: per-lane kernel, one global atomic per hit */
#define CGPU_SCHED_NO_CCACHE 4u  /* x4 classify without the LDS cold-slot cache */
#define CGPU_SCHED_FRAMES_SPLIT 8u /* classify_frames, 64-byte slots: a header pass writes tuple columns, then the classify pass (default: one fused kernel) */
/* bits 4-5: v6 prefilter LDS staging mode + 1 (0 = the deepest that fits) */
#define CGPU_SCHED_PF6_LDS(mode) ((((uint32_t)(mode)) + 1u) << 4)
/* cgpu_classify_v4 and cgpu_classify_v4_host (x4 schedule, no tunnel output)
 * without the cold-hit log: a hit on a counter slot past the LDS hot slots
 * that the LDS cold-slot cache did not take is one global atomic, deferred
 * behind the next tuples' column loads.  By default those two calls append
 * such a hit to a per-stream log with plain stores and a second kernel sums
 * the log after the classify kernel; a hit that finds its wave's part of the
 * log full takes the atomic.  A launch takes the atomic path for every such
 * hit, exactly as with this bit, when the cold slots need more than 8
 * LDS-sized partitions (about 160k slots) or their count does not fit the
 * log entry's 21 bits.  No other call logs: the service, cascade, IPv6,
 * tunnel and frames calls always use the atomics (the second kernel measured
 * more than the log saved them).
 * Memory: a stream that logs owns a log of one byte per tuple of its largest
 * call (at most 64 MiB, plus about 2 MiB), allocated by the first such call,
 * grown by a larger one after the stream's earlier launches finished, and
 * freed with the stream's packed counters (cgpu_stream_release, context
 * destroy, the recycling past 16 streams).  A call that takes the atomic
 * path allocates none.  As for those counters, the calls on one stream are
 * made from one thread at a time. */
#define CGPU_SCHED_NO_COLD_LOG 64u
/* bits 8-13: conntrack group-key radix sort bits (8..32; 0 = 24) */
#define CGPU_SCHED_CT_SORT_BITS(b) (((uint32_t)(b)) << 8)

#define CGPU_LB_L3 1u
#define CGPU_LB_L4 2u

typedef struct cgpu_ctx cgpu_ctx;

void cgpu_config_default(cgpu_config *cfg);
/* device: HIP device ordinal, or -1 for a host-only context (table
 * management and dumps work; batch entry points return -ENODEV). */
int cgpu_ctx_create(const cgpu_config *cfg, int device, cgpu_ctx **out);
void cgpu_ctx_destroy(cgpu_ctx *ctx);
const char *cgpu_last_error(void);
const char *cgpu_version(void);

/* ------------------------------------------------------------------ */
/* ipcache: pkg/maps/ipcache (Map.Update/Delete, LPM semantics of       */
/* kernel/bpf/lpm_trie.c; lookup is longest-prefix like bpf(2) lookup)  */
/* ------------------------------------------------------------------ */
int cgpu_ipcache_update(cgpu_ctx *ctx, const cgpu_ipcache_key *key,
			const cgpu_remote_endpoint_info *val, uint64_t flags);
int cgpu_ipcache_delete(cgpu_ctx *ctx, const cgpu_ipcache_key *key);
int cgpu_ipcache_lookup(cgpu_ctx *ctx, const cgpu_ipcache_key *key,
			cgpu_remote_endpoint_info *val_out);
/* GetNextKey: key == NULL returns the first key; -ENOENT after the last */
int cgpu_ipcache_get_next_key(cgpu_ctx *ctx, const cgpu_ipcache_key *key,
			      cgpu_ipcache_key *next_out);
size_t cgpu_ipcache_count(cgpu_ctx *ctx);
/* n updates in order; stops at the first failure (its -errno is returned,
 * the updates before it stay applied): the listener's sequence of
 * OnIPIdentityCacheChange writes in one call */
int cgpu_ipcache_update_batch(cgpu_ctx *ctx, const cgpu_ipcache_key *keys,
			      const cgpu_remote_endpoint_info *vals, size_t n, uint64_t flags);
/* ipcache_lookup4 / ipcache_lookup6 (bpf/lib/eps.h:56-80) over a batch of
 * addresses on the device, against the committed snapshot (device pointers;
 * addr: network-order u32, addr16: 16 bytes per address, any alignment).
 * found[i] = 1 for any match, a tombstone (sec_label 0) included; sec_label[i]
 * and tunnel[i] are the matched entry's raw words {sec_label, tunnel_endpoint}
 * (bpf/lib/common.h:175-178), 0 where nothing matched.  The tunnel is the
 * word the reference reads as info->tunnel_endpoint on every forwarded egress
 * packet (bpf_lxc.c:488-491 IPv4, :177-180 IPv6).  found, sec_label and tunnel
 * may each be NULL; tunnel must be NULL unless cgpu_config.ipcache_tunnel is
 * set (-EINVAL).  -ENODEV on a host-only context. */
int cgpu_ipcache_lookup_v4(cgpu_ctx *ctx, const uint32_t *addr, size_t n, uint8_t *found,
			   uint32_t *sec_label, uint32_t *tunnel, void *stream);
int cgpu_ipcache_lookup_v6(cgpu_ctx *ctx, const uint8_t *addr16, size_t n, uint8_t *found,
			   uint32_t *sec_label, uint32_t *tunnel, void *stream);

/* ------------------------------------------------------------------ */
/* policy maps: pkg/maps/policymap (AllowKey/DeleteKey/DumpToSlice/     */
/* Flush), one map per endpoint id                                      */
/* ------------------------------------------------------------------ */
int cgpu_policy_update(cgpu_ctx *ctx, uint32_t ep, const cgpu_policy_key *key,
		       const cgpu_policy_entry *entry, uint64_t flags);
int cgpu_policy_delete(cgpu_ctx *ctx, uint32_t ep, const cgpu_policy_key *key);
/* entry_out.packets/bytes include every committed-and-classified batch */
int cgpu_policy_lookup(cgpu_ctx *ctx, uint32_t ep, const cgpu_policy_key *key,
		       cgpu_policy_entry *entry_out);
int cgpu_policy_get_next_key(cgpu_ctx *ctx, uint32_t ep, const cgpu_policy_key *key,
			     cgpu_policy_key *next_out);
int cgpu_policy_flush(cgpu_ctx *ctx, uint32_t ep);
size_t cgpu_policy_count(cgpu_ctx *ctx, uint32_t ep);
/* AllowKey for n (ep, key) pairs in order (stops at the first failure) */
int cgpu_policy_update_batch(cgpu_ctx *ctx, const uint32_t *eps, const cgpu_policy_key *keys,
			     const cgpu_policy_entry *entries, size_t n, uint64_t flags);
/* cgpu_policy_lookup of n (ep, key) pairs with one read of the device
 * counters: rc_out[i] = 0 or -ENOENT (-EINVAL for an ep out of range) */
int cgpu_policy_lookup_batch(cgpu_ctx *ctx, const uint32_t *eps, const cgpu_policy_key *keys,
			     size_t n, cgpu_policy_entry *entries_out, int32_t *rc_out);
/* DumpToSlice (pkg/maps/policymap/policymap.go:208-240): every key of ep's
 * map with its entry, in GetNextKey order; *n_out = the key count
 * (-ENOSPC when it exceeds cap, nothing written) */
int cgpu_policy_dump(cgpu_ctx *ctx, uint32_t ep, cgpu_policy_key *keys_out,
		     cgpu_policy_entry *entries_out, size_t cap, size_t *n_out);

/* ------------------------------------------------------------------ */
/* prefilter CIDR maps: pkg/maps/cidrmap (InsertCIDR/DeleteCIDR/        */
/* CIDRExists/CIDRDump) and the endpoint map cilium_lxc (lxcmap)        */
/* ------------------------------------------------------------------ */
int cgpu_cidr_update(cgpu_ctx *ctx, int which, const cgpu_cidr_key *key, uint64_t flags);
int cgpu_cidr_delete(cgpu_ctx *ctx, int which, const cgpu_cidr_key *key);
/* exact key presence (CIDRExists semantics for fix; LPM lookup for dyn) */
int cgpu_cidr_lookup(cgpu_ctx *ctx, int which, const cgpu_cidr_key *key);
int cgpu_cidr_get_next_key(cgpu_ctx *ctx, int which, const cgpu_cidr_key *key,
			   cgpu_cidr_key *next_out);
/* n InsertCIDR writes in order (stops at the first failure) */
int cgpu_cidr_update_batch(cgpu_ctx *ctx, int which, const cgpu_cidr_key *keys, size_t n,
			   uint64_t flags);
/* PreFilter (pkg/policy/prefilter.go:30-203): the revisioned CIDR set the
 * agent's PATCH/DELETE /prefilter handlers drive (daemon/prefilter.go).
 * A prefix carries its address family as the mask size of net.IPNet
 * (bits 32 / 128).  selectMap (prefilter.go:108-122) routes /32 and /128 to
 * the exact ("fix") maps and shorter prefixes to the LPM ("dyn") maps; a map
 * whose cgpu_config switch is off does not exist (-EOPNOTSUPP, "No map
 * enabled").  revision != 0 must equal the current revision (else -ESTALE,
 * "Latest revision is ..."); it starts at 1 and each successful call adds 1.
 * insert: every prefix or none -- on the first failure the prefixes already
 * inserted are deleted again (prefilter.go:124-159).  delete: every prefix
 * must exist first (a map lookup: longest-prefix on the LPM maps, -ENOENT
 * before anything changed); a later failure re-inserts the deleted ones
 * (:161-203).  The map contents reach the device at cgpu_commit. */
typedef struct cgpu_prefix {
	uint32_t bits; /* 32: IPv4, 128: IPv6 */
	cgpu_cidr_key key;
} cgpu_prefix;
int cgpu_prefilter_insert(cgpu_ctx *ctx, int64_t revision, const cgpu_prefix *cidrs, size_t n);
int cgpu_prefilter_delete(cgpu_ctx *ctx, int64_t revision, const cgpu_prefix *cidrs, size_t n);
int cgpu_prefilter_revision(cgpu_ctx *ctx, int64_t *revision_out);

int cgpu_endpoint_update(cgpu_ctx *ctx, const cgpu_endpoint_key *key, uint64_t flags);
int cgpu_endpoint_delete(cgpu_ctx *ctx, const cgpu_endpoint_key *key);
int cgpu_endpoint_lookup(cgpu_ctx *ctx, const cgpu_endpoint_key *key);

/* The value of cilium_lxc, struct endpoint_info (bpf/lib/common.h:165-173,
 * 48 B; mac_t is __u64): what the forwarding step (cgpu_forward_v4 / _v6)
 * reads of a local endpoint.  The Go writer: pkg/maps/lxcmap/lxcmap.go:94-113. */
#define CGPU_ENDPOINT_F_HOST 1u /* ENDPOINT_F_HOST: the local host itself */
typedef struct cgpu_endpoint_info {
	uint32_t ifindex;
	uint16_t unused;
	uint16_t lxc_id;
	uint32_t flags;
	uint32_t pad0_;    /* the C layout's hole before the first __u64 */
	uint64_t mac;
	uint64_t node_mac;
	uint32_t pad[4];
} cgpu_endpoint_info;
#if defined(__cplusplus)
static_assert(sizeof(cgpu_endpoint_info) == 48, "struct endpoint_info is 48 bytes");
#else
_Static_assert(sizeof(cgpu_endpoint_info) == 48, "struct endpoint_info is 48 bytes");
#endif
/* cgpu_endpoint_update with a value (cgpu_endpoint_update itself writes an
 * all-zero one, also over an existing value; cgpu_endpoint_delete removes key
 * and value).  Same flags, errno and endpoints_max.  lookup_info: the stored
 * 48 bytes (the MACs included, for a caller that rewrites frames), -ENOENT. */
int cgpu_endpoint_update_info(cgpu_ctx *ctx, const cgpu_endpoint_key *key,
			      const cgpu_endpoint_info *info, uint64_t flags);
int cgpu_endpoint_lookup_info(cgpu_ctx *ctx, const cgpu_endpoint_key *key,
			      cgpu_endpoint_info *info_out);

/* ------------------------------------------------------------------ */
/* tunnel map cilium_tunnel_map (bpf/lib/maps.h:92-101,                 */
/* pkg/maps/tunnel/tunnel.go): prefix -> node, key and value both a raw */
/* 20-byte endpoint_key                                                 */
/* ------------------------------------------------------------------ */
/* A hash map compared on the whole 20-byte key (pad bytes and family
 * included); CGPU_ANY / NOEXIST / EXIST, -ENOENT, -E2BIG at
 * CGPU_TUNNEL_MAP_SIZE entries (TUNNEL_ENDPOINT_MAP_SIZE, bpf/node_config.h:54).
 * get_next_key (NULL = first) walks the keys in byte order.  Works on a
 * host-only context; reaches the device at cgpu_commit.  The datapath reads
 * only the first four bytes of a value (tunnel->ip4, bpf/lib/encap.h:59). */
#define CGPU_TUNNEL_MAP_SIZE 65536u
int cgpu_tunnel_update(cgpu_ctx *ctx, const cgpu_endpoint_key *key, const cgpu_endpoint_key *val,
		       uint64_t flags);
int cgpu_tunnel_delete(cgpu_ctx *ctx, const cgpu_endpoint_key *key);
int cgpu_tunnel_lookup(cgpu_ctx *ctx, const cgpu_endpoint_key *key, cgpu_endpoint_key *val_out);
int cgpu_tunnel_get_next_key(cgpu_ctx *ctx, const cgpu_endpoint_key *key, cgpu_endpoint_key *next_out);
size_t cgpu_tunnel_count(cgpu_ctx *ctx);

/* ------------------------------------------------------------------ */
/* service map cilium_lb4_services: pkg/maps/lbmap (UpdateService /     */
/* DeleteService, lbmap.go:341-429), bpf/lib/lb.h:70-76                  */
/* ------------------------------------------------------------------ */
/* struct lb4_key, bpf/lib/common.h:427-431: address and dport in network
 * order, slave host order (Go Service4Key.ToNetwork, lbmap/ipv4.go:99-104) */
typedef struct cgpu_lb4_key {
	uint32_t address;
	uint16_t dport;
	uint16_t slave; /* 0 = the service ("master"), 1.. = backends */
} cgpu_lb4_key;

/* struct lb4_service, bpf/lib/common.h:433-439: target, port, rev_nat_index,
 * weight in network order; count host order (lbmap/ipv4.go:135-181) */
typedef struct cgpu_lb4_service {
	uint32_t target;
	uint16_t port;
	uint16_t count;
	uint16_t rev_nat_index;
	uint16_t weight;
} cgpu_lb4_service;

int cgpu_lb4_update(cgpu_ctx *ctx, const cgpu_lb4_key *key, const cgpu_lb4_service *val,
		    uint64_t flags);
/* n updates in order; stops at the first failure (its -errno is returned,
 * the entries before it stay applied).  The Go writer issues one bpf(2)
 * call per entry; this is the same sequence in one call. */
int cgpu_lb4_update_batch(cgpu_ctx *ctx, const cgpu_lb4_key *keys, const cgpu_lb4_service *vals,
			  size_t n, uint64_t flags);
int cgpu_lb4_delete(cgpu_ctx *ctx, const cgpu_lb4_key *key);
int cgpu_lb4_lookup(cgpu_ctx *ctx, const cgpu_lb4_key *key, cgpu_lb4_service *val_out);
int cgpu_lb4_get_next_key(cgpu_ctx *ctx, const cgpu_lb4_key *key, cgpu_lb4_key *next_out);
size_t cgpu_lb4_count(cgpu_ctx *ctx);

/* struct lb6_key, bpf/lib/common.h:408-412 (packed, 20 B): address and dport
 * in network order, slave host order */
typedef struct cgpu_lb6_key {
	uint8_t address[16];
	uint16_t dport;
	uint16_t slave;
} cgpu_lb6_key;

/* struct lb6_service, bpf/lib/common.h:414-420 (packed, 24 B) */
typedef struct cgpu_lb6_service {
	uint8_t target[16];
	uint16_t port;
	uint16_t count;
	uint16_t rev_nat_index;
	uint16_t weight;
} cgpu_lb6_service;

/* cilium_lb6_services (lb.h:46-52), the map lbmap writes for IPv6
 * frontends (pkg/maps/lbmap/ipv6.go); same semantics as the lb4 calls.
 * Shares lb_max_entries with the lb4 map as a per-map capacity. */
int cgpu_lb6_update(cgpu_ctx *ctx, const cgpu_lb6_key *key, const cgpu_lb6_service *val,
		    uint64_t flags);
int cgpu_lb6_update_batch(cgpu_ctx *ctx, const cgpu_lb6_key *keys, const cgpu_lb6_service *vals,
			  size_t n, uint64_t flags);
int cgpu_lb6_delete(cgpu_ctx *ctx, const cgpu_lb6_key *key);
int cgpu_lb6_lookup(cgpu_ctx *ctx, const cgpu_lb6_key *key, cgpu_lb6_service *val_out);
int cgpu_lb6_get_next_key(cgpu_ctx *ctx, const cgpu_lb6_key *key, cgpu_lb6_key *next_out);
size_t cgpu_lb6_count(cgpu_ctx *ctx);

/* ------------------------------------------------------------------ */
/* reverse NAT maps cilium_lb4_reverse_nat / cilium_lb6_reverse_nat     */
/* (bpf/lib/lb.h:54-68; the agent fills them for every service,         */
/* daemon/loadbalancer.go:345-350, pkg/maps/lbmap/lbmap.go:229-260)      */
/* ------------------------------------------------------------------ */
#pragma pack(push, 1)
/* struct lb4_reverse_nat, bpf/lib/common.h:441-444 (packed, 6 B): the
 * service's address and port, network order */
typedef struct cgpu_lb4_reverse_nat {
	uint32_t address;
	uint16_t port;
} cgpu_lb4_reverse_nat;
/* struct lb6_reverse_nat, bpf/lib/common.h:422-425 (packed, 18 B) */
typedef struct cgpu_lb6_reverse_nat {
	uint8_t address[16];
	uint16_t port;
} cgpu_lb6_reverse_nat;
#pragma pack(pop)

/* Semantics of the cgpu_lb4_* calls (CGPU_ANY / NOEXIST / EXIST, -ENOENT,
 * -E2BIG at lb_max_entries per map: both are CILIUM_LB_MAP_MAX_ENTRIES in the
 * reference).  `index` is the __u16 key as the datapath holds it: the same
 * 16 raw bits as cgpu_lb4_service.rev_nat_index and cgpu_ct_entry.
 * rev_nat_index (lb.h:570 looks ct_state->rev_nat_index up as stored).
 * get_next_key (NULL = first) walks the indices in ascending raw order.  The
 * calls work on a host-only context; the maps always exist (there is no
 * switch) and reach the device at cgpu_commit as dense tables, built only
 * for a non-empty map.  Only the cgpu_classify_*_rnat calls read them. */
int cgpu_revnat4_update(cgpu_ctx *ctx, uint16_t index, const cgpu_lb4_reverse_nat *val, uint64_t flags);
int cgpu_revnat4_delete(cgpu_ctx *ctx, uint16_t index);
int cgpu_revnat4_lookup(cgpu_ctx *ctx, uint16_t index, cgpu_lb4_reverse_nat *val_out);
int cgpu_revnat4_get_next_key(cgpu_ctx *ctx, const uint16_t *index, uint16_t *next_out);
size_t cgpu_revnat4_count(cgpu_ctx *ctx);
int cgpu_revnat6_update(cgpu_ctx *ctx, uint16_t index, const cgpu_lb6_reverse_nat *val, uint64_t flags);
int cgpu_revnat6_delete(cgpu_ctx *ctx, uint16_t index);
int cgpu_revnat6_lookup(cgpu_ctx *ctx, uint16_t index, cgpu_lb6_reverse_nat *val_out);
int cgpu_revnat6_get_next_key(cgpu_ctx *ctx, const uint16_t *index, uint16_t *next_out);
size_t cgpu_revnat6_count(cgpu_ctx *ctx);

/* The flow hash the batch entry points use when no hash column is given
 * (skb->hash comes from the kernel's flow dissector, which the reference
 * does not contain: SURVEY §8c).  Over the stored (network-order) fields. */
uint32_t cgpu_flow_hash(uint32_t saddr, uint32_t daddr, uint16_t sport, uint16_t dport,
			uint8_t proto);
/* IPv6: cgpu_flow_hash over the two addresses folded to 32 bits each
 * (tables.h fold6: the 16 bytes as four little-endian words, murmur3-mixed) */
uint32_t cgpu_flow_hash6(const uint8_t *saddr16, const uint8_t *daddr16, uint16_t sport,
			 uint16_t dport, uint8_t proto);

/* ------------------------------------------------------------------ */
/* per-endpoint identity of the endpoint program (lxc_config.h)         */
/* ------------------------------------------------------------------ */
/* The #defines the agent writes per endpoint into lxc_config.h and that the
 * from-container program checks on every frame (bpf/lib/lxc.h:31-89):
 * LXC_MAC, LXC_IPV4, LXC_IP, and which checks are compiled in (the absence
 * of DISABLE_SMAC_VERIFICATION / DISABLE_DMAC_VERIFICATION /
 * DISABLE_SIP_VERIFICATION).  An endpoint without an entry verifies nothing. */
#define CGPU_VERIFY_SMAC 1u /* h_source == LXC_MAC      -> else DROP_INVALID_SMAC (-130) */
#define CGPU_VERIFY_DMAC 2u /* h_dest == NODE_MAC       -> else DROP_INVALID_DMAC (-131) */
#define CGPU_VERIFY_SIP 4u  /* saddr == LXC_IPV4/LXC_IP -> else DROP_INVALID_SIP (-132) */

typedef struct cgpu_lxc_info {
	uint8_t mac[6];   /* LXC_MAC */
	uint8_t verify;   /* CGPU_VERIFY_* */
	uint8_t pad;
	uint32_t ipv4;    /* LXC_IPV4: raw u32 compared with ip4->saddr (lxc.h:55-62) */
	uint8_t ipv6[16]; /* LXC_IP, network order */
	uint32_t sec_label; /* SECLABEL: src_sec_id of the entries the endpoint's egress
			       creates (bpf_lxc.c:517, conntrack.h:705) */
} cgpu_lxc_info;

int cgpu_lxc_update(cgpu_ctx *ctx, uint32_t ep, const cgpu_lxc_info *info);
int cgpu_lxc_delete(cgpu_ctx *ctx, uint32_t ep);
int cgpu_lxc_lookup(cgpu_ctx *ctx, uint32_t ep, cgpu_lxc_info *info_out);

/* ------------------------------------------------------------------ */
/* publication                                                          */
/* ------------------------------------------------------------------ */
/* Compile the host mirror into device tables and publish them as the new
 * snapshot read by later batch launches.  *epoch_out (optional) receives
 * the snapshot number.  Only the table groups that changed since the last
 * commit are uploaded (the rest is shared with the previous snapshot); a
 * few ipcache / policy changes patch the previous tables instead of
 * recompiling them, the way the reference writes each map key in place
 * (pkg/endpoint/endpoint.go:2572-2652 syncPolicyMap,
 * pkg/datapath/ipcache/listener.go:78-127).  Returns once the upload (on the
 * context's own stream) is complete; launches in flight on the previous
 * snapshot are never waited for.  Counter values supplied with a rewritten
 * policy entry reach the device here; hits that launches still running on
 * the previous snapshot add to that entry may land before or after. */
int cgpu_commit(cgpu_ctx *ctx, uint64_t *epoch_out);
/* order-independent checksum of the committed table contents; replicas on
 * different GPUs/ranks holding the same tables report the same value */
int cgpu_table_checksum(cgpu_ctx *ctx, uint64_t *sum_out);
/* Device bytes a lookup into each table group of the published snapshot
 * gathers from (0 for a group never committed; parts staged in LDS or read
 * only by fallback schedules excluded), and of the conntrack maps: bench.py
 * prices each map's lookups at the measured gather ceiling of the cache tier
 * a table of that size lives in. */
enum {
	CGPU_TBL_IPCACHE = 0, CGPU_TBL_POLICY, CGPU_TBL_PREFILTER, CGPU_TBL_ENDPOINT, CGPU_TBL_LB4,
	CGPU_TBL_LXC, CGPU_TBL_LB6, CGPU_TBL_CT4, CGPU_TBL_CT6, CGPU_TBL_N
};
int cgpu_table_bytes(cgpu_ctx *ctx, uint64_t *bytes_out /* [CGPU_TBL_N] */);
/* Failure detection: every group buffer a commit uploads is
 * summed on the device and compared with the host image's sum before the
 * snapshot is published (a mismatch fails the commit with -EIO).  This call
 * re-sums every buffer of the published snapshot on the device and returns
 * -EIO (naming the table group) when one no longer matches its host image;
 * a caller recovers by committing again from the authoritative host mirror. */
int cgpu_table_verify(cgpu_ctx *ctx);
/* checksum of which counter slot every committed policy key holds.  Slot
 * assignment is a function of the sequence of map operations and commits
 * only (never of GPU progress), so replicas that applied the same sequence
 * agree; ranks compare it before cgpu_counters_allreduce, which sums the
 * delta buffers slot by slot. */
int cgpu_counter_layout_checksum(cgpu_ctx *ctx, uint64_t *sum_out);

/* ------------------------------------------------------------------ */
/* batch classification (device pointers)                              */
/* ------------------------------------------------------------------ */
/* Tuple flag bits */
#define CGPU_F_EGRESS 1u   /* from-container (bpf_lxc.c handle_ipv4_from_lxc) */
#define CGPU_F_FRAGMENT 2u /* ipv4_is_fragment (bpf/lib/ipv4.h:50-61) */

typedef struct cgpu_tuples_v4 {
	const uint32_t *saddr; /* network order */
	const uint32_t *daddr; /* network order */
	const uint16_t *dport; /* network order (policy port, conntrack.h:471-524) */
	const uint8_t *proto;
	const uint8_t *flags;  /* CGPU_F_* */
	const uint32_t *len;   /* skb->len */
	const uint16_t *ep;    /* endpoint id: selects the policy map */
} cgpu_tuples_v4;

/*
 * For every tuple: ipcache LPM of the remote address, identity fallback,
 * the three-probe policy cascade of __policy_can_access (policy.h:46-110),
 * the per-entry packets/bytes counters and the {reason, dir} metrics.
 *   verdict[i]  : proxy port (raw be16 as int, e.g. 4000 -> 40975), 0 allow,
 *                 DROP_POLICY (-133), DROP_CT_UNKNOWN_PROTO (-137)
 *   identity[i] : label given to policy (dstID on egress, secctx on ingress)
 *   stage[i]    : optional (NULL ok): 1 exact, 2 L3-only, 3 identity-wildcard
 *                 L4, 0 miss, 4 protocol-gated (6: service drop, _lb only)
 */
int cgpu_classify_v4(cgpu_ctx *ctx, const cgpu_tuples_v4 *t, size_t n, int32_t *verdict,
		     uint32_t *identity, uint8_t *stage, void *stream);

/*
 * cgpu_classify_v4 over a HOST-resident batch (the reference
 * classifies each packet as the NIC hands it over, bpf_xdp.c:181-184 /
 * bpf_netdev.c:470; the engine takes batches that arrive in host memory
 * too): every column of t and the outputs are host pointers.  The batch
 * streams through device staging (up to 16 chunks of 8M tuples): uploads,
 * the classify of each chunk on `stream` and the stores of its outputs
 * overlap on queues of their own.  Returns once enqueued; the outputs are
 * complete when `stream` is (page-locked outputs are written by the CUs,
 * page-locked inputs uploaded by DMA, or read by the CUs for 64-byte frame
 * slots; pageable buffers are copied by the runtime and serialise).  Same results, counters
 * and metrics as cgpu_classify_v4 of the same tuples.  -ENODEV on a
 * host-only context, -EINVAL for a null column or output.
 */
int cgpu_classify_v4_host(cgpu_ctx *ctx, const cgpu_tuples_v4 *t, size_t n, int32_t *verdict,
			  uint32_t *identity, uint8_t *stage, void *stream);
/*
 * A host call pins ONE snapshot for its whole batch: a cgpu_commit from
 * another thread while the chunks are queued does not split the batch.  On
 * an error after the first chunk was queued, the call waits for every copy
 * it queued (they read and write the caller's buffers) before returning.
 * The staging (up to 16 x ~227 MB of device memory) stays allocated for the
 * next host call: cgpu_host_stage_bytes reports it, cgpu_host_stage_release
 * waits for the host calls queued on it and frees it (cgpu_ctx_destroy does
 * too).
 */
int cgpu_host_stage_release(cgpu_ctx *ctx);
size_t cgpu_host_stage_bytes(cgpu_ctx *ctx);

typedef struct cgpu_tuples_v6 {
	const uint8_t *saddr;  /* 16 bytes per tuple, network order */
	const uint8_t *daddr;  /* 16 bytes per tuple */
	const uint16_t *dport; /* network order */
	const uint8_t *proto;  /* nexthdr */
	const uint8_t *flags;  /* CGPU_F_EGRESS (fragments: IPv6 passes false) */
	const uint32_t *len;
	const uint16_t *ep;
} cgpu_tuples_v6;

/*
 * IPv6 form of cgpu_classify_v4: ipcache_lookup6 (eps.h:56-66), egress
 * fallback CLUSTER_ID when ipv6_match_prefix_64(daddr, ROUTER_IP)
 * (bpf_lxc.c:170-191), ingress identity without the HOST_ID exception
 * (bpf_netdev.c:203-211), protocol gate ICMPv6/TCP/UDP (conntrack.h:330-378).
 * The ingress label is the resolved source identity (FROM_HOST form).
 */
int cgpu_classify_v6(cgpu_ctx *ctx, const cgpu_tuples_v6 *t, size_t n, int32_t *verdict,
		     uint32_t *identity, uint8_t *stage, void *stream);

/*
 * cgpu_classify_v4 with the egress service step of handle_ipv4_from_lxc in
 * front (bpf_lxc.c:444-469; BASELINE config 5): every egress tuple is first
 * translated by lb4_local (stateless: conntrack empty, CT_NEW), ipcache then
 * resolves the translated tuple.daddr and policy sees the rewritten dport.
 * A DROP_NO_SERVICE (-158) ends the tuple: identity 0, stage 6, metrics
 * reason 158 egress (bpf_lxc.c:659-666).  Ingress tuples are as in
 * cgpu_classify_v4.  hash: skb->hash per tuple, or NULL for cgpu_flow_hash
 * over (saddr, daddr, sport, dport, proto); sport may be NULL when hash is
 * given.
 */
int cgpu_classify_v4_lb(cgpu_ctx *ctx, const cgpu_tuples_v4 *t, const uint16_t *sport,
			const uint32_t *hash, size_t n, int32_t *verdict, uint32_t *identity,
			uint8_t *stage, void *stream);

/*
 * BASELINE config 5 whole ("prefilter -> ipcache identity -> policy verdict ->
 * LB"): cgpu_classify_v4_lb with the netdev's XDP prefilter in front of every
 * INGRESS tuple, as a packet meets xdp_start -> check_filters -> check_v4
 * (bpf_xdp.c:97-121, :158-184) before from_netdev (bpf_netdev.c:470):
 *   saddr in the dyn4 LPM (CIDR4_LPM_PREFILTER) or a fix4 /32 (CIDR4_FILTER;
 *   both per cgpu_config.prefilter_*) -> XDP_DROP; else daddr must be a key
 *   of the endpoint map (check_v4_endpoint :88-95) -> XDP_PASS, else XDP_DROP.
 * An XDP_DROP ends the tuple: verdict CGPU_VERDICT_XDP_DROP, identity 0,
 * stage 8, no policy counters and no metrics (the XDP program notifies
 * nothing).  A passed ingress tuple and every egress tuple are classified
 * exactly as cgpu_classify_v4_lb (egress: lb4_local, then ipcache / policy).
 * Replaces, for a pre-parsed batch, the XDP program + bpf_netdev.c +
 * bpf_lxc.c sequence the kernel runs per packet.
 */
#define CGPU_VERDICT_XDP_DROP (-4097)
#define CGPU_STAGE_XDP_DROP 8
int cgpu_classify_v4_cascade(cgpu_ctx *ctx, const cgpu_tuples_v4 *t, const uint16_t *sport,
			     const uint32_t *hash, size_t n, int32_t *verdict, uint32_t *identity,
			     uint8_t *stage, void *stream);

/*
 * cgpu_classify_v6 with the egress service step of ipv6_l3_from_lxc in front
 * (bpf_lxc.c:108-139): lb6_extract_key, lb6_lookup_service and lb6_local
 * (lb.h:334-483) with an empty conntrack table (CT_NEW); ipcache then
 * resolves the translated tuple->daddr and policy sees the dport ct_lookup6
 * reloads from the rewritten packet.  IPv6 has no loopback case.  A
 * DROP_NO_SERVICE (-158) ends the tuple: identity 0, stage 6, metrics reason
 * 158 egress.  hash: skb->hash per tuple or NULL for cgpu_flow_hash6 (then
 * sport is required).
 */
int cgpu_classify_v6_lb(cgpu_ctx *ctx, const cgpu_tuples_v6 *t, const uint16_t *sport,
			const uint32_t *hash, size_t n, int32_t *verdict, uint32_t *identity,
			uint8_t *stage, void *stream);

/*
 * The stateless paths above with the tunnel endpoint of every tuple as one
 * more output (cgpu_config.ipcache_tunnel).  path selects the call this is:
 * CGPU_PATH_PLAIN cgpu_classify_v4 / _v6 (sport and hash ignored),
 * CGPU_PATH_LB cgpu_classify_v4_lb / _v6_lb, CGPU_PATH_CASCADE
 * cgpu_classify_v4_cascade (IPv4 only); verdicts, identities, stages,
 * counters and metrics are that call's.
 *   tunnel[i] = the reference's local tunnel_endpoint behind bpf_lxc.c:488-491
 *   (IPv4) / :177-180 (IPv6), which :595-598 / :291-294 hand to
 *   encap_and_redirect_with_nodeid: the tunnel_endpoint of the ipcache entry
 *   the identity came from (struct remote_endpoint_info, bpf/lib/common.h:
 *   175-178; ipcache_lookup4 / 6, bpf/lib/eps.h:56-80) when the tuple is
 *   egress, reached the lookup and matched an entry with sec_label != 0;
 *   0 otherwise: ingress tuples, no match, a label-0 (tombstone) match, and
 *   tuples that end before the lookup (stage 4 protocol gate, stage 6
 *   service drop, stage 8 XDP drop).  With the service step the address
 *   looked up is the one the identity is looked up on, the daddr after
 *   translation.  The value does not depend on the policy verdict: the
 *   consumer decides about encapsulation (cgpu_forward_v4 / _v6 take this
 *   column as their `tunnel` input).  Every element is written.
 * tunnel == NULL: exactly the call `path` names.  -ENODEV on a host-only
 * context; -EINVAL for a bad path, or a non-NULL tunnel on a context without
 * cgpu_config.ipcache_tunnel.
 */
#define CGPU_PATH_PLAIN 0
#define CGPU_PATH_LB 1
#define CGPU_PATH_CASCADE 2 /* v4 only */
int cgpu_classify_v4_tun(cgpu_ctx *ctx, const cgpu_tuples_v4 *t, const uint16_t *sport,
			 const uint32_t *hash, int path, size_t n, int32_t *verdict, uint32_t *identity,
			 uint8_t *stage, uint32_t *tunnel, void *stream);
int cgpu_classify_v6_tun(cgpu_ctx *ctx, const cgpu_tuples_v6 *t, const uint16_t *sport,
			 const uint32_t *hash, int path, size_t n, int32_t *verdict, uint32_t *identity,
			 uint8_t *stage, uint32_t *tunnel, void *stream);

/*
 * The HOST-resident forms of the service, cascade and IPv6 paths: the same
 * arguments, results, counters and metrics as the device call of the same
 * name without _host, with every column and output a host pointer, streamed
 * through the staging of cgpu_classify_v4_host (same snapshot pinning, same
 * error drain, same completion on `stream`).  The service forms upload the
 * hash column when one is given (it wins over sport, as on the device), else
 * sport.  The v6 address columns need no alignment here (the staging is
 * aligned).  -ENODEV on a host-only context.
 */
int cgpu_classify_v4_lb_host(cgpu_ctx *ctx, const cgpu_tuples_v4 *t, const uint16_t *sport,
			     const uint32_t *hash, size_t n, int32_t *verdict, uint32_t *identity,
			     uint8_t *stage, void *stream);
int cgpu_classify_v4_cascade_host(cgpu_ctx *ctx, const cgpu_tuples_v4 *t, const uint16_t *sport,
				  const uint32_t *hash, size_t n, int32_t *verdict, uint32_t *identity,
				  uint8_t *stage, void *stream);
int cgpu_classify_v6_host(cgpu_ctx *ctx, const cgpu_tuples_v6 *t, size_t n, int32_t *verdict,
			  uint32_t *identity, uint8_t *stage, void *stream);
int cgpu_classify_v6_lb_host(cgpu_ctx *ctx, const cgpu_tuples_v6 *t, const uint16_t *sport,
			     const uint32_t *hash, size_t n, int32_t *verdict, uint32_t *identity,
			     uint8_t *stage, void *stream);

/* Service translation alone (device pointers). */
#define CGPU_LB_NETDEV 0 /* bpf_lb.c handle_ipv4 (bpf_lb.c:118-170) */
#define CGPU_LB_LXC 1    /* lb4_local on the endpoint egress path (bpf_lxc.c:444-460) */
/* ret codes of CGPU_LB_LXC (CGPU_LB_NETDEV returns TC_ACT_OK 0 when the
 * packet is not load-balanced, TC_ACT_REDIRECT 7 when it is) */
#define CGPU_LB_NONE 0
#define CGPU_LB_XLATED 1
#define CGPU_LB_XLATED_LOOPBACK 2 /* source NAT to IPV4_LOOPBACK, lb.h:753-767 */
#define CGPU_DROP_NO_SERVICE (-158)

typedef struct cgpu_lb4_tuples {
	const uint32_t *saddr, *daddr; /* network order */
	const uint16_t *sport, *dport; /* network order; sport only for the default hash */
	const uint8_t *proto;
	const uint32_t *hash;          /* NULL: cgpu_flow_hash */
} cgpu_lb4_tuples;

/* outputs (device pointers; all but ret may be NULL): the packet's saddr /
 * daddr / dport after lb4_xlate, the chosen entry's rev_nat_index and slave */
typedef struct cgpu_lb4_out {
	int32_t *ret;
	uint32_t *saddr, *daddr;
	uint16_t *dport, *rev_nat, *slave;
} cgpu_lb4_out;

int cgpu_lb4_select(cgpu_ctx *ctx, int mode, const cgpu_lb4_tuples *t, size_t n,
		    const cgpu_lb4_out *out, void *stream);

/* XDP prefilter over pre-parsed packets (bpf_xdp.c:88-184).
 * flags: 0 IP packet of this family, 1 truncated (-> XDP_DROP),
 *        2 not IPv4/IPv6 (-> XDP_PASS).  verdict: XDP_DROP 1 / XDP_PASS 2. */
#define CGPU_PKT_OK 0u
#define CGPU_PKT_TRUNCATED 1u
#define CGPU_PKT_NOT_IP 2u
int cgpu_prefilter_v4(cgpu_ctx *ctx, const uint32_t *saddr, const uint32_t *daddr,
		      const uint8_t *flags, size_t n, uint8_t *verdict, void *stream);
/* saddr/daddr: 16 bytes per packet, contiguous */
int cgpu_prefilter_v6(cgpu_ctx *ctx, const uint8_t *saddr, const uint8_t *daddr,
		      const uint8_t *flags, size_t n, uint8_t *verdict, void *stream);
/* the prefilters over host-resident columns (as cgpu_classify_v4_host) */
int cgpu_prefilter_v4_host(cgpu_ctx *ctx, const uint32_t *saddr, const uint32_t *daddr,
			   const uint8_t *flags, size_t n, uint8_t *verdict, void *stream);
int cgpu_prefilter_v6_host(cgpu_ctx *ctx, const uint8_t *saddr, const uint8_t *daddr,
			   const uint8_t *flags, size_t n, uint8_t *verdict, void *stream);

/* ------------------------------------------------------------------ */
/* raw Ethernet frames                               */
/* ------------------------------------------------------------------ */
/*
 * A batch of frames in one device buffer: frame i is the first
 * min(len[i], stride) bytes at data + i * stride (a fixed-size receive ring
 * slot; the rest of the slot is ignored).  stride is a multiple of 16 and
 * >= 64; data is 16-byte aligned.  len[i] is the wire length (skb->len), the
 * bound of every header read as in skb_load_bytes / revalidate_data.
 * flags[i]: CGPU_F_EGRESS = from-container (the endpoint's egress program),
 * else to-container (ingress); other bits are ignored.  ep[i] selects the
 * policy map and the cgpu_lxc_info of the endpoint.
 */
typedef struct cgpu_frames {
	const uint8_t *data;
	const uint32_t *len;
	const uint8_t *flags;
	const uint16_t *ep;
	uint32_t stride;
	uint32_t reserved;
} cgpu_frames;

/* frame status / verdict values beyond the reference's DROP_* codes */
#define CGPU_FRAME_NOT_CLASSIFIED 1 /* egress ARP (tail call to the ARP responder,
				       bpf_lxc.c:703-706), an egress ICMPv6 frame the
				       ICMPv6 responders take (bpf_lxc.c:377-386) or
				       ingress non-IP (passed to the stack,
				       bpf_netdev.c:518-520) */
#define CGPU_STAGE_NOT_CLASSIFIED 7 /* the stage cgpu_classify_frames gives such a frame */
#define CGPU_DROP_SNAPLEN (-4096)   /* a header the reference would read lies past
				       the stored slot (stride < len): re-submit
				       with a larger stride */

/* The policy tuple a frame reaches the ipcache / policy step with. */
typedef struct cgpu_frame_tuples {
	int32_t *status;   /* 0 reached policy; CGPU_FRAME_NOT_CLASSIFIED; or the
			      DROP_* / -errno the program returned before policy */
	uint8_t *family;   /* 4, 6, or 0 (not IP) */
	uint8_t *saddr;    /* 16 bytes per frame (IPv4: first 4, rest zero) */
	uint8_t *daddr;    /* 16 bytes per frame */
	uint16_t *dport;   /* tuple.dport after ct_lookup (network order; 0 without
			      CONNTRACK, i.e. ct_proto_gate = 0) */
	uint8_t *proto;    /* tuple.nexthdr (after the IPv6 extension-header walk) */
	uint8_t *flags;    /* CGPU_F_EGRESS | CGPU_F_FRAGMENT (ingress IPv4 only) */
} cgpu_frame_tuples;

/*
 * Per frame, the steps of the endpoint programs before the ipcache lookup
 * (stateless: conntrack empty, every packet CT_NEW):
 *   egress : skb->protocol dispatch (bpf_lxc.c:683-711; other than IPv4,
 *            IPv6, ARP -> DROP_UNKNOWN_L3 -139), revalidate_data (-134),
 *            handle_ipv6's ICMPv6 responders (bpf_lxc.c:364-389: an ICMPv6
 *            frame shorter than its icmp6hdr -134; a neighbour solicitation
 *            for another target DROP_UNKNOWN_TARGET -150, for ROUTER_IP -134
 *            without its ND option, else -- and an echo request to ROUTER_IP
 *            -- handed to the responder: CGPU_FRAME_NOT_CLASSIFIED), the
 *            SMAC / DMAC / SIP checks (-130 / -131 / -132), ipv6_hdrlen
 *            (-156, -157, -134), extract_l4_port of lb{4,6}_extract_key
 *            (TCP/UDP dport past len -> -14, -EFAULT of skb_load_bytes),
 *            ct_lookup{4,6} port extraction (-135 truncated L4, -137 other
 *            than ICMP/ICMPv6/TCP/UDP; with ct_proto_gate = 0 the
 *            non-CONNTRACK stubs: no port load, no gate)
 *   ingress: bpf_netdev.c dispatch (non-IP passed), ipv4_policy /
 *            ipv6_policy up to ct_lookup (bpf_lxc.c:876-897, :731-773)
 * All outputs are device pointers; any but status may be NULL.
 */
int cgpu_frames_parse(cgpu_ctx *ctx, const cgpu_frames *f, size_t n,
		      const cgpu_frame_tuples *out, void *stream);

/*
 * Frames to the columns of the STATEFUL path: cgpu_frames_parse's steps and
 * statuses, and for a frame with status 0 the fields ct_lookup4 / ct_lookup6
 * load from the packet (bpf/lib/conntrack.h:471-530, :317-378) as the columns
 * cgpu_classify_v4_ct / _v6_ct take (declared further down; len and ep are the
 * frame's own).  Such a frame has passed every one of those loads: the parse
 * bounds the TCP 14-byte and UDP 4-byte loads and the ICMP type byte (-135)
 * and the protocol gate (-137).  A frame with status != 0 gets family, saddr,
 * daddr, proto and flags as cgpu_frames_parse writes them, and sport, dport
 * and l4 of 0.  It reads the published snapshot as cgpu_frames_parse does (the
 * lxc rows, node_mac, router_ip, lb_flags).  IPv4 options and IPv6 extension
 * headers are followed; every byte read lies within min(len, stride).
 *
 * -EINVAL, judged before the context: a null struct, with n > 0 a null status,
 * data, len, flags or ep, a stride that is not a multiple of 16 or is
 * below 64, data not 16-byte aligned, a nonzero reserved, a misaligned 2-, 4-
 * or 16-byte column.  Then -ENODEV on a host-only context, then -EINVAL on a
 * context with ct_proto_gate == 0 (the stateful path is the CONNTRACK build;
 * without the gate the parse bounds no L4 load); n == 0 then returns 0.
 */
typedef struct cgpu_frame_ct_cols { /* device pointers, n elements each, frame order */
	int32_t *status;  /* required: exactly cgpu_frames_parse's status */
	uint8_t *family;  /* 4, 6, 0: as cgpu_frames_parse */
	uint8_t *saddr;   /* 16 B per frame, 16-byte aligned (IPv4: first 4, rest zero) */
	uint8_t *daddr;
	uint16_t *sport;  /* the u16 at l4 + 0 as loaded (network order), TCP / UDP; else 0 */
	uint16_t *dport;  /* the u16 at l4 + 2, TCP / UDP; else 0 (the WIRE port, not the
			     policy tuple's dport that cgpu_frames_parse reports) */
	uint8_t *proto;
	uint16_t *l4;     /* cgpu_tuples_v4_ct.l4: TCP the u16 loaded at l4 + 12 (byte 12 in
			     the low half); ICMP / ICMPv6 the type byte at l4; UDP 0 */
	uint8_t *flags;   /* CGPU_F_EGRESS | CGPU_F_FRAGMENT as cgpu_frames_parse */
} cgpu_frame_ct_cols;
int cgpu_frames_parse_ct(cgpu_ctx *ctx, const cgpu_frames *f, size_t n,
			 const cgpu_frame_ct_cols *out, void *stream);

/*
 * Raw frames to verdicts in one pass: cgpu_frames_parse, then for frames
 * that reach policy the decision of cgpu_classify_v4 / cgpu_classify_v6 on
 * that tuple (mixed IPv4 / IPv6 batches).  Frames that end before policy get
 * verdict = their status, identity 0 and stage 5 (DROP_CT_UNKNOWN_PROTO keeps
 * stage 4 as in cgpu_classify_v4; NOT_CLASSIFIED: verdict 0, stage 7, not
 * counted in the metrics).  Metrics count every other frame
 * once at {reason = -verdict (u8) or 0, dir}; SNAPLEN frames are not counted.
 */
int cgpu_classify_frames(cgpu_ctx *ctx, const cgpu_frames *f, size_t n, int32_t *verdict,
			 uint32_t *identity, uint8_t *stage, void *stream);

/*
 * cgpu_classify_frames over a HOST-resident batch (the frames as the NIC's
 * receive ring holds them, bpf_xdp.c:181-184 / bpf_netdev.c:470): f's data,
 * len, flags and ep and the outputs are host pointers; the batch streams
 * through the staging of cgpu_classify_v4_host (~1M 64-byte slots per
 * chunk), with its snapshot, error and completion rules.  Same results,
 * counters and metrics as cgpu_classify_frames of the same frames.
 */
int cgpu_classify_frames_host(cgpu_ctx *ctx, const cgpu_frames *f, size_t n, int32_t *verdict,
			      uint32_t *identity, uint8_t *stage, void *stream);

/*
 * cgpu_classify_frames with the egress service step (the stateless one of
 * cgpu_classify_v4_lb / _v6_lb: CGPU_LB_* ret codes and cgpu_flow_hash are
 * declared further down) and, with CGPU_FLB_REWRITE, what that step writes
 * into the packet: handle_ipv4_from_lxc / ipv6_l3_from_lxc from the Ethernet
 * header to ct_lookup (bpf_lxc.c:426-481, :82-163), with lb4_xlate / lb6_xlate
 * (lib/lb.h:653-697, :398-424), l4_modify_port (lib/l4.h:50-60) and
 * lib/csum.h.  Per frame, in the reference's order:
 *
 *   a. cgpu_frames_parse's steps up to and including extract_l4_port, with
 *      its statuses and its CGPU_DROP_SNAPLEN rule.  A frame that ends here,
 *      and every ingress frame, gets cgpu_classify_frames' result; lb_ret 0.
 *   b. The decision of the stateless service step on the frame's own fields:
 *      the key dport is the u16 at l4 + 2 for TCP / UDP under CGPU_LB_L4,
 *      else 0; other protocols than TCP / UDP / ICMP / ICMPv6 skip the step
 *      under CGPU_LB_L4.  The hash is hash[i], or without a hash column
 *      cgpu_flow_hash / cgpu_flow_hash6 over (saddr, daddr, sport, key dport,
 *      proto) before translation, sport = the u16 at l4 for TCP / UDP when it
 *      lies within min(len, stride), else 0.  DROP_NO_SERVICE: verdict -158,
 *      identity 0, stage 6, metrics {158, egress}; the frame is untouched.
 *   c. The rewrite of a translated frame.  With c a checksum field as loaded
 *      (little-endian load of the wire bytes, as every word below),
 *      add(a, b) = (r = a + b, r + (r < b)) in u32 and fold(t) = two rounds of
 *      t = (t & 0xffff) + (t >> 16):
 *        D   = csum_diff: from 0 (IPv4 loopback: from the daddr's D), add(D,
 *              ~w) for every old word, then add(D, w) for every new word;
 *        l3_csum_replace(off, 0, D, 0), l4_csum_replace(off, 0, D, PSEUDO_HDR):
 *              c' = (u16)~fold(add(D, ~(u32)c));
 *        l4_csum_replace(off, from, to, 2):
 *              c' = (u16)~fold(add(add(~(u32)c, ~(u32)from), to));
 *        UDP (BPF_F_MARK_MANGLED_0): a field of 0 stays 0 through every
 *              patch, a patch that yields 0 stores 0xFFFF.
 *      IPv4: daddr to bytes 30..33; on loopback IPV4_LOOPBACK to the saddr at
 *      26..29; the header checksum at 24..25 patched by D; the L4 checksum of
 *      csum_l4_offset_and_flags (TCP l4 + 16, UDP l4 + 6, protocol 58 l4 + 2;
 *      ICMP and the rest have none) patched by the same D.
 *      IPv6: daddr to bytes 38..53; the L4 checksum (TCP l4 + 16, UDP l4 + 6,
 *      ICMPv6 l4 + 2) patched by the 16-byte D.  lb6_xlate tests `if
 *      (csum_off)`, the pointer: any other next header that reaches it has
 *      the two bytes at l4 + 0 patched.
 *      Both: svc->port && key.dport != svc->port on TCP / UDP under
 *      CGPU_LB_L4 patches the L4 checksum for the port (from = key.dport) and
 *      stores the port at l4 + 2.  key.dport is the key's as the lookups left
 *      it: lb{4,6}_lookup_service set it to 0 before they try the L3 key
 *      (lib/lb.h:617, :363), so behind an L3 frontend whose backend carries a
 *      port the patch starts from 0 and not from the packet's port, as in the
 *      reference; the checksum of such a frame does not verify afterwards.
 *      An L4 checksum field past len: CGPU_DROP_CSUM_L4, verdict = that code,
 *      identity 0, stage 5, metrics {154, egress}; inside len but past the
 *      stored slot: CGPU_DROP_SNAPLEN, not counted.  A frame dropped in (b) or
 *      here keeps every byte; drop codes are decided with or without
 *      CGPU_FLB_REWRITE.  Every store lies within len once (a) has passed
 *      (extract_l4_port has loaded the dport), so CGPU_DROP_WRITE_ERROR is
 *      defined and never returned.  A translated frame stays rewritten
 *      whatever a later stage decides.
 *   d. cgpu_frames_parse's remaining steps (ct_lookup's port extraction and
 *      protocol gate) with the dport as rewritten.
 *   e. The cgpu_classify_v4 / _v6 decision on (saddr after the step,
 *      tuple.daddr, that dport, proto); on loopback tuple.daddr keeps the
 *      service address.  Counters and metrics as cgpu_classify_v4_lb / _v6_lb
 *      of that tuple.
 *
 * The frame is taken as carrying full checksums (ip_summed is not
 * CHECKSUM_PARTIAL).  Every new value is computed from the frame as it came
 * and the stores follow in the reference's order; the two differ from the
 * reference only for an IPv4 header with ihl < 5, whose L4 header overlaps
 * the IP header.  Not in scope: the stateful (_ctlb) form on frames (reverse
 * NAT on frames is cgpu_rnat_frames_v4 / _v6), a _host form, bpf_lb.c's netdev mode, and skb->csum /
 * CHECKSUM_COMPLETE bookkeeping.
 *
 * -EINVAL, judged before the context, for a null struct or a null required
 * column (data, len, flags, ep, verdict, identity), unknown flag bits, a
 * nonzero reserved, a misaligned 2- or 4-byte column, a stride that is not a
 * multiple of 16 or is below 64, or data that is not 16-byte aligned; -ENODEV
 * on a host-only context; n == 0 is a no-op.  One snapshot serves the batch.
 */
#define CGPU_FLB_REWRITE 1u
#define CGPU_DROP_WRITE_ERROR (-141) /* DROP_WRITE_ERROR, bpf/lib/common.h */
#define CGPU_DROP_CSUM_L4 (-154)     /* DROP_CSUM_L4 */

typedef struct cgpu_flb_in { /* device pointers; the slots of cgpu_frames, same stride / alignment rules */
	uint8_t *data;             /* written only with CGPU_FLB_REWRITE */
	const uint32_t *len;
	const uint8_t *flags;      /* CGPU_F_EGRESS */
	const uint16_t *ep;
	uint32_t stride, reserved; /* reserved must be 0 */
	const uint32_t *hash;      /* skb->hash per frame, or NULL (above) */
} cgpu_flb_in;

typedef struct cgpu_flb_out { /* device pointers; each may be NULL; every element of a given column is written */
	int32_t *lb_ret;           /* CGPU_LB_NONE / CGPU_LB_XLATED / CGPU_LB_XLATED_LOOPBACK, or the drop of the step */
	uint16_t *rev_nat, *slave; /* the chosen entry's, 0 where not translated */
} cgpu_flb_out;

int cgpu_classify_frames_lb(cgpu_ctx *ctx, const cgpu_flb_in *in, uint32_t flags, size_t n,
			    int32_t *verdict, uint32_t *identity, uint8_t *stage,
			    const cgpu_flb_out *lb /* may be NULL */, void *stream);

/* ------------------------------------------------------------------ */
/* conntrack: the map cilium_ct4_global               */
/* ------------------------------------------------------------------ */
/* struct ipv4_ct_tuple (bpf/lib/common.h:359-366), packed, 14 B */
#pragma pack(push, 1)
typedef struct cgpu_ct4_tuple {
	uint32_t daddr;  /* network order */
	uint32_t saddr;
	uint16_t dport;  /* network order */
	uint16_t sport;
	uint8_t nexthdr;
	uint8_t flags;   /* TUPLE_F_OUT 0 / TUPLE_F_IN 1 | TUPLE_F_RELATED 2 */
} cgpu_ct4_tuple;
#pragma pack(pop)

/* struct ct_entry (bpf/lib/common.h:380-408), 56 B */
typedef struct cgpu_ct_entry {
	uint64_t rx_packets, rx_bytes, tx_packets, tx_bytes;
	uint32_t lifetime;
	uint16_t bits;   /* rx_closing:1 tx_closing:1 nat46:1 lb_loopback:1 seen_non_syn:1 */
	uint16_t rev_nat_index;
	uint16_t slave;
	uint8_t tx_flags_seen, rx_flags_seen;
	uint32_t src_sec_id;
	uint32_t last_tx_report, last_rx_report;
} cgpu_ct_entry;

/*
 * Map operations with the bpf(2) semantics the agent's ctmap package uses
 * (pkg/maps/ctmap/ctmap.go, pkg/bpf/bpf.go:153-245): update with
 * CGPU_ANY/NOEXIST/EXIST (-EEXIST / -ENOENT), -E2BIG for a new key past
 * ct_max; delete / lookup -ENOENT; get_next_key (NULL key = first) walks the
 * map in slot order.  The device table is authoritative once a batch ran:
 * these calls synchronize with it (they are control-plane operations).
 */
int cgpu_ct4_update(cgpu_ctx *ctx, const cgpu_ct4_tuple *key, const cgpu_ct_entry *val,
		    uint64_t flags);
int cgpu_ct4_delete(cgpu_ctx *ctx, const cgpu_ct4_tuple *key);
int cgpu_ct4_lookup(cgpu_ctx *ctx, const cgpu_ct4_tuple *key, cgpu_ct_entry *val_out);
int cgpu_ct4_get_next_key(cgpu_ctx *ctx, const cgpu_ct4_tuple *key, cgpu_ct4_tuple *next_out);
size_t cgpu_ct4_count(cgpu_ctx *ctx);
/* ctmap.GC with RemoveExpired (ctmap.go:306-310, :345-357): delete every
 * entry whose lifetime < time; *deleted_out (optional) = how many */
int cgpu_ct4_gc(cgpu_ctx *ctx, uint32_t time, uint64_t *deleted_out);
/* ctmap Flush (ctmap.go:361-367): delete every entry */
int cgpu_ct4_flush(cgpu_ctx *ctx);
/* (new, diagnostic) the map's slot statistics after everything queued on it:
 * out[0] live entries, out[1] tombstones, out[2] compactions so far (a batch
 * that finds more than a quarter of the slots tombstones first re-inserts the
 * live entries into a clean table, on the device).  v6: cilium_ct6_global. */
int cgpu_ct_stats(cgpu_ctx *ctx, int v6, uint64_t *out);
/* (new, diagnostic) LRU mode's totals of the map since the context was
 * created, after everything queued on it: out[0] evictions, out[1] creates
 * that found no victim (and failed).  Zeros without ct_lru.  -EINVAL on a
 * NULL argument. */
int cgpu_ct_lru_stats(cgpu_ctx *ctx, int v6, uint64_t out[2]);

/* A batch of IPv4 packets for the stateful path (device pointers). */
typedef struct cgpu_tuples_v4_ct {
	const uint32_t *saddr; /* network order */
	const uint32_t *daddr;
	const uint16_t *sport; /* L4 header ports as on the wire (TCP/UDP) */
	const uint16_t *dport;
	const uint8_t *proto;
	const uint16_t *l4;    /* TCP: header bytes 12-13 as loaded (byte 12 in the
				  low half: doff/NS, byte 13 in the high half: flags);
				  ICMP: the type in the low byte; else ignored */
	const uint8_t *flags;  /* CGPU_F_EGRESS | CGPU_F_FRAGMENT */
	const uint32_t *len;
	const uint16_t *ep;
} cgpu_tuples_v4_ct;

/* ct_lookup4 results (bpf/lib/common.h:331-336) as reported in ct_ret[] */
#define CGPU_CT_NEW 0
#define CGPU_CT_ESTABLISHED 1
#define CGPU_CT_REPLY 2
#define CGPU_CT_RELATED 3
#define CGPU_CT_NONE 255 /* ct_lookup4 failed (DROP_CT_UNKNOWN_PROTO) */
#define CGPU_DROP_CT_CREATE_FAILED (-155)

/*
 * The stateful decision of the endpoint programs for n packets, with the
 * result of processing them IN ORDER (packet i sees every conntrack change
 * of packets < i, as the reference's programs do for a packet sequence):
 *   ct_lookup4 (bpf/lib/conntrack.h:441-561): the reply-direction tuple,
 *     then the forward one; on a hit the entry's timeout / TCP flags /
 *     closing bits / rx|tx counters are updated (:198-259);
 *   identity as cgpu_classify_v4; policy on the tuple as ct_lookup4 left it
 *     (the reply tuple's dport for CT_REPLY / CT_RELATED);
 *   CT_REPLY / CT_RELATED pass whatever policy says; otherwise a denied
 *     packet is dropped (DROP_POLICY) and, if CT_ESTABLISHED, its entry
 *     deleted; an allowed CT_NEW creates the forward entry and its ICMP
 *     related entry (ct_create4, :653-744; src_sec_id = the endpoint's
 *     SECLABEL on egress, the source identity on ingress), or fails with
 *     DROP_CT_CREATE_FAILED when the map is full;
 *   bpf_lxc.c:506-576 (egress), :918-950 (ingress).
 *   verdict[i]: DROP_* (-133, -137, -155), the proxy port (egress: any
 *               ct state; ingress: CT_NEW / CT_ESTABLISHED), else 0
 *   ct_ret[i] : CGPU_CT_*; identity[i], stage[i] as cgpu_classify_v4
 *               (stage may be NULL)
 * now = bpf_ktime_get_sec() for the batch.  Packets of one address pair are
 * resolved in order by one lane; pairs are independent.  The one departure
 * from a sequential run: which creates fail when the map fills up DURING a
 * batch depends on the order lanes reach the capacity check.
 * The context has ONE conntrack map: batches of every caller run in order
 * on the context's internal conntrack stream (after `stream` reaches the
 * call; `stream` then waits for the batch).  The host reads the map's
 * tombstone count once per call, which waits for the previous batch.
 */
int cgpu_classify_v4_ct(cgpu_ctx *ctx, const cgpu_tuples_v4_ct *t, size_t n, uint32_t now,
			int32_t *verdict, uint8_t *ct_ret, uint32_t *identity, uint8_t *stage,
			void *stream);
/* cgpu_classify_v4_ct with the tunnel endpoint of every packet's forward tuple
 * as one more output (cgpu_config.ipcache_tunnel; the rule of
 * cgpu_classify_v4_tun, bpf_lxc.c:488-491): the ipcache entry's
 * tunnel_endpoint (bpf/lib/common.h:175-178) for an egress packet whose
 * ct_lookup4 succeeded (ct_ret != CGPU_CT_NONE) and whose daddr matched an
 * entry with sec_label != 0, whatever ct_ret and the verdict are (a CT_REPLY
 * packet skips the policy, not the lookup); 0 otherwise.  Results, counters
 * and the conntrack map are cgpu_classify_v4_ct's.  tunnel == NULL: that
 * call.  -ENODEV on a host-only context, -EINVAL for a non-NULL tunnel
 * without the flag. */
int cgpu_classify_v4_ct_tun(cgpu_ctx *ctx, const cgpu_tuples_v4_ct *t, size_t n, uint32_t now,
			    int32_t *verdict, uint8_t *ct_ret, uint32_t *identity, uint8_t *stage,
			    uint32_t *tunnel, void *stream);

/* outputs of cgpu_classify_v4_ctlb (device pointers; stage, daddr, dport
 * may be NULL) */
typedef struct cgpu_ctlb_out {
	int32_t *verdict;   /* as cgpu_classify_v4_ct, plus DROP_NO_SERVICE (-158) */
	uint8_t *ct_ret;    /* the CT_EGRESS / CT_INGRESS lookup; CGPU_CT_NONE for a
			       service drop or DROP_CT_UNKNOWN_PROTO */
	uint32_t *identity; /* 0 for a service drop */
	uint8_t *stage;     /* as cgpu_classify_v4_ct; 6 = service drop */
	uint32_t *daddr;    /* the frame's daddr after the service step (lb4_xlate) */
	uint16_t *dport;    /* the frame's dport after it (network order) */
} cgpu_ctlb_out;

/*
 * cgpu_classify_v4_ct with the STATEFUL service step of handle_ipv4_from_lxc
 * in front (bpf_lxc.c:444-469; lb4_local with CONNTRACK, lib/lb.h:700-775),
 * packets processed in order as the reference's programs would:
 *   egress packets whose {daddr, dport} (or {daddr, 0}) is a service
 *   (lb4_extract_key / lb4_lookup_service, lb.h:590-635) look up their
 *   CT_SERVICE entry (ct_lookup4 with TUPLE_F_SERVICE, no forward lookup):
 *   CT_NEW selects slave = hash % count + 1 and creates the entry and its
 *   ICMP entry (src_sec_id 0) -- a failed create drops the packet with
 *   DROP_NO_SERVICE (fail closed); a hit reuses the stored slave (and
 *   lb_loopback).  A slave whose backend is gone falls back to
 *   lb4_lookup_service with key.slave kept, re-selects from that entry's
 *   count and rewrites the entry's slave (ct_update4_slave); no service ->
 *   DROP_NO_SERVICE.  Loopback (saddr == target): source NAT to
 *   IPV4_LOOPBACK and tuple.daddr keeps the service address.
 *   Then the egress conntrack path of cgpu_classify_v4_ct on the translated
 *   tuple: ipcache of tuple.daddr, policy on the rewritten dport, and an
 *   allowed CT_NEW creates its entry with the service's rev_nat_index,
 *   slave and lb_loopback, the address entry of ct_create4 (tuple->daddr :=
 *   backend or IPV4_LOOPBACK; conntrack.h:697-725) and the ICMP entry.
 *   A hit entry's reverse NAT changes the frame only (lb.h:562-576): no
 *   output of this call depends on it; cgpu_classify_v4_ctlb_rnat reports
 *   it.  Ingress packets are as cgpu_classify_v4_ct.
 * hash: skb->hash per packet (NULL: cgpu_flow_hash over the 5-tuple).
 * Service drops: verdict -158, ct_ret CGPU_CT_NONE, identity 0, stage 6,
 * metrics reason 158 egress.  Ordering, streams and the capacity caveat as
 * cgpu_classify_v4_ct (an address entry's capacity is taken when its create
 * runs).  n < 2^30.
 */
int cgpu_classify_v4_ctlb(cgpu_ctx *ctx, const cgpu_tuples_v4_ct *t, const uint32_t *hash, size_t n,
			  uint32_t now, const cgpu_ctlb_out *out, void *stream);

/* ------------------------------------------------------------------ */
/* conntrack, IPv6: the map cilium_ct6_global (CT_MAP6, bpf_lxc.c:53-63) */
/* ------------------------------------------------------------------ */
/* struct ipv6_ct_tuple (bpf/lib/common.h:338-346), packed, 38 B */
#pragma pack(push, 1)
typedef struct cgpu_ct6_tuple {
	uint8_t daddr[16]; /* network order */
	uint8_t saddr[16];
	uint16_t dport;    /* network order */
	uint16_t sport;
	uint8_t nexthdr;
	uint8_t flags;     /* TUPLE_F_OUT 0 / TUPLE_F_IN 1 | TUPLE_F_RELATED 2 */
} cgpu_ct6_tuple;
#pragma pack(pop)

/* The cgpu_ct4_* map operations on cilium_ct6_global (capacity
 * cgpu_config.ct6_max, default ct_max). */
int cgpu_ct6_update(cgpu_ctx *ctx, const cgpu_ct6_tuple *key, const cgpu_ct_entry *val,
		    uint64_t flags);
int cgpu_ct6_delete(cgpu_ctx *ctx, const cgpu_ct6_tuple *key);
int cgpu_ct6_lookup(cgpu_ctx *ctx, const cgpu_ct6_tuple *key, cgpu_ct_entry *val_out);
int cgpu_ct6_get_next_key(cgpu_ctx *ctx, const cgpu_ct6_tuple *key, cgpu_ct6_tuple *next_out);
size_t cgpu_ct6_count(cgpu_ctx *ctx);
int cgpu_ct6_gc(cgpu_ctx *ctx, uint32_t time, uint64_t *deleted_out);
int cgpu_ct6_flush(cgpu_ctx *ctx);

/* A batch of IPv6 packets for the stateful path (device pointers). */
typedef struct cgpu_tuples_v6_ct {
	const uint8_t *saddr;  /* 16 bytes per packet, network order; 16-byte aligned */
	const uint8_t *daddr;
	const uint16_t *sport; /* L4 header ports as on the wire (TCP/UDP) */
	const uint16_t *dport;
	const uint8_t *proto;  /* nexthdr after the extension headers */
	const uint16_t *l4;    /* TCP: header bytes 12-13 as loaded; ICMPv6: the type
				  in the low byte; else ignored */
	const uint8_t *flags;  /* CGPU_F_EGRESS (IPv6 has no fragment flag) */
	const uint32_t *len;
	const uint16_t *ep;
} cgpu_tuples_v6_ct;

/*
 * cgpu_classify_v4_ct for IPv6 over cilium_ct6_global, in the order of
 * ipv6_l3_from_lxc (egress, bpf_lxc.c:108-203) and ipv6_policy (ingress,
 * :731-800): ct_lookup6 (conntrack.h:288-412; ICMPv6 errors 1-4 RELATED,
 * echo request / reply ports 128), identity as cgpu_classify_v6, policy on
 * the tuple ct_lookup6 left, ct_delete6 of a denied ESTABLISHED entry,
 * ct_create6 (:588-639, with its ICMPv6 related entry) of an allowed CT_NEW
 * packet.  An ingress entry is created with rev_nat_index =
 * daddr.s6_addr32[3] & 0xFFFF (bpf_lxc.c:748); a hit entry's reverse NAT
 * (lib/lb.h:305-317) changes the frame only: no output of this call depends
 * on it; cgpu_classify_v6_ct_rnat reports it.  Outputs, ordering and the
 * capacity caveat as cgpu_classify_v4_ct.
 */
int cgpu_classify_v6_ct(cgpu_ctx *ctx, const cgpu_tuples_v6_ct *t, size_t n, uint32_t now,
			int32_t *verdict, uint8_t *ct_ret, uint32_t *identity, uint8_t *stage,
			void *stream);
/* as cgpu_classify_v4_ct_tun over IPv6 (bpf_lxc.c:177-180) */
int cgpu_classify_v6_ct_tun(cgpu_ctx *ctx, const cgpu_tuples_v6_ct *t, size_t n, uint32_t now,
			    int32_t *verdict, uint8_t *ct_ret, uint32_t *identity, uint8_t *stage,
			    uint32_t *tunnel, void *stream);

/* cgpu_classify_v6_ctlb's outputs: as cgpu_ctlb_out with the frame's daddr
 * 16 bytes per packet (16-byte aligned) */
typedef struct cgpu_ctlb6_out {
	int32_t *verdict;
	uint8_t *ct_ret;
	uint32_t *identity;
	uint8_t *stage;
	uint8_t *daddr;     /* [n][16]: the frame's daddr after lb6_xlate */
	uint16_t *dport;
} cgpu_ctlb6_out;

/*
 * cgpu_classify_v6_ct with the stateful service step of ipv6_l3_from_lxc in
 * front (bpf_lxc.c:122-146; lb6_local with CONNTRACK, lib/lb.h:426-483):
 * egress packets whose {daddr, dport} (or {daddr, 0}) is an IPv6 service
 * (lb6_extract_key / lb6_lookup_service, lb.h:327-365) look up their
 * CT_SERVICE entry in cilium_ct6_global; CT_NEW selects slave = hash % count
 * + 1 and creates it (ct_create6 with its ICMPv6 entry; a failed create
 * drops with DROP_NO_SERVICE), a hit reuses the stored slave; a slave whose
 * backend is gone falls back to lb6_lookup_service with key.slave kept and
 * ct_update6_slave; no service -> DROP_NO_SERVICE.  lb6_xlate rewrites the
 * frame's daddr (and the dport for TCP / UDP under CGPU_LB_L4); the tuple's
 * daddr becomes the backend, its dport the rewritten one.  Then the egress
 * conntrack path of cgpu_classify_v6_ct on that tuple, identity from the
 * ipcache of the backend, CT_NEW creates the entry with the service's
 * rev_nat_index and slave (ct_create6 writes no address entry).  Outputs as
 * cgpu_classify_v4_ctlb.  n < 2^30; address columns 16-byte aligned.
 */
int cgpu_classify_v6_ctlb(cgpu_ctx *ctx, const cgpu_tuples_v6_ct *t, const uint32_t *hash, size_t n,
			  uint32_t now, const cgpu_ctlb6_out *out, void *stream);

/* ------------------------------------------------------------------ */
/* reverse NAT of service replies on the conntrack paths                */
/* ------------------------------------------------------------------ */
/*
 * The frame's source (IPv4: and destination) fields as the endpoint program
 * leaves them, per packet (device pointers, each may be NULL).  They start
 * as the input, on the _ctlb paths as the service step left them (daddr :=
 * the backend; IPv4 saddr := IPV4_LOOPBACK when the backend is the sender,
 * lb.h:761-766), and change where the program calls lb4_rev_nat / lb6_rev_nat
 * with the ct_state of the entry the packet hit:
 *   IPv4 egress  (bpf_lxc.c:531-541): ct_ret REPLY or RELATED, rev_nat_index != 0
 *   IPv4 ingress (bpf_lxc.c:909-918): ct_ret REPLY only, rev_nat_index != 0,
 *                                     !lb_loopback (REV_NAT_F_TUPLE_SADDR: the
 *                                     same frame result)
 *   IPv6 egress  (bpf_lxc.c:222-235): ct_ret REPLY or RELATED, rev_nat_index != 0
 *   IPv6 ingress (bpf_lxc.c:778-785): any hit (ESTABLISHED too) whose entry has
 *                                     rev_nat_index != 0; a CT_NEW packet never
 * The index is looked up as stored (lb.h:570 / :312); a miss changes nothing
 * (applied 0).  A hit (applied 1) is __lb4_rev_nat (lb.h:485-550) /
 * __lb6_rev_nat (:254-294): when nat->port != 0 the source port of a TCP or
 * UDP frame := nat->port (reverse_map_l4_port, :218-252; ICMP keeps its port
 * word; its DROP_UNKNOWN_L4 is unreachable behind ct_lookup's protocol gate);
 * IPv4 with the entry's lb_loopback: daddr := the old saddr; saddr :=
 * nat->address.  Verdicts, ct_ret, identities, counters, metrics and both
 * maps do not depend on this step.  These calls return the fields as columns;
 * cgpu_rnat_frames_v4 / _v6, below, write them into raw frames, checksums
 * included.
 */
typedef struct cgpu_rnat4_out {
	uint32_t *saddr, *daddr; /* network order */
	uint16_t *sport;
	uint8_t *applied;        /* 1: the map held the index and __lb4_rev_nat ran */
} cgpu_rnat4_out;
typedef struct cgpu_rnat6_out {
	uint8_t *saddr;          /* [n][16], 16-byte aligned */
	uint16_t *sport;
	uint8_t *applied;
} cgpu_rnat6_out;

/* The calls they extend, with that output; rn == NULL: exactly those calls
 * (their kernels).  With rn the conntrack walks run instantiations that also
 * store the hit entry's rev_nat_index | lb_loopback << 16 per packet, and a
 * rewrite pass follows the finish.  -ENODEV on a host-only context. */
int cgpu_classify_v4_ct_rnat(cgpu_ctx *ctx, const cgpu_tuples_v4_ct *t, size_t n, uint32_t now,
			     int32_t *verdict, uint8_t *ct_ret, uint32_t *identity, uint8_t *stage,
			     const cgpu_rnat4_out *rn, void *stream);
int cgpu_classify_v4_ctlb_rnat(cgpu_ctx *ctx, const cgpu_tuples_v4_ct *t, const uint32_t *hash, size_t n,
			       uint32_t now, const cgpu_ctlb_out *out, const cgpu_rnat4_out *rn,
			       void *stream);
int cgpu_classify_v6_ct_rnat(cgpu_ctx *ctx, const cgpu_tuples_v6_ct *t, size_t n, uint32_t now,
			     int32_t *verdict, uint8_t *ct_ret, uint32_t *identity, uint8_t *stage,
			     const cgpu_rnat6_out *rn, void *stream);
int cgpu_classify_v6_ctlb_rnat(cgpu_ctx *ctx, const cgpu_tuples_v6_ct *t, const uint32_t *hash, size_t n,
			       uint32_t now, const cgpu_ctlb6_out *out, const cgpu_rnat6_out *rn,
			       void *stream);

/*
 * Reverse NAT on raw frames: what __lb4_rev_nat / __lb6_rev_nat (lib/lb.h:
 * 485-550, :254-294) write into the packet, with reverse_map_l4_port /
 * l4_modify_port (lb.h:218-252, lib/l4.h:50-60) and lib/csum.h, for the
 * decision a cgpu_classify_v{4,6}_ct{,lb}_rnat call has made: a call behind
 * those, as cgpu_forward_frames is a call behind the classify calls.  The
 * inputs are the slots of cgpu_frames and the columns the _rnat call wrote
 * for the same packets; frame i must be the frame whose fields were packet i
 * of that call.  No table is read (the reverse-NAT map lookup has happened).
 *
 * Left alone (every byte kept, ret 0): a frame with applied[i] == 0 (its slot
 * and its saddr / daddr / sport elements are not read); a frame whose
 * ethertype is not the call's family; a frame whose fixed header (34 bytes
 * IPv4, 54 bytes IPv6) does not lie within min(len, stride); and a frame that
 * cannot have passed ct_lookup: an IPv6 frame whose ipv6_hdrlen walk (the
 * parse's, cgpu_frames_parse) fails, a protocol other than TCP / UDP / ICMP
 * (IPv4) or TCP / UDP / ICMPv6 (IPv6), a TCP / UDP frame whose u16 at l4 + 0
 * does not lie within min(len, stride).
 *
 * Offsets: IPv4 l4 = 14 + ihl * 4 and the header's protocol; IPv6 l4 = 14 +
 * ipv6_hdrlen and nexthdr as that walk leaves it.  The L4 checksum field of
 * csum_l4_offset_and_flags: TCP l4 + 16, UDP l4 + 6 (BPF_F_MARK_MANGLED_0),
 * ICMPv6 l4 + 2, IPv4 ICMP none.
 *
 * The rewrite of a frame with applied[i] == 1, in the reference's order, with
 * the arithmetic of cgpu_classify_frames_lb (add, fold, csum_diff, the two
 * csum_replace forms, the UDP rule) on the words as loaded:
 *   1. TCP / UDP, sport[i] != the u16 at l4 + 0 (the _rnat call leaves sport
 *      unchanged when nat->port == 0, so this is the reference's `port &&
 *      port != old_port`): l4_csum_replace(off, old_port, sport, 2), then the
 *      port to l4 + 0.
 *   2. IPv4, daddr[i] != the frame's daddr (ct_state->loopback, whose new
 *      daddr is the old saddr): daddr to bytes 30..33, D = csum_diff(old_dip,
 *      new_dip, 0).  Loopback is inferred from the columns: where the
 *      reference's branch runs with old saddr == old daddr this call starts
 *      from D = 0 where the reference starts from add(0xFFFFFFFF - x, x) =
 *      0xFFFFFFFF; every use of D is add(D, ~(u32)c) with ~(u32)c >=
 *      0xFFFF0000, and add(0xFFFFFFFF, y) == y for y >= 1, so the stored
 *      checksums are the same.
 *   3. saddr[i] to bytes 26..29 (IPv6: 22..37), D = csum_diff(old_sip,
 *      new_sip, D).
 *   4. IPv4: the header checksum at 24..25 patched by D.
 *   5. The L4 checksum patched by D with BPF_F_PSEUDO_HDR: IPv4 where the
 *      protocol has a checksum offset, IPv6 always.
 *   6. UDP: a checksum field of 0 stays 0 through every patch, a patch that
 *      yields 0 stores 0xFFFF.
 *
 * ret[i] (may be NULL), decided with or without CGPU_RNF_REWRITE: an L4
 * checksum field the step must patch that lies past len: CGPU_DROP_CSUM_L4;
 * inside len but past the stored slot: CGPU_DROP_SNAPLEN (an IPv6 TCP frame
 * needs slots of 80 bytes or more); else 0.  A dropped frame keeps every
 * byte (the convention of cgpu_classify_frames_lb; without a port change the
 * reference would already have stored the L3 part before the L4 patch
 * fails).  Every store lies within len (ct_lookup has loaded the ports), so
 * CGPU_DROP_WRITE_ERROR is never returned.  The endpoint program returns this
 * code in place of its verdict (bpf_lxc.c:538-539, :916-917, :783-784): the
 * call reports it, the caller combines it.
 *
 * The frame is taken as carrying full checksums.  Every new value is
 * computed from the frame as it came and the stores follow in the
 * reference's order; the two differ from the reference only for an IPv4
 * header with ihl < 5.  Not in scope: the IPv6 ingress daddr with its index
 * bits cleared (bpf_lxc.c:753-769), a frame of the _ctlb paths that was both
 * service-translated and reverse-NATed (the stateful service rewrite does not
 * exist on frames), a _host form, and skb->csum bookkeeping.
 *
 * -EINVAL, judged before the context, for a null struct or a null required
 * column (data, len, applied, saddr, sport; IPv4: daddr), unknown flag bits,
 * a nonzero reserved, a misaligned 2- / 4- / 16-byte column (ret included), a
 * stride that is not a multiple of 16 or is below 64, or data that is not
 * 16-byte aligned; n == 0 is a no-op that returns 0; -ENODEV on a host-only
 * context.
 */
#define CGPU_RNF_REWRITE 1u

typedef struct cgpu_rnf4_in { /* device pointers */
	uint8_t *data;                 /* slots as cgpu_frames; written only with CGPU_RNF_REWRITE */
	const uint32_t *len;
	uint32_t stride, reserved;     /* stride: multiple of 16, >= 64; reserved 0 */
	const uint8_t *applied;        /* cgpu_rnat4_out.applied */
	const uint32_t *saddr, *daddr; /* cgpu_rnat4_out.saddr / .daddr */
	const uint16_t *sport;         /* cgpu_rnat4_out.sport */
} cgpu_rnf4_in;
typedef struct cgpu_rnf6_in { /* device pointers */
	uint8_t *data;
	const uint32_t *len;
	uint32_t stride, reserved;
	const uint8_t *applied;        /* cgpu_rnat6_out.applied */
	const uint8_t *saddr;          /* cgpu_rnat6_out.saddr: [n][16], 16-byte aligned */
	const uint16_t *sport;         /* cgpu_rnat6_out.sport */
} cgpu_rnf6_in;

int cgpu_rnat_frames_v4(cgpu_ctx *ctx, const cgpu_rnf4_in *in, uint32_t flags, size_t n,
			int32_t *ret /* may be NULL */, void *stream);
int cgpu_rnat_frames_v6(cgpu_ctx *ctx, const cgpu_rnf6_in *in, uint32_t flags, size_t n,
			int32_t *ret /* may be NULL */, void *stream);

/*
 * The stateful decision on a mixed batch of raw frames: cgpu_frames_parse_ct,
 * then the conntrack calls on the frames that reach conntrack, their results
 * back at the frames' indices.  The call pins ONE snapshot for all it does.
 *
 * A frame with status 0 and family 4 is a packet of cgpu_classify_v4_ct (with
 * the rn group given: of cgpu_classify_v4_ct_rnat), one with family 6 a packet
 * of cgpu_classify_v6_ct (_rnat), on the columns of cgpu_frames_parse_ct and
 * the frame's len and ep.  The packets of each family run in frame order; the
 * two families use different maps (cilium_ct4_global, cilium_ct6_global), so
 * the result is that of processing the whole batch in order.  Each such
 * frame's verdict, ct_ret, identity, stage and rn elements are that call's
 * outputs for that packet (rn_saddr4 / rn_daddr4 of an IPv6 frame and
 * rn_saddr6 of an IPv4 frame are 0).  Policy counters, metrics, the conntrack
 * maps and LRU mode (ct_lru) are those calls', because those calls run.
 *
 * A frame that ends before conntrack (status != 0) gets cgpu_classify_frames'
 * result: verdict = status (0 for CGPU_FRAME_NOT_CLASSIFIED), identity 0,
 * stage 5 (4 for DROP_CT_UNKNOWN_PROTO, 7 for not classified), ct_ret
 * CGPU_CT_NONE, every rn element 0; it is counted in the metrics once at
 * {reason = (-status) & 0xff, dir} with its len, not-classified and
 * CGPU_DROP_SNAPLEN frames not at all.  For a -137 frame that is what
 * cgpu_classify_v4_ct reports for a packet of that protocol.
 *
 * The plain conntrack form: no service step runs in front (a _ctlb form on
 * frames does not exist).  cgpu_rnat_frames_v4 / _v6 take the rn columns as
 * they are, one call per family on the same frames: each leaves the other
 * family's frames alone.
 *
 * Scratch: per context, grow-only, freed by cgpu_ctx_destroy; 125 bytes per
 * frame of the largest batch seen (the parsed columns 42, two index lists 8,
 * the compacted packets and their results at most 75) besides the conntrack
 * calls' own.  Calls on one context serialise on it.  Like the conntrack
 * calls, the call waits on the host (once on `stream` for the two packet
 * counts, beside those calls' own wait) and may allocate: it cannot be
 * captured into a graph.
 *
 * -EINVAL, judged before the context: cgpu_frames_parse_ct's argument rules
 * (status and family are optional here; verdict, ct_ret and identity
 * required), an rn group given in part, a misaligned column, n > INT32_MAX.
 * Then -ENODEV on a host-only context, then -EINVAL with ct_proto_gate == 0;
 * n == 0 then returns 0.
 */
typedef struct cgpu_fct_out { /* device pointers, n elements each, frame order */
	int32_t *status;   /* optional: the parse's status */
	uint8_t *family;   /* optional */
	int32_t *verdict;  /* required */
	uint8_t *ct_ret;   /* required */
	uint32_t *identity; /* required */
	uint8_t *stage;    /* optional */
	/* reverse NAT: all five NULL (the plain calls run) or all five given (the _rnat calls run) */
	uint8_t *rn_applied;
	uint16_t *rn_sport;
	uint32_t *rn_saddr4, *rn_daddr4; /* cgpu_rnat4_out.saddr / .daddr of the IPv4 frames */
	uint8_t *rn_saddr6;              /* [n][16], 16-byte aligned: cgpu_rnat6_out.saddr */
} cgpu_fct_out;
int cgpu_classify_frames_ct(cgpu_ctx *ctx, const cgpu_frames *f, size_t n, uint32_t now,
			    const cgpu_fct_out *out, void *stream);

/* ------------------------------------------------------------------ */
/* checkpoint / resume                                      */
/* ------------------------------------------------------------------ */
/* The host mirror is authoritative (the device is rebuilt from it at any
 * commit), so a checkpoint is the mirror written to a file: every ipcache,
 * policy (with each entry's packets / bytes counters), prefilter CIDR,
 * endpoint, lb4 / lb6 and lxc entry, the PreFilter revision, both
 * conntrack maps and both reverse-NAT maps (a file written before those two
 * sections existed restores with them empty).  The reference's counterpart is its maps pinned in bpffs
 * plus the ipcache replay into listeners (pkg/ipcache/ipcache.go:328-338).
 * save: atomic (written to path.tmp, then renamed).  restore: into a context
 * whose maps are all empty (else -EEXIST); the file is validated whole
 * (-EINVAL on a bad header, section or checksum) and replayed through the
 * map calls with BPF_NOEXIST (capacity errors are returned as those calls
 * return them).  The tables reach the device at the next cgpu_commit.  The
 * {reason, dir} metrics are not part of a checkpoint (they restart at 0). */
int cgpu_mirror_save(cgpu_ctx *ctx, const char *path);
int cgpu_mirror_restore(cgpu_ctx *ctx, const char *path);

/* ------------------------------------------------------------------ */
/* L3 MapState compilation                           */
/* ------------------------------------------------------------------ */
/* The label decision computeDesiredL3PolicyMapEntries asks of the policy
 * repository for every (endpoint, identity) pair (pkg/endpoint/policy.go:
 * 317-390): Repository.AllowsIngressLabelAccess / AllowsEgressLabelAccess
 * (pkg/policy/repository.go:80-130, :443-490) over rule.canReachIngress /
 * canReachEgress (pkg/policy/rule.go:323-405).  Strings are interned by the
 * caller (cilium_amd/policy.py); every id below is such an interned id. */
#define CGPU_SEL_IN 0         /* In / = / ==: Has(key) && Get(key) in values */
#define CGPU_SEL_NOT_IN 1     /* NotIn / !=: !Has(key) || Get(key) not in values */
#define CGPU_SEL_EXISTS 2
#define CGPU_SEL_NOT_EXISTS 3 /* DoesNotExist */

/* a label of a LabelArray: ids of its key, of "source.key" and of its value */
typedef struct cgpu_label {
	uint32_t key, ext_key, value;
} cgpu_label;

/* labels.Requirement: any_source -> key is a key id matched against every
 * label's key (LabelArray.Has/Get with source "any", pkg/labels/array.go:
 * 92-130); else key is an ext_key id matched against "source.key" */
typedef struct cgpu_requirement {
	uint32_t any_source, key, op, values_off, n_values;
} cgpu_requirement;

/* EndpointSelector: requirements [reqs_off, +n_reqs), all must match;
 * match_all = matchLabels holds "reserved.all" (selector.go:290-294) */
typedef struct cgpu_selector {
	uint32_t reqs_off, n_reqs, match_all;
} cgpu_selector;

#define CGPU_L3_INGRESS 0
#define CGPU_L3_EGRESS 1
#define CGPU_L3_REQUIRES 0 /* FromRequires / ToRequires: must match, else Denied */
#define CGPU_L3_ALLOWS 1   /* FromEndpoints / ToEndpoints: match without ToPorts -> Allowed */
typedef struct cgpu_l3_clause {
	uint32_t dir, kind, selector, has_ports;
} cgpu_l3_clause;

typedef struct cgpu_l3_program {
	const cgpu_selector *selectors;
	uint32_t n_selectors;
	const cgpu_requirement *reqs;
	uint32_t n_reqs;
	const uint32_t *values;
	uint32_t n_values;
	const uint32_t *rule_subject; /* per rule: its EndpointSelector */
	const uint32_t *rule_clauses; /* n_rules + 1 offsets into clauses */
	uint32_t n_rules;
	const cgpu_l3_clause *clauses;
	uint32_t n_clauses;
} cgpu_l3_program;

/* label arrays: set i = labels[offsets[i] .. offsets[i + 1]) in array order */
typedef struct cgpu_label_sets {
	const uint32_t *offsets;
	const cgpu_label *labels;
	uint32_t n_sets;
} cgpu_label_sets;

#define CGPU_L3_INGRESS_ENFORCED 1u /* else ingress allows all (policy.go:351-360) */
#define CGPU_L3_EGRESS_ENFORCED 2u
/*
 * allow_out[e * n_identities + i] (host memory) = bit 0: ingress from
 * identity i to endpoint e is Allowed; bit 1: egress from e to i is Allowed.
 * All inputs are host pointers (a control-plane call: it uploads, evaluates
 * every pair on the device, one lane per pair, and copies the result back).
 */
int cgpu_l3_compile(cgpu_ctx *ctx, const cgpu_l3_program *prog, const cgpu_label_sets *endpoints,
		    const cgpu_label_sets *identities, uint32_t flags, uint8_t *allow_out);

/* ------------------------------------------------------------------ */
/* full MapState: L4 + localhost/world + L3 keys, synced into the maps  */
/* (pkg/endpoint/policy.go:143-390, endpoint.go:2572)   */
/* ------------------------------------------------------------------ */
/* One L4Filter of an endpoint's resolved L4 policy (pkg/policy/l4.go:83-103),
 * as Repository.ResolveL4{Ingress,Egress}Policy (repository.go:240-329) left
 * it, wildcardL3L4Rules included; the caller (cilium_amd/policy.py) resolves
 * the filters, which is O(rules) per endpoint.  Its Endpoints selectors are
 * ids into the program's selector table. */
typedef struct cgpu_l4_filter {
	uint32_t endpoint;         /* row of the endpoint label sets */
	uint32_t sels_off, n_sels; /* selectors filter_sels[sels_off, +n_sels) */
	uint16_t port;             /* L4Filter.Port, host order */
	uint8_t proto;             /* L4Filter.U8Proto */
	uint8_t dir;               /* CGPU_L3_INGRESS / CGPU_L3_EGRESS */
	uint16_t proxy_port;       /* realizedRedirects[ProxyID] (host order) of a redirect */
	uint8_t redirect;          /* L7Parser != "": no keys while proxy_port is 0 (policy.go:158-166) */
	uint8_t pad;
} cgpu_l4_filter;

#define CGPU_MS_ALLOW_LOCALHOST 4u   /* AlwaysAllowLocalhost() || DesiredL4Policy.HasRedirect() */
#define CGPU_MS_HOST_ALLOWS_WORLD 8u /* option HostAllowsWorld (policy.go:305-315) */
typedef struct cgpu_mapstate_spec {
	const cgpu_l4_filter *filters;
	uint32_t n_filters;
	const uint32_t *filter_sels;
	uint32_t n_filter_sels;
	const uint32_t *ep_map;   /* [n_endpoints] the policy-map index (`ep`) of each endpoint row */
	const uint32_t *ep_flags; /* [n_endpoints] CGPU_L3_*_ENFORCED | CGPU_MS_* */
	const uint32_t *identity; /* [n_identities] NumericIdentity of each identity row */
} cgpu_mapstate_spec;

typedef struct cgpu_mapstate_stats {
	uint64_t desired;   /* keys in the desired MapStates */
	uint64_t added;     /* AllowKey of a key the map did not hold */
	uint64_t updated;   /* AllowKey of a held key with another proxy port (counters restart) */
	uint64_t deleted;   /* DeleteKey of a held key no longer desired */
	uint64_t unchanged; /* desired keys already held with the same proxy port */
	uint64_t failed;    /* AllowKey / DeleteKey errors (e.g. -E2BIG) */
} cgpu_mapstate_stats;

/*
 * computeDesiredPolicyMapState for every endpoint row, then syncPolicyMap
 * into that endpoint's policy map:
 *   1. L4 keys {identity, port, proto, dir} -> proxy_port for every identity
 *      any of a filter's selectors matches (computeDesiredL4PolicyMapEntries,
 *      policy.go:143-192); one wave per (filter, 64 identities) on the device;
 *   2. {HOST_ID, 0, 0, ingress} if CGPU_MS_ALLOW_LOCALHOST, then
 *      {WORLD_ID, 0, 0, ingress} if also CGPU_MS_HOST_ALLOWS_WORLD
 *      (determineAllowLocalhost / determineAllowFromWorld, policy.go:284-315);
 *   3. the L3 keys of cgpu_l3_compile under the endpoint's enforcement bits
 *      (policy.go:317-390).
 * Sync (endpoint.go:2572-2652): held keys not desired are deleted; desired
 * keys absent or held with another proxy port are written (the value, and
 * with it the counters, restart); the rest are left alone.  Like the
 * reference, a failing key does not stop the others: the first error is
 * returned after all keys were tried.  Changes go to the host mirror and
 * become visible to classify at the next cgpu_commit (a small delta patches
 * the device tables in place).  All inputs are host pointers.
 */
int cgpu_mapstate_sync(cgpu_ctx *ctx, const cgpu_l3_program *prog, const cgpu_label_sets *endpoints,
		       const cgpu_label_sets *identities, const cgpu_mapstate_spec *spec,
		       cgpu_mapstate_stats *stats);

/* ------------------------------------------------------------------ */
/* forwarding decision of allowed packets                               */
/* ------------------------------------------------------------------ */
/*
 * Where a packet goes once a classify call allowed it: the rest of
 * handle_ipv4_from_lxc / ipv6_l3_from_lxc (bpf_lxc.c:547-657, :242-354,
 * CGPU_FWD_LXC) and of the netdev's handle_ipv4 / handle_ipv6
 * (bpf_netdev.c:422-452, :240-274, CGPU_FWD_NETDEV).  A call of its own, run
 * after a classify call on columns the caller already has; it walks no
 * ipcache and touches no counter, metric or conntrack entry.
 *
 * CGPU_FWD_LXC, per packet in this order:
 *   1. no CGPU_F_EGRESS: NONE, all outputs 0 (the to-container program's
 *      delivery is the redirect a LOCAL result already stands for);
 *   2. verdict < 0: DROP, ret = verdict;
 *   3. verdict > 0: PROXY, arg = verdict, ifindex = host_ifindex      [ttl]
 *   4. cilium_lxc holds daddr: with ENDPOINT_F_HOST HOST, ifindex =
 *      host_ifindex; else LOCAL, ifindex = ep->ifindex, arg = lxc_id   [ttl]
 *   5. CGPU_FWD_ENCAP: tunnel != 0: OVERLAY, arg = tunnel, ifindex =
 *      encap_ifindex; else a cilium_tunnel_map hit on {daddr & ipv4_mask} /
 *      {daddr / 96}: OVERLAY, arg = the value's ip4 word;
 *   6. STACK                                                           [ttl]
 * CGPU_FWD_NETDEV (verdict and flags are not read):
 *   1. cilium_lxc holds daddr: with ENDPOINT_F_HOST STACK, else LOCAL  [ttl]
 *   2. CGPU_FWD_ENCAP: tunnel != 0: OVERLAY; else, only where (daddr &
 *      ipv4_cluster_mask) == ipv4_cluster_range (IPv6: daddr's first 96 bits
 *      are ROUTER_IP's), the tunnel map as above;
 *   3. STACK.
 * [ttl]: the branch calls ipv4_l3 / ipv6_l3, so a packet with ttl <= 1 ends
 * there instead: IPv4 DROP with ret CGPU_DROP_INVALID (lib/l3.h:57-60), IPv6
 * TIME_EXCEEDED with the other outputs 0 (lib/l3.h:36-43).  Encapsulation
 * does not decrement.  The MAC rewrite, the decrement itself and checksums
 * are packet rewriting and not done here: cgpu_forward_frames, below, makes
 * the same decision on raw frames and rewrites them.
 */
#define CGPU_FWD_LXC 0u
#define CGPU_FWD_NETDEV 1u
#define CGPU_FWD_ENCAP 1u /* cgpu_fwd_params.flags: the ENCAP_IFINDEX build */

#define CGPU_FWD_NONE 0
#define CGPU_FWD_DROP 1
#define CGPU_FWD_PROXY 2
#define CGPU_FWD_LOCAL 3
#define CGPU_FWD_HOST 4
#define CGPU_FWD_OVERLAY 5
#define CGPU_FWD_STACK 6
#define CGPU_FWD_TIME_EXCEEDED 7
#define CGPU_DROP_INVALID (-134) /* DROP_INVALID, bpf/lib/common.h */

typedef struct cgpu_fwd_params {
	uint32_t mode;          /* CGPU_FWD_LXC | CGPU_FWD_NETDEV */
	uint32_t flags;         /* CGPU_FWD_ENCAP */
	uint32_t ipv4_mask;     /* IPV4_MASK (node_config.h:41), raw u32 as compared with daddr */
	uint32_t host_ifindex;  /* HOST_IFINDEX */
	uint32_t encap_ifindex; /* ENCAP_IFINDEX */
	uint32_t reserved[3];   /* must be 0 (-EINVAL) */
} cgpu_fwd_params;

typedef struct cgpu_fwd_in {
	const void *daddr;      /* v4: u32 per packet; v6: 16 bytes, any alignment; the
				   packet's daddr as it leaves the classify step */
	const int32_t *verdict; /* the classify call's verdict; NULL only in NETDEV mode */
	const uint32_t *tunnel; /* raw tunnel_endpoint word per packet; NULL = all 0 */
	const uint8_t *flags;   /* CGPU_F_EGRESS; NULL only in NETDEV mode */
	const uint8_t *ttl;     /* IPv4 ttl / IPv6 hop_limit; NULL = never expired */
} cgpu_fwd_in;

/* all device pointers; any output but action may be NULL; every element of a
 * given column is written */
typedef struct cgpu_fwd_out {
	uint8_t *action;   /* CGPU_FWD_* */
	int32_t *ret;      /* the DROP_* code of a DROP, else 0 */
	uint32_t *ifindex;
	uint32_t *arg;     /* PROXY: proxy port; LOCAL: lxc_id; OVERLAY: tunnel endpoint */
} cgpu_fwd_out;

/* The tunnel column is the one the caller has: the `tunnel` output of a
 * _tun / _ct_tun call in LXC mode, of cgpu_ipcache_lookup_v4 / _v6 in NETDEV
 * mode.  -ENODEV on a host-only context; -EINVAL for a null required column,
 * a bad mode, unknown flag bits, nonzero reserved words or a misaligned
 * 4-byte column. */
int cgpu_forward_v4(cgpu_ctx *ctx, const cgpu_fwd_params *params, const cgpu_fwd_in *in, size_t n,
		    const cgpu_fwd_out *out, void *stream);
int cgpu_forward_v6(cgpu_ctx *ctx, const cgpu_fwd_params *params, const cgpu_fwd_in *in, size_t n,
		    const cgpu_fwd_out *out, void *stream);
/* Device bytes of the published snapshot's forwarding tables: out[0..3] =
 * IPv4 endpoints, IPv6 endpoints, IPv4 tunnel map, IPv6 tunnel map.  They are
 * built only while some endpoint has a non-zero value or the tunnel map holds
 * a key (all 0 otherwise: the snapshot's endpoint sets answer), and are no
 * part of cgpu_table_bytes, cgpu_table_verify or the upload check. */
int cgpu_forward_table_bytes(cgpu_ctx *ctx, uint64_t *out);

/*
 * The forwarding step on raw frames: per frame of a mixed IPv4 / IPv6 batch
 * (the slots of cgpu_frames) the decision of cgpu_forward_v4 / _v6 on the
 * frame's own daddr and ttl / hop limit and, with CGPU_FWDF_REWRITE, that
 * branch's L2 / L3 rewrite in the frame's slot (ipv4_l3 / ipv6_l3,
 * bpf/lib/l3.h:31-69, with ipv4_dec_ttl, lib/ipv4.h:30-43, and
 * ipv6_dec_hoplimit, lib/ipv6.h:178-193; the call sites bpf_lxc.c:563, 629,
 * 643, 258, 337, 351 and lib/l3.h:83, 114).
 *
 * Per frame:
 *   a. ethertype (bytes 12..13) 0x0800: IPv4, 0x86DD: IPv6; any other, or a
 *      frame whose min(len, stride) does not cover 14 + 20 (IPv4) / 14 + 40
 *      (IPv6) bytes: NONE, all outputs 0, the frame untouched;
 *   b. CGPU_FWD_LXC only: stage == 7 (NOT_CLASSIFIED, the responders' frames,
 *      whose verdict is 0): NONE; then the list of cgpu_forward_v4 as written
 *      (no CGPU_F_EGRESS: NONE; verdict < 0, the parse drops and
 *      CGPU_DROP_SNAPLEN among them: DROP, ret = verdict);
 *   c. daddr = bytes 30..33 (IPv4, the u32 as loaded) / 38..53 (IPv6), ttl =
 *      byte 22 / hop limit = byte 21; action, ret, ifindex and arg are what
 *      cgpu_forward_v4 / _v6 return for these columns, the expired-ttl rule
 *      included;
 *   d. CGPU_FWDF_REWRITE, by the final action (any other keeps every byte:
 *      encapsulation does not decrement, an expired frame is not touched):
 *        PROXY, HOST (LXC)   smac = cgpu_config.node_mac (NODE_MAC,
 *                            bpf_lxc.c:87, 411), dmac = host_mac, decrement
 *        LOCAL               smac = the endpoint's node_mac, dmac = its mac
 *                            (the first six bytes, as stored, of the 8-byte
 *                            fields: eth_store_saddr(skb, (__u8 *)&router_mac,
 *                            0)), decrement; all-zero MACs while no endpoint
 *                            has a non-zero value
 *        STACK, CGPU_FWD_LXC smac unchanged, dmac = node_mac, decrement
 *        STACK, NETDEV       nothing (TC_ACT_OK, bpf_netdev.c:427, 452)
 *      dmac is bytes 0..5, smac bytes 6..11.  The IPv4 decrement stores
 *      ttl - 1 at byte 22 and patches the checksum as the kernel's
 *      bpf_l3_csum_replace(.., from = ttl, to = ttl - 1, 2) does: with c the
 *      u16 at bytes 24..25 (little-endian load) and add(a, b) = (r = a + b,
 *      r + (r < b)) in u32, t = add(add(~c, ~ttl), ttl - 1), folded twice by
 *      t = (t & 0xffff) + (t >> 16), and (u16)~t stored back.  Nothing is
 *      verified: an invalid checksum gets the same delta.  IPv6 decrements
 *      byte 21 and changes nothing else.
 *
 * Not modelled: the proxy's L4 port rewrite and its checksum
 * (ipv4_redirect_to_host_port), ipv6_store_flowlabel on the IPv6 egress STACK
 * branch (bpf_lxc.c:355), rewrite_dmac_to_host (bpf_netdev.c:165),
 * DROP_WRITE_ERROR, LXC_NAT46, the tunnel header of an OVERLAY frame, and an
 * ipcache tunnel lookup inside the call (the caller hands in a `tunnel` column
 * or none).
 *
 * -EINVAL, judged before the context, for a null struct, a null required
 * column, a bad mode, unknown flag bits, nonzero reserved or pad, a misaligned
 * 4-byte column, a stride that is not a multiple of 16 or is below 64, or data
 * that is not 16-byte aligned; -ENODEV on a host-only context; n == 0 is a
 * no-op.  One snapshot serves the whole batch.  The endpoints' MACs sit in
 * device arrays beside the forwarding tables (16 B per table slot), which
 * cgpu_forward_table_bytes does not report.
 */
#define CGPU_FWDF_REWRITE 1u

typedef struct cgpu_fwdf_params {
	cgpu_fwd_params fwd;  /* mode, CGPU_FWD_ENCAP, ipv4_mask, host_ifindex, encap_ifindex; reserved 0 */
	uint8_t host_mac[6];  /* HOST_IFINDEX_MAC (bpf/node_config.h:39) */
	uint8_t pad[2];       /* must be 0 */
	uint32_t flags;       /* CGPU_FWDF_REWRITE */
	uint32_t reserved[3]; /* must be 0 */
} cgpu_fwdf_params;

typedef struct cgpu_fwdf_in { /* device pointers */
	uint8_t *data;          /* the slots of cgpu_frames (same stride / alignment rules);
				   written only with CGPU_FWDF_REWRITE */
	const uint32_t *len;
	const uint8_t *flags;   /* CGPU_F_EGRESS; NULL only in NETDEV mode */
	uint32_t stride, reserved;
	const int32_t *verdict; /* cgpu_classify_frames' verdict; NULL only in NETDEV mode */
	const uint8_t *stage;   /* its stage; NULL only in NETDEV mode */
	const uint32_t *tunnel; /* raw tunnel_endpoint word per frame; NULL = all 0 */
} cgpu_fwdf_in;

int cgpu_forward_frames(cgpu_ctx *ctx, const cgpu_fwdf_params *params, const cgpu_fwdf_in *in, size_t n,
			const cgpu_fwd_out *out, void *stream);

/* ------------------------------------------------------------------ */
/* local delivery: the destination endpoint's ingress policy           */
/* ------------------------------------------------------------------ */
/*
 * The third call of the chain classify -> forward -> deliver.  A packet the
 * forwarding step marks CGPU_FWD_LOCAL is not through yet:
 * ipv4_local_delivery / ipv6_local_delivery (bpf/lib/l3.h:71-132) store
 * skb->cb[CB_SRC_LABEL] = seclabel and tail-call cilium_policy[ep->lxc_id],
 * the destination endpoint's handle_policy -> ipv4_policy / ipv6_policy
 * (bpf_lxc.c:863-978, :1002-1030), which runs policy_can_access_ingress(
 * src_label, dport, proto) (lib/policy.h:126-146) on that endpoint's policy
 * map and can still drop the packet or send it to the ingress proxy.
 *
 * Per packet, against the snapshot the call pins:
 *   1. action != CGPU_FWD_LOCAL: verdict 0, identity 0, stage
 *      CGPU_STAGE_NOT_LOCAL; no counter and no metric is touched, and the
 *      packet's other columns (arg included) are not interpreted.
 *   2. The label is src_label[i], or with src_ep the sending endpoint's
 *      cgpu_lxc_info.sec_label (SECLABEL; 0 for an endpoint without an entry).
 *      It is used exactly as handed in, reserved values included: unlike the
 *      ingress tuples of cgpu_classify_v4 / _v6 neither the ipcache nor
 *      ingress_src_identity / ingress_secctx_world replaces it (the sender's
 *      SECLABEL, bpf_lxc.c:592, :287; from the netdev or the overlay the
 *      secctx, bpf_netdev.c:429, bpf_overlay.c:115).
 *   3. With ct_proto_gate, a protocol outside ICMP (v4: 1, v6: 58), TCP and
 *      UDP: DROP_CT_UNKNOWN_PROTO (-137), identity 0, stage 4.
 *   4. The three probes of __policy_can_access on the policy map of endpoint
 *      `arg`, direction ingress, identity = the label, is_fragment =
 *      CGPU_F_FRAGMENT on IPv4 and false on IPv6: verdict, identity and stage
 *      are those of an ingress tuple of cgpu_classify_v4 / _v6 with that
 *      identity and ep (0, the raw be16 proxy port, or DROP_POLICY; stage
 *      1 / 2 / 3 / 0).  An arg above 0xFFFF or >= max_endpoints is a miss.
 *   5. Counters and metrics are that tuple's: the hit entry's packets / bytes
 *      and the {REASON_FORWARDED | 133 | 137, ingress} metrics; nothing for a
 *      proxy redirect.
 *
 * This is the stateless decision: ipv4_policy's conntrack lookup is taken as
 * CT_NEW, as on every stateless path here.  Not modelled: skip_proxy
 * (tc_index_skip_proxy); the ifindex of the proxy redirect;
 * DROP_MISSED_TAIL_CALL (-140) for an lxc_id whose program is not loaded (the
 * engine has a policy map for every id, and an empty one denies); and the
 * conntrack form, whose CT_INGRESS lookups and creates belong in batch order
 * in the one map.
 */
#define CGPU_STAGE_NOT_LOCAL 9

typedef struct cgpu_dlv_in { /* device pointers */
	const uint8_t *action;     /* cgpu_fwd_out.action */
	const uint32_t *arg;       /* cgpu_fwd_out.arg: the lxc_id of a LOCAL packet */
	const uint32_t *src_label; /* CB_SRC_LABEL per packet, or NULL ... */
	const uint16_t *src_ep;    /* ... then the sending endpoint (the classify call's ep) */
	const uint16_t *dport;     /* the classify call's policy port, network order */
	const uint8_t *proto;
	const uint8_t *flags;      /* CGPU_F_FRAGMENT is read (IPv4 only); CGPU_F_EGRESS is ignored */
	const uint32_t *len;
} cgpu_dlv_in;

typedef struct cgpu_dlv_out { /* device pointers; identity and stage may be NULL */
	int32_t *verdict;
	uint32_t *identity;
	uint8_t *stage;
} cgpu_dlv_out;

/* -EINVAL for a null struct, a null required column, both or neither of
 * src_label / src_ep, or a misaligned 2- / 4-byte column (all judged before
 * the context); -ENODEV on a host-only context; n == 0 returns 0. */
int cgpu_deliver_v4(cgpu_ctx *ctx, const cgpu_dlv_in *in, size_t n, const cgpu_dlv_out *out, void *stream);
int cgpu_deliver_v6(cgpu_ctx *ctx, const cgpu_dlv_in *in, size_t n, const cgpu_dlv_out *out, void *stream);

/* ------------------------------------------------------------------ */
/* counters                                                             */
/* ------------------------------------------------------------------ */
/*
 * Batch launches accumulate into a DELTA buffer of cgpu_counter_delta_bytes()
 * bytes: u64 {packets, bytes} per policy slot, then u64 {count, bytes} per
 * {reason 0..255, dir 0..3} metrics key.  By default the context owns it;
 * cgpu_counter_bind() points launches at a caller-owned device buffer (e.g.
 * a torch tensor that is all-reduced over RCCL across ranks holding the same
 * committed tables).  cgpu_counter_fold() adds the delta into the
 * totals reported by cgpu_policy_lookup / cgpu_metrics_read and zeroes it.
 */
size_t cgpu_counter_delta_bytes(cgpu_ctx *ctx);
int cgpu_counter_bind(cgpu_ctx *ctx, void *device_buf, size_t bytes);
int cgpu_counter_fold(cgpu_ctx *ctx, void *stream);
/* out: [256][4][2] u64 {count, bytes} (folds and synchronizes first) */
int cgpu_metrics_read(cgpu_ctx *ctx, uint64_t *out);
int cgpu_counters_reset(cgpu_ctx *ctx);
/* Popularity-ordered counter slots: hot slots [0, hot_counter_slots)
 * accumulate in LDS (one flush per workgroup), the others cost a global
 * atomic per hit.  Slots start out by key class (L3-only / identity-wildcard
 * keys hot); this re-assigns them by measured traffic: the keys with the most
 * packets so far take the hot slots (ties: class, endpoint, key -- replicas
 * with the same folded totals choose alike), counters move with their keys,
 * and the policy tables are republished.  A control-plane call: it
 * synchronizes the device and folds the delta buffer; every map change must be
 * committed (else -EBUSY) and no batch may run on the context meanwhile.
 * *moved_out (optional) = keys whose slot changed. */
int cgpu_counters_rebalance(cgpu_ctx *ctx, uint64_t *moved_out);
/* Classify launches keep a packed counter accumulator of 8 B per policy
 * slot (policy_max_total x 8 B of HBM) for each stream they ran on, at most
 * 16 of them; a 17th stream recycles the least recently used one after that
 * stream's last launch finished.  A caller that is done with a stream (e.g.
 * before hipStreamDestroy) releases its buffer here; waits for the stream's
 * last launch of this context. */
int cgpu_stream_release(cgpu_ctx *ctx, void *stream);

/* ------------------------------------------------------------------ */
/* multi-GPU counter reduction (consumer: the agent's      */
/* metrics export, pkg/maps/metricsmap/metricsmap.go:170 SyncMetricsMap)*/
/* ------------------------------------------------------------------ */
/* One process (or context) per GPU holds the same committed tables and
 * classifies its own shard of the stream.  Rank 0 creates a communicator id
 * and hands it to every rank out of band (the agent's own channel); each
 * rank then joins with cgpu_comm_init (collective: blocks until all
 * nranks joined).  cgpu_counters_allreduce enqueues the RCCL SUM (over
 * xGMI) of the delta buffer on `stream`; after it every rank's delta holds
 * the counts of all ranks, and cgpu_counter_fold adds them to the totals
 * (integer sums: bit-exact against one GPU classifying the whole stream). */
#define CGPU_COMM_ID_BYTES 128
int cgpu_comm_id_create(uint8_t *id_out /* [CGPU_COMM_ID_BYTES] */);
int cgpu_comm_init(cgpu_ctx *ctx, const uint8_t *id, int nranks, int rank);
int cgpu_counters_allreduce(cgpu_ctx *ctx, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CGPU_H */
