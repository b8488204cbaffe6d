/*
 * TEST INFRASTRUCTURE — CPU restatement ("port") of the reference's
 * classification semantics.  NOT part of the product.  Loaded only by
 * tests/, bench.py's cpu_baseline leg and __graft_entry__.smoke(), always as
 * the checker or the timed CPU baseline, never on the product path.
 *
 * Parity pinning: every function here is checked against golden vectors the
 * reference's own BPF C produced (oracle/ref/, tests/golden/).
 *
 * Structures are deliberately kernel-like (the "reference CPU path" of
 * BASELINE.md §2): a path-compressed binary LPM trie walked bit by bit as
 * kernel/bpf/lpm_trie.c does, and an open hash with whole-key compare as
 * kernel/bpf/hashtab.c does.  Keys/values use the reference byte layouts:
 *   policy_key 8 B / policy_entry 24 B       bpf/lib/common.h:180-193
 *   ipcache_key 24 B / remote_endpoint_info   bpf/lib/maps.h:135-148, common.h:175-178
 *   lpm_v4_key 8 B / lpm_v6_key 20 B          bpf/lib/xdp.h:23-31
 *   endpoint_key 20 B                         bpf/lib/common.h:147-160
 */
#ifndef CGPU_ORACLE_H
#define CGPU_ORACLE_H

#include <stddef.h>
#include <stdint.h>

typedef struct or_ctx or_ctx;

typedef struct or_config {
	uint32_t host_id, world_id, cluster_id, health_id; /* node_config.h:34-37 */
	uint32_t ipv4_cluster_mask, ipv4_cluster_range;    /* network-order u32 */
	int ct_proto_gate;      /* CONNTRACK: DROP_CT_UNKNOWN_PROTO before policy */
	uint32_t ingress_src_identity; /* identity handed to handle_ipv4 */
	int ingress_secctx_world;      /* non-FROM_HOST netdev: label = WORLD_ID */
	int dyn4, fix4, dyn6, fix6;    /* CIDR{4,6}_LPM_PREFILTER / CIDR{4,6}_FILTER */
	uint8_t router_ip[16];         /* ROUTER_IP (node_config.h:30) */
	int lb_l3, lb_l4;              /* LB_L3 / LB_L4 (lxc_config.h:44-45, init.sh:352) */
	uint32_t ipv4_loopback;        /* IPV4_LOOPBACK (node_config.h:45), network order */
	uint8_t node_mac[6];           /* NODE_MAC (node_config.h:51) */
} or_config;

or_ctx *or_create(void);
void or_destroy(or_ctx *c);
void or_set_config(or_ctx *c, const or_config *cfg);
void or_default_config(or_config *cfg);

/* reference map lookups of the batch calls since the last call, by map
 * (bench.py's roofline prices each at its tier's gather ceiling); the
 * conntrack operations are a call's probe_sum minus these.  Read and reset. */
enum { OR_CLS_IPCACHE = 0, OR_CLS_POLICY, OR_CLS_LB, OR_CLS_PREFILTER, OR_CLS_ENDPOINT, OR_CLS_N };
void or_probe_split(or_ctx *c, uint64_t *out /* [OR_CLS_N] */);
/* ipcache lookups through a DIR-24-8 (IPv4) and a multibit trie (IPv6)
 * built from the current ipcache (1), or the kernel-like trie (0): the
 * "optimized CPU" baseline of BASELINE.md §2, same answers.  An ipcache
 * change drops the fast tables; -EINVAL on a shard view. */
int or_set_fast(or_ctx *c, int on);
/* the batch paths' ipcache lookups (fast or trie): value or -ENOENT */
int or_ipcache_lookup4(or_ctx *c, uint32_t addr_be, void *val8_out);
int or_ipcache_lookup6(or_ctx *c, const uint8_t *addr16, void *val8_out);

/* table ops: 0 on success, -errno (bpf(2) convention) on failure */
int or_ipcache_update(or_ctx *c, const void *key24, const void *val8);
int or_ipcache_delete(or_ctx *c, const void *key24);
int or_ipcache_lookup(or_ctx *c, const void *key24, void *val8_out); /* LPM */
size_t or_ipcache_count(or_ctx *c);

int or_policy_update(or_ctx *c, uint32_t ep, const void *key8, const void *entry24);
int or_policy_delete(or_ctx *c, uint32_t ep, const void *key8);
int or_policy_lookup(or_ctx *c, uint32_t ep, const void *key8, void *entry24_out);

/* which: 0 v4 dyn (LPM), 1 v4 fix (hash), 2 v6 dyn (LPM), 3 v6 fix (hash) */
int or_cidr_update(or_ctx *c, int which, const void *key);
int or_cidr_delete(or_ctx *c, int which, const void *key);
int or_endpoint_update(or_ctx *c, const void *key20);
int or_endpoint_delete(or_ctx *c, const void *key20);

/*
 * Stateless IPv4 classification of n tuples (SoA, network byte order for
 * addresses and dport).  flags bit0 = egress, bit1 = is_fragment.
 * verdict: proxy port (raw be16 as int) / 0 allow / negative DROP_*.
 * identity: label given to policy.  stage: 1 exact, 2 L3, 3 wildcard L4,
 * 0 miss, 4 protocol-gated.  Per-entry packets/bytes and the metrics table
 * are accumulated.  *probe_sum receives sum(N_addr + N_pol).
 * stage / identity may be NULL.  nthreads <= 0 means 1.
 */
int or_classify_v4(or_ctx *c, size_t n, const uint32_t *saddr, const uint32_t *daddr,
		   const uint16_t *dport, const uint8_t *proto, const uint8_t *flags,
		   const uint32_t *len, const uint16_t *ep, int32_t *verdict,
		   uint32_t *identity, uint8_t *stage, int nthreads, uint64_t *probe_sum);

/* Stateless IPv6 classification: addresses 16 bytes per tuple. */
int or_classify_v6(or_ctx *c, size_t n, const uint8_t *saddr16, const uint8_t *daddr16,
		   const uint16_t *dport, const uint8_t *proto, const uint8_t *flags,
		   const uint32_t *len, const uint16_t *ep, int32_t *verdict,
		   uint32_t *identity, uint8_t *stage, int nthreads, uint64_t *probe_sum);

/*
 * XDP prefilter (bpf/bpf_xdp.c:88-184) over pre-parsed packets.
 * flags: 0 = IP packet of this family, 1 = truncated (xdp_no_room -> DROP),
 *        2 = not IPv4/IPv6 ethertype (-> PASS).
 * v4: addresses are network-order u32; v6: 16 bytes per packet.
 * verdict: XDP_DROP (1) / XDP_PASS (2).
 */
int or_prefilter_v4(or_ctx *c, size_t n, const uint32_t *saddr, const uint32_t *daddr,
		    const uint8_t *flags, uint8_t *verdict, int nthreads, uint64_t *probe_sum);
int or_prefilter_v6(or_ctx *c, size_t n, const uint8_t *saddr16, const uint8_t *daddr16,
		    const uint8_t *flags, uint8_t *verdict, int nthreads, uint64_t *probe_sum);

/*
 * Service load balancer: the map cilium_lb4_services with
 * raw struct lb4_key (8 B) -> struct lb4_service (12 B), bpf/lib/common.h:427-439.
 */
int or_lb_update(or_ctx *c, const void *key8, const void *val12);
int or_lb_update_many(or_ctx *c, const void *keys8, const void *vals12, size_t n);
int or_lb_delete(or_ctx *c, const void *key8);
/* kernel skb->hash stand-in used when no hash column is given (the kernel's
 * flow-dissector hash is unpinned); = cilium_amd.shard.flowhash_np */
uint32_t or_flow_hash(uint32_t saddr, uint32_t daddr, uint16_t sport, uint16_t dport, uint8_t proto);
/* IPv6 service map (lb6_key 20 B -> lb6_service 24 B) and the IPv6 flow hash */
int or_lb6_update(or_ctx *c, const void *key20, const void *val24);
int or_lb6_delete(or_ctx *c, const void *key20);
uint32_t or_flow_hash6(const uint8_t *saddr16, const uint8_t *daddr16, uint16_t sport, uint16_t dport,
		       uint8_t proto);
/* or_classify_v6 with the egress service step of ipv6_l3_from_lxc in front
 * (bpf_lxc.c:117-139; lb6_local, lb.h:426-483): hash NULL = or_flow_hash6 */
int or_classify_v6_lb(or_ctx *c, size_t n, const uint8_t *saddr16, const uint8_t *daddr16,
		      const uint16_t *sport, const uint16_t *dport, const uint8_t *proto,
		      const uint8_t *flags, const uint32_t *len, const uint16_t *ep,
		      const uint32_t *hash, int32_t *verdict, uint32_t *identity, uint8_t *stage,
		      int nthreads, uint64_t *probe_sum);

#define OR_LB_NETDEV 0 /* bpf_lb.c handle_ipv4 (bpf_lb.c:118-170) */
#define OR_LB_LXC 1    /* lb4_local from handle_ipv4_from_lxc, CT_NEW (bpf_lxc.c:444-460) */
/*
 * Per tuple (addresses / ports in network order; hash NULL = or_flow_hash):
 * ret  NETDEV: TC_ACT_OK (0, not load-balanced), TC_ACT_REDIRECT (7), or
 *              DROP_NO_SERVICE (-158)
 *      LXC:    0 no service, 1 translated, 2 translated with the loopback
 *              source NAT, or DROP_NO_SERVICE
 * saddr/daddr/dport_out: the packet's fields after lb4_xlate; tdaddr_out
 * (LXC): tuple.daddr afterwards (the backend, or the service address on
 * loopback); rev_nat/slave_out: the selected entry's rev_nat_index and slave.
 * Any output except ret may be NULL.  *probe_sum: service-map lookups.
 */
int or_lb4(or_ctx *c, int mode, size_t n, const uint32_t *saddr, const uint32_t *daddr,
	   const uint16_t *sport, const uint16_t *dport, const uint8_t *proto, const uint32_t *hash,
	   int32_t *ret, uint32_t *saddr_out, uint32_t *daddr_out, uint32_t *tdaddr_out,
	   uint16_t *dport_out, uint16_t *rev_nat_out, uint16_t *slave_out, int nthreads,
	   uint64_t *probe_sum);

/*
 * or_classify_v4 with the egress service step of handle_ipv4_from_lxc in
 * front (bpf_lxc.c:444-469, BASELINE config 5): egress tuples are translated
 * by lb4_local (OR_LB_LXC) first; ipcache then resolves tuple.daddr and the
 * policy sees the translated dport.  DROP_NO_SERVICE ends the tuple (verdict
 * -158, identity 0, stage 6, metrics reason 158 egress, bpf_lxc.c:659-666).
 * sport is needed only when hash is NULL.  *probe_sum includes the LB lookups.
 */
int or_classify_v4_lb(or_ctx *c, size_t n, const uint32_t *saddr, const uint32_t *daddr,
		      const uint16_t *sport, const uint16_t *dport, const uint8_t *proto,
		      const uint8_t *flags, const uint32_t *len, const uint16_t *ep,
		      const uint32_t *hash, int32_t *verdict, uint32_t *identity, uint8_t *stage,
		      int nthreads, uint64_t *probe_sum);

/*
 * BASELINE config 5, the full cascade: or_classify_v4_lb with the XDP
 * prefilter of the netdev in front of every INGRESS tuple (bpf_xdp.c:97-121,
 * xdp_start -> check_filters -> check_v4: saddr in the dyn LPM or the fix
 * /32 hash -> XDP_DROP, else daddr must be a local endpoint,
 * check_v4_endpoint :88-95).  An XDP_DROP ends the tuple before
 * from_netdev (bpf_netdev.c:470) ever sees it: verdict OR_VERDICT_XDP_DROP,
 * identity 0, stage 8, no counters and no metrics (bpf_xdp.c notifies
 * nothing).  Egress tuples take the service step as or_classify_v4_lb.
 * *probe_sum adds the prefilter and endpoint lookups.
 */
#define OR_VERDICT_XDP_DROP (-4097)
int or_classify_v4_cascade(or_ctx *c, size_t n, const uint32_t *saddr, const uint32_t *daddr,
			   const uint16_t *sport, const uint16_t *dport, const uint8_t *proto,
			   const uint8_t *flags, const uint32_t *len, const uint16_t *ep,
			   const uint32_t *hash, int32_t *verdict, uint32_t *identity, uint8_t *stage,
			   int nthreads, uint64_t *probe_sum);

/*
 * Raw Ethernet frames.  Per-endpoint identity of the
 * endpoint program (lxc_config.h LXC_MAC / LXC_IPV4 / LXC_IP and which of
 * the SMAC / DMAC / SIP checks are compiled in), 32 bytes in the layout of
 * cgpu_lxc_info: mac[6], verify (1 SMAC, 2 DMAC, 4 SIP), pad, ipv4 (raw u32),
 * ipv6[16], reserved.  An endpoint without one verifies nothing.
 */
int or_lxc_update(or_ctx *c, uint32_t ep, const void *info32);

/*
 * Frame i = the first min(len[i], stride) bytes at data + i * stride; flags
 * bit0 = egress.  Restates, per frame, the endpoint programs' steps before
 * ipcache (stateless, conntrack empty): see cgpu.h cgpu_frames_parse.
 * status: 0 reached policy, 1 not classified, or the DROP_* / -errno
 * (-4096 = a header past the stored slot).  Tuple outputs may be NULL.
 */
int or_frames_parse(or_ctx *c, size_t n, const uint8_t *data, uint32_t stride, const uint32_t *len,
		    const uint8_t *flags, const uint16_t *ep, int32_t *status, uint8_t *family,
		    uint8_t *saddr16, uint8_t *daddr16, uint16_t *dport, uint8_t *proto,
		    uint8_t *tflags);

/* or_frames_parse, then or_classify_v4 / or_classify_v6 of the tuples that
 * reach policy; the others get verdict = status, identity 0, stage 5 (4 for
 * DROP_CT_UNKNOWN_PROTO), or verdict 0 / stage 7 when not classified. */
int or_classify_frames(or_ctx *c, size_t n, const uint8_t *data, uint32_t stride,
		       const uint32_t *len, const uint8_t *flags, const uint16_t *ep, int32_t *verdict,
		       uint32_t *identity, uint8_t *stage, int nthreads, uint64_t *probe_sum);

/*
 * Conntrack: the map cilium_ct4_global with raw struct
 * ipv4_ct_tuple (14 B) -> struct ct_entry (56 B), bpf/lib/common.h:359-408.
 * Updates are BPF_ANY; a new key past max_elem fails with -E2BIG.
 */
void or_ct_set_max(or_ctx *c, size_t max_elem);
int or_ct4_update(or_ctx *c, const void *key14, const void *val56);
int or_ct4_delete(or_ctx *c, const void *key14);
int or_ct4_lookup(or_ctx *c, const void *key14, void *val56_out);
size_t or_ct4_count(or_ctx *c);
size_t or_ct4_dump(or_ctx *c, void *keys14, void *vals56, size_t max);
/* ctmap.go GC with RemoveExpired: delete entries with lifetime < time */
size_t or_ct4_gc(or_ctx *c, uint32_t time);
/* cilium_ct6_global: raw struct ipv6_ct_tuple (38 B) -> struct ct_entry */
void or_ct6_set_max(or_ctx *c, size_t max_elem);
int or_ct6_update(or_ctx *c, const void *key38, const void *val56);
int or_ct6_delete(or_ctx *c, const void *key38);
int or_ct6_lookup(or_ctx *c, const void *key38, void *val56_out);
size_t or_ct6_count(or_ctx *c);
size_t or_ct6_dump(or_ctx *c, void *keys38, void *vals56, size_t max);
size_t or_ct6_gc(or_ctx *c, uint32_t time);
/* the IPv6 form of or_classify_v4_ct (ct_lookup6 / ct_create6) */
int or_classify_v6_ct(or_ctx *c, size_t n, const uint8_t *saddr16, const uint8_t *daddr16,
		      const uint16_t *sport, const uint16_t *dport, const uint8_t *proto,
		      const uint16_t *l4b, const uint8_t *flags, const uint32_t *len,
		      const uint16_t *ep, uint32_t now, int32_t *verdict, uint8_t *ct_ret,
		      uint32_t *identity, uint8_t *stage, uint64_t *probe_sum);

/*
 * Stateful IPv4 classification of n packets IN ORDER (the sequence the
 * reference's programs see): ct_lookup4 -> ipcache -> policy -> reply /
 * related skip, delete on a denied ESTABLISHED flow, ct_create4 for an
 * allowed CT_NEW (see cgpu.h cgpu_classify_v4_ct).  sport/dport are the L4
 * header's ports (network order), l4b TCP header bytes 12-13 as loaded
 * (little-endian u16: byte 12 low) or the ICMP type, now
 * the bpf_ktime_get_sec() of the batch.  The egress src_sec_id is the
 * endpoint's SECLABEL (cgpu_lxc_info.sec_label).
 */
int or_classify_v4_ct(or_ctx *c, size_t n, const uint32_t *saddr, const uint32_t *daddr,
		      const uint16_t *sport, const uint16_t *dport, const uint8_t *proto,
		      const uint16_t *l4b, const uint8_t *flags, const uint32_t *len,
		      const uint16_t *ep, uint32_t now, int32_t *verdict, uint8_t *ct_ret,
		      uint32_t *identity, uint8_t *stage, uint64_t *probe_sum);

/*
 * or_classify_v4_ct with the stateful service step of handle_ipv4_from_lxc
 * in front (lb4_local with CONNTRACK, lb.h:700-775; see cgpu.h
 * cgpu_classify_v4_ctlb).  hash: skb->hash per packet (NULL: or_flow_hash);
 * xdaddr / xdport (optional): the frame's daddr / dport after the service
 * step.  Service drops: DROP_NO_SERVICE, ct_ret 255, stage 6, identity 0.
 */
int or_classify_v4_ctlb(or_ctx *c, size_t n, const uint32_t *saddr, const uint32_t *daddr,
			const uint16_t *sport, const uint16_t *dport, const uint8_t *proto,
			const uint16_t *l4b, const uint8_t *flags, const uint32_t *len,
			const uint16_t *ep, const uint32_t *hash, uint32_t now, int32_t *verdict,
			uint8_t *ct_ret, uint32_t *identity, uint8_t *stage, uint32_t *xdaddr,
			uint16_t *xdport, uint64_t *probe_sum);

/* the IPv6 form of or_classify_v4_ctlb (lb6_local with CONNTRACK, lb.h:426-483) */
int or_classify_v6_ctlb(or_ctx *c, size_t n, const uint8_t *saddr16, const uint8_t *daddr16,
			const uint16_t *sport, const uint16_t *dport, const uint8_t *proto,
			const uint16_t *l4b, const uint8_t *flags, const uint32_t *len,
			const uint16_t *ep, const uint32_t *hash, uint32_t now, int32_t *verdict,
			uint8_t *ct_ret, uint32_t *identity, uint8_t *stage, uint8_t *xdaddr16,
			uint16_t *xdport, uint64_t *probe_sum);

/*
 * Reverse NAT of service replies.  The maps cilium_lb4_reverse_nat /
 * cilium_lb6_reverse_nat: the key is the raw __u16 as a service entry's
 * rev_nat_index holds it, the value struct lb4_reverse_nat (6 B: address,
 * port) / lb6_reverse_nat (18 B), bpf/lib/common.h.  update is BPF_ANY;
 * delete of an absent index -ENOENT.  A shard view shares its base's maps.
 */
int or_revnat4_update(or_ctx *c, uint16_t index, const void *val6);
int or_revnat4_delete(or_ctx *c, uint16_t index);
int or_revnat6_update(or_ctx *c, uint16_t index, const void *val18);
int or_revnat6_delete(or_ctx *c, uint16_t index);

/*
 * The frame's source (IPv4: and destination) fields as the endpoint program
 * leaves them, per packet; every column may be NULL.  The frame starts as the
 * input, on the _ctlb paths as lb4_xlate / lb6_xlate left it (daddr the
 * backend; IPv4 saddr IPV4_LOOPBACK when the backend is the sender,
 * lb.h:761-766, :668-675), and changes where the program calls lb4_rev_nat /
 * lb6_rev_nat with the ct_state that ct_lookup4 / ct_lookup6 (CT_EGRESS /
 * CT_INGRESS) filled from the entry the packet hit (conntrack.h:213-217),
 * never the ct_state_new of the service step:
 *   IPv4 egress  bpf_lxc.c:531-541  CT_REPLY / CT_RELATED, rev_nat_index != 0
 *   IPv4 ingress bpf_lxc.c:909-918  CT_REPLY, rev_nat_index != 0, !loopback
 *   IPv6 egress  bpf_lxc.c:222-235  CT_REPLY / CT_RELATED, rev_nat_index != 0
 *   IPv6 ingress bpf_lxc.c:778-785  rev_nat_index != 0, whatever ct_lookup6
 *                                   returned (a CT_NEW packet's is 0)
 * applied: the map held the index and __lb4_rev_nat (lb.h:485-550) /
 * __lb6_rev_nat (:254-294) ran: sport := nat->port for TCP / UDP when the
 * port is nonzero (reverse_map_l4_port, :218-252), IPv4 with ct_state.loopback
 * daddr := the old saddr, saddr := nat->address.  A packet dropped before
 * ct_lookup keeps its frame.  Checksums are not modelled, and the map lookup
 * is not counted in *probe_sum.
 */
typedef struct or_rnat4_out {
	uint32_t *saddr, *daddr;
	uint16_t *sport;
	uint8_t *applied;
} or_rnat4_out;
typedef struct or_rnat6_out {
	uint8_t *saddr16;
	uint16_t *sport;
	uint8_t *applied;
} or_rnat6_out;

/* The four stateful calls with that output; rn == NULL: exactly those calls
 * (they forward here), which never read the two maps. */
int or_classify_v4_ct_rnat(or_ctx *c, size_t n, const uint32_t *saddr, const uint32_t *daddr,
			   const uint16_t *sport, const uint16_t *dport, const uint8_t *proto,
			   const uint16_t *l4b, const uint8_t *flags, const uint32_t *len,
			   const uint16_t *ep, uint32_t now, int32_t *verdict, uint8_t *ct_ret,
			   uint32_t *identity, uint8_t *stage, const or_rnat4_out *rn,
			   uint64_t *probe_sum);
int or_classify_v4_ctlb_rnat(or_ctx *c, size_t n, const uint32_t *saddr, const uint32_t *daddr,
			     const uint16_t *sport, const uint16_t *dport, const uint8_t *proto,
			     const uint16_t *l4b, const uint8_t *flags, const uint32_t *len,
			     const uint16_t *ep, const uint32_t *hash, uint32_t now, int32_t *verdict,
			     uint8_t *ct_ret, uint32_t *identity, uint8_t *stage, uint32_t *xdaddr,
			     uint16_t *xdport, const or_rnat4_out *rn, uint64_t *probe_sum);
int or_classify_v6_ct_rnat(or_ctx *c, size_t n, const uint8_t *saddr16, const uint8_t *daddr16,
			   const uint16_t *sport, const uint16_t *dport, const uint8_t *proto,
			   const uint16_t *l4b, const uint8_t *flags, const uint32_t *len,
			   const uint16_t *ep, uint32_t now, int32_t *verdict, uint8_t *ct_ret,
			   uint32_t *identity, uint8_t *stage, const or_rnat6_out *rn,
			   uint64_t *probe_sum);
int or_classify_v6_ctlb_rnat(or_ctx *c, size_t n, const uint8_t *saddr16, const uint8_t *daddr16,
			     const uint16_t *sport, const uint16_t *dport, const uint8_t *proto,
			     const uint16_t *l4b, const uint8_t *flags, const uint32_t *len,
			     const uint16_t *ep, const uint32_t *hash, uint32_t now, int32_t *verdict,
			     uint8_t *ct_ret, uint32_t *identity, uint8_t *stage, uint8_t *xdaddr16,
			     uint16_t *xdport, const or_rnat6_out *rn, uint64_t *probe_sum);

/*
 * L3 MapState compilation: the tables of cgpu.h
 * cgpu_l3_program / cgpu_label_sets (interned ids, see cilium_amd/policy.py);
 * allow[e * n_id + i] bit 0 = ingress Allowed, bit 1 = egress Allowed.
 */
int or_l3_compile(const void *selectors, const void *reqs, const uint32_t *values,
		  const uint32_t *rule_subject, const uint32_t *rule_clauses, uint32_t n_rules,
		  const void *clauses, const uint32_t *ep_off, const void *ep_labels, uint32_t n_ep,
		  const uint32_t *id_off, const void *id_labels, uint32_t n_id, uint32_t flags,
		  uint8_t *allow);

/* shard views (threaded stateful runs): share base's tables, own empty
 * conntrack maps and metrics; merge folds a finished view into base */
or_ctx *or_view_create(or_ctx *base);
void or_view_merge(or_ctx *base, or_ctx *v);
void or_view_destroy(or_ctx *v);

/* metrics {reason, dir} -> {count, bytes}; out is [256][4][2] u64 */
void or_metrics_read(or_ctx *c, uint64_t *out);
void or_counters_reset(or_ctx *c);

#endif
