/* Internal interface between host.cpp (C ABI, table compiler) and
 * kernels.hip (gfx950 kernels).  Not exported. */
#ifndef CGPU_LAUNCH_H
#define CGPU_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "tables.h"
#include "../../include/cgpu.h"

/* The cold-hit log of a stream's packed accumulator (k_classify_x4 appends,
 * k_cold_hist sums it into pk): `words` u32 of device memory owned by the
 * stream's pk buffer, or {nullptr, 0} (every cold hit is an atomic on pk). */
struct pk_log {
	uint32_t *p;
	uint64_t words;
};
struct classify_v4_args {
	const uint32_t *saddr, *daddr;
	const uint16_t *dport;
	const uint8_t *proto, *flags;
	const uint32_t *len;
	const uint16_t *ep;
	int32_t *verdict;
	uint32_t *identity;
	uint8_t *stage;
	uint64_t *delta; /* [2 * n_ctr_slots] policy + [CGPU_METRICS_WORDS] metrics */
	uint64_t n;
	uint64_t *pk;    /* [n_ctr_slots] packed cold-slot accumulator, zero between calls */
	/* egress service step first (cgpu_classify_v4_lb) */
	int lb;
	const uint16_t *sport;
	const uint32_t *hash; /* NULL: flow_hash(saddr, daddr, sport, dport, proto) */
	/* with lb: the XDP prefilter before every ingress tuple (cgpu_classify_v4_cascade) */
	int xdp;
	/* cgpu_classify_v4_tun: [n] tunnel endpoints out (NULL: none) from the
	 * tunnel tables `tun` */
	uint32_t *tunnel;
	const ipc_tun *tun;
	/* the stream's cold-hit log (only the plain kernel logs: no service
	 * step, no tunnel output) */
	pk_log log;
};

hipError_t launch_classify_v4(const cgpu_snapshot &s, const classify_v4_args &a, hipStream_t st);
/* bytes of log the call `a` wants, 0 when launch_classify_v4 would not use
 * one (a smaller log is used as far as it goes: entries that do not fit take
 * the atomic) */
size_t x4_log_bytes(const cgpu_snapshot &s, const classify_v4_args &a);

struct classify_v6_args {
	const uint8_t *saddr16, *daddr16;
	const uint16_t *dport;
	const uint8_t *proto, *flags;
	const uint32_t *len;
	const uint16_t *ep;
	int32_t *verdict;
	uint32_t *identity;
	uint8_t *stage;
	uint64_t *delta;
	uint64_t n;
	uint64_t *pk; /* packed cold-slot accumulator (per stream) */
	/* egress service step first (cgpu_classify_v6_lb) */
	int lb;
	const uint16_t *sport;
	const uint32_t *hash; /* NULL: flow_hash(fold6(saddr), fold6(daddr), sport, dport, proto) */
	/* scratch of n u32 (optional): the x4 schedule's ipcache pre-pass
	 * (k_ipc6_pre) writes every tuple's trie entry there */
	uint32_t *ipc_e;
	/* cgpu_classify_v6_tun: as classify_v4_args */
	uint32_t *tunnel;
	const ipc_tun *tun;
};

hipError_t launch_classify_v6(const cgpu_snapshot &s, const classify_v6_args &a, hipStream_t st);

/* batched ipcache lookup (cgpu_ipcache_lookup_v4 / _v6): any output may be
 * NULL; tunnel only with the tunnel tables compiled (t.t4.d16) */
struct ipc_lookup_args {
	const void *addr; /* u32 per address (v4); 16 bytes, any alignment (v6) */
	uint64_t n;
	uint8_t *found;
	uint32_t *label, *tunnel;
	int v6;
};

hipError_t launch_ipcache_lookup(const cgpu_snapshot &s, const ipc_tun &t, const ipc_lookup_args &a,
				 hipStream_t st);

/* forwarding decision (cgpu_forward_v4 / _v6): the columns of cgpu_fwd_in /
 * cgpu_fwd_out and the words of cgpu_fwd_params; the snapshot's parts the
 * kernel reads (endpoint sets for a context without forwarding tables, the
 * netdev gate's config words) are filled in by launch_forward */
struct fwd_args {
	const void *daddr;
	const int32_t *verdict;
	const uint32_t *tunnel;
	const uint8_t *flags, *ttl;
	uint8_t *action;
	int32_t *ret;
	uint32_t *ifindex, *arg;
	uint64_t n;
	uint32_t mode, encap, ipv4_mask, host_ifindex, encap_ifindex;
	int v6;
	addr_set4 ep4;
	addr_set16 ep6;
	uint32_t cluster_mask, cluster_range, router[3];
};

hipError_t launch_forward(const cgpu_snapshot &s, const fwd_tables &f, const fwd_args &a, hipStream_t st);

/* the forwarding step on raw frames (cgpu_forward_frames): the columns of
 * cgpu_fwdf_in / cgpu_fwd_out, the words of cgpu_fwdf_params (host_mac as the
 * little-endian words of its bytes 0-3 / 4-5); the snapshot's parts (as
 * fwd_args, and NODE_MAC) are filled in by launch_forward_frames */
struct fwdf_args {
	uint8_t *data;
	const uint32_t *len;
	const uint8_t *flags, *stage;
	const int32_t *verdict;
	const uint32_t *tunnel;
	uint8_t *action;
	int32_t *ret;
	uint32_t *ifindex, *arg;
	uint64_t n;
	uint32_t stride, mode, encap, rewrite, ipv4_mask, host_ifindex, encap_ifindex;
	uint32_t host_mac_lo, host_mac_hi, node_mac_lo, node_mac_hi;
	addr_set4 ep4;
	addr_set16 ep6;
	uint32_t cluster_mask, cluster_range, router[3];
};

hipError_t launch_forward_frames(const cgpu_snapshot &s, const fwd_tables &f, const fwd_macs &m,
				 const fwdf_args &a, hipStream_t st);

/* local delivery (cgpu_deliver_v4 / _v6): the columns of cgpu_dlv_in /
 * cgpu_dlv_out (exactly one of src_label / src_ep), the context's delta
 * buffer, and max_ep = min(max_endpoints, 0x10000): an `arg` at or above it
 * names no policy map */
struct dlv_args {
	const uint8_t *action;
	const uint32_t *arg, *src_label;
	const uint16_t *src_ep, *dport;
	const uint8_t *proto, *flags;
	const uint32_t *len;
	int32_t *verdict;
	uint32_t *identity;
	uint8_t *stage;
	uint64_t *delta;
	uint64_t n;
	uint32_t max_ep;
	int v6;
};

hipError_t launch_deliver(const cgpu_snapshot &s, const dlv_args &a, hipStream_t st);

struct prefilter_args {
	const uint32_t *saddr4, *daddr4;
	const uint8_t *saddr16, *daddr16;
	const uint8_t *flags;
	uint8_t *verdict;
	uint64_t n;
};

hipError_t launch_prefilter_v4(const cgpu_snapshot &s, const prefilter_args &a, hipStream_t st);
hipError_t launch_prefilter_v6(const cgpu_snapshot &s, const prefilter_args &a, hipStream_t st);

struct lb4_args {
	const uint32_t *saddr, *daddr;
	const uint16_t *sport, *dport;
	const uint8_t *proto;
	const uint32_t *hash;
	int32_t *ret;
	uint32_t *saddr_out, *daddr_out;
	uint16_t *dport_out, *rev_nat_out, *slave_out;
	uint64_t n;
	int mode; /* CGPU_LB_NETDEV / CGPU_LB_LXC */
};

hipError_t launch_lb4(const cgpu_snapshot &s, const lb4_args &a, hipStream_t st);

/* raw frames (cgpu_frames_parse / cgpu_classify_frames) */
struct frames_args {
	const uint8_t *data;
	const uint32_t *len;
	const uint8_t *flags;
	const uint16_t *ep;
	uint32_t stride;
	uint64_t n;
	/* parse outputs (any but status may be NULL) */
	int32_t *status;
	uint8_t *family, *saddr16, *daddr16;
	uint16_t *dport;
	uint8_t *proto, *tflags;
	/* classify outputs */
	int32_t *verdict;
	uint32_t *identity;
	uint8_t *stage;
	uint64_t *delta;
	uint64_t *pk; /* the stream's packed cold-slot accumulator (classify) */
};

hipError_t launch_frames_parse(const cgpu_snapshot &s, const frames_args &a, hipStream_t st);

/* scratch of the frames x4 schedule (launch_classify_frames_x4): the IPv4
 * policy-tuple columns [n] and the compacted IPv6 ones [n] with their
 * results; every column 16-byte aligned */
struct frames_x4 {
	uint32_t *sa4, *da4;
	uint16_t *dport;
	uint8_t *proto, *fl;
	uint4 *sa6, *da6;
	uint16_t *dport6;
	uint8_t *proto6, *fl6;
	uint32_t *len6;
	uint16_t *ep6;
	uint32_t *idx6;
	int32_t *v6;
	uint32_t *id6;
	uint8_t *st6;
	uint32_t *n6;
};
/* bytes of that scratch for n frames, and its carving */
size_t frames_x4_bytes(uint64_t n);
frames_x4 frames_x4_carve(void *base, uint64_t n);
hipError_t launch_classify_frames_x4(const cgpu_snapshot &s, const frames_args &a, const frames_x4 &c,
				     hipStream_t st);
hipError_t launch_classify_frames(const cgpu_snapshot &s, const frames_args &a, hipStream_t st);

/* the service step on raw frames (cgpu_classify_frames_lb): the columns of
 * cgpu_flb_in, the classify outputs and those of cgpu_flb_out */
struct frames_lb_args {
	uint8_t *data;
	const uint32_t *len;
	const uint8_t *flags;
	const uint16_t *ep;
	const uint32_t *hash; /* NULL: cgpu_flow_hash / _hash6 of the frame's fields */
	uint32_t stride, rewrite;
	uint64_t n;
	int32_t *verdict;
	uint32_t *identity;
	uint8_t *stage;
	int32_t *lb_ret;
	uint16_t *rev_nat, *slave;
	uint64_t *delta;
	uint64_t *pk;
};
hipError_t launch_classify_frames_lb(const cgpu_snapshot &s, const frames_lb_args &a, hipStream_t st);

/* reverse NAT on raw frames (cgpu_rnat_frames_v4 / _v6): the columns of
 * cgpu_rnf4_in / cgpu_rnf6_in (saddr: u32 per frame, or 16-byte rows) */
struct rnat_frames_args {
	uint8_t *data;
	const uint32_t *len;
	const uint8_t *applied;
	const void *saddr;
	const uint32_t *daddr; /* IPv4 */
	const uint16_t *sport;
	int32_t *ret;          /* may be NULL */
	uint32_t stride, rewrite;
	uint64_t n;
	int v6;
};
hipError_t launch_rnat_frames(const rnat_frames_args &a, hipStream_t st);

/* frames to the stateful path (cgpu_frames_parse_ct / cgpu_classify_frames_ct):
 * the slots of cgpu_frames and the columns of cgpu_frame_ct_cols (any but
 * status may be NULL).  launch_frames_ct_parse with fin != NULL is the parse
 * pass of cgpu_classify_frames_ct: it also writes the final outputs of the
 * frames that end in the parse (and the other family's rn columns of the
 * rest), counts their metrics and writes one select byte per family. */
struct frames_ct_args {
	const uint8_t *data;
	const uint32_t *len;
	const uint8_t *flags;
	const uint16_t *ep;
	uint32_t stride;
	uint64_t n;
	int32_t *status;
	uint8_t *family, *saddr16, *daddr16;
	uint16_t *sport, *dport;
	uint8_t *proto;
	uint16_t *l4;
	uint8_t *tflags;
};
/* the frame-order outputs of cgpu_fct_out (stage and the rn group may be NULL) */
struct fct_outs {
	int32_t *verdict;
	uint8_t *ct_ret;
	uint32_t *identity;
	uint8_t *stage;
	uint8_t *rn_applied;
	uint16_t *rn_sport;
	uint32_t *rn_saddr4, *rn_daddr4;
	uint8_t *rn_saddr6;
};
struct fct_fin {
	fct_outs o;
	uint8_t *sel4, *sel6; /* [n] 1: the frame reaches conntrack in that family */
	uint64_t *delta;
};
hipError_t launch_frames_ct_parse(const cgpu_snapshot &s, const frames_ct_args &a, const fct_fin *fin,
				  hipStream_t st);
/* bytes of block-count scratch launch_fct_select wants for n frames */
size_t fct_select_bytes(uint64_t n);
/* idx[0, *count) = the ascending i < n with sel[i] != 0 */
hipError_t launch_fct_select(const uint8_t *sel, uint64_t n, uint32_t *idx, uint32_t *count, void *temp,
			     hipStream_t st);
/* one family's compact columns: m packets, the conntrack call's inputs and
 * outputs (saddr / daddr / rn_saddr: u32 per packet, or 16-byte rows) */
struct fct_compact {
	const uint32_t *idx;
	uint64_t m;
	void *saddr, *daddr;
	uint16_t *sport, *dport;
	uint8_t *proto;
	uint16_t *l4;
	uint8_t *flags;
	uint32_t *len;
	uint16_t *ep;
	int32_t *verdict;
	uint8_t *ct_ret;
	uint32_t *identity;
	uint8_t *stage;
	uint8_t *rn_applied;
	uint16_t *rn_sport;
	void *rn_saddr;
	uint32_t *rn_daddr;
	int v6;
};
/* compact[j] = column[idx[j]] for the inputs (src: the parse's columns; len
 * and ep from the frames' own) */
hipError_t launch_fct_gather(const frames_ct_args &src, const fct_compact &c, hipStream_t st);
/* out[idx[j]] = compact[j] for the outputs (rn: with the rn group) */
hipError_t launch_fct_scatter(const fct_compact &c, const fct_outs &o, bool rn, hipStream_t st);

/* stateful classification (cgpu_classify_v4_ct): packet columns, outputs,
 * and the caller-allocated scratch (ct_scratch_layout in host.cpp) */
struct ct_launch {
	const void *saddr, *daddr; /* IPv4: u32 per packet; IPv6: 16 bytes (16-byte aligned) */
	const uint16_t *sport, *dport;
	const uint8_t *proto;
	const uint16_t *l4;
	const uint8_t *flags;
	const uint32_t *len;
	const uint16_t *ep;
	int32_t *verdict;
	uint8_t *ct_ret;
	uint32_t *identity;
	uint8_t *stage;
	uint64_t *delta;
	uint64_t n;
	uint32_t now;
	uint4 *rec; /* [2n] IPv4, [4n] IPv6 */
	uint32_t *gkey, *gkey_sorted, *idx, *idx_sorted;
	uint8_t *head;
	uint32_t *heads, *n_heads;
	uint32_t *heads_pos; /* [n] scratch for the longest-first group sort */
	void *temp;
	size_t temp_bytes;
	/* the stateful service step (cgpu_classify_v4_ctlb); rec is [3n] */
	const uint32_t *hash; /* NULL: cgpu_flow_hash */
	uint4 *svc_out;       /* [n] */
	uint32_t *ctl;        /* [4] */
	uint8_t *flags2;      /* [2n] plain path, [4n] service path: phase-2 candidates */
	uint8_t *pcls;        /* [n] service path: each packet's phase-2 class (k_ct_prep) */
	uint64_t *pk;         /* [n_ctr_slots] packed counters, zero between calls */
	void *xdaddr;         /* [n] optional (IPv6: 16 bytes each) */
	uint16_t *xdport;     /* [n] optional */
	uint32_t dflt;        /* nonzero: group-default results (CT_DFLT) */
	/* cgpu_classify_v{4,6}_ct_tun: [n] tunnel endpoints out (NULL: none) from
	 * the tunnel tables `tun` (plain paths only) */
	uint32_t *tunnel;
	const ipc_tun *tun;
	/* cgpu_classify_v{4,6}_ct{,lb}_rnat: rn != NULL selects the walkers that
	 * fill it ([n] scratch, zeroed by the caller before the launch: the hit
	 * entry's rev_nat_index | lb_loopback << 16) and the rewrite kernel after
	 * the finish; the dense reverse-NAT tables (NULL: that map is empty) and
	 * the outputs (any NULL; IPv6 rn_saddr 16 bytes per packet, no rn_daddr) */
	uint32_t *rn;
	const void *rn_t4, *rn_t6;
	void *rn_saddr;
	uint32_t *rn_daddr;
	uint16_t *rn_sport;
	uint8_t *rn_applied;
};

size_t ct_temp_bytes(uint64_t n);
/* ctmap.GC RemoveExpired on the device map; compaction into an empty table */
hipError_t launch_ct_gc(const ct_table &T, bool v6, uint32_t time, uint32_t *deleted, hipStream_t st);
hipError_t launch_ct_rehash(const ct_table &src, const ct_table &dst, bool v6, hipStream_t st);

hipError_t launch_classify_v4_ct(const cgpu_snapshot &s, const ct_table &T, const ct_launch &L,
				 hipStream_t st);
/* the same over cilium_ct6_global (tables.h CtK6 slots), rec [4n] */
hipError_t launch_classify_v6_ct(const cgpu_snapshot &s, const ct_table &T, const ct_launch &L,
				 hipStream_t st);

/* behind the IPv6 stateful service step (cilium_ct6_global, rec [4n],
 * svc_out [2n], xdaddr 16 bytes per packet) */
hipError_t launch_classify_v6_ctlb(const cgpu_snapshot &s, const ct_table &T, const ct_launch &L,
				   hipStream_t st);
/* the same behind the stateful service step (cilium_ct4_global, rec [3n]) */
hipError_t launch_classify_v4_ctlb(const cgpu_snapshot &s, const ct_table &T, const ct_launch &L,
				   hipStream_t st);

/* L3 MapState compilation (cgpu_l3_compile): device copies of the program */
struct l3_launch {
	const cgpu_selector *sel;
	const cgpu_requirement *req;
	const uint32_t *val;
	const uint32_t *rule_subject, *rule_clauses;
	uint32_t n_rules;
	const cgpu_l3_clause *cl;
	const uint32_t *ep_off, *id_off;
	const cgpu_label *ep_lab, *id_lab;
	uint32_t n_ep, n_id, flags;
	uint8_t *subj, *allow;
	/* cgpu_mapstate_sync only (nullptr / 0 for cgpu_l3_compile) */
	const uint32_t *ep_flags; /* per endpoint: replaces `flags` */
	const cgpu_l4_filter *flt;
	const uint32_t *flt_sels;
	uint32_t n_flt;
	uint64_t *l4bits; /* [n_flt][ceil(n_id / 64)] identity bitmaps */
};

hipError_t launch_l3_compile(const l3_launch &L, hipStream_t st);

/* *out += sum of table_sum_word over `bytes` bytes of buf from byte `off`
 * (a multiple of 8) */
hipError_t launch_table_sum(const void *buf, size_t off, size_t bytes, uint64_t *out, hipStream_t st);

/* totals[i] += delta[i]; delta[i] = 0 over n u64 words */
hipError_t launch_fold(uint64_t *totals, uint64_t *delta, uint64_t n, hipStream_t st);
/* a copy by the CUs between device memory and a device-visible page-locked
 * host range (either way); hipErrorInvalidValue unless dst and src are
 * 16-byte aligned */
hipError_t launch_copy_host(void *dst, const void *src, uint64_t bytes, hipStream_t st);
/* up to 8 such copies in one launch (every segment 16-byte aligned) */
struct copy_seg {
	void *dst;
	const void *src;
	uint64_t bytes;
};
struct copy_segs {
	copy_seg seg[8];
	uint32_t n;
};
hipError_t launch_copy_host_multi(const copy_segs &d, hipStream_t st);
/* totals[2*slot[i]] = pk[i]; totals[2*slot[i]+1] = by[i]; delta[..] = 0 */
hipError_t launch_slot_init(uint64_t *totals, uint64_t *delta, const uint32_t *slot,
			    const uint64_t *pk, const uint64_t *by, uint32_t n, hipStream_t st);

#endif
