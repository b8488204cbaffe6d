"""The reverse NAT outputs (rn_saddr / rn_daddr / rn_sport / rn_applied of the
cgpu_classify_*_rnat calls) against the CPU restatement on whole streams:
every entry a packet hits was created, re-created, evicted or re-selected by
the stream itself, so only a reference that tracks the conntrack map can say
which entry's rev_nat_index and lb_loopback the rewrite must use.

Every comparison is assert_array_equal of all rn_* columns over the whole
batch (on top of verdict, ct_ret, identity, translated daddr / dport), against
or_classify_*_rnat, which tests/test_oracle_revnat.py pins to an independent
numpy restatement and to a table of literal cases.  The reverse NAT map is
"every service's index -> {VIP, port}" as the agent writes it.  Non-vacuity
(applied packets, evictions, loopback replies) is counted on the
restatement's outputs and printed per batch.

Walker instantiations reached with creates and evictions in one batch:
sections a-c run k_ct_walk<CtK4S / CtK6S, service walk, RN, LRU> and
<CtK4 / CtK6, WALK_PKT / WALK_OWED, RN, LRU> behind it, section d the plain
paths' <CtK4 / CtK6, RN, LRU>; section f rebuilds and frees the device table
of the reverse NAT map (both branches of rn4_dirty / rn6_dirty in
cgpu_commit)."""
import functools

import numpy as np
import pytest

from cilium_amd import build, layouts as L, synth
from revnat_cases import ACK, IDX_MISS, IDX_PORT, IDX_PORT0, LOOPBACK, TCP, UDP, _a6, _rmap4, _rmap6
from test_gpu_ctlb_lru import (FIELDS, _batch, _engine, _fill_to_max, _lru_engine, _oracle, _run, _same_results,
                               _world)

pytestmark = pytest.mark.gpu

NOWS = (1000, 1010, 1020, 1030)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a device"
    build.build()
    return torch


def _rn_cols(v6):
    return ("rn_saddr", "rn_sport", "rn_applied") if v6 else ("rn_saddr", "rn_daddr", "rn_sport", "rn_applied")


def _same_rn(out, exp, v6, msg):
    for f in _rn_cols(v6):
        np.testing.assert_array_equal(out[f], exp[f], err_msg=f"{msg} {f}")


def _svc_rmap(svcs):
    """every service's index -> {VIP, port}: {raw index: (address, port)}"""
    ns = len(svcs.vip)
    rmap = {}
    for k, raw in zip(svcs.keys[ns:], svcs.vals["rev_nat_index"][ns:]):
        a = k["address"]
        rmap[int(raw)] = (bytes(a) if a.ndim else int(a), int(k["dport"]))
    return rmap


def _put(target, ix, addr, port, v6):
    if v6:
        v = np.zeros((), L.LB6_REVERSE_NAT)
        v["address"][:], v["port"] = _a6(addr), port
        assert target.revnat6_update(ix, v) == 0
    else:
        v = np.zeros((), L.LB4_REVERSE_NAT)
        v["address"], v["port"] = addr, port
        assert target.revnat4_update(ix, v) == 0


def _load_rmap(target, rmap, v6):
    """into an Engine (commit afterwards) or an Oracle"""
    for ix, (addr, port) in rmap.items():
        _put(target, ix, addr, port, v6)


def _counts(t, exp, v6, msg, ev=None):
    """The restatement's counts of one batch: applied, loopback replies
    (IPv4: applied with the daddr rewritten), evictions of the engine."""
    ap = exp["rn_applied"] == 1
    eg = (t["flags"] & 1) == 1
    c = {"applied": int(ap.sum()), "egress": int((ap & eg).sum()), "ingress": int((ap & ~eg).sum()),
         "ingress_established": int((ap & ~eg & (exp["ct_ret"] == L.CT_ESTABLISHED)).sum())}
    if not v6:
        before = exp["xdaddr"] if "xdaddr" in exp else t["daddr"]
        c["loopback_replies"] = int((ap & eg & (exp["rn_daddr"] != before) & (exp["rn_daddr"] == t["saddr"])).sum())
    if ev is not None:
        c["evictions"] = int(ev)
    print(f"{msg}: restatement {c}")
    return c


# --------------------------------------------------------------------------
# a-c. LRU under eviction on the service paths
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _streams_rn(v6):
    """The four streams of test_gpu_ctlb_lru._world.  The IPv4 ones get, on
    top of their packets (all kept, in order), the packets the synth streams
    lack: where the backend of a service connection is the sending endpoint
    itself (lb4_local's loopback source NAT), the endpoint's own answers, which
    leave it as egress packets to IPV4_LOOPBACK and hit the address entry of
    ct_create4 as CT_REPLY with lb_loopback (the one case where the rewrite
    also sets the daddr).  Which packets those are is read from a run of the
    restatement over the streams (an unlimited map, no reverse NAT); an answer
    follows its packet at a distance of 1 to 22 packets."""
    W = _world(v6)
    F, T, svcs, streams, _ = W
    if v6:
        return streams
    o = _oracle(W)
    res = []
    for t, now in zip(streams, NOWS):
        exp = o.classify_v4_ctlb(t, now)
        eg = (t["flags"] & 1) == 1
        src = np.flatnonzero(eg & (exp["xdaddr"] == t["saddr"]) & (exp["verdict"] == 0) & np.isin(t["proto"], [TCP, UDP]))
        add = {"saddr": t["saddr"][src], "daddr": np.full(len(src), LOOPBACK, np.uint32),
               "sport": exp["xdport"][src], "dport": t["sport"][src], "proto": t["proto"][src],
               "l4b": np.where(t["proto"][src] == TCP, ACK, 0).astype(np.uint16),
               "flags": np.ones(len(src), np.uint8), "len": np.full(len(src), 100, np.uint32),
               "ep": t["ep"][src], "hash": np.zeros(len(src), np.uint32)}
        pos = np.concatenate([np.arange(len(eg), dtype=np.float64), src + 0.5 + (src % 4) * 7])
        order = np.argsort(pos, kind="stable")
        res.append({k: np.ascontiguousarray(np.concatenate([t[k], add[k]])[order]) for k in t})
    return res


def _rn_engine(W, ct_max, rmap):
    e = _lru_engine(W, ct_max)
    _load_rmap(e, rmap, W[0].v6)
    e.commit()
    return e


def _rn_batch(torch, e, W, rmap, t, now, msg, edit=None):
    """_batch with rev_nat on both sides, the restatement started from the
    map the batch found and holding the same reverse NAT map (`edit`: further
    changes to the restatement before it runs); then every rn_* column."""
    F = W[0]
    o = _oracle(W, getattr(e, F.dump)())
    _load_rmap(o, rmap, F.v6)
    if edit:
        edit(o)
    out, exp, ev = _batch(torch, e, W, t, now, msg, o=o, rev_nat=True)
    c = _counts(t, exp, F.v6, msg, ev)
    _same_rn(out, exp, F.v6, msg)
    return out, exp, c


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_lru_eviction_service_paths(torch_cuda, v6):
    """a. The four streams in order into ct_max 4096 (IPv6 8192) with
    ct_lru = 1, every batch through the _rnat call: every batch evicts and
    the restatement applies at least 25 (IPv4) / 100 (IPv6) rewrites per batch.
    The first two streams together fit an empty map, so the map starts filled
    to ct_max with plain entries: from the first batch on every create evicts.

    Counted with the restatement on the synth streams alone: 24 / 48 / 42 / 89
    (IPv4) and 130 / 270 / 143 / 437 (IPv6) applied packets, all ingress.  The
    first IPv4 stream has 30 ingress CT_REPLY packets from a backend address,
    but 6 of them belong to plain connections whose remote address happens to
    be some service's backend (both are drawn from the same ipcache prefixes):
    their entries carry no index.  The streams' egress REPLY / RELATED packets
    answer connections opened from outside, whose entries carry no index
    either, and the synth streams hold no egress packet to IPV4_LOOPBACK, so no
    loopback entry is ever hit as a reply.  _streams_rn adds those answers;
    with them every IPv4 batch is well past the floor, which stays at 25."""
    W = _world(v6)
    F, T, svcs, _, _ = W
    rmap = _svc_rmap(svcs)
    e = _rn_engine(W, F.ct_max, rmap)
    _fill_to_max(e, W, F.ct_max)
    for bi, (t, now) in enumerate(zip(_streams_rn(v6), NOWS)):
        out, exp, c = _rn_batch(torch_cuda, e, W, rmap, t, now, f"batch {bi}")
        assert c["evictions"] > 0, c
        assert c["applied"] >= (100 if v6 else 25), c
        assert getattr(e, F.count)() <= F.ct_max
        if not v6 and bi == 3:
            assert c["loopback_replies"] >= 1, c
    assert e.ct_lru_stats(v6)["no_victim"] == 0
    e.close()


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_lru_map_full_of_plain_entries(torch_cuda, v6):
    """b. The map filled to exactly ct_max with plain entries, then stream 44:
    every create of a service connection evicts."""
    W = _world(v6)
    F, T, svcs, _, _ = W
    rmap = _svc_rmap(svcs)
    e = _rn_engine(W, F.ct_max, rmap)
    _fill_to_max(e, W, F.ct_max)
    out, exp, c = _rn_batch(torch_cuda, e, W, rmap, _streams_rn(v6)[3], 1000, "full of plain entries")
    assert c["evictions"] > 1000 and c["applied"] >= (100 if v6 else 25), c
    if not v6:
        assert c["loopback_replies"] >= 1, c
    assert e.ct_lru_stats(v6)["no_victim"] == 0
    e.close()


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_lru_stored_and_reselected_slaves(torch_cuda, v6):
    """c. The scenario of test_ctlb_lru_stored_and_reselected_slaves: stream 41,
    then a tenth of the backends deleted and half of those put back with other
    targets, the map filled up, and the same packets again through the _rnat
    call: replies now come from backends the connection no longer maps to,
    and forward packets re-select."""
    W = _world(v6)
    F, T, svcs, _, _ = W
    rmap = _svc_rmap(svcs)
    e = _rn_engine(W, F.ct_max, rmap)
    t = _streams_rn(v6)[0]
    _rn_batch(torch_cuda, e, W, rmap, t, 1000, "first run")
    rng = np.random.Generator(np.random.PCG64(12))
    ns = len(svcs.vip)
    gone = rng.choice(np.arange(ns, len(svcs.keys)), (len(svcs.keys) - ns) // 10, replace=False)
    back = gone[: len(gone) // 2]
    nv = svcs.vals[back].copy()
    nv["target"] = svcs.vals["target"][rng.integers(ns, len(svcs.keys), len(back))]
    for d in gone:
        assert getattr(e, F.lb_del)(svcs.keys[d]) == 0
    for d, v in zip(back, nv):
        assert getattr(e, F.lb_upd)(svcs.keys[d], v) == 0
    e.commit()
    _fill_to_max(e, W, F.ct_max)

    def edit(o):
        for d in gone:
            assert getattr(o, F.olb_del)(svcs.keys[d]) == 0
        for d, v in zip(back, nv):
            assert getattr(o, F.olb_upd)(svcs.keys[d], v) == 0

    out, exp, c = _rn_batch(torch_cuda, e, W, rmap, t, 1100, "second run", edit=edit)
    assert c["evictions"] > 0 and c["applied"] > 0, c
    assert e.ct_lru_stats(v6)["no_victim"] == 0
    e.close()


# --------------------------------------------------------------------------
# d. LRU on the plain paths
# --------------------------------------------------------------------------
IDX_SET = [0] + IDX_PORT + IDX_PORT0 + IDX_MISS  # 0, mapped, unmapped, byte-swapped twins


def _run_plain(torch, e, F, t, now):
    out = getattr(e, F.run_plain)(synth.to_device(t), now, rev_nat=True)
    torch.cuda.synchronize()
    sa = out["rn_saddr"].cpu().numpy()
    res = {"verdict": out["verdict"].cpu().numpy(), "ct_ret": out["ct_ret"].cpu().numpy(),
           "identity": out["identity"].cpu().numpy().view(np.uint32), "stage": out["stage"].cpu().numpy(),
           "rn_saddr": sa if F.v6 else sa.view(np.uint32), "rn_sport": out["rn_sport"].cpu().numpy().view(np.uint16),
           "rn_applied": out["rn_applied"].cpu().numpy()}
    if not F.v6:
        res["rn_daddr"] = out["rn_daddr"].cpu().numpy().view(np.uint32)
    return res


def _oracle_plain(o, F, t, now):
    v, cr, ident, st, _, rn = getattr(o, F.run_plain)(t, now, rev_nat=True)
    return dict(rn, verdict=v, ct_ret=cr, identity=ident, stage=st)


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_lru_plain_paths(torch_cuda, v6):
    """d. cgpu_classify_v{4,6}_ct_rnat with ct_lru = 1: stream 41, then every
    entry it left gets a rev_nat_index from IDX_SET and (a quarter of them)
    lb_loopback, the map is filled up, and stream 42 runs with stream 41's
    packets mixed in: hits of entries with an index and creates that evict in
    one walk.  On IPv6 a quarter of stream 42's connections use a local
    address whose s6_addr32[3] & 0xFFFF names an index, which ipv6_policy
    stores in the entry it creates (bpf_lxc.c:753, :808)."""
    W = _world(v6)
    F, T = W[0], W[1]
    rmap = _rmap6() if v6 else _rmap4()
    e = _rn_engine(W, F.ct_max, rmap)
    ta = F.mk_plain(T, 1400, seed=41, mean_pkts=5.0, span=0.9)[0]
    tb = F.mk_plain(T, 1400, seed=42, mean_pkts=5.0, span=0.9)[0]
    o = _oracle(W)
    _load_rmap(o, rmap, v6)
    out = _run_plain(torch_cuda, e, F, ta, 1000)
    exp = _oracle_plain(o, F, ta, 1000)
    for f in ("verdict", "ct_ret", "identity"):
        np.testing.assert_array_equal(out[f], exp[f], err_msg=f"first batch {f}")
    _same_rn(out, exp, v6, "first batch")
    # the entries of the first batch, rewritten in the engine
    rng = np.random.Generator(np.random.PCG64(7))
    keys, vals = getattr(e, F.dump)()
    vals = vals.copy()
    vals["rev_nat_index"] = rng.choice(IDX_SET, len(vals))
    vals["bits"] |= np.where(rng.random(len(vals)) < 0.25, 8, 0).astype(vals["bits"].dtype)
    for k, v in zip(keys, vals):
        assert getattr(e, F.upd)(k, v) == 0
    _fill_to_max(e, W, F.ct_max)
    if v6:
        tb = {k: x.copy() for k, x in tb.items()}
        eg = (tb["flags"] & 1) == 1
        lport = np.where(eg, tb["sport"], tb["dport"])
        pick = lport % 4 == 0
        ix = np.array(IDX_PORT + IDX_PORT0 + IDX_MISS, np.uint16)[lport % 9]
        for col, m in (("saddr", pick & eg), ("daddr", pick & ~eg)):
            tb[col][m, 12] = ix[m] & 0xFF
            tb[col][m, 13] = ix[m] >> 8
    n1, n2 = len(ta["flags"]), len(tb["flags"])
    from_a = np.zeros(n1 + n2, bool)
    from_a[rng.choice(n1 + n2, n1, replace=False)] = True
    t2 = {}
    for k in ta:
        col = np.empty((n1 + n2,) + ta[k].shape[1:], ta[k].dtype)
        col[from_a], col[~from_a] = ta[k], tb[k]
        t2[k] = col
    # the restatement from the map the second batch finds
    o2 = _oracle(W, getattr(e, F.dump)())
    _load_rmap(o2, rmap, v6)
    ev0 = e.ct_lru_stats(v6)["evictions"]
    out = _run_plain(torch_cuda, e, F, t2, 1010)
    exp = _oracle_plain(o2, F, t2, 1010)
    c = _counts(t2, exp, v6, "second batch", e.ct_lru_stats(v6)["evictions"] - ev0)
    for f in ("verdict", "ct_ret", "identity"):
        np.testing.assert_array_equal(out[f], exp[f], err_msg=f"second batch {f}")
    _same_rn(out, exp, v6, "second batch")
    assert c["evictions"] > 300 and c["applied"] > 100, c
    assert not (out["verdict"] == L.DROP_CT_CREATE_FAILED).any()
    assert getattr(e, F.count)() <= F.ct_max and e.ct_lru_stats(v6)["no_victim"] == 0
    if v6:
        assert c["ingress_established"] >= 1, c
        created = (exp["ct_ret"] == L.CT_NEW) & ((t2["flags"] & 1) == 0) & (t2["daddr"][:, 12:14] != 0).any(axis=1)
        assert created.sum() > 0  # entries created with the index their daddr names
    else:
        assert c["loopback_replies"] >= 1, c
    e.close()


# --------------------------------------------------------------------------
# e-f. a synth service stream without LRU
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synth_world(v6):
    """The stream of test_synth_ctlb_properties (tests/test_gpu_revnat.py) and
    its IPv6 counterpart, in the shape of test_gpu_ctlb_lru._world."""
    from test_gpu_ctlb_lru import Fam
    F = Fam(v6)
    if v6:
        T = synth.make_tables6(n_prefixes=2000, n_identities=200, n_endpoints=2, keys_per_ep=3000)
        svcs = synth.make_services6(T, 300)
    else:
        T = synth.make_tables(n_prefixes=2000, n_identities=200, n_endpoints=2, keys_per_ep=3000)
        svcs = synth.make_services(T, 300)
    t, _, seclabels, svcs = F.mk(T, svcs, 2_500, mean_pkts=8.0, span=0.5)
    assert 15_000 < len(t["flags"]) < 25_000
    return F, T, svcs, [t], seclabels


def _cut(t, parts):
    n = len(t["flags"])
    b = [n * i // parts for i in range(parts + 1)]
    return [{k: x[b[i]:b[i + 1]] for k, x in t.items()} for i in range(parts)]


def _plain_engine(W, **cfg):
    F, T, svcs, _, seclabels = W
    e = _engine(**T.engine_config(), ct_max=1 << 18, **cfg)
    synth.load_engine(e, T)
    F.load_svcs(e, svcs)
    synth.load_lxc(e, seclabels)
    return e


def _step(torch, e, o, F, t, now, msg):
    out = _run(torch, e, F, t, now, rev_nat=True)
    exp = getattr(o, F.run)(t, now, rev_nat=True)
    c = _counts(t, exp, F.v6, msg)
    _same_results(out, exp, t, msg)
    _same_rn(out, exp, F.v6, msg)
    return out, exp, c


@pytest.mark.parametrize("schedule", [0, 8 << 8], ids=["default", "sort8"])
@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_synth_service_stream(torch_cuda, v6, schedule):
    """e. Default mode and the sorted schedule, two batches of the same
    connections (the stream cut in the middle), the restatement running on."""
    W = _synth_world(v6)
    F, T, svcs, (t,), _ = W
    rmap = _svc_rmap(svcs)
    e = _plain_engine(W, schedule=schedule)
    _load_rmap(e, rmap, v6)
    e.commit()
    o = _oracle(W)
    _load_rmap(o, rmap, v6)
    total = 0
    for bi, tb in enumerate(_cut(t, 2)):
        _, _, c = _step(torch_cuda, e, o, F, tb, 1000 + bi, f"batch {bi}")
        total += c["applied"]
    assert total > 100
    e.close()


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_map_edited_between_batches(torch_cuda, tmp_path, v6):
    """f. One engine, the stream cut in three, the reverse NAT map edited and
    committed between the cuts, the restatement edited alike: a third of the
    indices deleted and a third pointed elsewhere (half of those with port 0);
    then every index deleted (the device table is freed: nothing is applied,
    the frame is what the service step left); then the map put back, a
    checkpoint taken, and the first batch's replies run again on this engine
    and on a fresh one restored from the checkpoint."""
    W = _synth_world(v6)
    F, T, svcs, (t,), _ = W
    rmap = _svc_rmap(svcs)
    e = _plain_engine(W)
    _load_rmap(e, rmap, v6)
    e.commit()
    o = _oracle(W)
    _load_rmap(o, rmap, v6)
    dele = "revnat6_delete" if v6 else "revnat4_delete"
    t1, t2, t3 = _cut(t, 3)
    _, exp1, c1 = _step(torch_cuda, e, o, F, t1, 1000, "batch 1")
    assert c1["applied"] > 25
    idx = sorted(rmap)
    gone, moved = idx[0::3], idx[1::3]
    for tgt in (e, o):
        for ix in gone:
            assert getattr(tgt, dele)(ix) == 0
        for j, ix in enumerate(moved):
            addr = bytes([0xFD, 0, 0, 0x99] + [0] * 10 + [j >> 8, j & 0xFF]) if v6 else L.ip4_be(0x0A630000 + j)
            _put(tgt, ix, addr, 0 if j % 2 else rmap[ix][1], v6)
    e.commit()
    _, exp2, c2 = _step(torch_cuda, e, o, F, t2, 1001, "batch 2")
    assert 0 < c2["applied"]
    for tgt in (e, o):
        for ix in idx:
            if ix not in gone:
                assert getattr(tgt, dele)(ix) == 0
    assert (e.revnat6_count() if v6 else e.revnat4_count()) == 0
    e.commit()
    out3, exp3, c3 = _step(torch_cuda, e, o, F, t3, 1002, "batch 3")
    assert c3["applied"] == 0 and not out3["rn_applied"].any()
    np.testing.assert_array_equal(out3["rn_sport"], t3["sport"])
    if v6:
        np.testing.assert_array_equal(out3["rn_saddr"], t3["saddr"])
    else:
        np.testing.assert_array_equal(out3["rn_daddr"], out3["xdaddr"])
        assert ((out3["rn_saddr"] == t3["saddr"]) | (out3["rn_saddr"] == LOOPBACK)).all()
    # the map back, then batch 1's replies
    for tgt in (e, o):
        _load_rmap(tgt, rmap, v6)
    e.commit()
    path = str(tmp_path / "ckpt.bin")
    e.mirror_save(path)
    rep = np.isin(exp1["ct_ret"], [L.CT_REPLY, L.CT_RELATED])
    tr = {k: np.ascontiguousarray(x[rep]) for k, x in t1.items()}
    out4, exp4, c4 = _step(torch_cuda, e, o, F, tr, 1003, "replies again")
    assert c4["applied"] > 25
    f = _engine(**T.engine_config(), ct_max=1 << 18)
    f.mirror_restore(path)
    f.commit()
    out5 = _run(torch_cuda, f, F, tr, 1003, rev_nat=True)
    for k in FIELDS + _rn_cols(v6):
        np.testing.assert_array_equal(out5[k], out4[k], err_msg=f"restored {k}")
    e.close()
    f.close()
