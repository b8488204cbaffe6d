"""The cold-hit log of the x4 classify kernels (k_classify_x4 appends a word
per counter hit on a slot past the LDS hot slots, k_cold_hist sums the log
into the packed accumulator).  Every check is bit-exact against the
restatement: verdict, identity and stage of every tuple, every per-entry
counter through policy_lookup, and metrics(); each runs with the log
(schedule 0) and with CGPU_SCHED_NO_COLD_LOG, the in-loop atomics that also
take the entries a full region turns away."""
import numpy as np
import pytest

from cilium_amd import build, layouts as L, synth

pytestmark = pytest.mark.gpu

NO_CCACHE = 4     # CGPU_SCHED_NO_CCACHE
NO_COLD_LOG = 64  # CGPU_SCHED_NO_COLD_LOG
SCHEDS = [0, NO_COLD_LOG]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a device"
    build.build()
    return torch


def _engine(**kw):
    from cilium_amd.engine import Engine
    return Engine(device=0, **kw)


def _check_out(out, exp):
    v0, i0, s0 = exp
    np.testing.assert_array_equal(out["verdict"].cpu().numpy(), v0)
    np.testing.assert_array_equal(out["identity"].cpu().numpy().view(np.uint32), i0)
    np.testing.assert_array_equal(out["stage"].cpu().numpy(), s0)


def _check_counters(e, o, keys, eps):
    for k, ep in zip(keys, eps):
        rc, got = e.policy_lookup(int(ep), k)
        rc0, raw = o.policy_lookup(int(ep), k)
        want = np.frombuffer(raw, L.POLICY_ENTRY)[0]
        assert rc == 0 and rc0 == 0
        assert (int(got["packets"]), int(got["bytes"])) == (int(want["packets"]), int(want["bytes"]))
    np.testing.assert_array_equal(e.metrics(), o.metrics())


def _oracle(T):
    from oracle import Oracle
    o = Oracle(**T.oracle_config())
    synth.load_oracle(o, T)
    return o


@pytest.fixture(scope="module")
def cpu_tables():
    return synth.make_tables(**synth.CONFIGS["cpu"])


@pytest.fixture(scope="module")
def gpu_tables():
    return synth.make_tables(**synth.CONFIGS["gpu"])


# --------------------------------------------------------------------------
# 1. regions that overflow into the atomic
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def overflow_case(torch_cuda, cpu_tables):
    """n = 2 * CUs * 4096 + 3 * 4096 + 1: workgroups of the resident grid run
    two and three trips of the loop, the last quad is ragged."""
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    n = 2 * cus * 4096 + 3 * 4096 + 1
    t = synth.make_tuples(cpu_tables, n)
    o = _oracle(cpu_tables)
    v, idt, st, _ = o.classify_v4(t, nthreads=8)
    assert np.isin(st, (1, 2, 3)).mean() > 0.5, "far more hits than the regions' quarter"
    return t, o, (v, idt, st)


@pytest.mark.parametrize("sched", SCHEDS + [NO_CCACHE])
def test_region_overflow(torch_cuda, cpu_tables, overflow_case, sched):
    """No LDS hot slots (hot_counter_slots = 0), so every counter hit is cold.
    A wave's region holds a quarter of its tuples: with the LDS cold-slot
    cache off (NO_CCACHE) every hit beyond that, and with it on whatever the
    cache turns away beyond that, takes the atomic."""
    T = cpu_tables
    t, o, exp = overflow_case
    e = _engine(**T.engine_config(), hot_counter_slots=0, schedule=sched)
    synth.load_engine(e, T)
    e.commit()
    out = e.classify_v4(synth.to_device(t))
    torch_cuda.cuda.synchronize()
    _check_out(out, exp)
    _check_counters(e, o, T.pol_keys, T.pol_ep)
    e.close()


# --------------------------------------------------------------------------
# 2. / 3. several partitions; a small launch after a large one
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def partitions_case(gpu_tables):
    """Config "gpu" tables: 64k keys, so the cold slots past the default hot
    slots need three LDS-sized partitions.  300k tuples, then 5, then 1; the
    restatement's counters after each."""
    T = gpu_tables
    t = synth.make_tuples(T, 300_000 + 5 + 1)
    cuts = [(0, 300_000), (300_000, 300_005), (300_005, 300_006)]
    o = _oracle(T)
    steps = []
    for lo, hi in cuts:
        part = {k: np.ascontiguousarray(v[lo:hi]) for k, v in t.items()}
        v, idt, st, _ = o.classify_v4(part, nthreads=8)
        ctr = [tuple(int(x) for x in np.frombuffer(o.policy_lookup(int(ep), k)[1], L.POLICY_ENTRY)[0][
            ["packets", "bytes"]]) for k, ep in zip(T.pol_keys, T.pol_ep)]
        steps.append((part, (v, idt, st), ctr, o.metrics().copy()))
    return steps


def _counters(e, T):
    """every entry's {packets, bytes}, read in one batch (64k keys, three times)"""
    return [(int(p), int(b)) for p, b in e.policy_counters(T.pol_ep, T.pol_keys)]


@pytest.mark.parametrize("sched", SCHEDS)
def test_partitions_then_small_launches(torch_cuda, gpu_tables, partitions_case, sched):
    """One engine and stream: the 300k call (every partition of the cold
    slots), then n = 5 and n = 1, which start one workgroup.  The counts the
    large launch's other waves left in the log are stale by then: a second
    pass that read them would count their entries again."""
    T = gpu_tables
    assert len(T.pol_keys) >= 60_000
    e = _engine(**T.engine_config(), schedule=sched)
    synth.load_engine(e, T)
    e.commit()
    for part, exp, ctr, met in partitions_case:
        out = e.classify_v4(synth.to_device(part))
        torch_cuda.cuda.synchronize()
        _check_out(out, exp)
        assert _counters(e, T) == ctr
        np.testing.assert_array_equal(e.metrics(), met)
    e.close()


# --------------------------------------------------------------------------
# 4. the length boundary of a logged hit
# --------------------------------------------------------------------------
@pytest.mark.parametrize("sched", SCHEDS)
def test_length_boundary(torch_cuda, cpu_tables, sched):
    """Lengths 2047 (the largest a log entry or a packed word holds) and 2048
    (the two-word path into the delta buffer) mixed on cold keys."""
    T = cpu_tables
    n = 40_000 + 3
    t = synth.make_tuples(T, n, seed=77)
    rng = np.random.default_rng(4)
    t["len"] = rng.choice(np.array([2047, 2048], np.uint32), n)
    o = _oracle(T)
    v, idt, st, _ = o.classify_v4(t, nthreads=8)
    hit = st != 0
    assert (t["len"][hit] == 2047).sum() > 1000 and (t["len"][hit] == 2048).sum() > 1000
    e = _engine(**T.engine_config(), hot_counter_slots=0, schedule=sched | NO_CCACHE)
    synth.load_engine(e, T)
    e.commit()
    out = e.classify_v4(synth.to_device(t))
    torch_cuda.cuda.synchronize()
    _check_out(out, (v, idt, st))
    _check_counters(e, o, T.pol_keys, T.pol_ep)
    e.close()


# --------------------------------------------------------------------------
# 5. two streams, each with its own log
# --------------------------------------------------------------------------
@pytest.mark.parametrize("sched", SCHEDS)
def test_two_streams(torch_cuda, cpu_tables, sched):
    """Two streams of one context classify at once; the totals are the sum of
    the restatement's two runs."""
    torch = torch_cuda
    T = cpu_tables
    ta, tb = synth.make_tuples(T, 200_000 + 1, seed=5), synth.make_tuples(T, 150_000 + 2, seed=6)
    o = _oracle(T)
    ea = o.classify_v4(ta, nthreads=8)[:3]
    eb = o.classify_v4(tb, nthreads=8)[:3]
    e = _engine(**T.engine_config(), hot_counter_slots=0, schedule=sched)
    synth.load_engine(e, T)
    e.commit()
    da, db = synth.to_device(ta), synth.to_device(tb)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        oa = e.classify_v4(da, stream=sa)
    with torch.cuda.stream(sb):
        ob = e.classify_v4(db, stream=sb)
    with torch.cuda.stream(sa):
        oa2 = e.classify_v4(da, stream=sa)
    torch.cuda.synchronize()
    o.classify_v4(ta, nthreads=8)
    _check_out(oa, ea)
    _check_out(ob, eb)
    _check_out(oa2, ea)
    _check_counters(e, o, T.pol_keys, T.pol_ep)
    e.stream_release(sa)
    e.stream_release(sb)
    e.close()


# --------------------------------------------------------------------------
# 6. more partitions than the second pass takes: atomics for the launch
# --------------------------------------------------------------------------
@pytest.mark.parametrize("sched", SCHEDS)
def test_fallback_whole_launch(torch_cuda, cpu_tables, sched):
    """policy_max_total = 2^20 with half of it reserved as hot slots: the
    cold slots start at 2^19, more than 8 LDS-sized partitions above the hot
    slots LDS holds, so the launch keeps the atomics."""
    T = cpu_tables
    n = 100_000 + 1
    t = synth.make_tuples(T, n, seed=9)
    o = _oracle(T)
    exp = o.classify_v4(t, nthreads=8)[:3]
    cfg = dict(T.engine_config(), policy_max_total=1 << 20, hot_counter_slots=1 << 19)
    e = _engine(**cfg, schedule=sched)
    synth.load_engine(e, T)
    e.commit()
    out = e.classify_v4(synth.to_device(t))
    torch_cuda.cuda.synchronize()
    _check_out(out, exp)
    _check_counters(e, o, T.pol_keys, T.pol_ep)
    e.close()


# --------------------------------------------------------------------------
# 7. the other instantiations of the kernel
# --------------------------------------------------------------------------
# Only the plain IPv4 kernel logs (the second pass cost the others more than
# the log saved them); these share its counter code and take the atomic for
# every cold hit under either schedule.  Few hot slots and no cold-slot
# cache, so that most of their hits go that way.
@pytest.mark.parametrize("sched", SCHEDS)
def test_cascade_cold_heavy(torch_cuda, cpu_tables, sched):
    T = cpu_tables
    S = synth.make_services(T, 2000)
    P = synth.make_prefilter4(T, n_dyn=500, n_fix=2000)
    t = synth.add_prefilter_traffic(synth.add_service_traffic(synth.make_tuples(T, 6000 + 3, seed=12), S), P)
    o = _oracle(T)
    synth.load_services(o, S)
    synth.load_prefilter4(o, P)
    exp = o.classify_v4_cascade(t, nthreads=4)[:3]
    e = _engine(**T.engine_config(), lb_max_entries=len(S.keys), hot_counter_slots=16, schedule=sched | NO_CCACHE)
    synth.load_engine(e, T)
    synth.load_services(e, S)
    synth.load_prefilter4(e, P)
    e.commit()
    out = e.classify_v4_cascade(synth.to_device(t))
    torch_cuda.cuda.synchronize()
    _check_out(out, exp)
    _check_counters(e, o, T.pol_keys, T.pol_ep)
    e.close()


@pytest.mark.parametrize("sched", SCHEDS)
def test_fused_frames_cold_heavy(torch_cuda, cpu_tables, sched):
    """64-byte slots: the kernel that parses the frames itself."""
    T = cpu_tables
    f = synth.frames_from_tuples(synth.make_tuples(T, 6000 + 1, seed=13), stride=64)
    o = _oracle(T)
    exp = o.classify_frames(f, nthreads=4)[:3]
    assert (exp[2] != 0).sum() > 1000
    e = _engine(**T.engine_config(), hot_counter_slots=16, schedule=sched | NO_CCACHE)
    synth.load_engine(e, T)
    e.commit()
    out = e.classify_frames(synth.frames_to_device(f))
    torch_cuda.cuda.synchronize()
    _check_out(out, exp)
    _check_counters(e, o, T.pol_keys, T.pol_ep)
    e.close()


@pytest.mark.parametrize("sched", SCHEDS)
def test_classify_v6_cold_heavy(torch_cuda, sched):
    T = synth.make_tables6(n_prefixes=2000, n_identities=500, n_endpoints=2, keys_per_ep=4000)
    t = synth.make_tuples6(T, 6000 + 2)
    o = _oracle(T)
    exp = o.classify_v6(t, nthreads=4)[:3]
    assert (exp[2] != 0).sum() > 1000
    e = _engine(**T.engine_config(), hot_counter_slots=16, schedule=sched | NO_CCACHE)
    synth.load_engine(e, T)
    e.commit()
    out = e.classify_v6(synth.to_device(t))
    torch_cuda.cuda.synchronize()
    _check_out(out, exp)
    _check_counters(e, o, T.pol_keys, T.pol_ep)
    e.close()
