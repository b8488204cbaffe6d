"""The local delivery step without a device: its reference (tests/
deliver_cases.py) against the literal table, the call's argument checks on a
host-only context, the Python wrapper's refusals, and a guard on the crafted
inputs the device tests use."""
import ctypes as C
import errno

import numpy as np
import pytest

import deliver_cases as DC
from cilium_amd import layouts as L
from cilium_amd._abi import DlvIn, DlvOut
from cilium_amd.engine import Engine


# --------------------------------------------------------------------------
# the reference against the literal table
# --------------------------------------------------------------------------
@pytest.mark.parametrize("case", DC.CASES, ids=[c[0] for c in DC.CASES])
def test_reference_matches_the_literal_table(case):
    name, v6, gate = case[:3]
    c = DC.columns([case])
    o = DC.new_oracle(DC.load_policy, gate)
    got = DC.reference(o, v6, c["action"], c["arg"], DC.labels(c), c["dport"], c["proto"], c["flags"], c["len"],
                       max_ep=DC.MAX_EP)
    o.close()
    assert (int(got["verdict"][0]), int(got["identity"][0]), int(got["stage"][0])) == case[11], name


def test_table_covers_what_the_step_decides():
    for v6 in (False, True):
        rows = [c for c in DC.CASES if c[1] == v6]
        assert {c[3] for c in rows} == set(range(8))                       # every action value
        assert all(c[4] == 0xFFFFFFFF for c in rows if c[3] != DC.LOCAL and c[6] is None and c[8] != DC.GRE)
        loc = [c for c in rows if c[3] == DC.LOCAL]
        assert {c[11][2] for c in loc} == {0, 1, 2, 3, 4}                  # every stage
        assert any(c[11][0] > 0 for c in loc) and any(c[2] == 0 for c in loc)
        assert any(c[9] & DC.F_FRAGMENT for c in loc) and any(c[9] & DC.F_EGRESS for c in loc)
        assert any(c[5] == 0 for c in loc) and any(c[5] == L.HOST_ID for c in loc)
        assert any(c[6] is not None and c[6] not in DC.SECLABELS for c in loc)
        assert any(c[4] == DC.MAX_EP for c in loc) and any(c[4] > 0xFFFF for c in loc)
    assert L.STAGE_NOT_LOCAL == DC.NOT_LOCAL == 9 and L.FWD_LOCAL == DC.LOCAL


def test_reference_counts_only_local_packets():
    """counters and metrics of a batch: the hit entries' packets / bytes, the
    {0, 133, 137} x ingress metrics, nothing for a redirect or a packet that
    is not LOCAL"""
    rows = DC.case_rows(False, 1, False)
    c = DC.columns(rows)
    o = DC.new_oracle(DC.load_policy)
    got = DC.reference(o, False, c["action"], c["arg"], DC.labels(c), c["dport"], c["proto"], c["flags"], c["len"],
                       max_ep=DC.MAX_EP)
    exp = DC.expected(rows)
    for k in exp:
        np.testing.assert_array_equal(got[k], exp[k], err_msg=k)
    m = np.asarray(o.metrics()).reshape(256, 4, 2)
    loc = c["action"] == DC.LOCAL
    for reason, sel in ((0, exp["verdict"] == 0), (133, exp["verdict"] == DC.DROP_POLICY),
                        (137, exp["verdict"] == DC.DROP_CT_UNKNOWN_PROTO)):
        sel = sel & loc
        assert sel.any()
        assert (int(m[reason, 1, 0]), int(m[reason, 1, 1])) == (int(sel.sum()), int(c["len"][sel].sum())), reason
    assert int(m[:, :, 0].sum()) == int((loc & (exp["verdict"] <= 0)).sum())
    rc, e = o.policy_lookup(5, L.policy_key(1001, 80, DC.TCP, 0))
    e = np.frombuffer(e, L.POLICY_ENTRY)[0]
    hits = [r for r in rows if r[3] == DC.LOCAL and r[5] == 1001 and r[7] == L.htons(80) and r[11][2] == 1]
    assert rc == 0 and int(e["packets"]) == len(hits) >= 3 and int(e["bytes"]) == sum(r[10] for r in hits)
    rc, e = o.policy_lookup(5, L.policy_key(1001, 8080, DC.TCP, 0))
    assert rc == 0 and int(np.frombuffer(e, L.POLICY_ENTRY)[0]["packets"]) == 1  # the redirect counts on its entry
    o.close()


# --------------------------------------------------------------------------
# the call's argument checks (no device)
# --------------------------------------------------------------------------
def _cols(n=8):
    """host arrays standing in for device columns: the checks read no element"""
    a = {"action": np.zeros(n, np.uint8), "arg": np.zeros(n, np.uint32), "src_label": np.zeros(n, np.uint32),
         "src_ep": np.zeros(n, np.uint16), "dport": np.zeros(n, np.uint16), "proto": np.zeros(n, np.uint8),
         "flags": np.zeros(n, np.uint8), "len": np.zeros(n, np.uint32), "verdict": np.zeros(n, np.int32),
         "identity": np.zeros(n, np.uint32), "stage": np.zeros(n, np.uint8)}
    return a, {k: v.ctypes.data for k, v in a.items()}


def _call(e, v6, p, n=4, iv=True, ov=True):
    i = DlvIn(*[p.get(k) for k in ("action", "arg", "src_label", "src_ep", "dport", "proto", "flags", "len")])
    o = DlvOut(*[p.get(k) for k in ("verdict", "identity", "stage")])
    fn = e.L.cgpu_deliver_v6 if v6 else e.L.cgpu_deliver_v4
    return fn(e.h, C.byref(i) if iv else None, n, C.byref(o) if ov else None, None)


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_deliver_on_a_host_only_context(v6):
    e = Engine(device=-1)
    keep, p = _cols()
    good = {k: v for k, v in p.items() if k != "src_ep"}
    assert _call(e, v6, good) == -errno.ENODEV
    assert _call(e, v6, {k: v for k, v in p.items() if k != "src_label"}) == -errno.ENODEV
    assert _call(e, v6, {k: v for k, v in good.items() if k not in ("identity", "stage")}) == -errno.ENODEV
    assert _call(e, v6, good, n=0) == -errno.ENODEV                 # no device: nothing to return 0 from
    # a malformed call is -EINVAL whatever the context
    assert _call(e, v6, good, iv=False) == -errno.EINVAL
    assert _call(e, v6, good, ov=False) == -errno.EINVAL
    for k in ("action", "arg", "dport", "proto", "flags", "len", "verdict"):
        assert _call(e, v6, {a: b for a, b in good.items() if a != k}) == -errno.EINVAL, k
    assert _call(e, v6, p) == -errno.EINVAL                          # both label forms
    assert _call(e, v6, {k: v for k, v in good.items() if k != "src_label"}) == -errno.EINVAL  # neither
    for k in ("arg", "src_label", "len", "verdict", "identity"):
        for off in (1, 2):
            assert _call(e, v6, dict(good, **{k: good[k] + off})) == -errno.EINVAL, (k, off)
    for k in ("src_ep", "dport"):
        q = {a: b for a, b in p.items() if a != "src_label"}
        assert _call(e, v6, dict(q, **{k: q[k] + 1})) == -errno.EINVAL, k
    fn = e.L.cgpu_deliver_v6 if v6 else e.L.cgpu_deliver_v4
    assert fn(None, C.byref(DlvIn()), 0, C.byref(DlvOut()), None) == -errno.EINVAL
    del keep
    e.close()


class _T:
    """what the wrapper reads of a tensor before the library refuses the call"""

    def __init__(self, a):
        self.a = a
        self.device = "cpu"

    def numel(self):
        return self.a.size

    def data_ptr(self):
        return self.a.ctypes.data


def test_wrapper_value_errors():
    e = Engine(device=-1)
    a, _ = _cols()
    t = {k: _T(v) for k, v in a.items()}
    args = [t[k] for k in ("action", "arg", "dport", "proto", "flags", "len")]
    for fn in (e.deliver_v4, e.deliver_v6):
        with pytest.raises(ValueError):
            fn(*args)                                               # neither label form
        with pytest.raises(ValueError):
            fn(*args, src_label=t["src_label"], src_ep=t["src_ep"])  # both
    fwd = dict(mode=L.FWD_LXC, encap=True, ipv4_mask=0xFFFF, host_ifindex=1, encap_ifindex=1)
    for fn in (e.classify_v4, e.classify_v6):
        with pytest.raises(ValueError):
            fn({}, deliver=True)                                    # no forward=
        with pytest.raises(ValueError):
            fn({}, forward=dict(fwd, mode=L.FWD_NETDEV), deliver=True)
    for fn in (e.classify_v4_ct, e.classify_v6_ct):
        with pytest.raises(ValueError, match="conntrack form"):
            fn({}, 0, forward=fwd, deliver=True)
        with pytest.raises(ValueError, match="conntrack form"):
            fn({}, 0, deliver=True)
    for fn in (e.classify_v4_lb, e.classify_v6_lb, e.classify_v4_cascade):
        with pytest.raises(ValueError):
            fn({}, forward=fwd)                                     # the service paths: as before
    for fn in (e.classify_v4_ctlb, e.classify_v6_ctlb):
        with pytest.raises(ValueError):
            fn({}, 0, forward=fwd)
    e.close()


# --------------------------------------------------------------------------
# the crafted inputs of the device tests
# --------------------------------------------------------------------------
@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_crafted_batch_holds_its_categories(v6):
    b = DC.crafted_batch(v6)
    n = len(b["action"])
    assert n > 10_000 and n % 4 != 0
    o = DC.new_oracle(lambda t: DC.load_crafted_policy(t, 1))
    r = DC.reference(o, v6, b["action"], b["arg"], b["src_label"], b["dport"], b["proto"], b["flags"], b["len"])
    o.close()
    assert set(np.unique(r["stage"]).tolist()) == {0, 1, 2, 3, 4}
    assert (b["flags"] & DC.F_FRAGMENT).any() and (r["verdict"] > 0).any() and (b["len"] >= 2048).any()
    assert (b["len"] >= (1 << 18)).any()                            # past a packed counter's length bound
    gated = r["stage"] == 4
    assert (r["identity"][~gated] == b["src_label"][~gated]).all() and (r["identity"][gated] == 0).all()
    assert len(np.unique(b["src_label"])) > 100 and (b["src_label"] < 256).any()  # a reserved label among them
