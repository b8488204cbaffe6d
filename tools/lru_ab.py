"""Cost of LRU conntrack mode (cgpu_config.ct_lru) on the four conntrack paths.

    python tools/lru_ab.py [--config ctlb|ctlb6|ct|ct6] [--steps K] [--warmup W] [--tuples N] [--out FILE]   (GPU box)

bench.py's workload of that config (ct / ct6: config-2 tables, packets of ~32
per connection; ctlb / ctlb6: the same behind 1M / 100k services) on three
contexts:

  roomy, ct_lru = 0 and roomy, ct_lru = 1: the same batch classified from an
      emptied map (as bench.py's steps), alternating call by call.  Nothing
      is evicted, so the ratio is the price of the mode itself: the filter's
      clear and the mark passes (on the service paths the candidate-backend
      pass before the service walk and the record pass after the prep).
  evicting, ct_lru = 1: the batch's two halves (mostly disjoint connections)
      alternate, the map carried across calls, on a map of 1.5 times the
      entries one half needs: every call evicts what the other half left.
      Read against the same halves on the roomy ct_lru = 0 context, each from
      an emptied map (about as many creates, no evictions).

Every call is timed with device events after W warm-up rounds.  Prints one JSON
line: median / min ms of each, the two ratios, evictions and no-victim creates
per evicting call.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cilium_amd import synth  # noqa: E402
from cilium_amd.engine import Engine  # noqa: E402

PKTS_PER_CONN = 32  # bench.py CT_PKTS_PER_CONN


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ctlb", choices=["ctlb", "ctlb6", "ct", "ct6"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tuples", type=int, default=synth.CONFIGS["gpu"]["n_tuples"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    v6, svc = a.config.endswith("6"), a.config.startswith("ctlb")
    n = a.tuples
    T = synth.make_tables6(**synth.CONFIGS["v6"]) if v6 else synth.make_tables(**synth.CONFIGS["gpu"])
    S = None
    if svc:
        S = synth.make_services6(T, 100_000) if v6 else synth.make_services(T, synth.CONFIGS["cascade"]["n_services"])
        mk = synth.make_ctlb6_workload if v6 else synth.make_ctlb_workload
        tup, _, seclabels, S = mk(T, S, n // PKTS_PER_CONN, mean_pkts=PKTS_PER_CONN, loop_frac=1e-4)
    else:
        mk = synth.make_ct6_workload if v6 else synth.make_ct_workload
        tup, _, seclabels = mk(T, n // PKTS_PER_CONN, mean_pkts=PKTS_PER_CONN)
    n = min(n, len(tup["saddr"])) & ~1
    tup = {k: np.ascontiguousarray(v[:n]) for k, v in tup.items()}
    roomy_max = 1 << max(20, int(np.ceil(np.log2((4.5 if svc else 2.5) * n / PKTS_PER_CONN))))
    ecfg = T.engine_config()
    if S is not None:
        ecfg["lb_max_entries"] = len(S.keys)

    def engine(ct_max, lru):
        e = Engine(device=0, **ecfg, ct_max=ct_max, ct_lru=lru)
        synth.load_engine(e, T)
        synth.load_lxc(e, seclabels)
        if S is not None:
            (synth.load_services6 if v6 else synth.load_services)(e, S)
        e.commit()
        return e

    def outs(m):
        o = {"verdict": torch.empty(m, dtype=torch.int32, device="cuda"),
             "ct_ret": torch.empty(m, dtype=torch.uint8, device="cuda"),
             "identity": torch.empty(m, dtype=torch.int32, device="cuda"), "stage": None}
        if svc:
            o["daddr"] = (torch.empty((m, 16), dtype=torch.uint8, device="cuda") if v6 else
                          torch.empty(m, dtype=torch.int32, device="cuda"))
            o["dport"] = torch.empty(m, dtype=torch.int16, device="cuda")
        return o

    meth = f"classify_v{6 if v6 else 4}_ct{'lb' if svc else ''}"
    flush, count = ("ct6_flush", "ct6_count") if v6 else ("ct4_flush", "ct4_count")

    def timed(e, d, o, now):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        getattr(e, meth)(d, now, out=o)
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1)

    d = synth.to_device(tup)
    halves = [{k: v[:n // 2] for k, v in d.items()}, {k: v[n // 2:] for k, v in d.items()}]
    e0, e1 = engine(roomy_max, 0), engine(roomy_max, 1)
    o0, o1, oh = outs(n), outs(n), outs(n // 2)
    ms = {"lru0": [], "lru1": [], "half_lru0": [], "evicting": []}
    for it in range(a.warmup + a.steps):
        for k, e, o in (("lru0", e0, o0), ("lru1", e1, o1)):
            getattr(e, flush)()  # every call starts from an empty conntrack map
            t = timed(e, d, o, 1000)
            if it >= a.warmup:
                ms[k].append(t)
    for f in ("verdict", "ct_ret", "identity"):
        assert torch.equal(o0[f], o1[f]), f
    assert e1.ct_lru_stats(v6) == {"evictions": 0, "no_victim": 0}
    e1.close()
    need = []
    for h in halves:  # entries one half needs (and the roomy reference of the evicting runs)
        getattr(e0, flush)()
        timed(e0, h, oh, 1000)
        need.append(getattr(e0, count)())
    evict_max = int(1.5 * max(need))
    e2 = engine(evict_max, 1)
    st0 = None
    for it in range(a.warmup + a.steps):
        for h in halves:
            getattr(e0, flush)()
            t0 = timed(e0, h, oh, 1000)
            if it == a.warmup and st0 is None:
                st0 = e2.ct_lru_stats(v6)
            t2 = timed(e2, h, oh, 1000 + it)
            if it >= a.warmup:
                ms["half_lru0"].append(t0)
                ms["evicting"].append(t2)
    st1 = e2.ct_lru_stats(v6)
    calls = 2 * a.steps
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rec = {"tool": "lru_ab", "config": a.config, "packets": n, "steps": a.steps, "warmup": a.warmup,
           "roomy_ct_max": roomy_max,
           "lru0_ms_median": round(med["lru0"], 4), "lru0_ms_min": round(min(ms["lru0"]), 4),
           "lru1_ms_median": round(med["lru1"], 4), "lru1_ms_min": round(min(ms["lru1"]), 4),
           "ratio_roomy_median": round(med["lru1"] / med["lru0"], 4),
           "evict_ct_max": evict_max, "entries_per_half": need,
           "half_lru0_ms_median": round(med["half_lru0"], 4), "half_lru0_ms_min": round(min(ms["half_lru0"]), 4),
           "evicting_ms_median": round(med["evicting"], 4), "evicting_ms_min": round(min(ms["evicting"]), 4),
           "ratio_evicting_median": round(med["evicting"] / med["half_lru0"], 4),
           "evictions_per_call": (st1["evictions"] - st0["evictions"]) // calls,
           "no_victim_per_call": (st1["no_victim"] - st0["no_victim"]) // calls,
           "entries_evicting_map": getattr(e2, count)()}
    e0.close()
    e2.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
