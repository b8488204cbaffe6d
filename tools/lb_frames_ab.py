"""Cost of the service step on raw frames (cgpu_classify_frames_lb) against the
frames call without it and against the tuple path with it.

    python tools/lb_frames_ab.py [--steps K] [--warmup W] [--tuples N] [--step-timeout S] [--out FILE]   (GPU box)

bench.py's config-5 workload (the config-2 tables, 1M IPv4 services, 64M
tuples of which 30 % of the egress ones aim at a service) as frames in 64-byte
slots (synth.frames_from_tuples).  Three contexts over the same tables: one on
the per-lane schedule (CGPU_SCHED_PER_LANE: the kernel the new one is shaped
after), one with an empty service map, one with the 1M services.  Timed with
device events, medians after W warm-ups, the kinds alternating call by call,
every call under a time limit of its own (the process is killed when one takes
longer than S seconds):

  frames_per_lane   classify_frames, per-lane schedule, no service step
  empty_decide      classify_frames_lb(rewrite=False), empty service map
  empty_rewrite     classify_frames_lb(rewrite=True),  empty service map
  svc_decide        classify_frames_lb(rewrite=False), 1M services
  svc_rewrite       classify_frames_lb(rewrite=True),  1M services; the slots are
                    put back from a pristine copy before every call, outside
                    the timed span (a translated frame no longer aims at a service)
  tuples_lb         classify_v4_lb on the tuples the frames were made of

The hash column is the tuples' own in every service run.  Prints one JSON line
(and writes it to --out, by default under profiles/lb_frames/).
"""
import argparse
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cilium_amd import layouts as L, synth  # noqa: E402
from cilium_amd.engine import Engine  # noqa: E402

SCHED_PER_LANE = 1  # CGPU_SCHED_PER_LANE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tuples", type=int, default=synth.CONFIGS["cascade"]["n_tuples"])
    ap.add_argument("--services", type=int, default=synth.CONFIGS["cascade"]["n_services"])
    ap.add_argument("--step-timeout", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lb_frames", "lb_frames_ab.json"))
    a = ap.parse_args()
    n = a.tuples

    def note(msg):   # progress on stderr: the run is long and silent otherwise
        print(f"lb_frames_ab: {msg}", file=sys.stderr, flush=True)
    cfg = {k: v for k, v in synth.CONFIGS["cascade"].items() if k not in ("n_tuples", "n_services")}
    T = synth.make_tables(**cfg)
    S = synth.make_services(T, a.services)
    tup = synth.add_service_traffic(synth.make_tuples(T, n), S)
    note(f"{n} tuples, {a.services} services made")

    def engine(services, **kw):
        e = Engine(device=0, **T.engine_config(), lb_flags=L.LB_L3 | L.LB_L4, lb_max_entries=len(S.keys), **kw)
        synth.load_engine(e, T)
        if services:
            synth.load_services(e, S)
        e.commit()
        return e
    e_lane, e_empty, e_svc = engine(False, schedule=SCHED_PER_LANE), engine(False), engine(True)
    f = synth.frames_to_device(synth.frames_from_tuples(tup, stride=64))
    pristine = f["data"].clone()
    d = synth.to_device(tup)
    h = d["hash"]
    note("engines committed, frames on the device")

    def outs(lb):
        o = {"verdict": torch.empty(n, dtype=torch.int32, device="cuda"),
             "identity": torch.empty(n, dtype=torch.int32, device="cuda"),
             "stage": torch.empty(n, dtype=torch.uint8, device="cuda")}
        if lb:
            o.update(lb_ret=torch.empty(n, dtype=torch.int32, device="cuda"),
                     rev_nat=torch.empty(n, dtype=torch.int16, device="cuda"),
                     slave=torch.empty(n, dtype=torch.int16, device="cuda"))
        return o
    o = {k: outs(k not in ("frames_per_lane", "tuples_lb")) for k in
         ("frames_per_lane", "empty_decide", "empty_rewrite", "svc_decide", "svc_rewrite", "tuples_lb")}
    runs = {"frames_per_lane": lambda: e_lane.classify_frames(f, out=o["frames_per_lane"]),
            "empty_decide": lambda: e_empty.classify_frames_lb(f, hash=h, rewrite=False, out=o["empty_decide"]),
            "empty_rewrite": lambda: e_empty.classify_frames_lb(f, hash=h, rewrite=True, out=o["empty_rewrite"]),
            "svc_decide": lambda: e_svc.classify_frames_lb(f, hash=h, rewrite=False, out=o["svc_decide"]),
            "svc_rewrite": lambda: e_svc.classify_frames_lb(f, hash=h, rewrite=True, out=o["svc_rewrite"]),
            "tuples_lb": lambda: e_svc.classify_v4_lb(d, out=o["tuples_lb"])}

    def timed(k):
        """one call between two device events, killed past the time limit"""
        if k == "svc_rewrite":
            f["data"].copy_(pristine)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        signal.alarm(a.step_timeout)
        ev0.record()
        runs[k]()
        ev1.record()
        ev1.synchronize()
        signal.alarm(0)
        if k == "svc_rewrite":
            f["data"].copy_(pristine)
        return ev0.elapsed_time(ev1)
    for i in range(a.warmup):
        for k in runs:
            timed(k)
        note(f"warm-up {i + 1} of {a.warmup}")
    ms = {k: [] for k in runs}
    for i in range(a.steps):
        for k in runs:
            ms[k].append(timed(k))
        note(f"step {i + 1} of {a.steps}: " + " ".join(f"{k} {ms[k][-1]:.3f}" for k in runs))
    # the runs agree where they must: an empty map is the call without the step and the flag changes no
    # column; how many frames decide otherwise than the tuples they were made of is reported
    for k in ("verdict", "identity", "stage"):
        assert torch.equal(o["frames_per_lane"][k], o["empty_decide"][k]), k
        assert torch.equal(o["empty_decide"][k], o["empty_rewrite"][k]), k
        assert torch.equal(o["svc_decide"][k], o["svc_rewrite"][k]), k
    differ = int((o["svc_decide"]["verdict"] != o["tuples_lb"]["verdict"]).sum())
    ret = o["svc_decide"]["lb_ret"].cpu().numpy()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rec = {"tool": "lb_frames_ab", "frames": n, "stride": 64, "services": a.services, "steps": a.steps,
           "warmup": a.warmup,
           **{f"{k}_ms_median": round(med[k], 4) for k in ms}, **{f"{k}_ms_min": round(min(ms[k]), 4) for k in ms},
           **{f"{k}_ms_max": round(max(ms[k]), 4) for k in ms},
           "verdicts_differing_from_tuples_lb": differ, "frames_translated": int((ret > 0).sum()),
           "frames_no_service": int((ret == L.DROP_NO_SERVICE).sum()),
           "empty_decide_over_frames_per_lane": round(med["empty_decide"] / med["frames_per_lane"], 3),
           "svc_decide_over_frames_per_lane": round(med["svc_decide"] / med["frames_per_lane"], 3),
           "svc_rewrite_over_svc_decide": round(med["svc_rewrite"] / med["svc_decide"], 3),
           "svc_decide_over_tuples_lb": round(med["svc_decide"] / med["tuples_lb"], 3)}
    for e in (e_lane, e_empty, e_svc):
        e.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
