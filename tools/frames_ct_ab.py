"""Cost of the stateful path on raw frames (cgpu_classify_frames_ct) beside the
conntrack call on pre-parsed columns that it wraps.

    python tools/frames_ct_ab.py [--steps K] [--warmup W] [--tuples N] [--step-timeout S] [--family 4|6|both]
                                 [--out FILE]                                                        (GPU box)

bench.py's conntrack workload (the config-2 tables, 16.8M packets of ~32 per
connection; tools/rnat_frames_ab.py runs on the same) as frames in 64-byte
slots (synth.frames_from_ct), and the IPv6 conntrack workload (--config ct6)
in 80-byte slots.  Timed with device events around each call (the calls wait
on the host inside: the span covers that), medians after W warm-ups, the kinds
alternating call by call, the conntrack map emptied before every conntrack
call, every call under a time limit of its own (the process is killed when one
takes longer than S seconds):

  ct_columns     (a) classify_v4_ct / classify_v6_ct on the pre-parsed columns
  parse          (b) frames_parse_ct alone
  frames_ct      (c) classify_frames_ct
  frames_ct_rn   (d) (c) with rev_nat=dict(rewrite=True) (the _rnat conntrack call and the two
                     rnat_frames passes; the workload's entries carry index 0, so nothing is applied)

(c) is judged against (a) + (b): the difference is the price of the two
selections, the gather, the scatter and the extra host wait.  The frames on which (c)'s verdict,
ct_ret, identity or stage differ from (a)'s are counted before anything is
timed (0 is expected: the frames carry the columns).
Prints one JSON line per family (and writes them to --out, by default under
profiles/frames_ct/).
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

from cilium_amd import synth  # noqa: E402
from cilium_amd.engine import Engine  # noqa: E402

PKTS_PER_CONN = 32  # bench.py CT_PKTS_PER_CONN


def note(msg):   # progress on stderr: the run is long and silent otherwise
    print(f"frames_ct_ab: {msg}", file=sys.stderr, flush=True)


def family(v6: bool, a) -> dict:
    stride = 80 if v6 else 64
    if v6:
        T = synth.make_tables6(**synth.CONFIGS["v6"])
        tup, _, seclabels = synth.make_ct6_workload(T, a.tuples // PKTS_PER_CONN, mean_pkts=PKTS_PER_CONN)
    else:
        T = synth.make_tables(**synth.CONFIGS["gpu"])
        tup, _, seclabels = synth.make_ct_workload(T, a.tuples // PKTS_PER_CONN, mean_pkts=PKTS_PER_CONN)
    n = min(a.tuples, len(tup["saddr"]))
    tup = {k: np.ascontiguousarray(v[:n]) for k, v in tup.items()}
    fr, tup = synth.frames_from_ct(tup, stride=stride, v6=v6)
    note(f"IPv{6 if v6 else 4}: {n} packets made")
    ct_max = 1 << max(20, int(np.ceil(np.log2(2.5 * n / PKTS_PER_CONN))))
    e = Engine(device=0, **T.engine_config(), ct_max=ct_max, ct6_max=ct_max)
    synth.load_engine(e, T)
    synth.load_lxc(e, seclabels)
    e.commit()
    f = synth.frames_to_device(fr)
    del fr
    d = synth.to_device(tup)
    flush = e.ct6_flush if v6 else e.ct4_flush
    ct = e.classify_v6_ct if v6 else e.classify_v4_ct

    def outs(keys):
        dt = {"status": torch.int32, "family": torch.uint8, "verdict": torch.int32, "ct_ret": torch.uint8,
              "identity": torch.int32, "stage": torch.uint8}
        return {k: torch.empty(n, dtype=dt[k], device="cuda") for k in keys}
    o_a = outs(("verdict", "ct_ret", "identity", "stage"))
    o_c = outs(("status", "family", "verdict", "ct_ret", "identity", "stage"))
    o_d = outs(("status", "family", "verdict", "ct_ret", "identity", "stage"))
    o_b = e.frames_parse_ct(f)
    # (c) against (a) once: the frames carry the columns
    flush()
    ct(d, 1000, out=o_a)
    flush()
    e.classify_frames_ct(f, 1000, out=o_c)
    torch.cuda.synchronize()
    differ = int(torch.stack([o_a[k] != o_c[k] for k in ("verdict", "ct_ret", "identity", "stage")]).any(0).sum().item())
    reach = int((o_c["status"] == 0).sum().item())
    note(f"IPv{6 if v6 else 4}: engine committed, {reach} of {n} frames reach conntrack, "
         f"{differ} frames differ from (a)")
    runs = {"ct_columns": lambda: ct(d, 1000, out=o_a),
            "parse": lambda: e.frames_parse_ct(f, out=o_b),
            "frames_ct": lambda: e.classify_frames_ct(f, 1000, out=o_c),
            "frames_ct_rn": lambda: e.classify_frames_ct(f, 1000, out=o_d, rev_nat=dict(rewrite=True))}

    def timed(k):
        """one call between two device events, killed past the time limit"""
        if k != "parse":
            flush()   # every conntrack call starts from an empty map
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        signal.alarm(a.step_timeout)
        ev0.record()
        runs[k]()
        ev1.record()
        ev1.synchronize()
        signal.alarm(0)
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
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rec = {"tool": "frames_ct_ab", "family": 6 if v6 else 4, "frames": n, "stride": stride, "steps": a.steps,
           "warmup": a.warmup, "frames_reaching_conntrack": reach, "frames_differing_from_ct_columns": differ,
           **{f"{k}_ms_median": round(med[k], 4) for k in ms}, **{f"{k}_ms_min": round(min(ms[k]), 4) for k in ms},
           **{f"{k}_ms_max": round(max(ms[k]), 4) for k in ms},
           "frames_ct_minus_ct_columns_minus_parse_ms": round(med["frames_ct"] - med["ct_columns"] - med["parse"], 4),
           "frames_ct_over_ct_columns": round(med["frames_ct"] / med["ct_columns"], 3),
           "rev_nat_chain_ms": round(med["frames_ct_rn"] - med["frames_ct"], 4)}
    e.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tuples", type=int, default=synth.CONFIGS["gpu"]["n_tuples"])
    ap.add_argument("--step-timeout", type=int, default=60)
    ap.add_argument("--family", default="both", choices=("4", "6", "both"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_ct", "frames_ct_ab.json"))
    a = ap.parse_args()
    lines = []
    for v6 in (False, True):
        if a.family in ("both", "6" if v6 else "4"):
            lines.append(json.dumps(family(v6, a)))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
