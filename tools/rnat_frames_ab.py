"""Cost of reverse NAT on raw frames (cgpu_rnat_frames_v4) beside the two passes
it stands next to: the reverse-NAT output of the conntrack call that feeds it,
and the forwarding step on the same frames.

    python tools/rnat_frames_ab.py [--steps K] [--warmup W] [--tuples N] [--step-timeout S] [--out FILE]   (GPU box)

bench.py's conntrack workload (the config-2 tables, 64M packets of 2M
connections; tools/revnat_ab.py --config ct, with its reverse-NAT map of every
index) as frames in 64-byte slots (synth.frames_from_tuples, the tuple's sport
on the wire), and the rn columns of one classify_v4_ct(rev_nat=True) call over
it.  That stream's entries carry index 0, so the batch's own applied share is
what the call finds (reported; 0 unless the workload changes): the step is
therefore also timed on synthetic applied columns, one frame in ten (seeded)
and every frame, with the same saddr / daddr / sport columns.  Timed with
device events, medians after W warm-ups, the kinds alternating call by call,
every call under a time limit of its own (the process is killed when one takes
longer than S seconds); a rewriting call gets its slots back from a pristine
copy before the call, outside the timed span:

  own_decide / own_rewrite      rnat_frames(rewrite=False / True), the batch's own applied column
  tenth_decide / tenth_rewrite  the same with applied = 1 on one frame in ten
  all_decide / all_rewrite      the same with applied = 1 everywhere
  ct_plain / ct_rev_nat         classify_v4_ct without / with rev_nat=True (conntrack map emptied
                                before every call): their difference is the k_ct_rnat pass
  forward_rewrite               forward_frames(rewrite=True) on the same frames with the
                                conntrack call's verdicts

Prints one JSON line (and writes it to --out, by default under
profiles/rnat_frames/), with the bytes per frame each kind of lane moves and
the floor that gives at the measured streamed rates (profiles/ceilings.json).
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

PKTS_PER_CONN = 32  # bench.py CT_PKTS_PER_CONN
# bytes per frame: every lane reads applied (1) and writes ret (4); an applied lane of a deciding call also
# reads the slot's 64 bytes and len (4); a rewriting one also sport, saddr, daddr (10) and stores up to three
# 16-byte words (a TCP frame: the address / header-checksum words 16..47 and the checksum's word 48..63)
IDLE_READ, IDLE_WRITE = 1, 4
APPLIED_READ, APPLIED_READ_RW, APPLIED_WRITE_RW = 64 + 4, 64 + 4 + 10, 48


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tuples", type=int, default=synth.CONFIGS["gpu"]["n_tuples"])
    ap.add_argument("--step-timeout", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnat_frames", "rnat_frames_ab.json"))
    a = ap.parse_args()

    def note(msg):   # progress on stderr: the run is long and silent otherwise
        print(f"rnat_frames_ab: {msg}", file=sys.stderr, flush=True)
    T = synth.make_tables(**synth.CONFIGS["gpu"])
    tup, _, seclabels = synth.make_ct_workload(T, a.tuples // PKTS_PER_CONN, mean_pkts=PKTS_PER_CONN)
    n = min(a.tuples, len(tup["saddr"]))
    tup = {k: np.ascontiguousarray(v[:n]) for k, v in tup.items()}
    note(f"{n} packets made")
    ct_max = 1 << max(20, int(np.ceil(np.log2(2.5 * n / PKTS_PER_CONN))))
    e = Engine(device=0, **T.engine_config(), ct_max=ct_max)
    synth.load_engine(e, T)
    synth.load_lxc(e, seclabels)
    for ix in range(1, 65536):
        v = np.zeros((), L.LB4_REVERSE_NAT)
        v["address"], v["port"] = 0x0A600000 + ix, ix
        assert e.revnat4_update(ix, v) == 0
    e.commit()
    fr = synth.frames_from_tuples(tup, stride=64)
    fr["data"][:, 34:36] = np.ascontiguousarray(tup["sport"], np.uint16).view(np.uint8).reshape(n, 2)
    f = synth.frames_to_device(fr)
    del fr
    pristine = f["data"].clone()
    d = synth.to_device(tup)
    note("engine committed, frames on the device")

    def ct_outs(rn):
        o = {"verdict": torch.empty(n, dtype=torch.int32, device="cuda"),
             "ct_ret": torch.empty(n, dtype=torch.uint8, device="cuda"),
             "identity": torch.empty(n, dtype=torch.int32, device="cuda"),
             "stage": torch.empty(n, dtype=torch.uint8, device="cuda")}
        if rn:
            o.update(rn_saddr=torch.empty(n, dtype=torch.int32, device="cuda"),
                     rn_daddr=torch.empty(n, dtype=torch.int32, device="cuda"),
                     rn_sport=torch.empty(n, dtype=torch.int16, device="cuda"),
                     rn_applied=torch.empty(n, dtype=torch.uint8, device="cuda"))
        return o
    plain, rn = ct_outs(False), ct_outs(True)
    e.ct4_flush()
    e.classify_v4_ct(d, 1000, out=rn, rev_nat=True)
    torch.cuda.synchronize()
    own_share = float(rn["rn_applied"].float().mean().item())
    # synthetic columns: a service address and port for every frame, applied on one in ten / on all
    g = torch.Generator(device="cuda")
    g.manual_seed(20)
    syn = {"rn_saddr": torch.full((n,), int(L.ip4_be("10.96.0.10")), dtype=torch.int32, device="cuda"),
           "rn_daddr": rn["rn_daddr"], "rn_sport": torch.full((n,), int(L.htons(80)), dtype=torch.int16, device="cuda")}
    tenth = dict(syn, rn_applied=(torch.rand(n, device="cuda", generator=g) < 0.1).to(torch.uint8))
    every = dict(syn, rn_applied=torch.ones(n, dtype=torch.uint8, device="cuda"))
    own = {k: rn[k].clone() for k in ("rn_saddr", "rn_daddr", "rn_sport", "rn_applied")}
    ret = {k: torch.empty(n, dtype=torch.int32, device="cuda") for k in ("own", "tenth", "all")}
    fwd = {"action": torch.empty(n, dtype=torch.uint8, device="cuda"),
           "ret": torch.empty(n, dtype=torch.int32, device="cuda"),
           "ifindex": torch.empty(n, dtype=torch.int32, device="cuda"),
           "arg": torch.empty(n, dtype=torch.int32, device="cuda")}
    verdict, stage = rn["verdict"].clone(), rn["stage"].clone()
    cols = {"own": own, "tenth": tenth, "all": every}
    runs = {}
    for k, c in cols.items():
        runs[f"{k}_decide"] = lambda c=c, k=k: e.rnat_frames(f, c, rewrite=False, out={"ret": ret[k]})
        runs[f"{k}_rewrite"] = lambda c=c, k=k: e.rnat_frames(f, c, rewrite=True, out={"ret": ret[k]})
    runs["ct_plain"] = lambda: e.classify_v4_ct(d, 1000, out=plain)
    runs["ct_rev_nat"] = lambda: e.classify_v4_ct(d, 1000, out=rn, rev_nat=True)
    runs["forward_rewrite"] = lambda: e.forward_frames(f, verdict=verdict, stage=stage, rewrite=True, out=fwd)
    writes = {"own_rewrite", "tenth_rewrite", "all_rewrite", "forward_rewrite"}
    decided = {}

    def timed(k):
        """one call between two device events, killed past the time limit"""
        if k in writes:
            f["data"].copy_(pristine)
        if k.startswith("ct_"):
            e.ct4_flush()   # every call starts from an empty conntrack map
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        signal.alarm(a.step_timeout)
        ev0.record()
        runs[k]()
        ev1.record()
        ev1.synchronize()
        signal.alarm(0)
        if k.endswith("_decide"):
            assert torch.equal(f["data"], pristine), k   # a deciding call changes no byte
            decided[k[:-7]] = ret[k[:-7]].clone()
        elif k in writes and k != "forward_rewrite":
            assert torch.equal(ret[k[:-8]], decided[k[:-8]]), k   # and gives the rewriting call's ret
        if k in writes:
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
    med = {k: float(np.median(v)) for k, v in ms.items()}
    c = json.load(open(os.path.join(ROOT, "profiles", "ceilings.json")))["stream"]
    rd, wr = c.get("read_gbs", c["write_gbs"]) * 1e9, c["write_gbs"] * 1e9

    def floor(share, rw):
        r = IDLE_READ + share * (APPLIED_READ_RW if rw else APPLIED_READ)
        w = IDLE_WRITE + (share * APPLIED_WRITE_RW if rw else 0)
        return round(n * (r / rd + w / wr) * 1e3, 4)
    shares = {"own": own_share, "tenth": float(tenth["rn_applied"].float().mean().item()), "all": 1.0}
    rec = {"tool": "rnat_frames_ab", "frames": n, "stride": 64, "steps": a.steps, "warmup": a.warmup,
           **{f"{k}_applied_share": round(s, 6) for k, s in shares.items()},
           **{f"{k}_ms_median": round(med[k], 4) for k in ms}, **{f"{k}_ms_min": round(min(ms[k]), 4) for k in ms},
           **{f"{k}_ms_max": round(max(ms[k]), 4) for k in ms},
           **{f"{k}_{m}_floor_ms": floor(s, m == "rewrite") for k, s in shares.items() for m in ("decide", "rewrite")},
           "ct_rnat_pass_ms_median": round(med["ct_rev_nat"] - med["ct_plain"], 4),
           "frames_dropped_all_applied": int((decided["all"] != 0).sum().item()),
           "all_rewrite_over_forward_rewrite": round(med["all_rewrite"] / med["forward_rewrite"], 3),
           "tenth_rewrite_over_forward_rewrite": round(med["tenth_rewrite"] / med["forward_rewrite"], 3)}
    e.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
