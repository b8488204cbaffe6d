"""Cost of the tunnel output of the stateless classify (cgpu_classify_v4_tun /
cgpu_classify_v6_tun, cgpu_config.ipcache_tunnel).

    python tools/tunnel_ab.py [--config 2|v6] [--steps K] [--warmup W] [--tuples N] [--out FILE]   (GPU box)

One context with the flag set, bench.py's workload of that config (config 2:
64M IPv4 tuples; v6: the IPv6 tables), every ipcache entry's tunnel drawn from
a pool of 4096 node addresses (a realistic cluster).  The same batch is
classified with and without the tunnel output, alternating call by call, each
call timed with device events after W warm-up calls of each kind; a third
context without the flag gives the device bytes the flag adds.  Prints one JSON
line: median / min ms of each, the overhead, and the two floors it is to be
read against: 4 B per tuple of output at the measured streamed
write rate, and one more lookup per egress tuple at the gather ceiling of the
ipcache's cache tier (profiles/ceilings.json).
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

def ceilings():
    """(streamed write TB/s, [(table bytes, G gathers/s)]) of profiles/ceilings.json"""
    c = json.load(open(os.path.join(ROOT, "profiles", "ceilings.json")))
    return c["stream"]["write_gbs"] / 1e3, sorted((float(b), float(r)) for b, r in c["gather"])


def gather_ceiling(pts, nbytes):
    """G gathers/s of the smallest measured table that holds nbytes"""
    best = [r for b, r in pts if b >= nbytes]
    return best[0] if best else pts[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="2", choices=["2", "v6"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tuples", type=int, default=synth.CONFIGS["gpu"]["n_tuples"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    v6 = a.config == "v6"
    n = a.tuples
    if v6:
        T = synth.make_tables6(**synth.CONFIGS["v6"])
        tup = synth.make_tuples6(T, n)
    else:
        T = synth.make_tables(**synth.CONFIGS["gpu"])
        tup = synth.make_tuples(T, n)
    pool = np.random.default_rng(7).integers(0x0A000001, 0x0AFFFFFF, 4096, dtype=np.uint64).astype(np.uint32)
    T.ipc_vals["tunnel_endpoint"] = pool[np.random.default_rng(8).integers(0, 4096, len(T.ipc_vals))]
    bytes_of = {}
    for flag in (0, 1):
        e = Engine(device=0, **{**T.engine_config(), "ipcache_tunnel": flag})
        synth.load_engine(e, T)
        e.commit()
        bytes_of[flag] = e.table_bytes()["ipcache"]
        if not flag:
            e.close()
    d = synth.to_device(tup)
    out = {"verdict": torch.empty(n, dtype=torch.int32, device="cuda"),
           "identity": torch.empty(n, dtype=torch.int32, device="cuda"), "stage": None}
    tun = dict(out, tunnel=torch.empty(n, dtype=torch.int32, device="cuda"))
    cls = e.classify_v6 if v6 else e.classify_v4
    runs = {"plain": lambda: cls(d, out=out, stage=False), "tunnel": lambda: cls(d, out=tun, stage=False, tunnel=True)}
    for _ in range(a.warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.steps):
        for k, f in runs.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            f()
            ev1.record()
            ev1.synchronize()
            ms[k].append(ev0.elapsed_time(ev1))
    assert torch.equal(out["verdict"], tun["verdict"]) and torch.equal(out["identity"], tun["identity"])
    egress = int((np.asarray(tup["flags"]) & 1).sum())
    nz = int((tun["tunnel"] != 0).sum().item())
    write_tbs, pts = ceilings()
    ceil = gather_ceiling(pts, bytes_of[1] - bytes_of[0])
    rec = {"tool": "tunnel_ab", "config": a.config, "tuples": n, "steps": a.steps, "warmup": a.warmup,
           "plain_ms_median": round(float(np.median(ms["plain"])), 4), "plain_ms_min": round(min(ms["plain"]), 4),
           "tunnel_ms_median": round(float(np.median(ms["tunnel"])), 4), "tunnel_ms_min": round(min(ms["tunnel"]), 4),
           "overhead_ms_median": round(float(np.median(ms["tunnel"]) - np.median(ms["plain"])), 4),
           "egress_tuples": egress, "tunnels_nonzero": nz,
           "ipcache_bytes_flag_off": bytes_of[0], "ipcache_bytes_flag_on": bytes_of[1],
           "floor_write_ms": round(4.0 * n / (write_tbs * 1e12) * 1e3, 4),
           "floor_lookup_ms": round(egress / (ceil * 1e9) * 1e3, 4),
           "gather_ceiling_glookups_s": ceil}
    e.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
