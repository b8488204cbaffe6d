"""Cost of the forwarding step (cgpu_forward_v4 / _v6) alone and behind the
stateless classify.

    python tools/forward_ab.py [--config 2|v6] [--steps K] [--warmup W] [--tuples N] [--out FILE]   (GPU box)

One context with cgpu_config.ipcache_tunnel, bench.py's workload of that config
(config 2: 64M IPv4 tuples; v6: the IPv6 tables), 4096 endpoints and 4096
tunnel prefixes taken from the batch's own destinations, so that every branch
of the decision occurs.  Timed with device events, medians after W warm-ups,
the kinds alternating call by call:

  forward        the forwarding call alone, on the tunnel form's outputs
  classify_tun   classify_v4(tunnel=True) / classify_v6(tunnel=True)
  classify_fwd   the same with forward=... (the two calls back to back)

Prints one JSON line with the times and the floor the forwarding call is to
be read against: its streamed bytes in and out at the measured
streamed read / write rates (profiles/ceilings.json), plus one gather per
looked-up packet of each forwarding table at the gather ceiling of the cache
tier that table's size falls in.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cilium_amd import layouts as L, synth  # noqa: E402
from cilium_amd.engine import Engine  # noqa: E402

FWD = dict(mode=L.FWD_LXC, encap=True, ipv4_mask=0xFFFF, host_ifindex=1, encap_ifindex=2)


def ceilings():
    """(streamed read TB/s, write TB/s, [(table bytes, G gathers/s)]) of profiles/ceilings.json"""
    c = json.load(open(os.path.join(ROOT, "profiles", "ceilings.json")))
    return (c["stream"]["read_gbs"] / 1e3, c["stream"]["write_gbs"] / 1e3,
            sorted((float(b), float(r)) for b, r in c["gather"]))


def gather_ceiling(pts, nbytes):
    """G gathers/s of the smallest measured table that holds nbytes"""
    best = [r for b, r in pts if b >= nbytes]
    return best[0] if best else pts[-1][1]


def load_maps(e, daddr, v6, n_each=4096):
    """n_each endpoints (every 16th the host's) and n_each tunnel prefixes out of
    the batch's destinations"""
    u = np.unique(daddr[:1 << 20], axis=0)
    rng = np.random.default_rng(3)
    u = u[rng.permutation(len(u))]
    fam = bytes([2 if v6 else 1, 0, 0, 0])
    for i, a in enumerate(u[:n_each]):
        raw = (a.tobytes() if v6 else int(a).to_bytes(4, "little") + bytes(12)) + fam
        info = L.endpoint_info(i + 1, i & 0xFFFF, L.ENDPOINT_F_HOST if i % 16 == 0 else 0)
        assert e.endpoint_update(np.frombuffer(raw, L.ENDPOINT_KEY)[0], 0, info) == 0
    seen = 0
    for a in u[n_each:]:
        raw = (a.tobytes()[:12] + bytes(4) if v6 else (int(a) & 0xFFFF).to_bytes(4, "little") + bytes(12)) + fam
        if e.tunnel_update(np.frombuffer(raw, L.ENDPOINT_KEY)[0], L.endpoint_key(f"10.250.{seen >> 8 & 255}.{seen & 255}"),
                           1) == 0:  # NOEXIST: distinct prefixes
            seen += 1
        if seen == n_each:
            break


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
    e = Engine(device=0, **{**T.engine_config(), "ipcache_tunnel": 1})
    synth.load_engine(e, T)
    load_maps(e, np.asarray(tup["daddr"]), v6)
    e.commit()
    tb = e.forward_table_bytes()
    d = synth.to_device(tup)
    d["ttl"] = torch.from_numpy(np.random.default_rng(9).choice(np.array([1, 2, 64, 64, 64, 255], np.uint8), n)).cuda()

    def outs():
        return {"verdict": torch.empty(n, dtype=torch.int32, device="cuda"),
                "identity": torch.empty(n, dtype=torch.int32, device="cuda"), "stage": None,
                "tunnel": torch.empty(n, dtype=torch.int32, device="cuda")}
    tun, both = outs(), outs()
    fo = {"action": torch.empty(n, dtype=torch.uint8, device="cuda")}
    for k in ("ret", "ifindex", "arg"):
        fo[k] = torch.empty(n, dtype=torch.int32, device="cuda")
    both.update({"fwd_" + k: torch.empty_like(v) for k, v in fo.items()})
    cls = e.classify_v6 if v6 else e.classify_v4
    fwd = e.forward_v6 if v6 else e.forward_v4
    cls(d, out=tun, stage=False, tunnel=True)
    runs = {"forward": lambda: fwd(d["daddr"], verdict=tun["verdict"], tunnel=tun["tunnel"], flags=d["flags"],
                                   ttl=d["ttl"], out=fo, **FWD),
            "classify_tun": lambda: cls(d, out=tun, stage=False, tunnel=True),
            "classify_fwd": lambda: cls(d, out=both, stage=False, forward=FWD)}
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
    for k in fo:
        assert torch.equal(fo[k], both["fwd_" + k]), k
    act = fo["action"].cpu().numpy()
    verdict = tun["verdict"].cpu().numpy()
    egress = (np.asarray(tup["flags"]) & 1) == 1
    look_ep = int((egress & (verdict == 0)).sum())  # packets whose decision reads the endpoint table
    look_tm = int((egress & (verdict == 0) & ~np.isin(act, (L.FWD_LOCAL, L.FWD_HOST)) &
                   (tun["tunnel"].cpu().numpy() == 0)).sum())  # ... and the tunnel map
    rd, wr, pts = ceilings()
    b_in = (16 if v6 else 4) + 4 + 4 + 1 + 1
    b_out = 1 + 4 + 4 + 4
    ep_b, tm_b = (tb["endpoints6"], tb["tunnel6"]) if v6 else (tb["endpoints4"], tb["tunnel4"])
    c_ep, c_tm = gather_ceiling(pts, ep_b), gather_ceiling(pts, tm_b)
    floor_stream = (b_in * n / (rd * 1e12) + b_out * n / (wr * 1e12)) * 1e3
    floor_gather = (look_ep / (c_ep * 1e9) + look_tm / (c_tm * 1e9)) * 1e3
    # the kernel gathers both home slots for every packet (no branch around a load)
    floor_gather_all = (n / (c_ep * 1e9) + n / (c_tm * 1e9)) * 1e3
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rec = {"tool": "forward_ab", "config": a.config, "tuples": n, "steps": a.steps, "warmup": a.warmup,
           **{f"{k}_ms_median": round(med[k], 4) for k in ms}, **{f"{k}_ms_min": round(min(ms[k]), 4) for k in ms},
           "forward_behind_classify_ms": round(med["classify_fwd"] - med["classify_tun"], 4),
           "actions": {str(i): int((act == i).sum()) for i in range(8)},
           "lookups_endpoint": look_ep, "lookups_tunnel_map": look_tm, "forward_table_bytes": tb,
           "bytes_in_per_packet": b_in, "bytes_out_per_packet": b_out,
           "gather_ceiling_endpoint_g_s": c_ep, "gather_ceiling_tunnel_map_g_s": c_tm,
           "floor_stream_ms": round(floor_stream, 4), "floor_gather_ms": round(floor_gather, 4),
           "floor_ms": round(floor_stream + floor_gather, 4),
           "floor_every_lane_gathers_ms": round(floor_stream + floor_gather_all, 4),
           "forward_over_floor": round(med["forward"] / (floor_stream + floor_gather), 2)}
    e.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
