"""Cost of the forwarding step on raw frames (cgpu_forward_frames): the decision
alone, the decision with the rewrite, and the route there was before it.

    python tools/forward_frames_ab.py [--steps K] [--warmup W] [--tuples N] [--step-timeout S] [--out FILE]   (GPU box)

One context, bench.py's config-2 workload (64M IPv4 tuples) as frames in
64-byte slots (synth.frames_from_tuples), tools/forward_ab.py's 4096 endpoints
(with MACs) and 4096 tunnel prefixes taken from the batch's own destinations.
The verdict and stage columns are classify_frames' own, computed once.  Timed
with device events, medians after W warm-ups, the kinds alternating call by
call, every call under a time limit of its own (the process is killed when
one takes longer than S seconds):

  decide    forward_frames(rewrite=False)
  rewrite   forward_frames(rewrite=True), on the same slots every time (the
            ttl of a forwarded frame goes down by one per call; it starts at 64)
  columns   frames_parse, the daddr and ttl columns cut out of its output and
            of the slots with tensor copies, then forward_v4 on them

Prints one JSON line with the times and the floor the call is to be read
against: 64 B in per frame and the four input columns at the
measured streamed read rate, the four output columns and 32 B per rewritten
frame at the streamed write rate (profiles/ceilings.json), one gather per
frame of the endpoint table and of the tunnel map (every lane gathers both
home slots) and one of the MAC array per LOCAL frame of a rewriting call, each
at the gather ceiling of the cache tier that table's size falls in.
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
from tools.forward_ab import ceilings, gather_ceiling  # noqa: E402

FWD = dict(mode=L.FWD_LXC, encap=True, ipv4_mask=0xFFFF, host_ifindex=1, encap_ifindex=2)
HOST_MAC = bytes.fromhex("021122334455")


def load_maps(e, daddr, n_each=4096):
    """forward_ab.load_maps for IPv4, every endpoint with a MAC pair"""
    u = np.unique(daddr[:1 << 20])
    u = u[np.random.default_rng(3).permutation(len(u))]
    fam = bytes([1, 0, 0, 0])
    for i, a in enumerate(u[:n_each]):
        raw = int(a).to_bytes(4, "little") + bytes(12) + fam
        info = L.endpoint_info(i + 1, i & 0xFFFF, L.ENDPOINT_F_HOST if i % 16 == 0 else 0,
                               0x020000000000 | i, 0x060000000000 | i)
        assert e.endpoint_update(np.frombuffer(raw, L.ENDPOINT_KEY)[0], 0, info) == 0
    seen = 0
    for a in u[n_each:]:
        raw = (int(a) & 0xFFFF).to_bytes(4, "little") + bytes(12) + fam
        if e.tunnel_update(np.frombuffer(raw, L.ENDPOINT_KEY)[0],
                           L.endpoint_key(f"10.250.{seen >> 8 & 255}.{seen & 255}"), 1) == 0:
            seen += 1
        if seen == n_each:
            break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tuples", type=int, default=synth.CONFIGS["gpu"]["n_tuples"])
    ap.add_argument("--step-timeout", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.tuples
    T = synth.make_tables(**synth.CONFIGS["gpu"])
    tup = synth.make_tuples(T, n)
    e = Engine(device=0, **T.engine_config())
    synth.load_engine(e, T)
    load_maps(e, np.asarray(tup["daddr"]))
    e.commit()
    tb = e.forward_table_bytes()
    f = synth.frames_to_device(synth.frames_from_tuples(tup, stride=64))
    cls = e.classify_frames(f)
    verdict, stage = cls["verdict"], cls["stage"]

    def fwd_out():
        o = {"action": torch.empty(n, dtype=torch.uint8, device="cuda")}
        for k in ("ret", "ifindex", "arg"):
            o[k] = torch.empty(n, dtype=torch.int32, device="cuda")
        return o
    o_dec, o_rw, o_col = fwd_out(), fwd_out(), fwd_out()
    parsed = e.frames_parse(f)
    daddr4 = torch.empty(n, dtype=torch.int32, device="cuda")
    ttl = torch.empty(n, dtype=torch.uint8, device="cuda")

    def columns():
        e.frames_parse(f, out=parsed)
        daddr4.view(torch.uint8).view(n, 4).copy_(parsed["daddr"][:, :4])
        ttl.copy_(f["data"][:, 22])
        e.forward_v4(daddr4, verdict=verdict, flags=f["flags"], ttl=ttl, out=o_col, **FWD)
    runs = {"decide": lambda: e.forward_frames(f, verdict=verdict, stage=stage, rewrite=False, out=o_dec,
                                               host_mac=HOST_MAC, **FWD),
            "rewrite": lambda: e.forward_frames(f, verdict=verdict, stage=stage, rewrite=True, out=o_rw,
                                                host_mac=HOST_MAC, **FWD),
            "columns": columns}

    def timed(fn):
        """one call between two device events, killed past the time limit"""
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        signal.alarm(a.step_timeout)
        ev0.record()
        fn()
        ev1.record()
        ev1.synchronize()
        signal.alarm(0)
        return ev0.elapsed_time(ev1)
    for _ in range(a.warmup):
        for fn in runs.values():
            timed(fn)
    ms = {k: [] for k in runs}
    for _ in range(a.steps):
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    for k in o_dec:  # the three routes decide alike (every frame here is an IPv4 frame that reaches policy or drops)
        assert torch.equal(o_dec[k], o_rw[k]) and torch.equal(o_dec[k], o_col[k]), k
    act = o_dec["action"].cpu().numpy()
    n_rw = int(np.isin(act, (L.FWD_PROXY, L.FWD_LOCAL, L.FWD_HOST, L.FWD_STACK)).sum())
    n_local = int((act == L.FWD_LOCAL).sum())
    rd, wr, pts = ceilings()
    b_in, b_out = 64 + 4 + 1 + 4 + 1, 1 + 4 + 4 + 4
    c_ep, c_tm = gather_ceiling(pts, tb["endpoints4"]), gather_ceiling(pts, tb["tunnel4"])
    # the IPv4 MAC array has 16 B per slot, as the table itself; the batch holds no IPv6 frame, so the IPv6
    # array (16 B per 32-B row, counted in mac_array_bytes) is never gathered from here
    c_mac = gather_ceiling(pts, tb["endpoints4"])
    stream = (b_in * n / (rd * 1e12) + b_out * n / (wr * 1e12)) * 1e3
    gather = (n / (c_ep * 1e9) + n / (c_tm * 1e9)) * 1e3
    rw_extra = (32 * n_rw / (wr * 1e12) + n_local / (c_mac * 1e9)) * 1e3
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rec = {"tool": "forward_frames_ab", "frames": n, "stride": 64, "steps": a.steps, "warmup": a.warmup,
           **{f"{k}_ms_median": round(med[k], 4) for k in ms}, **{f"{k}_ms_min": round(min(ms[k]), 4) for k in ms},
           **{f"{k}_ms_max": round(max(ms[k]), 4) for k in ms},
           "actions": {str(i): int((act == i).sum()) for i in range(8)}, "frames_rewritten": n_rw,
           "forward_table_bytes": tb, "mac_array_bytes": tb["endpoints4"] + tb["endpoints6"] // 2,
           "bytes_in_per_frame": b_in, "bytes_out_per_frame": b_out,
           "gather_ceiling_endpoint_g_s": c_ep, "gather_ceiling_tunnel_map_g_s": c_tm,
           "floor_slots_only_ms": round((64 * n / (rd * 1e12)) * 1e3 + gather, 4),
           "floor_decide_ms": round(stream + gather, 4), "floor_rewrite_ms": round(stream + gather + rw_extra, 4),
           "decide_over_floor": round(med["decide"] / (stream + gather), 2),
           "rewrite_over_floor": round(med["rewrite"] / (stream + gather + rw_extra), 2),
           "columns_over_rewrite": round(med["columns"] / med["rewrite"], 2)}
    e.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
