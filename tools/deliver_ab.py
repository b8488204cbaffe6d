"""Cost of the local delivery step (cgpu_deliver_v4 / _v6) alone and behind
classify + forward.

    python tools/deliver_ab.py [--config 2|v6] [--local-share S] [--steps K] [--warmup W] [--tuples N]
                               [--out FILE]                                                  (GPU box)

One context with cgpu_config.ipcache_tunnel and bench.py's workload of that
config (config 2: 64M IPv4 tuples; v6: the IPv6 tables), endpoints and tunnel
prefixes taken from the batch's own destinations as tools/forward_ab.py does,
every endpoint's lxc_id one of the workload's policy maps.  Timed with device
events, medians after W warm-ups, the kinds alternating call by call:

  classify_fwd      classify_v4 / _v6(forward=...): what a caller ran before
  classify_fwd_dlv  the same with deliver=True (src_ep = the tuples' ep)
  deliver           the delivery call alone (its kernel's time: one launch),
                    on an action column in which a packet is LOCAL with
                    probability S (else STACK, arg 0xFFFFFFFF), arg a random
                    policy map, src_label a random identity of the ingress keys

Prints one JSON line: the times, the LOCAL share of the chained call's own
batch and of the stand-alone column, and the floor the stand-alone call is to
be read against: its streamed bytes in and out at the
measured stream rates (profiles/ceilings.json) plus its LOCAL packets' gathers
(the group slot of every packet that reaches the cascade, a key-table slot for
every probe 1 and probe 3 it must have made) at the gather ceiling of the tier
the policy tables' bytes fall in.
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
from tools.forward_ab import FWD, ceilings, gather_ceiling  # noqa: E402


def load_maps(e, daddr, v6, n_eps, n_each=4096):
    """forward_ab.load_maps with lxc_id = a policy map of the workload"""
    u = np.unique(daddr[:1 << 20], axis=0)
    u = u[np.random.default_rng(3).permutation(len(u))]
    fam = bytes([2 if v6 else 1, 0, 0, 0])
    for i, a in enumerate(u[:n_each]):
        raw = (a.tobytes() if v6 else int(a).to_bytes(4, "little") + bytes(12)) + fam
        info = L.endpoint_info(i + 1, i % n_eps, L.ENDPOINT_F_HOST if i % 16 == 0 else 0)
        assert e.endpoint_update(np.frombuffer(raw, L.ENDPOINT_KEY)[0], 0, info) == 0
    seen = 0
    for a in u[n_each:]:
        raw = (a.tobytes()[:12] + bytes(4) if v6 else (int(a) & 0xFFFF).to_bytes(4, "little") + bytes(12)) + fam
        if e.tunnel_update(np.frombuffer(raw, L.ENDPOINT_KEY)[0], L.endpoint_key(f"10.250.{seen >> 8 & 255}.{seen & 255}"),
                           1) == 0:
            seen += 1
        if seen == n_each:
            break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="2", choices=["2", "v6"])
    ap.add_argument("--local-share", type=float, default=0.03)
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
    e = Engine(device=0, **{**T.engine_config(), "ipcache_tunnel": 1})
    synth.load_engine(e, T)
    ing = T.pol_keys[(T.pol_keys["egress"] & 1) == 0]
    ids = np.unique(ing["sec_label"][ing["sec_label"] != 0])
    synth.load_lxc(e, ids[:T.n_endpoints])  # the senders' SECLABELs: identities the ingress keys name
    load_maps(e, np.asarray(tup["daddr"]), v6, T.n_endpoints)
    e.commit()
    tb = e.table_bytes()
    d = synth.to_device(tup)
    rng = np.random.default_rng(11)
    local = rng.random(n) < a.local_share
    col = {"action": np.where(local, L.FWD_LOCAL, L.FWD_STACK).astype(np.uint8),
           "arg": np.where(local, rng.integers(0, T.n_endpoints, n), 0xFFFFFFFF).astype(np.uint32).view(np.int32),
           "src_label": ids[rng.integers(0, len(ids), n)].astype(np.uint32).view(np.int32)}
    col = {k: torch.from_numpy(v).cuda() for k, v in col.items()}

    def outs(dlv):
        o = {"verdict": torch.empty(n, dtype=torch.int32, device="cuda"),
             "identity": torch.empty(n, dtype=torch.int32, device="cuda"), "stage": None,
             "tunnel": torch.empty(n, dtype=torch.int32, device="cuda"),
             "fwd_action": torch.empty(n, dtype=torch.uint8, device="cuda")}
        for k in ("fwd_ret", "fwd_ifindex", "fwd_arg") + (("dlv_verdict", "dlv_identity") if dlv else ()):
            o[k] = torch.empty(n, dtype=torch.int32, device="cuda")
        if dlv:
            o["dlv_stage"] = torch.empty(n, dtype=torch.uint8, device="cuda")
        return o
    two, three = outs(False), outs(True)
    do = {"verdict": torch.empty(n, dtype=torch.int32, device="cuda"),
          "identity": torch.empty(n, dtype=torch.int32, device="cuda"),
          "stage": torch.empty(n, dtype=torch.uint8, device="cuda")}
    cls = e.classify_v6 if v6 else e.classify_v4
    dlv = e.deliver_v6 if v6 else e.deliver_v4
    runs = {"classify_fwd": lambda: cls(d, out=two, stage=False, forward=FWD),
            "classify_fwd_dlv": lambda: cls(d, out=three, stage=False, forward=FWD, deliver=True),
            "deliver": lambda: dlv(col["action"], col["arg"], d["dport"], d["proto"], d["flags"], d["len"],
                                   src_label=col["src_label"], out=do)}
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
    for k in ("verdict", "identity", "fwd_action", "fwd_arg"):
        assert torch.equal(two[k], three[k]), k
    chain_local = int((three["fwd_action"] == L.FWD_LOCAL).sum())
    assert int((three["dlv_stage"] != L.STAGE_NOT_LOCAL).sum()) == chain_local
    st = do["stage"].cpu().numpy()
    frag = (np.asarray(tup["flags"]) & 2) != 0 if not v6 else np.zeros(n, bool)
    reach = local & (st != 4)
    g_group = int(reach.sum())
    g_key = int((reach & ((st == 1) | (st == 3) | ((st == 0) & ~frag))).sum())
    rd, wr, pts = ceilings()
    b_in = 1 + 4 + 4 + 2 + 1 + 1 + 4
    b_out = 4 + 4 + 1
    c_pol = gather_ceiling(pts, tb["policy"])
    floor_stream = (b_in * n / (rd * 1e12) + b_out * n / (wr * 1e12)) * 1e3
    floor_gather = (g_group + g_key) / (c_pol * 1e9) * 1e3
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rec = {"tool": "deliver_ab", "config": a.config, "tuples": n, "steps": a.steps, "warmup": a.warmup,
           "local_share": a.local_share, "local_packets": int(local.sum()),
           "chain_local_packets": chain_local, "chain_local_share": round(chain_local / n, 5),
           **{f"{k}_ms_median": round(med[k], 4) for k in ms}, **{f"{k}_ms_min": round(min(ms[k]), 4) for k in ms},
           "deliver_behind_classify_fwd_ms": round(med["classify_fwd_dlv"] - med["classify_fwd"], 4),
           "stages": {str(i): int((st == i).sum()) for i in (0, 1, 2, 3, 4, 9)},
           "bytes_in_per_packet": b_in, "bytes_out_per_packet": b_out, "policy_table_bytes": tb["policy"],
           "gathers_group": g_group, "gathers_key": g_key, "gather_ceiling_g_s": c_pol,
           "floor_stream_ms": round(floor_stream, 4), "floor_gather_ms": round(floor_gather, 4),
           "floor_ms": round(floor_stream + floor_gather, 4),
           "deliver_over_floor": round(med["deliver"] / (floor_stream + floor_gather), 2)}
    e.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
