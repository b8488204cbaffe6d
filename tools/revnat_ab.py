"""Cost of the reverse-NAT output of the conntrack paths
(cgpu_classify_v4_ct_rnat / cgpu_classify_v4_ctlb_rnat, Engine rev_nat=True).

    python tools/revnat_ab.py [--config ct|ctlb] [--steps K] [--warmup W] [--tuples N] [--out FILE]   (GPU box)

bench.py's workload of that config on one context (ct: config 2 tables, 64M
packets of 2M connections; ctlb: the same behind 1M services).  The reverse-NAT
map holds what the agent writes for the services: every service's
rev_nat_index -> {VIP, port} (on ct, which has no services, every index
1..65535 -> an address, so the table is as large as it gets; its stream's
entries carry index 0, so nothing is rewritten).  The same batch is classified
with and without the output, alternating call by call, the conntrack map
emptied before every call (as bench.py's steps), each call timed with device
events after W warm-up calls of each kind.  Prints one JSON line: median / min
ms of each, the ratio, how many packets were rewritten, and the floor the
overhead is to be read against: the bytes per packet the
output adds (side array zeroed and read back, three inputs re-read, four
output columns) at the measured streamed rates (profiles/ceilings.json).
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

PKTS_PER_CONN = 32  # bench.py CT_PKTS_PER_CONN

# bytes per packet the output adds, IPv4: the side array (4 zeroed + 4 read),
# the rewrite pass's inputs (flags 1, proto 1, ct_ret 1, sport 2, saddr 4,
# daddr 4; ctlb: + svc_out 16) and its outputs (saddr 4, daddr 4, sport 2,
# applied 1); the walkers' stores and the table gathers come on top per
# rewritten packet (4 B store, 8 B gather)
BYTES_WRITTEN = 4 + 4 + 4 + 2 + 1
BYTES_READ = {"ct": 4 + 1 + 1 + 1 + 2 + 4 + 4, "ctlb": 4 + 1 + 1 + 1 + 2 + 4 + 4 + 16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ct", choices=["ct", "ctlb"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tuples", type=int, default=synth.CONFIGS["gpu"]["n_tuples"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctlb = a.config == "ctlb"
    n = a.tuples
    T = synth.make_tables(**synth.CONFIGS["gpu"])
    S = None
    if ctlb:
        S = synth.make_services(T, synth.CONFIGS["cascade"]["n_services"])
        tup, _, seclabels, S = synth.make_ctlb_workload(T, S, n // PKTS_PER_CONN, mean_pkts=PKTS_PER_CONN,
                                                        loop_frac=1e-4)
    else:
        tup, _, seclabels = synth.make_ct_workload(T, n // PKTS_PER_CONN, mean_pkts=PKTS_PER_CONN)
    n = min(n, len(tup["saddr"]))
    tup = {k: np.ascontiguousarray(v[:n]) for k, v in tup.items()}
    ct_max = 1 << max(20, int(np.ceil(np.log2((4.5 if ctlb else 2.5) * n / PKTS_PER_CONN))))
    ecfg = T.engine_config()
    if S is not None:
        ecfg["lb_max_entries"] = len(S.keys)
    e = Engine(device=0, **ecfg, ct_max=ct_max)
    synth.load_engine(e, T)
    synth.load_lxc(e, seclabels)
    if S is not None:
        synth.load_services(e, S)
        ns = len(S.vip)
        # one entry per index: the first service that carries it (65,535 indices
        # over 1M services: the synthetic services share them)
        raw, first = np.unique(S.vals["rev_nat_index"][ns:], return_index=True)
        for r, j in zip(raw, first):
            v = np.zeros((), L.LB4_REVERSE_NAT)
            v["address"], v["port"] = S.keys["address"][ns + j], S.keys["dport"][ns + j]
            assert e.revnat4_update(int(r), v) == 0
    else:
        for ix in range(1, 65536):
            v = np.zeros((), L.LB4_REVERSE_NAT)
            v["address"], v["port"] = 0x0A600000 + ix, ix
            assert e.revnat4_update(ix, v) == 0
    e.commit()
    d = synth.to_device(tup)

    def outs(rn):
        o = {"verdict": torch.empty(n, dtype=torch.int32, device="cuda"),
             "ct_ret": torch.empty(n, dtype=torch.uint8, device="cuda"),
             "identity": torch.empty(n, dtype=torch.int32, device="cuda"), "stage": None}
        if ctlb:
            o["daddr"] = torch.empty(n, dtype=torch.int32, device="cuda")
            o["dport"] = torch.empty(n, dtype=torch.int16, device="cuda")
        if rn:
            o["rn_saddr"] = torch.empty(n, dtype=torch.int32, device="cuda")
            o["rn_daddr"] = torch.empty(n, dtype=torch.int32, device="cuda")
            o["rn_sport"] = torch.empty(n, dtype=torch.int16, device="cuda")
            o["rn_applied"] = torch.empty(n, dtype=torch.uint8, device="cuda")
        return o
    plain, rn = outs(False), outs(True)
    cls = e.classify_v4_ctlb if ctlb else e.classify_v4_ct
    runs = {"plain": lambda: cls(d, 1000, out=plain), "rev_nat": lambda: cls(d, 1000, out=rn, rev_nat=True)}
    ms = {k: [] for k in runs}
    for it in range(a.warmup + a.steps):
        for k, f in runs.items():
            e.ct4_flush()  # every call starts from an empty conntrack map
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            f()
            ev1.record()
            ev1.synchronize()
            if it >= a.warmup:
                ms[k].append(ev0.elapsed_time(ev1))
    for f in ("verdict", "ct_ret", "identity"):
        assert torch.equal(plain[f], rn[f]), f
    c = json.load(open(os.path.join(ROOT, "profiles", "ceilings.json")))["stream"]
    floor = n * (BYTES_WRITTEN / (c["write_gbs"] * 1e9) + BYTES_READ[a.config] / (c["read_gbs"] * 1e9)) * 1e3 \
        if "read_gbs" in c else n * (BYTES_WRITTEN + BYTES_READ[a.config]) / (c["write_gbs"] * 1e9) * 1e3
    mp, mr = float(np.median(ms["plain"])), float(np.median(ms["rev_nat"]))
    rec = {"tool": "revnat_ab", "config": a.config, "packets": n, "steps": a.steps, "warmup": a.warmup,
           "plain_ms_median": round(mp, 4), "plain_ms_min": round(min(ms["plain"]), 4),
           "rev_nat_ms_median": round(mr, 4), "rev_nat_ms_min": round(min(ms["rev_nat"]), 4),
           "ratio_median": round(mr / mp, 4), "overhead_ms_median": round(mr - mp, 4),
           "rewritten": int(rn["rn_applied"].sum().item()), "revnat_entries": e.revnat4_count(),
           "added_bytes_per_packet": BYTES_WRITTEN + BYTES_READ[a.config], "floor_ms": round(floor, 4)}
    e.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
