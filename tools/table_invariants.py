"""cgpu_table_bytes and cgpu_table_checksum of one fixed synth configuration,
for the package under a given root: what a change that must not move the
device tables of existing contexts is compared on.

    python tools/table_invariants.py [--root DIR] [--label NAME] [--out FILE]   (GPU box)

DIR is a checkout with a built cilium_amd/libcgpu.so (default: this one).
The configuration uses only calls every version of the library has: config 1's
tables (synth.CONFIGS["cpu"]), 1000 IPv4 and 200 IPv6 endpoint keys, 500
services, the tunnel flag on and off.  Prints (and appends to FILE) one JSON
line per flag value.
"""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from cilium_amd import build, layouts as L, synth
    from cilium_amd.engine import Engine
    T = synth.make_tables(**synth.CONFIGS["cpu"])
    svcs = synth.make_services(T, 500)
    for flag in (0, 1):
        e = Engine(device=0, **{**T.engine_config(), "ipcache_tunnel": flag})
        synth.load_engine(e, T)
        synth.load_services(e, svcs)
        for i in range(1000):
            assert e.endpoint_update(L.endpoint_key(f"10.7.{i >> 8}.{i & 255}")) == 0
        for i in range(200):
            assert e.endpoint_update(L.endpoint_key(f"fd00::7:{i:x}")) == 0
        e.commit()
        e.verify()
        rec = {"tool": "table_invariants", "label": a.label, "lib": build.lib_identity().get("lib_sha256"),
               "ipcache_tunnel": flag, "table_bytes": e.table_bytes(), "table_checksum": e.checksum()}
        e.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
