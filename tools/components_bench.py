#!/usr/bin/env python3
"""The weakly connected components of a config-4-shaped index (GBZ::weakly_connected_components, src/gbz.rs:570-598) on one GPU.

Synth.genome at the shape of tools/c4_bench.py's SIZES[size], opened for extraction only (the lean handle); the components are made by the
first call on a handle, so every pass opens the file again and asks once.  One JSON line:

  components / slots / nodes   what was found (components must be contigs x fragments)
  hook_ms / jump_ms / shape_ms HIP-event time of the build's phases and their launches (gbwt_hip_last_components_ms), of the best pass
  counted_bytes                what the passes must move: a hook pass reads the record bytes and the record starts once; a jump pass reads
                               and writes 4 bytes per slot (8 bytes per slot)
  hook_TBps / jump_TBps        those bytes over the time of their phase, and as fractions of 8 TB/s (HBM peak) and of 6.29 TB/s (measured copy rate)
  hook_bytes_per_record        counted bytes of ONE hook pass per record
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def run(size="small", passes=3, device=0):
    import c4_bench as C4
    import gbwt_rs_amd as G
    import bench
    p = C4.SIZES[size]
    tmpdir = tempfile.mkdtemp(prefix="gbwt_comp_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        path = os.path.join(tmpdir, "c4.gbz")
        g = C4.generate(size, path, threads=min(16, os.cpu_count() or 1))
        runs = []
        for _ in range(passes + 1):                                   # (the first pass also starts the HIP runtime: not reported)
            gbz = G.GBZ.load(path, device=device, flags=G.OPEN_EXTRACT)
            before = gbz.memory_usage()["index_device_bytes"]
            t0 = time.perf_counter()
            view = gbz.components_device()
            wall_ms = (time.perf_counter() - t0) * 1e3
            t = gbz.last_components_ms()
            t.update(wall_ms=wall_ms, components=int(view.components), slots=int(view.slots), nodes=int(view.nodes),
                     kept_bytes=int(gbz.memory_usage()["index_device_bytes"] - before), records=int(gbz.stats.records), data_bytes=int(gbz.stats.data_bytes),
                     distinct_path_components=int(len(np.unique(gbz.path_components(np.arange(g.paths))))))
            runs.append(t)
            gbz.close()
        best = min(runs[1:], key=lambda r: r["hook_ms"] + r["jump_ms"] + r["shape_ms"])
        starts_bytes = (4 if best["data_bytes"] < (1 << 32) else 8) * (best["records"] + 1)
        hook_pass = best["data_bytes"] + starts_bytes
        hook_bytes, jump_bytes = hook_pass * best["hook_launches"], 8 * best["slots"] * best["jump_launches"]
        hook_rate = hook_bytes / (best["hook_ms"] * 1e-3) if best["hook_ms"] > 0 else 0.0
        jump_rate = jump_bytes / (best["jump_ms"] * 1e-3) if best["jump_ms"] > 0 else 0.0
        parts = p["contigs"] * p["fragments"]
        return {
            "tool": "components_bench", "size": size, "workload": f"Synth.genome[{size} shape, seed 42]: {g.paths} paths over {best['slots']} node slots, {best['records']} records",
            "components": best["components"], "expected_components": parts, "distinct_path_components": best["distinct_path_components"], "slots": best["slots"],
            "nodes": best["nodes"], "records": best["records"], "data_bytes": best["data_bytes"], "kept_device_bytes": best["kept_bytes"], "passes": passes,
            "hook_ms": round(best["hook_ms"], 3), "jump_ms": round(best["jump_ms"], 3), "shape_ms": round(best["shape_ms"], 3),
            "device_ms": round(best["hook_ms"] + best["jump_ms"] + best["shape_ms"], 3), "wall_ms": [round(r["wall_ms"], 2) for r in runs[1:]],
            "hook_launches": best["hook_launches"], "jump_launches": best["jump_launches"], "shape_launches": best["shape_launches"],
            "hook_counted_bytes": hook_bytes, "jump_counted_bytes": jump_bytes, "hook_bytes_per_record": hook_pass / max(1, best["records"]),
            "hook_TBps": hook_rate / 1e12, "hook_frac_of_8TBps": hook_rate / 8e12, "hook_frac_of_6.29TBps": hook_rate / 6.29e12,
            "jump_TBps": jump_rate / 1e12, "jump_frac_of_8TBps": jump_rate / 8e12, "jump_frac_of_6.29TBps": jump_rate / 6.29e12,
            "ok": bool(best["components"] == parts == best["distinct_path_components"]), "generator_seconds": round(g.generator_seconds, 1),
            "source_fingerprint": bench.source_fingerprint(),
        }
    finally:
        shutil.rmtree(tmpdir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="small", choices=["tiny", "medium", "small", "full"])
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="", help="write the JSON line to this file (default: profiles/r08_components_<size>.json)")
    a = ap.parse_args()
    res = run(a.size, a.passes, a.device)
    line = json.dumps(res)
    print(line, flush=True)
    out = a.out or os.path.join(ROOT, "profiles", f"r08_components_{a.size}.json")
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
