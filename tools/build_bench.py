#!/usr/bin/env python3
"""GBWT construction on the device (include/gbwt_hip.h, "construction") on one GPU: the index of the paths of a bubble chain.

The chain of --sites x --haplotypes (2 alleles, mosaic, seed 42; default 100 000 x 1 000 = 4.0e8 visits over both orientations) is made by
the host's sweep generator; its paths go to GBWT.from_paths behind a warm-up build of a small input, --passes times.  The bytes of every
build are compared with the generator's at that full size.  One JSON line, also written to profiles/r13_build_small.json:

  total_ms / expand_ms / rank_ms / edges_ms / encode_ms   HIP events around the four phases of the construction, median over the passes
  open_ms                       the open behind them (host clock);  wall_ms: host clock around the whole call (with the upload of the paths)
  rounds                        doubling rounds of the ranking
  visits_per_s                  visits / total_ms
  peak_scratch_bytes            the most HBM the construction held at once besides the rows; scratch_bytes_per_visit
  host_sweep_seconds            the host generator for the same index: a different algorithm on a restricted input, no speed-up is stated
  brute_force                   Synth.from_paths against the device on a chain of 2 000 x 200, where the brute force finishes: the same job"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def same_index(dev, s):
    data, starts = dev.records()
    return (bytes(data) == bytes(s.data()) and np.array_equal(starts, s.starts()) and
            (dev.sequences(), dev.len(), dev.alphabet_offset(), dev.alphabet_size()) == (s.sequences, s.size, s.alphabet_offset, s.alphabet_size))


def timed_builds(G, paths, passes, device):
    """(infos, wall ms, the last handle) of `passes` builds."""
    infos, wall, dev = [], [], None
    for _ in range(passes):
        if dev is not None:
            dev.close()
        t0 = time.perf_counter()
        dev = G.GBWT.from_paths(paths, bidirectional=True, device=device)
        wall.append((time.perf_counter() - t0) * 1e3)
        infos.append(dev.last_build_info())
    return infos, wall, dev


def note(what, t0):
    print(f"[build_bench] {what}: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)


def run(sites=100000, haplotypes=1000, passes=3, device=0):
    import bench
    import gbwt_rs_amd as G
    from gbwt_rs_amd import synth as S
    t0 = time.perf_counter()
    s = S.Synth.chain(sites, haplotypes, alleles=2, model=S.MOSAIC, founders=32, switch_rate=2e-3, seed=42)
    sweep_s = time.perf_counter() - t0
    note("host sweep generator", t0)
    paths = [s.path(h) for h in range(s.paths)]
    G.GBWT.from_paths([[2, 4, 6], [2, 6]], device=device).close()         # warm-up: the runtime, the kernels
    t0 = time.perf_counter()
    infos, wall, dev = timed_builds(G, paths, passes, device)
    note(f"{passes} builds", t0)
    parity = same_index(dev, s)
    note("builds and comparison", t0)
    dev.close()
    med = lambda key: float(np.median([i[key] for i in infos]))
    phases = {k: med(k) for k in ("expand_ms", "rank_ms", "edges_ms", "encode_ms")}
    total_ms = sum(phases.values())
    visits = int(infos[-1]["visits"])
    # the same job on the host, at a size the brute force finishes
    small = S.Synth.chain(2000, 200, alleles=2, model=S.MOSAIC, founders=32, switch_rate=2e-3, seed=42)
    small_paths = [small.path(h) for h in range(small.paths)]
    t0 = time.perf_counter()
    witness = S.Synth.from_paths(small_paths, bidirectional=True)
    brute_ms = (time.perf_counter() - t0) * 1e3
    s_infos, s_wall, s_dev = timed_builds(G, small_paths, passes, device)
    small_parity = same_index(s_dev, witness) and same_index(s_dev, small)
    s_dev.close()
    s_total = sum(float(np.median([i[k] for i in s_infos])) for k in phases)
    res = {
        "tool": "build_bench", "workload": f"bubble chain {sites} sites x {haplotypes} haplotypes (2 alleles, mosaic, seed 42), both orientations",
        "visits": visits, "sequences": int(infos[-1]["sequences"]), "records": int(infos[-1]["records"]), "data_bytes": int(infos[-1]["data_bytes"]),
        "total_ms": total_ms, **phases, "open_ms": med("open_ms"), "wall_ms": float(np.median(wall)), "rounds": int(infos[-1]["rounds"]),
        "visits_per_s": visits / (total_ms * 1e-3) if total_ms else 0.0,
        "peak_scratch_bytes": int(infos[-1]["peak_scratch_bytes"]), "scratch_bytes_per_visit": infos[-1]["peak_scratch_bytes"] / visits if visits else 0.0,
        "total_ms_all": [round(sum(i[k] for k in phases), 3) for i in infos], "passes": passes,
        "host_sweep_seconds": round(sweep_s, 2),
        "brute_force": {"workload": "bubble chain 2000 sites x 200 haplotypes", "visits": int(s_infos[-1]["visits"]), "host_from_paths_ms": round(brute_ms, 2),
                        "device_total_ms": s_total, "device_wall_ms": float(np.median(s_wall)), "host_over_device_wall": brute_ms / float(np.median(s_wall)),
                        "parity_ok": bool(small_parity)},
        "parity_ok": bool(parity), "source_fingerprint": bench.source_fingerprint(),
    }
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sites", type=int, default=100000)
    ap.add_argument("--haplotypes", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="", help="where the JSON line goes (default: profiles/r13_build_small.json)")
    a = ap.parse_args()
    res = run(a.sites, a.haplotypes, a.passes, a.device)
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out or os.path.join(ROOT, "profiles", "r13_build_small.json"), "w") as f:
        f.write(line + "\n")
    return 0 if res["parity_ok"] and res["brute_force"]["parity_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
