#!/usr/bin/env python3
"""Suffix array and BWT of the text of one contig of a config-4-shaped GBZ on one GPU: the step between gbz-extract's `sequences` and
`tag-array` modes, chained on the device (bases -> suffix array -> tags of that suffix array).

The graph is the one tools/tags_bench.py uses -- Synth.genome with labels of realistic length at the shape of tools/c4_bench.py's SIZES[size]
-- and the text that of the leading paths of select_paths("chr1") whose bases and endmarkers make at most 2^32 - 2 positions, the builder's
limit (u32 ranks).  The cut is made on the host from the generator's own label lengths, before any suffix array is built.  At the small size (measured:
1.04 G positions) and below the whole contig fits.  At the full size it cannot: the shape has 334 G bases over 24 contigs, some 14 G per
contig, so `--size full` measures the first ~4.29 G positions of chr1 (210 GB of scratch and 39 GB of results: a device without that much
free memory answers GBWT_HIP_CAPACITY, which the tool prints) -- this rests on that arithmetic, no full run is recorded.  `tiny` and
`medium` are the sizes at which the host certificate is affordable (profiles/r18_suffix_array_tiny.json).  One JSON line, also written to
profiles/r18_suffix_array_<size>.json:

  positions, paths            the length of the text (bases and one endmarker per path) and the paths behind it; contig_paths,
                              contig_positions: the whole contig's, where the text is a part of it
  rounds, active, round_ms    doubling rounds, the active set behind the first keys and behind every round, device time of every sort with
                              its renumbering (HIP events)
  text_ms, pack_ms, rank_ms, output_ms, total_ms; positions_per_s = positions / (pack + rank + output)
  bytes_per_position          peak scratch of the ranking / positions (planned_bytes_per_position: what the plan promised)
  radix_floor_frac            per round: the time its radix passes need at 8 TB/s -- ceil(key bits / 8) passes that read and write a key of
                              8 and a suffix of 4 bytes per entry -- over the time the round took
  tags_ms, tag_runs           the tag kernel over the device suffix array as it lies there; bwt_runs
  check                       the linear certificate of tests/sa_expect.py over the text copied out (skipped above --check-max positions)

The reference has no builder and no CPU suffix sorter is at hand: no speed-up is stated."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


SA_MAX_TEXT = (1 << 32) - 2          # gbwt_hip.h: ranks and positions inside the builder are 32 bits wide


def run(size="small", device=0, check_max=200_000_000):
    import torch
    import c4_bench as C4
    import gbwt_rs_amd as G
    from gbwt_rs_amd import synth as S
    import bench
    import sa_expect as A
    p = dict(C4.SIZES[size])
    tmpdir = tempfile.mkdtemp(prefix="gbwt_sa_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        path = os.path.join(tmpdir, "c4.gbz")
        t0 = time.perf_counter()
        g = S.Synth.genome(contigs=p["contigs"], fragments=p["fragments"], haplotypes=p["haplotypes"], sites=p["sites"], seed=42, labels=1,
                           min_walkers=p["min_walkers"], wrap_contig=p["wrap_contig"], threads=min(16, os.cpu_count() or 1))
        g.save(path, as_gbz=True)
        gen_s = time.perf_counter() - t0
        gbz = G.GBZ.load(path, device=device, flags=G.OPEN_EXTRACT | G.OPEN_GFA)
        contig = "chr1"                                                      # (Synth.genome names its contigs chr1 .. chrN)
        contig_ids = gbz.select_paths(contig=contig)
        # the leading paths that fit the builder's width, from the generator's label lengths (path_text_stats: nodes, digits, bases)
        ends = np.cumsum(np.array([g.path_text_stats(int(q))[2] + 1 for q in contig_ids], dtype=np.uint64))
        ids = contig_ids[: int(np.searchsorted(ends, np.uint64(SA_MAX_TEXT), side="right"))]
        if len(ids) == 0:
            raise SystemExit(f"the first path of {contig} alone has {int(ends[0])} positions: more than {SA_MAX_TEXT}")
        gbz.path_sequences_device(ids[:1], endmarker=0)                      # (untimed) the node labels reach HBM with the first request for bases
        t0 = time.perf_counter()
        out = gbz.suffix_array_device(ids, endmarker=0)
        wall_ms = (time.perf_counter() - t0) * 1e3
        info = gbz.last_suffix_array_info()
        n = int(out.total)
        d_tags = torch.empty(max(n, 1), dtype=torch.int64, device=torch.device("cuda", device))
        tag_runs = gbz.tags_device(ids, out.d_sa, n, d_tags.data_ptr())
        tags_ms = gbz.last_tags_ms()[2]
        checked = None
        if n <= check_max:
            sa, bwt, runs = gbz.suffix_array(ids, endmarker=0, return_bwt=True)     # (the memo: a copy, not a second build)
            _, text = gbz.path_sequences(ids, endmarker=0)
            problem = A.check(text, sa)
            checked = problem is None and bool(np.array_equal(bwt, A.bwt(text, sa, 0))) and runs == A.runs(bwt) == out.bwt_runs
        bits = 2 * info["rank_bits"]
        floor = []
        for k, ms in enumerate(info["round_ms"]):
            entries = n if k == 0 else info["active"][k - 1]
            passes = -(-(64 if k == 0 else bits) // 8)
            floor.append((24 * entries * passes / 8e12 * 1e3) / ms if ms > 0 else 0.0)
        build_ms = info["pack_ms"] + info["rank_ms"] + info["output_ms"]
        return {
            "tool": "suffix_array_bench", "size": size,
            "workload": f"Synth.genome[{size} shape, labels 1..1024 bp, seed 42]: the first {len(ids)} of the {len(contig_ids)} paths of contig {contig!r}, {n} positions",
            "paths": int(len(ids)), "positions": n, "contig_paths": int(len(contig_ids)), "contig_positions": int(ends[-1]), "length_ok": n == int(ends[len(ids) - 1]),
            "generator_seconds": round(gen_s, 1), "rounds": info["rounds"], "rank_bits": info["rank_bits"],
            "active": info["active"], "round_ms": [round(x, 3) for x in info["round_ms"]], "radix_floor_frac": [round(x, 4) for x in floor],
            "text_ms": round(info["text_ms"], 3), "pack_ms": round(info["pack_ms"], 3), "rank_ms": round(info["rank_ms"], 3), "output_ms": round(info["output_ms"], 3),
            "build_ms": round(build_ms, 3), "wall_ms": round(wall_ms, 2), "positions_per_s": n / (build_ms * 1e-3) if build_ms > 0 else 0.0,
            "peak_scratch_bytes": info["peak_scratch_bytes"], "bytes_per_position": info["peak_scratch_bytes"] / max(n, 1),
            "planned_bytes_per_position": info["planned_scratch_bytes"] / max(n, 1), "bwt_runs": int(out.bwt_runs), "tags_ms": round(tags_ms, 3), "tag_runs": int(tag_runs),
            "check": checked, "source_fingerprint": bench.source_fingerprint(),
        }
    finally:
        shutil.rmtree(tmpdir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="small", choices=["tiny", "medium", "small", "full"])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--check-max", type=int, default=200_000_000, help="run the certificate on the host up to this many positions")
    ap.add_argument("--out", default="", help="where the JSON line goes as well (default: profiles/r18_suffix_array_<size>.json)")
    a = ap.parse_args()
    import gbwt_rs_amd as G
    try:
        res = run(a.size, a.device, a.check_max)
    except G.GbwtHipError as e:                     # (CAPACITY with the bytes needed, UNSUPPORTED: the library's message is the answer)
        print(f"suffix_array_bench --size {a.size}: {e}", file=sys.stderr)
        return 2
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out or os.path.join(ROOT, "profiles", f"r18_suffix_array_{a.size}.json"), "w") as f:
        f.write(line + "\n")
    return 0 if res["check"] is not False and res["length_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
