#!/usr/bin/env python3
"""The chains of seeds (FMIndex.chains_device: colinear chaining of a read's hits) over the index and the three batches of reads that
tools/seed_bench.py measures: reads sampled from the text, the same with two bases substituted, and uniform random ACGT reads; both strands.

A chains request is a seeds request with hits followed by the chaining, so min_length and max_occurrences are part of what is measured
and stand in the output.  One JSON line, also written to profiles/r21_chains_<size>.json:

  positions, paths, reads, read_length, min_length, max_occurrences, max_gap, max_skew, gap_cost, tile_matches
  per batch: seeds_ms (the seeds step of the same request: anchor + refine + emit + hits), expand_ms, sort_ms, dp_ms, peel_ms, fill_ms (HIP
             events; the median of --repeats requests behind one that is not timed), dp_over_seeds (dp_ms / seeds_ms), matches, pairs,
             chains, chain_matches, skipped_items, pairs_per_s (over dp_ms), matches_per_read, scratch_bytes, scratch_bytes_per_match

The figure to read dp_ms against is seeds_ms of the same request.  The reference has no counterpart: no speed-up is stated."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

PHASES = ("seeds_ms", "expand_ms", "sort_ms", "dp_ms", "peel_ms", "fill_ms")


def run(size="small", device=0, repeats=3, reads=None, min_length=19, max_occurrences=64, max_gap=0, max_skew=0, gap_cost=1):
    import bench
    import gbwt_rs_amd as G
    import seed_bench as SB
    reads = reads or SB.READS
    with SB.workload(size, device, reads) as w:
        fm, offsets = w["fm"], w["offsets"]
        options = dict(min_length=min_length, strands=G.STRAND_BOTH, max_occurrences=max_occurrences, max_gap=max_gap, max_skew=max_skew, gap_cost=gap_cost)

        def measured(d_bytes):
            runs = []
            for k in range(repeats + 1):
                fm.chains_device(offsets.data_ptr(), d_bytes.data_ptr(), reads, reads * SB.LENGTH, **options)
                if k:
                    runs.append(fm.last_chain_info())
            last = runs[-1]
            ms = {k: statistics.median(r[k] for r in runs) for k in PHASES}
            return {**{k: round(v, 4) for k, v in ms.items()}, "dp_over_seeds": ms["dp_ms"] / ms["seeds_ms"] if ms["seeds_ms"] else None,
                    **{k: int(last[k]) for k in ("matches", "pairs", "chains", "chain_matches", "skipped_items")},
                    "pairs_per_s": last["pairs"] / (ms["dp_ms"] * 1e-3) if ms["dp_ms"] else None, "matches_per_read": last["matches"] / reads,
                    "scratch_bytes": int(last["peak_scratch_bytes"]), "scratch_bytes_per_match": last["peak_scratch_bytes"] / last["matches"] if last["matches"] else None,
                    "planned_is_peak": last["peak_scratch_bytes"] == last["planned_scratch_bytes"]}

        batches = {kind: measured(d_bytes) for kind, d_bytes in w["batches"].items()}
        info = fm.last_chain_info()
        return {
            "tool": "chain_bench", "size": size,
            "workload": f"Synth.genome[{size} shape, labels 1..1024 bp, seed 42]: the first {len(w['ids'])} of the {len(w['contig_ids'])} paths of contig 'chr1', {w['n']} positions; "
                        f"{reads} reads of {SB.LENGTH} bytes per batch, both strands",
            "paths": int(len(w["ids"])), "positions": w["n"], "reads": reads, "read_length": SB.LENGTH, "repeats": repeats,
            "min_length": min_length, "max_occurrences": max_occurrences, "max_gap": max_gap or 5000, "max_skew": max_skew or 500, "gap_cost": gap_cost,
            "tile_matches": int(info["tile_matches"]), "path_offset_bytes": int(info["path_offset_bytes"]),
            **batches,
            "dp_below_seeds_on_substituted": batches["substituted"]["dp_ms"] < batches["substituted"]["seeds_ms"],
            "source_fingerprint": bench.source_fingerprint(),
        }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="small", choices=["tiny", "small"])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0, help="reads per batch (default: seed_bench's 2^20)")
    ap.add_argument("--min-length", type=int, default=19)
    ap.add_argument("--max-occurrences", type=int, default=64)
    ap.add_argument("--out", default="", help="where the JSON line goes as well (default: profiles/r21_chains_<size>.json)")
    a = ap.parse_args()
    import gbwt_rs_amd as G
    try:
        res = run(a.size, a.device, a.repeats, a.reads, a.min_length, a.max_occurrences)
    except G.GbwtHipError as e:                     # (CAPACITY or UNSUPPORTED with the numbers: the library's message is the answer)
        print(f"chain_bench --size {a.size}: {e}", file=sys.stderr)
        return 2
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out or os.path.join(ROOT, "profiles", f"r21_chains_{a.size}.json"), "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
