#!/usr/bin/env python3
"""The alignments of chains (FMIndex.alignments_device: banded edit distance and CIGARs of a read's best chains) over the index and the three
batches of reads that tools/seed_bench.py and tools/chain_bench.py measure: reads sampled from the text, the same with two bases
substituted, and uniform random ACGT reads; both strands.  The object keeps the text of its paths (PathFMIndex.keep_text).

An alignments request is a chains request followed by the alignment, so the seed and chain options of tools/chain_bench.py are part of what
is measured and stand in the output; max_alignments 1 (the best chain of every read and strand), band 16.  One JSON line, also written to
profiles/r22_align_<size>.json:

  positions, paths, reads, read_length, the options, tile_bytes, text_bytes
  per batch: seeds_ms and chaining_ms (the seeds step and the chaining of the same request), select_ms, dp_ms, trace_ms (0: the walk back runs
             inside the DP kernel), rows_ms (HIP events; the median of --repeats requests behind one that is not timed), dp_over_seeds,
             alignments, wide, unreachable, cells, cigar_ops, cells_per_s (over dp_ms), lds_alignments, global_alignments, scratch_bytes,
             scratch_bytes_per_alignment

The figures to read dp_ms against are seeds_ms and chaining_ms of the same request.  The reference has no counterpart: no speed-up is stated.
On a GPU machine every step runs under a time limit of its own:
  timeout -k 10 600 python tools/align_bench.py --size tiny && timeout -k 10 900 python tools/align_bench.py --size small"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

PHASES = ("select_ms", "dp_ms", "trace_ms", "rows_ms")
CHAINING = ("expand_ms", "sort_ms", "dp_ms", "peel_ms", "fill_ms")


def run(size="small", device=0, repeats=3, reads=None, min_length=19, max_occurrences=64, max_gap=0, max_skew=0, gap_cost=1, band=16, max_width=0, max_alignments=1):
    import bench
    import gbwt_rs_amd as G
    import seed_bench as SB
    reads = reads or SB.READS
    with SB.workload(size, device, reads) as w:
        fm, offsets = w["fm"], w["offsets"]
        fm.keep_text()
        options = dict(min_length=min_length, strands=G.STRAND_BOTH, max_occurrences=max_occurrences, max_gap=max_gap, max_skew=max_skew, gap_cost=gap_cost, band=band,
                       max_width=max_width, max_alignments=max_alignments)

        def measured(d_bytes):
            runs = []
            for k in range(repeats + 1):
                fm.alignments_device(offsets.data_ptr(), d_bytes.data_ptr(), reads, reads * SB.LENGTH, **options)
                if k:
                    chain = fm.last_chain_info()
                    runs.append({**fm.last_align_info(), "seeds_ms": chain["seeds_ms"], "chaining_ms": sum(chain[name] for name in CHAINING)})
            last = runs[-1]
            ms = {k: statistics.median(r[k] for r in runs) for k in PHASES + ("seeds_ms", "chaining_ms", "chains_ms")}
            computed = last["alignments"] - last["wide"]
            return {**{k: round(v, 4) for k, v in ms.items()}, "dp_over_seeds": ms["dp_ms"] / ms["seeds_ms"] if ms["seeds_ms"] else None,
                    **{k: int(last[k]) for k in ("alignments", "wide", "unreachable", "cells", "cigar_ops", "lds_alignments", "global_alignments")},
                    "cells_per_s": last["cells"] / (ms["dp_ms"] * 1e-3) if ms["dp_ms"] else None, "alignments_per_read": last["alignments"] / reads,
                    "scratch_bytes": int(last["peak_scratch_bytes"]), "scratch_bytes_per_alignment": last["peak_scratch_bytes"] / computed if computed else None,
                    "planned_is_peak": last["peak_scratch_bytes"] == last["planned_scratch_bytes"]}

        batches = {kind: measured(d_bytes) for kind, d_bytes in w["batches"].items()}
        info = fm.last_align_info()
        return {
            "tool": "align_bench", "size": size,
            "workload": f"Synth.genome[{size} shape, labels 1..1024 bp, seed 42]: the first {len(w['ids'])} of the {len(w['contig_ids'])} paths of contig 'chr1', {w['n']} positions; "
                        f"{reads} reads of {SB.LENGTH} bytes per batch, both strands",
            "paths": int(len(w["ids"])), "positions": w["n"], "reads": reads, "read_length": SB.LENGTH, "repeats": repeats,
            "min_length": min_length, "max_occurrences": max_occurrences, "max_gap": max_gap or 5000, "max_skew": max_skew or 500, "gap_cost": gap_cost,
            "band": band, "max_width": max_width or 256, "max_alignments": max_alignments,
            "tile_bytes": int(info["tile_bytes"]), "text_bytes": int(info["text_bytes"]),
            **batches,
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
    ap.add_argument("--band", type=int, default=16)
    ap.add_argument("--max-alignments", type=int, default=1)
    ap.add_argument("--out", default="", help="where the JSON line goes as well (default: profiles/r22_align_<size>.json)")
    a = ap.parse_args()
    import gbwt_rs_amd as G
    try:
        res = run(a.size, a.device, a.repeats, a.reads, a.min_length, a.max_occurrences, band=a.band, max_alignments=a.max_alignments)
    except G.GbwtHipError as e:                     # (CAPACITY or UNSUPPORTED with the numbers: the library's message is the answer)
        print(f"align_bench --size {a.size}: {e}", file=sys.stderr)
        return 2
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out or os.path.join(ROOT, "profiles", f"r22_align_{a.size}.json"), "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
