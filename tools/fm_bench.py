#!/usr/bin/env python3
"""The FM-index over the text of one contig of a config-4-shaped GBZ on one GPU: build, batched count and locate.

The text is the one tools/suffix_array_bench.py measures at the same size -- the paths of select_paths("chr1") of Synth.genome at the shape
of tools/c4_bench.py's SIZES[size], labels of realistic length, an endmarker 0 behind every path -- and the index is GBZ.fm_index over it:
text, suffix array and index never leave the device.  Two batches of 2^20 patterns of 32 bytes, made on the device with torch: k-mers
sampled from the text (all of them occur: every one is searched to its first byte) and uniform random ACGT 32-mers (most of them die
within some 16 steps).  One JSON line, also written to profiles/r19_fm_<size>.json:

  positions, paths, sigma, packed, block_rows, blocks
  build: suffix_array_ms (the suffix array family's request: pack + ranking + output), histogram_ms, codes_ms, counts_ms, fill_ms, narrow_ms
  index_bytes, index_bytes_per_position (the suffix array's 4 included), sa_bytes
  per batch: count_ms (the search kernel, HIP events; the median of --repeats launches behind one that is not timed, and the fastest),
             patterns_per_s, steps, steps_per_s, bytes_per_step (the lines a step reads x 128 B: two ranks, one line each, in the packed
             layout), counted_bytes_per_s = steps_per_s x bytes_per_step, hits (patterns that occur)
  locate over the sampled batch: located (positions), locate_ms (search + scan + fill), located_per_s

The reference has no FM-index: no speed-up is stated."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

PATTERNS = 1 << 20
LENGTH = 32
SA_MAX_TEXT = (1 << 32) - 2


def run(size="small", device=0, repeats=5, patterns=PATTERNS):
    import torch
    import c4_bench as C4
    import gbwt_rs_amd as G
    from gbwt_rs_amd import dist as D
    from gbwt_rs_amd import synth as S
    import bench
    p = dict(C4.SIZES[size])
    dev = torch.device("cuda", device)
    tmpdir = tempfile.mkdtemp(prefix="gbwt_fm_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        path = os.path.join(tmpdir, "c4.gbz")
        t0 = time.perf_counter()
        g = S.Synth.genome(contigs=p["contigs"], fragments=p["fragments"], haplotypes=p["haplotypes"], sites=p["sites"], seed=42, labels=1,
                           min_walkers=p["min_walkers"], wrap_contig=p["wrap_contig"], threads=min(16, os.cpu_count() or 1))
        g.save(path, as_gbz=True)
        gen_s = time.perf_counter() - t0
        gbz = G.GBZ.load(path, device=device, flags=G.OPEN_EXTRACT | G.OPEN_GFA)
        contig_ids = gbz.select_paths(contig="chr1")
        ends = np.cumsum(np.array([g.path_text_stats(int(q))[2] + 1 for q in contig_ids], dtype=np.uint64))
        ids = contig_ids[: int(np.searchsorted(ends, np.uint64(SA_MAX_TEXT), side="right"))]
        gbz.path_sequences_device(ids[:1], endmarker=0)                      # (untimed) the node labels reach HBM with the first request for bases
        t0 = time.perf_counter()
        fm = gbz.fm_index(ids, endmarker=0)
        build_wall_ms = (time.perf_counter() - t0) * 1e3
        info = fm.info()
        sa_info = gbz.last_suffix_array_info()
        n = int(info["n"])
        # the patterns, on the device
        text = gbz.path_sequences_device(ids, endmarker=0)
        d_text = D.device_view(text.d_text, n, torch.uint8, dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(19)
        at = torch.randint(0, n - LENGTH + 1, (patterns,), device=dev, generator=gen)
        sampled = d_text[(at[:, None] + torch.arange(LENGTH, device=dev)[None, :]).reshape(-1)].contiguous()
        letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
        random = letters[torch.randint(0, 4, (patterns * LENGTH,), device=dev, generator=gen)].contiguous()
        offsets = (torch.arange(patterns + 1, device=dev, dtype=torch.int64) * LENGTH).contiguous()
        torch.cuda.synchronize(dev)

        def counted(d_bytes):
            times = []
            for k in range(repeats + 1):
                out = fm.count_device(offsets.data_ptr(), d_bytes.data_ptr(), patterns, patterns * LENGTH)
                if k:
                    times.append(fm.info()["last_count_ms"])
            last = fm.info()
            ranges = D.device_view(out.d_ranges, 2 * patterns * 8, torch.uint8, dev).cpu().numpy().view(np.uint64).reshape(patterns, 2)
            ms, steps = statistics.median(times), int(last["last_steps"])
            lines_per_step = 2                                                # two ranks; one line each in the packed layout, the count's line and the symbols' in the plain one
            bytes_per_step = lines_per_step * 128 if info["packed"] else None
            return {"count_ms": round(ms, 4), "count_ms_min": round(min(times), 4), "patterns_per_s": patterns / (ms * 1e-3), "steps": steps, "steps_per_pattern": steps / patterns,
                    "steps_per_s": steps / (ms * 1e-3), "bytes_per_step": bytes_per_step, "counted_bytes_per_s": (steps / (ms * 1e-3)) * bytes_per_step if bytes_per_step else None,
                    "hits": int(np.count_nonzero(ranges[:, 1] > ranges[:, 0])), "occurrences": int((ranges[:, 1] - ranges[:, 0]).sum())}

        res_sampled, res_random = counted(sampled), counted(random)
        locate_times = []
        for k in range(repeats + 1):
            rows = fm.locate_device(offsets.data_ptr(), sampled.data_ptr(), patterns, patterns * LENGTH)
            if k:
                last = fm.info()
                locate_times.append(last["last_count_ms"] + last["last_fill_ms"])
        locate_ms = statistics.median(locate_times)
        result = {
            "tool": "fm_bench", "size": size,
            "workload": f"Synth.genome[{size} shape, labels 1..1024 bp, seed 42]: the first {len(ids)} of the {len(contig_ids)} paths of contig 'chr1', {n} positions; "
                        f"{patterns} patterns of {LENGTH} bytes per batch",
            "paths": int(len(ids)), "positions": n, "generator_seconds": round(gen_s, 1), "sigma": int(info["sigma"]), "packed": int(info["packed"]), "block_rows": int(info["block_rows"]),
            "blocks": int(info["blocks"]), "repeats": repeats,
            "build": {"suffix_array_ms": round(sa_info["pack_ms"] + sa_info["rank_ms"] + sa_info["output_ms"], 3), "text_ms": round(sa_info["text_ms"], 3),
                      **{k: round(info[k], 4) for k in ("histogram_ms", "codes_ms", "counts_ms", "fill_ms", "narrow_ms")}, "wall_ms": round(build_wall_ms, 2)},
            "index_bytes": int(info["index_bytes"]), "sa_bytes": int(info["sa_bytes"]), "index_bytes_per_position": info["index_bytes"] / max(n, 1),
            "build_scratch_bytes": int(info["peak_scratch_bytes"]),
            "sampled": res_sampled, "random": res_random,
            "locate": {"located": int(rows.total), "locate_ms": round(locate_ms, 4), "located_per_s": rows.total / (locate_ms * 1e-3) if locate_ms > 0 else 0.0},
            "all_sampled_occur": res_sampled["hits"] == patterns,
            "source_fingerprint": bench.source_fingerprint(),
        }
        fm.close()
        return result
    finally:
        shutil.rmtree(tmpdir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="small", choices=["tiny", "small"])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="", help="where the JSON line goes as well (default: profiles/r19_fm_<size>.json)")
    a = ap.parse_args()
    import gbwt_rs_amd as G
    try:
        res = run(a.size, a.device, a.repeats)
    except G.GbwtHipError as e:                     # (CAPACITY with the bytes needed: the library's message is the answer)
        print(f"fm_bench --size {a.size}: {e}", file=sys.stderr)
        return 2
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out or os.path.join(ROOT, "profiles", f"r19_fm_{a.size}.json"), "w") as f:
        f.write(line + "\n")
    return 0 if res["all_sampled_occur"] else 1


if __name__ == "__main__":
    sys.exit(main())
