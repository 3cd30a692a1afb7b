#!/usr/bin/env python3
"""The seeds of reads (FMIndex.seeds_device: maximal exact matches on both strands) over the FM-index that tools/fm_bench.py measures.

The text is fm_bench's at the same size -- the paths of select_paths("chr1") of Synth.genome at the shape of tools/c4_bench.py's SIZES[size],
an endmarker 0 behind every path -- and the index is GBZ.fm_index over it.  Three batches of 2^20 reads of 150 bytes, made on the device
with torch: reads sampled from the text (on their own strand every anchor reads back to the start of the read and nothing is refined), the same with
two bases substituted (the starts move around both, the intervals there are refined), and uniform random ACGT reads (no match is longer
than some 16 bases: every interval is refined, as on the other strand of a sampled read).  Both strands.  One JSON line, also written to profiles/r20_seeds_<size>.json:

  positions, paths, stride (K), reads, read_length
  per batch: request_ms (anchor + refine + emit phases, HIP events; the median of --repeats requests behind one that is not timed), search_ms
             (anchor + refine: the two search kernels with their count and scan), reads_per_s (over request_ms), steps, steps_per_read,
             steps_per_s (over search_ms), per_end_steps_per_read (one whole search per end -- what a caller without this request pays:
             every prefix of a sample of the reads, both strands, sent to count; the steps it reports), anchors, refined_ends_per_read,
             seeds_per_read, idle_share (lane-steps a wave waits for its longest lane), the four phase times, scratch_bytes_per_read_byte
  count_steps_per_s: k_fm_count's rate on the sampled 32-mers of profiles/r19_fm_<size>.json, where that file exists: the loop is the same
  stride_trials (--trials): the rows of runs of libraries built with another stride, as their own JSON lines gave them

The reference has no counterpart: no speed-up is stated."""
import argparse
import contextlib
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

READS = 1 << 20
LENGTH = 150
SAMPLE = 64
SA_MAX_TEXT = (1 << 32) - 2
KINDS = ("sampled", "substituted", "random")


def summary(result):
    """What a stride trial keeps of a run."""
    return {"stride": result["stride"], **{kind: {k: result[kind][k] for k in ("request_ms", "search_ms", "reads_per_s", "steps_per_read", "steps_per_s", "refined_ends_per_read",
                                                                                 "idle_share")} for kind in KINDS}}


@contextlib.contextmanager
def workload(size="small", device=0, reads=READS):
    """The index and the three batches of reads on the device (tools/chain_bench.py measures the same): a dict with fm, n, ids, contig_ids,
    generator_seconds, offsets and batches {kind: bytes}, the tensors on the device."""
    import torch
    import c4_bench as C4
    import gbwt_rs_amd as G
    from gbwt_rs_amd import dist as D
    from gbwt_rs_amd import synth as S
    p = dict(C4.SIZES[size])
    dev = torch.device("cuda", device)
    tmpdir = tempfile.mkdtemp(prefix="gbwt_seeds_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    opened = []
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
        fm = gbz.fm_index(ids, endmarker=0)
        n = int(fm.info()["n"])
        # the reads, on the device
        text = gbz.path_sequences_device(ids, endmarker=0)
        d_text = D.device_view(text.d_text, n, torch.uint8, dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(20)
        at = torch.randint(0, n - LENGTH + 1, (reads,), device=dev, generator=gen)
        sampled = d_text[(at[:, None] + torch.arange(LENGTH, device=dev)[None, :]).reshape(-1)].contiguous()
        letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
        index_of = torch.zeros(256, dtype=torch.int64, device=dev)
        index_of[letters.long()] = torch.arange(4, device=dev)
        substituted = sampled.clone().reshape(reads, LENGTH)
        for _ in range(2):                                                    # another base at a random place, twice
            where = torch.randint(0, LENGTH, (reads,), device=dev, generator=gen)
            old = substituted[torch.arange(reads, device=dev), where]
            substituted[torch.arange(reads, device=dev), where] = letters[(index_of[old.long()] + torch.randint(1, 4, (reads,), device=dev, generator=gen)) % 4]
        substituted = substituted.reshape(-1).contiguous()
        random = letters[torch.randint(0, 4, (reads * LENGTH,), device=dev, generator=gen)].contiguous()
        offsets = (torch.arange(reads + 1, device=dev, dtype=torch.int64) * LENGTH).contiguous()
        torch.cuda.synchronize(dev)
        opened.append(fm)
        yield {"fm": fm, "n": n, "ids": ids, "contig_ids": contig_ids, "generator_seconds": gen_s, "offsets": offsets, "batches": dict(zip(KINDS, (sampled, substituted, random)))}
    finally:
        for fm in opened:
            fm.close()
        shutil.rmtree(tmpdir, ignore_errors=True)


def run(size="small", device=0, repeats=3, reads=READS):
    import gbwt_rs_amd as G
    import bench
    with workload(size, device, reads) as w:
        fm, n, ids, contig_ids, gen_s, offsets = w["fm"], w["n"], w["ids"], w["contig_ids"], w["generator_seconds"], w["offsets"]

        def measured(d_bytes):
            runs = []
            for k in range(repeats + 1):
                fm.seeds_device(offsets.data_ptr(), d_bytes.data_ptr(), reads, reads * LENGTH, strands=G.STRAND_BOTH)
                if k:
                    runs.append(fm.last_seed_info())
            last = runs[-1]
            request_ms = statistics.median(r["anchor_ms"] + r["refine_ms"] + r["emit_ms"] for r in runs)
            search_ms = statistics.median(r["anchor_ms"] + r["refine_ms"] for r in runs)
            # one search per end, on a sample: every prefix of both strands as a pattern of its own
            sample = d_bytes[: SAMPLE * LENGTH].cpu().numpy().tobytes()
            prefixes = [strand[:e] for k in range(SAMPLE) for strand in (sample[k * LENGTH:(k + 1) * LENGTH], G.reverse_complement(sample[k * LENGTH:(k + 1) * LENGTH]))
                        for e in range(1, LENGTH + 1)]
            fm.count(prefixes)
            per_end = fm.info()["last_steps"] / SAMPLE
            return {"request_ms": round(request_ms, 4), "search_ms": round(search_ms, 4), "reads_per_s": reads / (request_ms * 1e-3), "steps": int(last["steps"]),
                    "steps_per_read": last["steps"] / reads, "steps_per_s": last["steps"] / (search_ms * 1e-3), "per_end_steps_per_read": per_end, "per_end_sample": SAMPLE,
                    "anchors": int(last["anchors"]), "refined_ends_per_read": last["refined_ends"] / reads, "seeds_per_read": last["seeds"] / reads, "idle_share": round(last["idle_share"], 4),
                    **{k: round(statistics.median(r[k] for r in runs), 4) for k in ("anchor_ms", "refine_ms", "emit_ms", "hits_ms")},
                    "scratch_bytes": int(last["peak_scratch_bytes"]), "scratch_bytes_per_read_byte": last["peak_scratch_bytes"] / (reads * LENGTH)}

        batches = {kind: measured(d_bytes) for kind, d_bytes in w["batches"].items()}
        info = fm.last_seed_info()
        return {
            "tool": "seed_bench", "size": size,
            "workload": f"Synth.genome[{size} shape, labels 1..1024 bp, seed 42]: the first {len(ids)} of the {len(contig_ids)} paths of contig 'chr1', {n} positions; "
                        f"{reads} reads of {LENGTH} bytes per batch, both strands",
            "paths": int(len(ids)), "positions": n, "generator_seconds": round(gen_s, 1), "stride": int(info["stride"]), "reads": reads, "read_length": LENGTH, "repeats": repeats,
            **batches,
            "every_sampled_read_has_a_seed": batches["sampled"]["seeds_per_read"] >= 1,
            "source_fingerprint": bench.source_fingerprint(),
        }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="small", choices=["tiny", "small"])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="", help="where the JSON line goes as well (default: profiles/r20_seeds_<size>.json)")
    ap.add_argument("--trials", nargs="*", default=[], help="JSON lines of runs with libraries built with another stride: their rows go into stride_trials")
    a = ap.parse_args()
    import gbwt_rs_amd as G
    try:
        res = run(a.size, a.device, a.repeats)
    except G.GbwtHipError as e:                     # (CAPACITY with the bytes needed: the library's message is the answer)
        print(f"seed_bench --size {a.size}: {e}", file=sys.stderr)
        return 2
    count_file = os.path.join(ROOT, "profiles", f"r19_fm_{a.size}.json")
    if os.path.exists(count_file):
        with open(count_file) as f:
            res["count_steps_per_s"] = json.load(f)["sampled"]["steps_per_s"]
    if a.trials:
        res["stride_trials"] = sorted([summary(json.load(open(t))) for t in a.trials] + [summary(res)], key=lambda row: row["stride"])
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out or os.path.join(ROOT, "profiles", f"r20_seeds_{a.size}.json"), "w") as f:
        f.write(line + "\n")
    return 0 if res["every_sampled_read_has_a_seed"] else 1


if __name__ == "__main__":
    sys.exit(main())
