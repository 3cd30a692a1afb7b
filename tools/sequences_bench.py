#!/usr/bin/env python3
"""The bases of every path of a config-4-shaped GBZ (gbz-extract's `sequences` mode, src/bin/gbz-extract.rs:266-294) on one GPU.

Synth.genome with labels of realistic length (1 .. 1 024 bp) at the shape of tools/c4_bench.py's SIZES[size]; every path forward with its
endmarker, in batches bounded by bytes (--batch-gib) left in HBM (gbwt_hip_path_sequences_device).  One JSON line:

  total_bases / bytes         bases of all paths; bytes = bases + one endmarker per path
  first_request_ms            wall time of the first request on the handle, which uploads the node labels (label_device_bytes)
  walk_ms / bases_kernel_ms   steady passes, summed over the batches, from HIP events (gbwt_hip_last_sequences_ms; sizes_ms apart)
  bases_per_s                 total_bases / the steady wall time of a pass (the requests alone)
  counted_bytes               4 B node id + label bytes read + bases written, per position: what the bases kernel must move at least;
                              kernel_TBps and its fraction of 8 TB/s (HBM peak) and of 6.29 TB/s (measured copy rate)
  parity                      a seeded sample of paths against a CPU construction: the generator's own node ids with the labels of the
                              host image (gbwt_hip_node_sequence), reverse-complemented in numpy; and every batch's size against the
                              generator's summed label lengths
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

COMPLEMENT = np.full(256, ord("N"), dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    COMPLEMENT[_a] = _b


def cpu_bases(gbz, nodes, labels):
    """Bases of a path of GBWT-encoded nodes, built on the host: labels[node id] from the host image, reverse ones reverse-complemented."""
    parts = []
    for v in nodes.tolist():
        node = v >> 1
        if node not in labels:
            labels[node] = np.frombuffer(gbz.node_sequence(node), dtype=np.uint8)
        lab = labels[node]
        parts.append(COMPLEMENT[lab[::-1]] if v & 1 else lab)
    return np.concatenate(parts).tobytes() if parts else b""


def run(size="small", passes=3, batch_gib=16.0, sample=16, device=0, seed=7):
    import c4_bench as C4
    import gbwt_rs_amd as G
    from gbwt_rs_amd import synth as S
    import bench
    p = dict(C4.SIZES[size])
    p["labels"] = 1
    tmpdir = tempfile.mkdtemp(prefix="gbwt_seq_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        path = os.path.join(tmpdir, "c4.gbz")
        t0 = time.perf_counter()
        g = S.Synth.genome(contigs=p["contigs"], fragments=p["fragments"], haplotypes=p["haplotypes"], sites=p["sites"], seed=42, labels=1,
                           min_walkers=p["min_walkers"], wrap_contig=p["wrap_contig"], threads=min(16, os.cpu_count() or 1))
        g.save(path, as_gbz=True)
        gen_s = time.perf_counter() - t0
        stats = [g.path_text_stats(q) for q in range(g.paths)]
        nodes = np.array([s[0] for s in stats], dtype=np.int64)
        bases = np.array([s[2] for s in stats], dtype=np.int64)
        # the HIP runtime started before anything is timed (a tiny index, one extraction)
        tiny = S.Synth.chain(sites=8, haplotypes=4, alleles=2, model=S.MOSAIC, founders=2, switch_rate=0.1, seed=1)
        tiny_dev = G.GBWT.from_records(tiny.data(), tiny.starts(), tiny.alphabet_offset, tiny.alphabet_size, tiny.sequences, tiny.size, True, device=device)
        tiny_dev.sequences_csr(np.arange(tiny.sequences, dtype=np.uint64))
        tiny_dev.close()
        t0 = time.perf_counter()
        gbz = G.GBZ.load(path, device=device, flags=G.OPEN_EXTRACT | G.OPEN_GFA)
        open_ms = (time.perf_counter() - t0) * 1e3
        # byte-bounded batches, in path order
        budget = int(batch_gib * (1 << 30))
        batches, lo, acc = [], 0, 0
        for q in range(g.paths):
            if q > lo and acc + bases[q] + 1 > budget:
                batches.append((lo, q)); lo, acc = q, 0
            acc += bases[q] + 1
        batches.append((lo, g.paths))
        mem0 = gbz.memory_usage()["index_device_bytes"]
        ok_sizes = True
        t0 = time.perf_counter()
        first = gbz.path_sequences_device(np.arange(*batches[0], dtype=np.uint64), endmarker=0)
        first_request_ms = (time.perf_counter() - t0) * 1e3
        ok_sizes &= first.total == int(bases[batches[0][0]:batches[0][1]].sum()) + (batches[0][1] - batches[0][0])
        label_device_bytes = gbz.memory_usage()["index_device_bytes"] - mem0
        walls, walk, sizes, kern = [], [], [], []
        empty = np.zeros(0, dtype=np.uint64)
        for _ in range(passes):
            w = s = k = wall = 0.0
            for a, b in batches:
                ids = np.arange(a, b, dtype=np.uint64)
                gbz.path_sequences_device(empty)          # (untimed) a request that repeats the workspace's last one would only find it there
                t0 = time.perf_counter()
                out = gbz.path_sequences_device(ids, endmarker=0)
                wall += (time.perf_counter() - t0) * 1e3
                ok_sizes &= out.total == int(bases[a:b].sum()) + (b - a)
                x, y, z = gbz.last_sequences_ms()
                w += x; s += y; k += z
            walls.append(wall); walk.append(w); sizes.append(s); kern.append(k)
        # parity: a seeded sample, host copies of the device's rows against the CPU construction
        rng = np.random.default_rng(seed)
        picks = sorted(rng.choice(g.paths, size=min(sample, g.paths), replace=False).tolist())
        labels, parity = {}, True
        for q in picks:
            _, got = gbz.path_sequences([q], endmarker=0)
            parity &= got == cpu_bases(gbz, g.path(q), labels) + b"\x00"
        _, got = gbz.path_sequences(picks, G.REVERSE)
        want = b"".join(COMPLEMENT[np.frombuffer(cpu_bases(gbz, g.path(q), labels), dtype=np.uint8)[::-1]].tobytes() for q in picks)
        parity &= got == want
        best = int(np.argmin(kern))
        total_bases, positions = int(bases.sum()), int(nodes.sum())
        counted = 4 * positions + 2 * total_bases + g.paths
        kernel_s = kern[best] * 1e-3
        return {
            "tool": "sequences_bench", "size": size, "workload": f"Synth.genome[{size} shape, labels 1..1024 bp, seed 42]: {g.paths} paths, {positions} positions",
            "paths": int(g.paths), "positions": positions, "total_bases": total_bases, "bytes": total_bases + int(g.paths),
            "batches": len(batches), "batch_gib": batch_gib, "open_ms": round(open_ms, 1), "generator_seconds": round(gen_s, 1),
            "first_request_ms": round(first_request_ms, 2), "first_request_bytes": int(first.total), "label_device_bytes": int(label_device_bytes),
            "passes": passes, "wall_ms": [round(x, 2) for x in walls], "walk_ms": round(walk[best], 3), "sizes_ms": round(sizes[best], 3),
            "bases_kernel_ms": round(kern[best], 3), "bases_per_s": total_bases / (min(walls) * 1e-3),
            "counted_bytes": counted, "kernel_TBps": counted / kernel_s / 1e12, "frac_of_8TBps": counted / kernel_s / 8e12,
            "frac_of_6.29TBps": counted / kernel_s / 6.29e12, "parity_sample": len(picks), "parity_ok": bool(parity), "sizes_ok": bool(ok_sizes),
            "source_fingerprint": bench.source_fingerprint(),
        }
    finally:
        shutil.rmtree(tmpdir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="small", choices=["tiny", "medium", "small", "full"])
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--batch-gib", type=float, default=16.0, help="bytes of bases per request (byte-bounded batches)")
    ap.add_argument("--sample", type=int, default=16, help="paths of the parity check")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="", help="also append the JSON line to this file")
    a = ap.parse_args()
    res = run(a.size, a.passes, a.batch_gib, a.sample, a.device)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0 if res["parity_ok"] and res["sizes_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
