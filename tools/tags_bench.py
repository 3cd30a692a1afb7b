#!/usr/bin/env python3
"""The tags of a suffix array over the text of every path of a config-4-shaped GBZ (gbz-extract's `tag-array` mode,
src/bin/gbz-extract.rs:408-482) on one GPU.

Synth.genome with labels of realistic length (1 .. 1 024 bp) at the shape of tools/c4_bench.py's SIZES[size].  The suffix array is a seeded
random permutation of 0 .. expected_len - 1 -- a Feistel network over the next power of four, walked until the value is in range -- made ON
THE DEVICE batch by batch (torch), so that no host ever holds it; every batch goes through gbwt_hip_tags_device.  One JSON line:

  entries / expected_len      suffix-array entries looked up (all of them unless --entries) / the length of the text
  plan_ms, walk_ms            the plan of the path list (HIP events: the walk of its extraction, and everything behind it); plan_bytes =
                              what the workspace holds more once the plan is made (12 B per position + 4 B per 32 text offsets, rounded up)
  gather_ms                   the gather kernel, summed over the batches (HIP events); entries_per_s = entries / that
  counted bytes per entry     streamed: 8 B of suffix array read + 8 B of tag written = 16; lookup: the cache lines a lookup touches when
                              nothing is shared between entries -- hint, text offsets, node id = 3 lines of 128 B -- stated apart; each as a
                              rate and as a fraction of 8 TB/s (HBM peak) and of 6.29 TB/s (measured copy rate)
  parity                      a seeded sample of paths: the tags of their rows (a slice of the text order) against a CPU construction from the
                              generator's own node ids and the label lengths of the host image; the sum of all suffix-array values modulo 2^64
                              against n (n - 1) / 2 (what a permutation sums to); runs of the text order = entries
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


class Permutation:
    """A seeded bijection of 0 .. n - 1 evaluated on the device: four Feistel rounds on the two halves of 2 h bits (4^h >= n), values that
    land outside the range encrypted again (cycle walking: a bijection of the smaller set)."""

    def __init__(self, n, seed, device):
        import torch
        self.torch, self.n, self.device = torch, n, device
        self.half = max(1, ((max(n, 2) - 1).bit_length() + 1) // 2)
        self.mask = (1 << self.half) - 1
        rng = np.random.default_rng(seed)
        self.keys = [int(k) for k in rng.integers(1, 1 << 31, size=4)]

    def _round(self, r, key):
        x = (r * 0x9E3779B1 + key) & 0xFFFFFFFFFFFF
        x = (x ^ (x >> 15)) * 0x85EBCA6B & 0xFFFFFFFFFFFF
        return (x ^ (x >> 13)) & self.mask

    def _encrypt(self, x):
        left, right = x >> self.half, x & self.mask
        for key in self.keys:
            left, right = right, left ^ self._round(right, key)
        return (left << self.half) | right

    def values(self, first, count):
        """Entries first .. first + count - 1 of the permutation: an int64 tensor on the device."""
        torch = self.torch
        x = self._encrypt(torch.arange(first, first + count, dtype=torch.int64, device=self.device))
        while True:
            outside = x >= self.n
            if not bool(outside.any()):
                return x
            x = torch.where(outside, self._encrypt(x), x)


def cpu_tags(gbz, nodes, lengths):
    """Tags of one row (its bases and its endmarker) from GBWT-encoded nodes and the label lengths of the host image."""
    lens = []
    for v in nodes.tolist():
        node = v >> 1
        if node not in lengths:
            lengths[node] = len(gbz.node_sequence(node))
        lens.append(lengths[node])
    lens = np.array(lens, dtype=np.int64)
    at = np.zeros(lens.size, dtype=np.int64)
    np.cumsum(lens[:-1], out=at[1:])
    within = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(at, lens)
    start = nodes.astype(np.uint64) << np.uint64(10)                       # ((id << 11) | (orientation << 10)) of 2 id + orientation
    return np.append(np.repeat(start, lens) + within.astype(np.uint64), np.uint64(0))


def run(size="small", batch_mib=2048, entries=0, sample=16, device=0, seed=7):
    import torch
    import c4_bench as C4
    import gbwt_rs_amd as G
    from gbwt_rs_amd import synth as S
    import bench
    p = dict(C4.SIZES[size])
    tmpdir = tempfile.mkdtemp(prefix="gbwt_tags_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        path = os.path.join(tmpdir, "c4.gbz")
        t0 = time.perf_counter()
        g = S.Synth.genome(contigs=p["contigs"], fragments=p["fragments"], haplotypes=p["haplotypes"], sites=p["sites"], seed=42, labels=1,
                           min_walkers=p["min_walkers"], wrap_contig=p["wrap_contig"], threads=min(16, os.cpu_count() or 1))
        g.save(path, as_gbz=True)
        gen_s = time.perf_counter() - t0
        stats = [g.path_text_stats(q) for q in range(g.paths)]
        positions = int(sum(s[0] for s in stats)) + g.paths
        row_start = np.zeros(g.paths + 1, dtype=np.int64)
        np.cumsum(np.array([s[2] + 1 for s in stats], dtype=np.int64), out=row_start[1:])
        t0 = time.perf_counter()
        gbz = G.GBZ.load(path, device=device, flags=G.OPEN_EXTRACT | G.OPEN_GFA)
        open_ms = (time.perf_counter() - t0) * 1e3
        ids = np.arange(g.paths, dtype=np.uint64)
        gbz.path_sequences_device(ids[:1], endmarker=0)                      # (untimed) the node labels reach HBM with the first request for bases
        mem0 = gbz.memory_usage()["workspace_device_bytes"]
        t0 = time.perf_counter()
        expected_len = gbz.text_length(ids)
        plan_wall_ms = (time.perf_counter() - t0) * 1e3
        walk_ms, plan_ms, _ = gbz.last_tags_ms()
        plan_bytes = gbz.memory_usage()["workspace_device_bytes"] - mem0
        ok_len = expected_len == int(row_start[-1])
        dev = torch.device("cuda", device)
        total = expected_len if entries <= 0 else min(entries, expected_len)
        batch = max(1, min(total, (batch_mib << 20) // 8))
        perm = Permutation(expected_len, seed, dev)
        d_tags = torch.empty(batch, dtype=torch.int64, device=dev)
        gather_ms, wall_ms, value_sum, batches = 0.0, 0.0, 0, 0
        for first in range(0, total, batch):
            count = min(batch, total - first)
            d_sa = perm.values(first, count)
            value_sum = (value_sum + int(d_sa.sum().item())) & 0xFFFFFFFFFFFFFFFF      # (int64 sums wrap: exact modulo 2^64)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            gbz.tags_device(ids, d_sa.data_ptr(), count, d_tags.data_ptr())
            wall_ms += (time.perf_counter() - t0) * 1e3
            gather_ms += gbz.last_tags_ms()[2]
            batches += 1
            del d_sa
        # parity: rows of a seeded sample of paths in text order against the CPU construction; the text order has a run per entry
        rng = np.random.default_rng(seed)
        picks = sorted(rng.choice(g.paths, size=min(sample, g.paths), replace=False).tolist())
        lengths, parity = {}, True
        for q in picks:
            a, b = int(row_start[q]), int(row_start[q + 1])
            d_sa = torch.arange(a, b, dtype=torch.int64, device=dev)
            d_out = torch.empty(b - a, dtype=torch.int64, device=dev)
            runs = gbz.tags_device(ids, d_sa.data_ptr(), b - a, d_out.data_ptr())
            want = cpu_tags(gbz, g.path(q), lengths)
            parity &= bool(np.array_equal(d_out.cpu().numpy().view(np.uint64), want)) and runs == b - a
        sum_ok = total != expected_len or value_sum == (total * (total - 1) // 2) & 0xFFFFFFFFFFFFFFFF
        seconds = gather_ms * 1e-3
        streamed, lookup = 16 * total, 3 * 128 * total
        return {
            "tool": "tags_bench", "size": size, "workload": f"Synth.genome[{size} shape, labels 1..1024 bp, seed 42]: {g.paths} paths, {positions} positions, a seeded permutation as suffix array",
            "paths": int(g.paths), "positions": positions, "expected_len": int(expected_len), "entries": int(total), "batches": batches, "batch_mib": batch_mib,
            "open_ms": round(open_ms, 1), "generator_seconds": round(gen_s, 1), "walk_ms": round(walk_ms, 3), "plan_ms": round(plan_ms, 3), "plan_wall_ms": round(plan_wall_ms, 2),
            "plan_bytes": int(plan_bytes), "plan_bytes_per_position": plan_bytes / positions, "gather_ms": round(gather_ms, 3), "gather_wall_ms": round(wall_ms, 2),
            "entries_per_s": total / seconds, "streamed_bytes_per_entry": 16, "lookup_line_bytes_per_entry": 384,
            "streamed_TBps": streamed / seconds / 1e12, "streamed_frac_of_8TBps": streamed / seconds / 8e12, "streamed_frac_of_6.29TBps": streamed / seconds / 6.29e12,
            "lookup_lines_TBps": lookup / seconds / 1e12, "lookup_lines_frac_of_8TBps": lookup / seconds / 8e12, "lookup_lines_frac_of_6.29TBps": lookup / seconds / 6.29e12,
            "parity_sample": len(picks), "parity_ok": bool(parity), "length_ok": bool(ok_len), "permutation_sum_ok": bool(sum_ok),
            "source_fingerprint": bench.source_fingerprint(),
        }
    finally:
        shutil.rmtree(tmpdir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="small", choices=["tiny", "medium", "small", "full"])
    ap.add_argument("--batch-mib", type=int, default=2048, help="bytes of suffix array per request")
    ap.add_argument("--entries", type=int, default=0, help="look up only the first ENTRIES values of the permutation (0 = all)")
    ap.add_argument("--sample", type=int, default=16, help="paths of the parity check")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    a = ap.parse_args()
    res = run(a.size, a.batch_mib, a.entries, a.sample, a.device)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["parity_ok"] and res["length_ok"] and res["permutation_sum_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
