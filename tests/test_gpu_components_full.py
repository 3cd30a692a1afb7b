"""Weakly connected components at the sizes of BASELINE config 4 (tools/c4_bench.py: SIZES), where the oracle is too slow per record: the
test checks what the generator guarantees -- one graph component per (contig, fragment), every walk inside one of them."""
import os
import sys

import numpy as np
import pytest

import gbwt_rs_amd as G
from gbwt_rs_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.parametrize("size", ["small", "full"])
def test_config_c4_components(size):
    """Synth.genome at config 4's small size (16 M nodes, 32 000 walks) and at its stated size (109 M node ids, 42 000 walks, 5.7 G path
    positions), opened for extraction only (the lean handle):
      * the number of components is contigs x fragments;
      * EVERY node of every path -- extracted with extract_device, looked up in d_component on the device -- lies in the component of its path;
      * the number of distinct path components is the number of parts;
      * the node counts of all components sum to the number of nodes that exist, and every slot is in exactly the component its CSR row says."""
    import torch
    import c4_bench
    from gbwt_rs_amd import dist as D
    tmp = "/dev/shm" if os.path.isdir("/dev/shm") else "/tmp"
    path = os.path.join(tmp, f"gbwt_components_{size}.gbz")
    p = c4_bench.SIZES[size]
    parts = p["contigs"] * p["fragments"]
    try:
        g = c4_bench.generate(size, path)
        dev = G.GBZ.load(path, flags=_lib.OPEN_EXTRACT)
        view = dev.components_device()
        t = dev.last_components_ms()
        print(f"components[{size}]: {view.components} components over {view.slots} slots, {t}")
        assert view.components == parts
        assert view.min_node == 1 and view.slots == g.alphabet_size // 2 - 1 and view.paths == g.paths
        device = torch.device("cuda", 0)
        component = D.device_view(view.d_component, view.slots, torch.int32, device)              # (0xFFFFFFFF reads as -1)
        exists = component >= 0
        assert int(exists.sum()) == view.nodes
        assert bool((component[exists] < parts).all())
        # the CSR against the per-slot array, on the device
        offsets = D.device_view(view.d_offsets, view.components + 1, torch.int64, device)
        nodes = D.device_view(view.d_nodes, view.nodes, torch.int32, device).long()
        assert int(offsets[0]) == 0 and int(offsets[-1]) == view.nodes and bool((offsets[1:] > offsets[:-1]).all())
        row = torch.repeat_interleave(torch.arange(parts, device=device), offsets[1:] - offsets[:-1])
        assert bool((component[nodes - view.min_node].long() == row).all())
        assert bool((nodes[1:] > nodes[:-1])[row[1:] == row[:-1]].all())                           # ascending inside a component
        firsts = nodes[offsets[:-1]]
        assert bool((firsts[1:] > firsts[:-1]).all())                                              # components in order of their smallest node
        del row, nodes
        # every node of every path, in batches of paths
        of_path = dev.path_components(np.arange(g.paths))
        assert len(np.unique(of_path)) == parts and int(of_path.max()) < parts
        d_of_path = torch.from_numpy(of_path.astype(np.int64)).to(device)
        checked = 0
        for lo in range(0, g.paths, 2048):
            hi = min(lo + 2048, g.paths)
            rows = dev.extract_device(2 * np.arange(lo, hi, dtype=np.uint64))
            off, ids = D.paths_tensors(rows, device)
            want = torch.repeat_interleave(d_of_path[lo:hi], off[1:] - off[:-1])
            got = component[(ids.long() >> 1) - view.min_node].long()
            assert bool((got == want).all()), (lo, hi)
            checked += int(rows.total)
        assert checked == (g.size - g.sequences) // 2
        # the selection of a contig is the walks of its fragments (+ its generic paths): every path of the contig's components
        names = np.asarray(g.path_names)
        for contig in (0, p["contigs"] - 1):
            assert np.array_equal(dev.select_paths(f"chr{contig + 1}"), np.flatnonzero(names[:, 1] == contig).astype(np.uint64))
        dev.close()
    finally:
        for name in (path, path + ".generic.npy", path + ".tmp"):
            if os.path.exists(name):
                os.remove(name)
