"""GBWT path removal without a GPU: the deletion (tests/remove_expect.py) against the brute-force builder over the kept paths, the argument
checks that answer before the device is touched, the metadata assembly (csrc/remove_meta.hpp) as a program of its own under ASan + UBSan,
and the resources of the removal kernels."""
import ctypes as C
import itertools
import os
import random
import re
import subprocess

import pytest

import kat
import merge_expect as MX
import remove_expect as RX
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S
from test_merge_cpu import sanitized_program
from test_synth import random_paths


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-C", _lib.CSRC], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", os.path.dirname(S.LIB_PATH)], stdout=subprocess.DEVNULL)


def message():
    return _lib.lib().gbwt_hip_last_error().decode()


def check_removal(paths, removed, bidirectional=True):
    """Records, starts and header of the deletion equal those of the builder over the kept paths."""
    whole = S.Synth.from_paths(paths, bidirectional=bidirectional)
    kept = S.Synth.from_paths([p for k, p in enumerate(paths) if k not in set(removed)], bidirectional=bidirectional)
    index = MX.Index.of(whole)
    edges, body, sequences, removed_steps = RX.remove(index, RX.sequences_of(removed, bidirectional))
    want = MX.Index.of(kept)
    assert body == want.body and edges == want.edges
    assert removed_steps == (2 if bidirectional else 1) * sum(len(paths[k]) for k in removed)
    data, starts, hdr = RX.remove_paths(whole, removed)
    assert data == bytes(kept.data()) and starts == [int(s) for s in kept.starts()]
    assert hdr == (kept.sequences, kept.size, kept.alphabet_offset, kept.alphabet_size, kept.bidirectional)


def subsets(n):
    return [list(c) for k in range(n + 1) for c in itertools.combinations(range(n), k)]


@pytest.mark.parametrize("removed", subsets(6), ids=lambda r: "-".join(map(str, r)) or "none")
def test_deletion_on_every_subset_of_the_fixture(removed):
    check_removal(kat.true_paths(False), removed)


@pytest.mark.parametrize("removed", range(7))
def test_deletion_of_one_path_of_the_fixture_with_an_empty_path(removed):
    check_removal(kat.true_paths(True), [removed])


@pytest.mark.parametrize("name", [name for name, _, _, _ in RX.special_removals()])
def test_deletion_on_the_special_shapes(name):
    _, paths, removed, bidirectional = next(s for s in RX.special_removals() if s[0] == name)
    check_removal(paths, removed, bidirectional)


def random_removal(seed):
    rng = random.Random(seed)
    paths = random_paths(rng, n_paths=12, n_nodes=9, max_len=14, cyclic=seed % 2 == 1)
    removed = sorted(rng.sample(range(len(paths)), rng.randrange(len(paths) + 1)))
    return paths, removed


@pytest.mark.parametrize("seed", range(20))
def test_deletion_on_random_sets(seed):
    check_removal(*random_removal(seed))


def test_bad_removals_are_refused_before_the_device():
    L = _lib.lib()
    fake = 1 << 40                                               # nothing is read through the handle before these checks are done
    h = C.c_void_p(7)
    ids = (C.c_uint64 * 2)(0, 1)

    def remove(index=fake, path_ids=ids, n=2, opts=None, flags=_lib.OPEN_ALL, out=h):
        return L.gbwt_hip_remove_paths(index, path_ids, n, C.byref(opts) if opts is not None else None, flags, C.byref(out) if out is not None else None)

    assert remove(out=None) == _lib.BAD_ARGUMENT and "null output" in message()
    assert remove(index=None) == _lib.BAD_ARGUMENT and "null index" in message()
    assert h.value is None                                       # the output is cleared by a call that fails
    h.value = 7
    assert remove(path_ids=None) == _lib.BAD_ARGUMENT and "null path ids" in message() and h.value is None
    for flags in (0, 8, 0x17):
        assert remove(flags=flags) == _lib.BAD_ARGUMENT and "flags" in message()
    for algorithm in (3, 7, 0xFFFFFFFF):
        assert remove(opts=_lib.RemoveOptions(algorithm, 0)) == _lib.BAD_ARGUMENT and "algorithm" in message()
    assert remove(opts=_lib.RemoveOptions(_lib.REMOVE_AUTO, 1)) == _lib.BAD_ARGUMENT and "reserved" in message()
    for slot in (0, 1):
        opts = _lib.RemoveOptions(_lib.REMOVE_DELETE, 0)
        opts.reserved[slot] = 1
        assert remove(opts=opts) == _lib.BAD_ARGUMENT and "reserved" in message()
    info = _lib.RemoveInfo()
    assert L.gbwt_hip_last_remove_info(None, C.byref(info)) == _lib.BAD_ARGUMENT
    assert C.sizeof(_lib.RemoveInfo) == 112 and C.sizeof(_lib.RemoveOptions) == 24


def test_python_mirror():
    import gbwt_rs_amd as G
    assert (G.REMOVE_AUTO, G.REMOVE_REBUILD, G.REMOVE_DELETE) == (0, 1, 2)
    for cls in (G.GBWT, G.GBZ):
        assert callable(cls.remove_paths) and callable(cls.keep_paths) and callable(cls.last_remove_info)
    assert callable(G.GBZ.remove_contig)
    assert {"REMOVE_AUTO", "REMOVE_REBUILD", "REMOVE_DELETE"} <= set(G.__all__)


def test_remove_metadata_assembly_under_sanitizers(tmp_path):
    """tests/cpp/remove_meta.cpp: remove_meta.hpp on the host, built with ASan + UBSan and run as a program; it prints one line per case.
    The refusals of a path id at or above the path count and of one that appears twice, which need a handle on the device, are checked
    here through the function the library calls for them (remove_check_ids) and end to end in tests/test_gpu_remove.py."""
    got, lines = sanitized_program(tmp_path, "remove_meta")
    assert got["ids_good"] == "1" and got["ids_none"] == "1"
    assert got["ids_high"].startswith("0 path id 6 ") and got["ids_twice"] == "0 path id 3 appears twice"
    assert got["some_samples"] == "_gbwt_ref s1 s3"                # s2 was used by a removed path alone; the rest keep their order
    assert got["some_contigs"] == "chrA chrC"
    assert got["some_paths"] == "0,0,0,0 1,0,1,0 2,0,1,0 2,1,1,0"  # sample and contig ids remapped
    assert got["some_counts"] == "3 3 2 7"                         # samples, haplotypes = distinct (sample, phase), contigs, flags
    assert got["nothing_samples"] == "_gbwt_ref s1 s2 s3" and got["nothing_contigs"] == "chrA chrB chrC"
    assert got["nothing_paths"] == "0,0,0,0 1,0,1,0 1,1,2,5 2,1,1,0 3,0,1,0 3,2,1,0" and got["nothing_counts"] == "4 5 3 7"
    assert got["all_samples"] == "" and got["all_contigs"] == "" and "all_paths" in lines and got["all_counts"] == "0 0 0 6"
    assert got["without"] == "none"
    assert got["incomplete"] == "UNSUPPORTED the metadata lacks path names, sample names or contig names"
    assert got["tags"] == "source=x|reference_samples=s1 elsewhere|k=v"
    assert got["tags_gone"] == "k=v" and got["tags_plain"] == "source=x"
    assert got["labels"] == "2 C||GG"                              # node 12 is no longer visited: its label is cleared
    assert got["labels_none"] == "0 0"
    assert got["translation"] == "UNSUPPORTED named"


def test_remove_kernels_compile_without_scratch():
    """Every kernel of remove.hip for gfx950: nothing spilled, no scratch."""
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                          os.path.join(_lib.CSRC, "remove.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    seen = set()
    for at, line in enumerate(lines):
        if "Function Name" in line and "k_remove_" in line:
            block = "\n".join(lines[at:at + 14])
            assert int(re.search(r"VGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"SGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)) == 0, block
            seen.add(re.search(r"(k_remove_[a-z_]+?)E", line).group(1))
    assert seen == {"k_remove_mark", "k_remove_compact", "k_remove_edge_offsets"}, sorted(seen)
