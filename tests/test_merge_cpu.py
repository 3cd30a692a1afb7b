"""GBWT merging without a GPU: the recurrence of the merge (tests/merge_expect.py) against the brute-force builder over the concatenated
paths, the argument checks that answer before the device is touched, the metadata assembly (csrc/merge_meta.hpp) as a program of its own
under ASan + UBSan, and the resources of the merge kernels."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import pytest

import merge_expect as MX
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S
from test_synth import random_paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-C", _lib.CSRC], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", os.path.dirname(S.LIB_PATH)], stdout=subprocess.DEVNULL)


def message():
    return _lib.lib().gbwt_hip_last_error().decode()


def check_pair(paths_a, paths_b):
    a, b = MX.Index.of(S.Synth.from_paths(paths_a)), MX.Index.of(S.Synth.from_paths(paths_b))
    whole = MX.Index.of(S.Synth.from_paths(list(paths_a) + list(paths_b)))
    edges, body, walked = MX.merge(a, b)
    assert walked == (1 if b.visits <= a.visits else 0)
    assert body == whole.body
    assert edges == whole.edges


@pytest.mark.parametrize("name", [name for name, _, _ in MX.special_pairs()])
def test_recurrence_on_the_special_shapes(name):
    _, pa, pb = next(p for p in MX.special_pairs() if p[0] == name)
    if name == "ties":
        pa, pb = pa[:20], pb[:20]                                # (the device test takes all 200; the host's counting is quadratic)
    check_pair(pa, pb)


@pytest.mark.parametrize("k", [128, 129, 254, 255, 256, 300])
def test_recurrence_on_hubs(k):
    check_pair(*MX.hub_pair(k))


@pytest.mark.parametrize("pa,pb", [([], []), ([[]], []), ([], [[], []]), ([[2, 4]], []), ([], [[2, 4]]), ([[]], [[2, 5]]), ([[3, 2]], [[], []])])
def test_recurrence_with_sets_without_visits(pa, pb):
    check_pair(pa, pb)


@pytest.mark.parametrize("seed", range(20))
def test_recurrence_on_random_pairs(seed):
    rng = random.Random(seed)
    paths = random_paths(rng, n_paths=12, n_nodes=9, max_len=14, cyclic=seed % 2 == 1)
    k = rng.randrange(len(paths) + 1)
    check_pair(paths[:k], paths[k:])


def test_bad_merges_are_refused_before_the_device():
    L = _lib.lib()
    fake = 1 << 40                                               # nothing is read through the handles before these checks are done
    h = C.c_void_p(7)

    def merge(a=fake, b=fake, opts=None, flags=_lib.OPEN_ALL, out=h):
        return L.gbwt_hip_merge(a, b, C.byref(opts) if opts is not None else None, flags, C.byref(out) if out is not None else None)

    assert merge(out=None) == _lib.BAD_ARGUMENT and "null output" in message()
    assert merge(a=None) == _lib.BAD_ARGUMENT and "null index" in message()
    assert h.value is None                                       # the output is cleared by a call that fails
    h.value = 7
    assert merge(b=None) == _lib.BAD_ARGUMENT and "null index" in message() and h.value is None
    for flags in (0, 8, 0x17):
        assert merge(flags=flags) == _lib.BAD_ARGUMENT and "flags" in message()
    for algorithm in (3, 7, 0xFFFFFFFF):
        assert merge(opts=_lib.MergeOptions(algorithm, 0)) == _lib.BAD_ARGUMENT and "algorithm" in message()
    assert merge(opts=_lib.MergeOptions(_lib.MERGE_AUTO, 1)) == _lib.BAD_ARGUMENT and "reserved" in message()
    for slot in (0, 1):
        opts = _lib.MergeOptions(_lib.MERGE_REBUILD, 0)
        opts.reserved[slot] = 1
        assert merge(opts=opts) == _lib.BAD_ARGUMENT and "reserved" in message()
    info = _lib.MergeInfo()
    assert L.gbwt_hip_last_merge_info(None, C.byref(info)) == _lib.BAD_ARGUMENT
    assert C.sizeof(_lib.MergeInfo) == 112 and C.sizeof(_lib.MergeOptions) == 24


def test_python_mirror():
    import gbwt_rs_amd as G
    assert (G.MERGE_AUTO, G.MERGE_REBUILD, G.MERGE_INSERT) == (0, 1, 2)
    for cls in (G.GBWT, G.GBZ):
        assert callable(cls.merge) and callable(cls.last_merge_info)
    with pytest.raises(ValueError):
        G.GBWT.merge([])
    with pytest.raises(TypeError):
        G.GBWT.merge(1, 2)


def host_compiler():
    for name in ("g++", "clang++", "c++"):
        found = shutil.which(name)
        if found:
            return found
    raise AssertionError("no host C++ compiler")


def sanitized_program(tmp_path, name, *more_sources):
    """tests/cpp/<name>.cpp, built with ASan + UBSan and run as a program: ({first word of a line: its rest}, the lines); the last one is "done"."""
    exe = tmp_path / name
    subprocess.run([host_compiler(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", _lib.CSRC,
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), *more_sources, "-ldl", "-lpthread", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert not any(line.startswith("FAIL") for line in lines), out.stdout
    assert lines[-1] == "done"
    return {line.split(" ", 1)[0]: line.split(" ", 1)[1] for line in lines if " " in line}, lines


def test_merge_metadata_assembly_under_sanitizers(tmp_path):
    """tests/cpp/merge_meta.cpp: merge_meta.hpp on the host; it checks itself and prints one line per case."""
    got, _ = sanitized_program(tmp_path, "merge_meta")
    assert got["samples"] == "_gbwt_ref s1 s2 s3"                # a's in order, then those of b that a lacks, in b's order
    assert got["contigs"] == "chrA chrB chrC"
    assert got["paths"] == "0,0,0,0 1,0,1,0 1,1,2,5 2,1,1,0 3,2,1,0 1,0,2,0"     # b's with sample and contig ids remapped
    assert got["counts"] == "4 5 3 7"                             # samples, haplotypes = distinct (sample, phase), contigs, flags
    assert got["duplicate"] == "INVALID path 1 of b"
    assert got["one_sided"] == "UNSUPPORTED UNSUPPORTED" and got["incomplete"] == "UNSUPPORTED"
    assert got["neither"] == "none"
    assert got["tags"] == "source=x|reference_samples=r1 r2 r3|k=a|only_b=q"
    assert got["rs_only_b"] == "source=x|reference_samples=r9" and got["rs_absent"] == "source=x"
    assert got["labels"] == "3 ACG||T|GG" and got["conflict"] == "INVALID node 12" and got["translation"] == "UNSUPPORTED"


def test_adopt_metadata_under_sanitizers(tmp_path):
    """tests/cpp/adopt_metadata.cpp: what a maker assembled beside the records, moved into the image made from the records (host_index.hpp)."""
    got, _ = sanitized_program(tmp_path, "adopt_metadata", os.path.join(_lib.CSRC, "host_index.cpp"))
    assert got["fresh.tags"] == " ; " and got["fresh.metadata"] == "0 flags 0 counts 0 0 0 generic 1 paths samples  contigs "
    assert got["fresh.graph"] == "0 translation 0 nodes 0 labels  segments 0 0 0"
    assert got["fresh.records"] == "0 sequences 0 alphabet 21 28 bidirectional 1 data 1 starts 2"
    assert got["all.tags"] == "source=x|reference_samples=s1 ; source=y|k=v"
    assert got["all.metadata"] == "1 flags 7 counts 2 3 1 generic 0 paths 0,0,0,0 1,0,1,0 1,0,2,7 samples s1|s2 contigs chr"
    assert got["all.graph"] == "1 translation 0 nodes 3 labels A|CC|GGG segments 0 0 0"
    for case, part in (("no_metadata", "metadata"), ("no_graph", "graph")):      # the part the assembled image lacks stays as index_from_records made it
        for key in ("tags", "metadata", "graph"):
            assert got[case + "." + key] == got[("fresh." if key == part else "all.") + key], (case, key)
    assert all(got[case + ".records"] == got["fresh.records"] for case in ("all", "no_metadata", "no_graph"))


def test_merge_kernels_compile_without_scratch():
    """Every kernel of merge.hip for gfx950: nothing spilled, no scratch."""
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                          os.path.join(_lib.CSRC, "merge.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    seen = set()
    for at, line in enumerate(lines):
        if "Function Name" in line and "k_merge_" in line:
            block = "\n".join(lines[at:at + 14])
            assert int(re.search(r"VGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"SGPRs Spill: (\d+)", block).group(1)) == 0, block
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)) == 0, block
            seen.add(re.search(r"(k_merge_[a-z_]+?)E", line).group(1))
    for kernel in ("k_merge_count", "k_merge_decode", "k_merge_decode_long", "k_merge_walk", "k_merge_interleave", "k_merge_edge_offsets", "k_merge_concat"):
        assert kernel in seen, (kernel, sorted(seen))
