"""GBZ::reference_positions (src/gbz.rs:600-657) through the device, every id, length, base offset and GBWT position compared -- exact
equality -- with tests/refpos_expect.py: the reference's loop over OracleGBWT.start / forward, label lengths from S-lines or from the
generator's label_lengths, the metadata as the test built it."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import gbwt_rs_amd as G
import oracle_lib as O
import refpos_expect as R
import seq_expect as E
import tangled_graphs as T
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S

pytestmark = pytest.mark.gpu

FIXTURES = {"example.gbz": [0, 1], "example-v1.gbz": [0, 1], "translation.gbz": [0], "translation-v1.gbz": [0]}   # the reference paths: the P-lines
INTERVALS = [0, 1, 2, 7, 64, 1000, 10 ** 6, 2 ** 64 - 1]
TAG = "s0 s3 nosuch"


def expect(starts, ids, interval):
    return [R.positions_of(starts[p], p, interval) for p in ids]


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixtures_like_the_reference(name):
    path = os.path.join(O.GOLDEN, name)
    dev, gbwt = G.GBZ.load(path), O.OracleGBZ(path).gbwt()
    lengths, samples, path_samples = R.golden(name)
    visited = {v // 2 for p in range(dev.paths()) for v in gbwt.sequence(2 * p)}
    for v in range(1, lengths.size):                                           # the lengths read off the GFA are those of the host image
        label = dev.node_sequence(v)                                           # (a node on no path does not exist: GBZ::has_node)
        assert (label is None) == (v not in visited) and (label is None or len(label) == lengths[v]), v
    ref = R.reference_paths(samples, path_samples, None)
    assert ref == FIXTURES[name] and dev.reference_paths().tolist() == ref
    assert dev.reference_paths(also_generic=False).size == 0
    assert dev.reference_sample_names(True) == ["_gbwt_ref"] and dev.reference_sample_names(False) == []
    starts = {p: R.node_starts(gbwt, p, lengths) for p in range(dev.paths())}
    for interval in range(10):
        assert R.same(dev.reference_positions(interval), expect(starts, ref, interval)), interval
    if name == "example.gbz":                                                  # src/gbz/tests.rs:521-567's fixture: lengths 5 and 4
        got = dev.reference_positions(2)
        assert [(p, n, o.tolist()) for p, n, o, _ in got] == [(0, 5, [0, 2, 4]), (1, 4, [0, 2])]
    every = list(range(dev.paths()))                                           # the W-lines as well (reverse visits in example.gbz)
    for interval in (0, 1, 3):
        assert R.same(dev.path_positions(every, interval), expect(starts, every, interval)), interval


class Genome:
    """A Synth.genome GBZ with long labels, ragged walks, generic paths of 1 400 - 4 000 nodes and a reference_samples tag that names two
    samples and one the metadata does not hold; the node starts of every path from one oracle walk."""

    def __init__(self, directory):
        self.gbz = os.path.join(directory, "genome.gbz")
        g = S.Synth.genome(contigs=3, fragments=2, haplotypes=8, sites=1200, seed=5, labels=1)
        g.set_tag("reference_samples", TAG)
        g.save(self.gbz, as_gbz=True)
        oracle = O.OracleGBZ(self.gbz)
        self.lengths = E.LabelTable.from_gfa(oracle.gfa()).len
        self.paths = g.paths
        self.sample_names, self.path_samples = g.sample_names, [int(x[0]) for x in g.path_names]
        self.ref = R.reference_paths(self.sample_names, self.path_samples, TAG)
        self.generic = g.generic_paths()
        self.nodes = [len(g.path(p)) for p in range(g.paths)]
        gbwt = oracle.gbwt()
        self.starts = {p: R.node_starts(gbwt, p, self.lengths) for p in range(g.paths)}


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    return Genome(str(tmp_path_factory.mktemp("refpos")))


def test_genome_reference_positions(genome):
    dev = G.GBZ.load(genome.gbz)
    assert genome.lengths.max() == 1024 and len(set(genome.nodes)) > 10        # long labels, ragged walks
    assert [genome.nodes[p] for p in genome.generic] == [2888, 1382, 4034]     # more than one workgroup of positions, more than 2^11 chain elements
    assert R.reference_sample_names(genome.sample_names, TAG, True) == ["s0", "s3", "_gbwt_ref"] == dev.reference_sample_names(True)
    assert dev.reference_sample_names(False) == ["s0", "s3"]
    assert dev.reference_paths().tolist() == genome.ref and set(genome.generic) < set(genome.ref) and len(genome.ref) == 22
    assert dev.reference_paths(False).tolist() == [p for p in genome.ref if p not in genome.generic]
    before = dev.memory_usage()["workspace_device_bytes"]
    for interval in INTERVALS:
        got = dev.reference_positions(interval)
        assert R.same(got, expect(genome.starts, genome.ref, interval)), interval
        if interval >= 10 ** 6:                                                # longer than every path: its first node alone
            assert all(o.tolist() == [0] for _, _, o, _ in got)
        if interval <= 1:                                                      # labels have a base at least: every node
            assert [o.size for _, _, o, _ in got] == [genome.nodes[p] for p in genome.ref]
        # round t of the pointer doubling marks the chain elements of rank 2^t .. 2^(t+1) - 1 (and, where lanes of one round see each other's
        # marks, some behind them): a chain of k elements keeps at most ceil(log2 k) rounds busy, one of a single element none
        rounds, launches = dev.last_positions_rounds()
        longest = max(o.size for _, _, o, _ in got)
        assert (1 if longest > 1 else 0) <= rounds <= (longest - 1).bit_length() and launches >= 8, (interval, rounds, launches)
    positions = sum(genome.nodes[p] for p in genome.ref)
    assert dev.memory_usage()["workspace_device_bytes"] - before >= 24 * positions   # the scratch is counted


@pytest.mark.parametrize("flags", [_lib.OPEN_GFA, _lib.OPEN_ALL], ids=["gfa", "all"])
@pytest.mark.parametrize("sample_interval", ["8", "37", "0"])
def test_genome_sample_intervals_and_handles(genome, monkeypatch, sample_interval, flags):
    """Segments of 8 and of 37 nodes and none at all (one lane per row), on a handle opened for GFA lines alone (with samples it has given its
    raw descriptors back: the step on the record bytes) and on one opened for everything (the O(1) step).  Interval 0 keeps every node: the
    first and the last node of every segment and of every row."""
    monkeypatch.setenv("GBWT_HIP_SAMPLE_INTERVAL", sample_interval)
    dev = G.GBZ.load(genome.gbz, flags=flags)
    if flags == _lib.OPEN_GFA:
        # with samples the handle is lean: its raw descriptors (64 B per record) are gone, and the walk steps on the record bytes; without
        # samples it keeps them (capi_open.hip: release_for_lean_extraction)
        full = G.GBZ.load(genome.gbz, flags=_lib.OPEN_ALL)
        gave_back = dev.memory_usage()["index_device_bytes"] <= full.memory_usage()["index_device_bytes"] - 64 * int(full.stats.records)
        assert gave_back == (sample_interval != "0")
        full.close()
    monkeypatch.delenv("GBWT_HIP_SAMPLE_INTERVAL")
    assert (dev.open_times()["samples"] > 0) == (sample_interval != "0")
    for interval in (0, 1, 7, 64, 1000):
        assert R.same(dev.reference_positions(interval), expect(genome.starts, genome.ref, interval)), interval
    got = dev.reference_positions(0)
    assert all(o.size == genome.nodes[p] and int(o[-1]) < n for (p, n, o, _) in got)


def test_genome_path_positions_any_ids(genome):
    dev = G.GBZ.load(genome.gbz)
    every = list(range(genome.paths))
    assert sum(genome.nodes) > 100000 and any(sum(genome.nodes[:k]) % 256 for k in range(1, genome.paths))   # row ends inside workgroups
    for interval in (0, 7, 5000):
        assert R.same(dev.path_positions(every, interval), expect(genome.starts, every, interval)), interval
    others = [p for p in every if p not in genome.ref]
    order = others[::-1] + [others[3], others[3], others[0]]                   # descending, then duplicates: each a row of its own
    got = dev.path_positions(order, 300)
    assert R.same(got, expect(genome.starts, order, 300))
    assert dev.path_positions([], 5) == []
    paths, positions = dev.path_positions_csr([], 5)
    assert paths.size == 0 and positions.size == 0
    with pytest.raises(G.GbwtHipError) as err:
        dev.path_positions([0, genome.paths], 5)
    assert err.value.status == _lib.BAD_ARGUMENT
    # the device form: the same bytes in HBM
    import torch
    from gbwt_rs_amd import dist as D
    device = torch.device("cuda", 0)
    paths, positions = dev.path_positions_csr(order, 300)
    d_paths, d_positions, total = dev.path_positions_device(order, 301)
    d_paths, d_positions, total = dev.path_positions_device(order, 300)
    assert total == positions.size
    raw_paths = D.device_view(d_paths, len(order) * 32, torch.uint8, device).cpu().numpy()
    raw_positions = D.device_view(d_positions, total * 24, torch.uint8, device).cpu().numpy()
    assert raw_paths.tobytes() == paths.tobytes() and raw_positions.tobytes() == positions.tobytes()
    assert np.array_equal(paths["first"], np.concatenate([[0], np.cumsum(paths["count"])[:-1]]).astype(np.uint64))


def test_genome_positions_scanned_in_pieces(genome, monkeypatch):
    """The two scans of a request -- bases in front of every position, slots of the kept ones -- in pieces of 4 096 positions, on a workspace of
    its own (GBWT_HIP_SCAN_PIECE is read when a workspace is made): what only requests of more than 2^30 positions get otherwise.  Every piece
    is a launch, which the launch count shows."""
    dev = G.GBZ.load(genome.gbz)
    every = list(range(genome.paths))
    positions = sum(genome.nodes)
    assert positions > 8 * 4096
    monkeypatch.setenv("GBWT_HIP_SCAN_PIECE", "4096")
    pieces = dev.another_workspace()
    monkeypatch.delenv("GBWT_HIP_SCAN_PIECE")
    for interval in (0, 5000):
        want = expect(genome.starts, every, interval)
        assert R.same(dev.path_positions(every, interval), want), interval
        assert R.same(pieces.path_positions(every, interval), want), interval
        whole, cut = dev.last_positions_rounds()[1], pieces.last_positions_rounds()[1]
        assert cut > whole and cut - whole == 2 * (-(-positions // 4096) - 1), (interval, whole, cut)   # a launch more per further piece of either scan


class Tangle:
    def __init__(self, directory):
        self.gbz = os.path.join(directory, "tangle.gbz")
        self.label_lengths = T.tangle_label_lengths()
        self.paths, _ = T.tangle(lengths=self.label_lengths)
        S.Synth.from_paths(self.paths).attach_gbz(seed=3, label_lengths=self.label_lengths).save(self.gbz, as_gbz=True)
        self.lengths = np.concatenate([[0], self.label_lengths]).astype(np.int64)        # by node id
        gbwt = O.OracleGBZ(self.gbz).gbwt()
        self.starts = {p: R.node_starts(gbwt, p, self.lengths) for p in range(len(self.paths))}


@pytest.fixture(scope="module")
def tangle(tmp_path_factory):
    return Tangle(str(tmp_path_factory.mktemp("refpos_tangle")))


def test_tangle_orientations_revisits_and_long_labels(tangle, monkeypatch):
    dev = G.GBZ.load(tangle.gbz)
    n = len(tangle.paths)
    every = list(range(n))
    longest = n - 1
    walk = tangle.paths[longest]
    assert any(int(v) ^ 1 in set(walk.tolist()) for v in walk[:200])           # both orientations of a node on one path
    pos = tangle.starts[longest][2]
    visits = pos[pos[:, 0] == pos[5000, 0]]
    assert visits.shape[0] >= 2 and np.unique(visits[:, 1]).size == visits.shape[0]    # several visits of one record, each with its own offset
    assert [tangle.starts[p][2][:, 0].tolist() for p in every] == [q.tolist() for q in tangle.paths]
    offsets = tangle.starts[longest][1]
    exact = int(offsets[7])                                                    # lands exactly on the start of node 7: `>=`
    assert R.kept(offsets, exact)[:2].tolist() == [0, 7]
    for interval in (0, 16, 1000, exact, T.TANGLE_GIANT):
        got = dev.path_positions(every, interval)
        assert R.same(got, expect(tangle.starts, every, interval)), interval
    # without LF tables the O(1) step opens the records of more than two edges through their descriptors and decodes their bytes
    assert dev.stats.max_outdegree > 2
    monkeypatch.setenv("GBWT_HIP_TABLE_BYTES", "0")
    bare = G.GBZ.load(tangle.gbz)
    monkeypatch.delenv("GBWT_HIP_TABLE_BYTES")
    assert bare.memory_usage()["index_device_bytes"] < dev.memory_usage()["index_device_bytes"]
    for interval in (0, 1000):
        assert R.same(bare.path_positions(every, interval), expect(tangle.starts, every, interval)), interval
    kept = R.kept(offsets, 1000)
    assert np.any(np.diff(kept) == 1) and np.any(np.diff(kept) > 1)            # a label longer than several intervals: neighbours both kept
    # an empty path among the requested ones (the generator writes one into the GBZ): len 0, count 0
    assert len(tangle.paths[0]) == 0 and tangle.starts[0][0] == 0
    paths, positions = dev.path_positions_csr([3, 0, 0, longest, 0], 16)
    assert paths["len"][[1, 2, 4]].tolist() == [0, 0, 0] and paths["count"][[1, 2, 4]].tolist() == [0, 0, 0]
    assert R.same(dev.path_positions([0], 16), [(0, 0, np.zeros(0, np.uint64), np.zeros((0, 2), np.uint64))])
    # the reference paths of this file: path 0, of the generic sample, which is the empty one
    assert dev.reference_paths().tolist() == [0] and R.same(dev.reference_positions(4), expect(tangle.starts, [0], 4))


def test_base_offsets_past_four_gibibases(tmp_path):
    """One node of 4 194 299 bases visited 1 100 times: 4 MB of labels, a path of 4.6 G bases."""
    length, visits = 4194299, 1100
    middle = [T.fwd(2) if k % 3 else T.rev(2) for k in range(visits)]
    paths = [np.array([T.fwd(1)] + middle + [T.fwd(3)], dtype=np.uint64)]
    gbz = str(tmp_path / "long.gbz")
    S.Synth.from_paths(paths).attach_gbz(seed=5, label_lengths=np.array([1, length, 1], dtype=np.uint64)).save(gbz, as_gbz=True)
    assert os.path.getsize(gbz) < 8 << 20
    dev, gbwt = G.GBZ.load(gbz), O.OracleGBZ(gbz).gbwt()
    starts = {0: R.node_starts(gbwt, 0, np.array([0, 1, length, 1], dtype=np.int64))}
    assert starts[0][0] == visits * length + 2 > 2 ** 32 and int(starts[0][1][-1]) > 2 ** 32
    for interval in (2 ** 31, 0, length, 2 ** 32 + 5):
        got = dev.path_positions([0], interval)
        assert R.same(got, expect(starts, [0], interval)), interval
    got = dev.path_positions([0], 2 ** 31)[0]
    assert got[1] == 4613728902 and got[2].size == 3 and int(got[2][-1]) == 1 + 1026 * length > 2 ** 32
    assert R.kept(starts[0][1], length)[:3].tolist() == [0, 2, 3]              # 1 + 2 length >= (1 + length) + length: `>=`


def test_status_codes(genome, tmp_path):
    bare = G.GBWT.load(os.path.join(O.GOLDEN, "example.gbwt"))
    L = _lib.lib()
    n, total = C.c_uint64(7), C.c_uint64(7)
    assert L.gbwt_hip_reference_positions(bare._h, bare._ws, 5, None, 0, C.byref(n), None, 0, C.byref(total)) == _lib.UNSUPPORTED
    ids = np.zeros(1, dtype=np.uint64)
    assert L.gbwt_hip_path_positions(bare._h, bare._ws, ids.ctypes.data, 1, 5, None, None, 0, C.byref(total)) == _lib.UNSUPPORTED
    count = C.c_uint64(0)
    assert L.gbwt_hip_reference_paths(bare._h, 1, None, 0, C.byref(count)) == _lib.OK      # example.gbwt has metadata: host only
    for flags in (_lib.OPEN_EXTRACT, _lib.OPEN_SEARCH, _lib.OPEN_EXTRACT | _lib.OPEN_SEARCH):
        dev = G.GBZ.load(genome.gbz, flags=flags)
        with pytest.raises(G.GbwtHipError) as err:
            dev.reference_positions(5)
        assert err.value.status == _lib.BAD_ARGUMENT
        with pytest.raises(G.GbwtHipError) as err:
            dev.path_positions([0], 5)
        assert err.value.status == _lib.BAD_ARGUMENT
        assert dev.reference_paths().tolist() == genome.ref                    # (host only: whatever the flags)
    dev = G.GBZ.load(genome.gbz)
    with pytest.raises(G.GbwtHipError) as err:
        dev.last_positions_ms()
    assert err.value.status == _lib.BAD_ARGUMENT
    want = expect(genome.starts, genome.ref, 500)
    positions = sum(o.size for _, _, o, _ in want)
    out_paths = np.zeros(len(genome.ref), dtype=G.api.REFPATH_DTYPE)
    out = np.zeros(positions, dtype=G.api.REFPOS_DTYPE)
    st = L.gbwt_hip_reference_positions(dev._h, dev._ws, 500, out_paths.ctypes.data, out_paths.size, C.byref(n), out.ctypes.data, positions - 1, C.byref(total))
    assert st == _lib.CAPACITY and total.value == positions and n.value == len(genome.ref)
    st = L.gbwt_hip_reference_positions(dev._h, dev._ws, 500, out_paths.ctypes.data, out_paths.size - 1, C.byref(n), out.ctypes.data, positions, C.byref(total))
    assert st == _lib.CAPACITY and total.value == positions and n.value == len(genome.ref)
    ids = np.array(genome.ref, dtype=np.uint64)
    assert L.gbwt_hip_path_positions(dev._h, dev._ws, ids.ctypes.data, ids.size, 500, None, out.ctypes.data, positions - 1, C.byref(total)) == _lib.CAPACITY
    assert total.value == positions
    count = C.c_uint64(0)
    assert L.gbwt_hip_reference_paths(dev._h, 1, ids.ctypes.data, ids.size - 1, C.byref(count)) == _lib.CAPACITY and count.value == ids.size
    assert L.gbwt_hip_reference_positions(dev._h, dev._ws, 500, out_paths.ctypes.data, out_paths.size, C.byref(n), out.ctypes.data, positions, C.byref(total)) == _lib.OK
    assert R.same(dev._reference_rows(out_paths, out), want)
    walk_ms, select_ms, offsets_ms = dev.last_positions_ms()
    assert walk_ms > 0 and select_ms > 0 and offsets_ms > 0


def test_cpp_mirror_of_the_reference_test(tmp_path):
    """tests/cpp/test_reference_positions.cpp: src/gbz/tests.rs:521-567 restated against include/gbwt_hip.hpp."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "test_reference_positions"
    csrc = os.path.join(root, "gbwt_rs_amd", "csrc")
    subprocess.run([shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "include"), "-o", str(exe),
                    os.path.join(root, "tests", "cpp", "test_reference_positions.cpp"), "-L", csrc, "-lgbwt_hip", "-Wl,-rpath," + csrc], check=True)
    out = subprocess.run([str(exe), O.GOLDEN], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
