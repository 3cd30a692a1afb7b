"""Weakly connected components (GBZ::weakly_connected_components, src/gbz.rs:570-598) and gbz-extract's contig path selection
(select_paths, src/bin/gbz-extract.rs:196-264) through the device, against the reference's own known answer, against answers written out
here, and against tests/components_expect.py: a union-find over the CPU oracle's records, and select_paths restated in Python."""
import ctypes as C
import os
import struct
import threading

import numpy as np
import pytest

import components_expect as X
import gbwt_rs_amd as G
import oracle_lib as O
import seq_expect as E
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S

pytestmark = pytest.mark.gpu

GBZ_FIXTURES = ["example.gbz", "example-v1.gbz", "translation.gbz", "translation-v1.gbz"]
GBWT_FIXTURES = ["example.gbwt", "translation.gbwt", "with-empty.gbwt"]
EXAMPLE = [[11, 12, 13, 14, 15, 16, 17], [21, 22, 23, 24, 25]]            # src/gbz/tests.rs:508-511
OPEN_FLAGS = [_lib.OPEN_EXTRACT, _lib.OPEN_SEARCH, _lib.OPEN_GFA, _lib.OPEN_ALL]


def as_lists(components):
    return [[int(x) for x in c] for c in components]


def oracle_gbwt(path):
    return O.OracleGBZ(path).gbwt() if path.endswith(".gbz") else O.OracleGBWT.load(path)


def check_against_helper(dev, gbwt):
    """Components, their CSR, the device view's counts and the component of every path against the helper."""
    want = X.components(gbwt)
    assert as_lists(dev.weakly_connected_components()) == want
    offsets, ids = dev.components_csr()
    assert offsets.tolist() == np.cumsum([0] + [len(c) for c in want]).tolist() and ids.tolist() == [n for c in want for n in c]
    view = dev.components_device()
    min_node, slots = X.geometry(gbwt)
    assert (view.min_node, view.slots, view.components, view.nodes) == (min_node, slots, len(want), sum(len(c) for c in want))
    stride = 2 if gbwt.is_bidirectional() else 1
    paths = gbwt.sequences() // stride
    assert view.paths == paths
    got = dev.path_components(np.arange(paths))
    assert got.dtype == np.uint32 and got.tolist() == X.path_components(want, X.first_nodes(gbwt, paths, stride))
    return want


def test_example_gbz_against_the_reference_vector():
    dev = G.GBZ.load(os.path.join(O.GOLDEN, "example.gbz"))
    assert as_lists(dev.weakly_connected_components()) == EXAMPLE
    offsets, ids = dev.components_csr()
    assert offsets.tolist() == [0, 7, 12] and ids.dtype == np.uint64 and ids.tolist() == EXAMPLE[0] + EXAMPLE[1]
    view = dev.components_device()
    assert (view.min_node, view.slots, view.components, view.nodes, view.paths) == (11, 15, 2, 12, 6)
    # P-line A starts at 11, P-line B at 21 (tests/golden/example.gfa); every walk of sample#1/#2 on A or B
    assert dev.path_components([0, 1]).tolist() == [0, 1]
    t = dev.last_components_ms()
    assert t["hook_launches"] >= 2 and t["jump_launches"] >= 1 and t["shape_launches"] >= 1 and t["hook_ms"] > 0 and t["jump_ms"] > 0 and t["shape_ms"] > 0


@pytest.mark.parametrize("name", GBZ_FIXTURES + GBWT_FIXTURES)
def test_fixtures_against_the_helper(name):
    path = os.path.join(O.GOLDEN, name)
    dev = (G.GBZ if name.endswith(".gbz") else G.GBWT).load(path)
    want = check_against_helper(dev, oracle_gbwt(path))
    assert len(want) == (1 if name.startswith("translation") else 2)      # translation.gfa is one connected graph
    if name.startswith("example"):
        assert want == EXAMPLE


def test_empty_path_has_no_component():
    path = os.path.join(O.GOLDEN, "with-empty.gbwt")
    dev, gbwt = G.GBWT.load(path), O.OracleGBWT.load(path)
    paths = gbwt.sequences() // 2
    empty = [p for p in range(paths) if gbwt.sequence(2 * p) == []]
    assert empty == [4]                                                     # tests/golden/with-empty.txt
    got = dev.path_components(np.arange(paths))
    assert int(got[4]) == 0xFFFFFFFF == X.NONE and (np.delete(got, 4) < 2).all()
    with pytest.raises(G.GbwtHipError) as e:
        dev.path_components([paths])
    assert e.value.status == _lib.BAD_ARGUMENT
    with pytest.raises(ValueError):
        dev.path_components([[0, 1]])


def genome(tmp_path, name="genome.gbz", **kw):
    path = str(tmp_path / name)
    g = S.Synth.genome(**kw)
    g.save(path, as_gbz=True)
    return path, g


@pytest.mark.parametrize("flags", OPEN_FLAGS)
def test_every_open_group_answers(tmp_path, flags):
    """Record bytes, starts and the endmarker are on every handle: the components do not depend on what it was opened for -- the lean
    extraction handle, which has given its raw descriptors back, included."""
    dev = G.GBZ.load(os.path.join(O.GOLDEN, "example.gbz"), flags=flags)
    assert as_lists(dev.weakly_connected_components()) == EXAMPLE
    path, g = genome(tmp_path, contigs=3, fragments=2, haplotypes=8, sites=25, seed=11)
    dev = G.GBZ.load(path, flags=flags)
    want = check_against_helper(dev, O.OracleGBZ(path).gbwt())
    assert len(want) == 6
    s = S.Synth.chain(sites=40, haplotypes=6, seed=2)
    bare = G.GBWT.from_records(s.data(), s.starts(), s.alphabet_offset, s.alphabet_size, s.sequences, s.size, True, flags=flags)
    assert len(bare.weakly_connected_components()) == 1


def fwd(n):
    return 2 * n


def rev(n):
    return 2 * n + 1


TOPOLOGIES = {
    # name: (paths of GBWT-encoded nodes, expected components)
    "cycle": ([[fwd(1), fwd(2), fwd(3), fwd(1), fwd(2)], [fwd(4), fwd(5)]], [[1, 2, 3], [4, 5]]),
    "self-loop": ([[fwd(1), fwd(1), fwd(1), fwd(2)], [fwd(3)], [fwd(4), fwd(4)]], [[1, 2], [3], [4]]),
    "hairpin": ([[fwd(1), fwd(2), rev(2), rev(1)], [fwd(3), fwd(4)]], [[1, 2], [3, 4]]),
    # 1-2-3 and 4-5-6 meet only in the edge 3+ -> 6- (read backwards: 6+ -> 3-)
    "joined-through-a-reverse-edge": ([[fwd(1), fwd(2), fwd(3)], [fwd(4), fwd(5), fwd(6)], [fwd(3), rev(6)], [fwd(7), fwd(8)]], [[1, 2, 3, 4, 5, 6], [7, 8]]),
    "gaps": ([[fwd(1), fwd(2), fwd(5)], [fwd(7), fwd(9)], [fwd(12)]], [[1, 2, 5], [7, 9], [12]]),
    "outdegree-5": ([[fwd(1), fwd(k)] for k in (2, 3, 4, 5, 6)] + [[fwd(8), fwd(9)]], [[1, 2, 3, 4, 5, 6], [8, 9]]),
    "isolated-node": ([[fwd(1), fwd(2)], [fwd(3)], [fwd(4), fwd(5)], [rev(6)]], [[1, 2], [3], [4, 5], [6]]),
    # components that only close over several rounds: a long chain whose ids run against the path, and a star around the LARGEST id
    "descending-chain": ([[fwd(k) for k in range(300, 0, -1)], [fwd(301), fwd(302)]], [list(range(1, 301)), [301, 302]]),
    "star-around-the-largest": ([[fwd(k), fwd(40)] for k in range(1, 40)] + [[fwd(41)]], [list(range(1, 41)), [41]]),
    "interleaved": ([[fwd(1), fwd(3), fwd(5), fwd(7)], [fwd(2), fwd(4), fwd(6), fwd(8)], [rev(7), fwd(9)]], [[1, 3, 5, 7, 9], [2, 4, 6, 8]]),
}


@pytest.mark.parametrize("name", sorted(TOPOLOGIES))
def test_topologies_written_out(tmp_path, name):
    paths, want = TOPOLOGIES[name]
    s = S.Synth.from_paths(paths, bidirectional=True).attach_gbz(seed=3)
    path = str(tmp_path / "topology.gbz")
    s.save(path, as_gbz=True)
    gbwt = O.OracleGBZ(path).gbwt()
    assert X.components(gbwt) == want
    if name == "outdegree-5":
        assert gbwt.bwt().record(fwd(1) - gbwt.alphabet_offset()).outdegree == 5
    dev = G.GBZ.load(path)
    assert as_lists(dev.weakly_connected_components()) == want
    check_against_helper(dev, gbwt)
    lean = G.GBZ.load(path, flags=_lib.OPEN_EXTRACT)
    assert as_lists(lean.weakly_connected_components()) == want
    bare = G.GBWT.from_records(s.data(), s.starts(), s.alphabet_offset, s.alphabet_size, s.sequences, s.size, True)
    assert as_lists(bare.weakly_connected_components()) == want
    where = {n: c for c, nodes in enumerate(want) for n in nodes}
    assert dev.path_components(np.arange(len(paths))).tolist() == [where[p[0] // 2] for p in paths]


def test_genome_components_are_contigs_times_fragments(tmp_path):
    path, g = genome(tmp_path, contigs=5, fragments=4, haplotypes=12, sites=30, seed=6, labels=1)
    dev = G.GBZ.load(path)
    want = check_against_helper(dev, O.OracleGBZ(path).gbwt())
    assert len(want) == 20 == dev.components_device().components
    assert len(set(dev.path_components(np.arange(dev.paths())).tolist())) == 20
    # a unidirectional index of forward nodes only: half of the records are empty, the nodes are the same
    s = S.Synth.from_paths([[fwd(1), fwd(2), fwd(3)], [fwd(5), fwd(6)], [fwd(2), fwd(4)]], bidirectional=False)
    uni = G.GBWT.from_records(s.data(), s.starts(), s.alphabet_offset, s.alphabet_size, s.sequences, s.size, False)
    bwt = O.OracleBWT.from_parts(bytes(s.data()), s.starts())
    gbwt = O.OracleGBWT.from_bwt(bwt, s.sequences, s.size, s.alphabet_offset, s.alphabet_size, False)
    assert check_against_helper(uni, gbwt) == [[1, 2, 3, 4], [5, 6]]


# ---- select_paths ---------------------------------------------------------------------------------------------------------------------

CONTIGS = ["chr1", "chr2", "chr3", "unplaced", "chrEmpty"]


def merged_with_unplaced(tmp_path, contig_names=CONTIGS, name="merged.gbz"):
    """Five components of four haplotypes each: chr1 owns two of them (one with an unplaced walker), chr2 one (with an unplaced walker),
    chr3 one, and one belongs to unplaced walkers alone.  chrEmpty is a contig name no path carries."""
    layout = [[0, 0, 0, 3], [0, 0, 0, 0], [1, 3, 1, 1], [2, 2, 2, 2], [3, 3, 3, 3]]      # contig id of every walker of every part
    parts = [S.Synth.chain(sites=12 + 3 * k, haplotypes=4, seed=20 + k) for k in range(len(layout))]
    names = [(h // 2, contig, h % 2 + 1, 0) for part in layout for h, contig in enumerate(part)]
    merged = S.Synth.merge(parts, names, ["s0", "s1"], contig_names, 4)
    path = str(tmp_path / name)
    merged.save(path, as_gbz=True)
    return path, [contig for part in layout for contig in part]


def test_select_paths_takes_whole_components(tmp_path):
    path, contigs = merged_with_unplaced(tmp_path)
    dev, gbwt = G.GBZ.load(path), O.OracleGBZ(path).gbwt()
    comps = check_against_helper(dev, gbwt)
    assert len(comps) == 5 and dev.paths() == 20
    firsts = X.first_nodes(gbwt, 20)
    for contig in (None, "chr1", "chr2", "chr3", "unplaced"):
        got = dev.select_paths(contig)
        assert got.dtype == np.uint64 and got.tolist() == X.select_paths(comps, firsts, contigs, CONTIGS, contig), contig
    assert dev.select_paths().tolist() == list(range(20))
    assert dev.select_paths("chr1").tolist() == list(range(0, 8))              # the unplaced walker 3 of chr1's first component comes along
    assert dev.select_paths("chr2").tolist() == list(range(8, 12))
    assert dev.select_paths("unplaced").tolist() == list(range(0, 4)) + list(range(8, 12)) + list(range(16, 20))
    assert dev.select_paths(b"chr3").tolist() == list(range(12, 16))
    # the C idiom: size query, too small, fill
    total = C.c_uint64(0)
    assert dev._L.gbwt_hip_select_paths(dev._h, dev._ws, b"chr1", None, 0, C.byref(total)) == _lib.OK and total.value == 8
    out = np.zeros(8, dtype=np.uint64)
    assert dev._L.gbwt_hip_select_paths(dev._h, dev._ws, b"chr1", out.ctypes.data, 7, C.byref(total)) == _lib.CAPACITY and total.value == 8
    assert dev._L.gbwt_hip_select_paths(dev._h, dev._ws, b"chr1", out.ctypes.data, 8, C.byref(total)) == _lib.OK and out.tolist() == list(range(8))
    with pytest.raises(TypeError):
        dev.select_paths(7)


def test_select_paths_errors(tmp_path):
    path, _ = merged_with_unplaced(tmp_path)
    dev = G.GBZ.load(path)
    for contig, message in (("chr9", "The graph does not contain contig chr9"), ("chrEmpty", "The graph does not contain any paths for contig chrEmpty")):
        with pytest.raises(G.GbwtHipError) as e:
            dev.select_paths(contig)
        assert e.value.status == _lib.BAD_ARGUMENT and message in str(e.value)
    # the same index without contig names: no names in the dictionary, and the flag of the metadata header (the fifth word behind its tag,
    # Metadata, src/gbwt.rs:623-640) cleared in the file
    nameless, _ = merged_with_unplaced(tmp_path, contig_names=[], name="nameless.gbz")
    raw = bytearray(open(nameless, "rb").read())
    at = raw.find(struct.pack("<Q", 0x6B375E7A | (2 << 32)))
    assert at > 0 and struct.unpack_from("<Q", raw, at + 32)[0] == 7
    struct.pack_into("<Q", raw, at + 32, 3)
    open(nameless, "wb").write(bytes(raw))
    dev = G.GBZ.load(nameless, flags=_lib.OPEN_EXTRACT)
    assert dev.select_paths().tolist() == list(range(20))
    with pytest.raises(G.GbwtHipError) as e:
        dev.select_paths("chr1")
    assert e.value.status == _lib.BAD_ARGUMENT and "Cannot select a contig without contig names" in str(e.value)
    # an index without metadata
    s = S.Synth.chain(sites=10, haplotypes=4, seed=1)
    bare = G.GBZ.from_records(s.data(), s.starts(), s.alphabet_offset, s.alphabet_size, s.sequences, s.size, True)
    for contig in (None, "chr1"):
        with pytest.raises(G.GbwtHipError) as e:
            bare.select_paths(contig)
        assert e.value.status == _lib.BAD_ARGUMENT and str(e.value)
    assert len(bare.weakly_connected_components()) == 1                      # (the components themselves need no metadata)


def test_write_sequences_of_a_contig(tmp_path):
    path, _ = merged_with_unplaced(tmp_path)
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    table = E.LabelTable.from_gfa(oracle.gfa())
    for contig, endmarker in (("chr1", 0), ("unplaced", ord("$")), ("chr3", None)):
        ids = dev.select_paths(contig)
        a, b = tmp_path / f"{contig}.contig", tmp_path / f"{contig}.ids"
        dev.write_sequences(str(a), contig=contig, endmarker=endmarker)
        dev.write_sequences(str(b), path_ids=ids, endmarker=endmarker)
        assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > len(ids)
        assert a.with_name(a.name + ".names").read_bytes() == b.with_name(b.name + ".names").read_bytes()
        seq_ids = [2 * int(p) for p in ids]
        rows = E.node_rows(oracle.gbwt().extract(np.array(seq_ids, dtype=np.uint64)), seq_ids, 2 * dev.paths())
        assert a.read_bytes() == E.expected_rows(table, rows, endmarker)[1]
        assert [line.split("\t")[0] for line in a.with_name(a.name + ".names").read_text().splitlines()] == [str(int(p)) for p in ids]
    # the call forms of before: everything, and a list of ids
    dev.write_sequences(str(tmp_path / "all"))
    dev.write_sequences(str(tmp_path / "all.ids"), np.arange(dev.paths()))
    assert (tmp_path / "all").read_bytes() == (tmp_path / "all.ids").read_bytes()
    with pytest.raises(ValueError):
        dev.write_sequences(str(tmp_path / "both"), path_ids=[0], contig="chr1")
    with pytest.raises(G.GbwtHipError) as e:
        dev.write_sequences(str(tmp_path / "bad"), contig="chr9")
    assert e.value.status == _lib.BAD_ARGUMENT
    gbwt = G.GBWT.load(os.path.join(O.GOLDEN, "example.gbwt"))            # no node labels: nothing to write
    assert gbwt._L.gbwt_hip_write_sequences_contig(gbwt._h, gbwt._ws, os.fsencode(str(tmp_path / "bare")), b"A", 0) == _lib.BAD_ARGUMENT


# ---- laziness and accounting ------------------------------------------------------------------------------------------------------------

def test_components_made_once_on_first_call(tmp_path):
    path, g = genome(tmp_path, contigs=4, fragments=3, haplotypes=16, sites=30, seed=4)
    dev = G.GBZ.load(path)
    other = dev.another_workspace()
    times = _lib.ComponentsTimes()
    assert dev._L.gbwt_hip_last_components_ms(dev._h, C.byref(times)) == _lib.BAD_ARGUMENT       # an open never makes them
    before = dev.memory_usage()["index_device_bytes"]
    results, views, errors = [None, None], [None, None], []
    barrier = threading.Barrier(2)

    def ask(k, handle):
        try:
            barrier.wait()
            results[k] = handle.components_csr()
            views[k] = handle.components_device()
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append(e)

    threads = [threading.Thread(target=ask, args=(0, dev)), threading.Thread(target=ask, args=(1, other))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    fields = [name for name, _ in _lib.Components._fields_]
    assert [getattr(views[0], f) for f in fields] == [getattr(views[1], f) for f in fields]     # the same arrays, not two builds
    assert as_lists(dev.weakly_connected_components()) == X.components(O.OracleGBZ(path).gbwt())
    after = dev.memory_usage()["index_device_bytes"]
    slots = views[0].slots
    assert slots == g.alphabet_size // 2 - 1
    assert after - before >= 4 * slots + 4 * views[0].nodes + 8 * (views[0].components + 1)
    assert after - before < 16 * slots + (1 << 16)                              # (the scratch of the build is not kept)
    launches = dev.last_components_ms()
    dev.weakly_connected_components(); dev.path_components([0]); dev.select_paths("chr1"); other.components_device()
    assert dev.memory_usage()["index_device_bytes"] == after and dev.last_components_ms() == launches
