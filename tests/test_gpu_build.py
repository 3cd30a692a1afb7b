"""GBWT construction on the device against the host builders: gbwt_rs_amd.synth's brute-force reverse-prefix sort (Synth.from_paths, pinned
byte for byte on the reference's fixtures by tests/test_synth.py) and, as a second and independent witness, its PBWT-sweep chain generator.
Every comparison is exact: the record stream, the record starts and the header fields."""
import os
import random

import numpy as np
import pytest

import gbwt_rs_amd as G
import kat
import locate_expect as LX
import oracle_lib as O
import tangled_graphs as TG
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S
from test_synth import random_paths

pytestmark = pytest.mark.gpu


def header(x):
    if isinstance(x, S.Synth):
        return x.sequences, x.size, x.alphabet_offset, x.alphabet_size, x.bidirectional
    return x.sequences(), x.len(), x.alphabet_offset(), x.alphabet_size(), x.is_bidirectional()


def assert_same_index(dev, data, starts, hdr):
    got_data, got_starts = dev.records()
    assert got_data.dtype == np.uint8 and got_starts.dtype == np.uint64
    assert np.array_equal(got_starts, np.asarray(starts, dtype=np.uint64))
    assert bytes(got_data) == bytes(data)
    assert header(dev) == tuple(hdr)


def build_and_check(paths, bidirectional=True):
    """The device's index of the paths equals the brute-force builder's; returns (device handle, witness)."""
    witness = S.Synth.from_paths(paths, bidirectional=bidirectional)
    dev = G.GBWT.from_paths(paths, bidirectional=bidirectional)
    assert_same_index(dev, witness.data(), witness.starts(), header(witness))
    return dev, witness


def rounds_bound(paths):
    longest = max((len(p) for p in paths), default=0)
    return int(np.ceil(np.log2(longest + 1)))


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,with_empty", [("example.gbwt", False), ("with-empty.gbwt", True)])
def test_fixture_records(name, with_empty):
    ref = O.OracleGBWT.load(os.path.join(O.GOLDEN, name))
    dev, _ = build_and_check(kat.true_paths(with_empty))
    assert_same_index(dev, ref.bwt().data(), ref.bwt().starts(), (ref.sequences(), ref.len(), ref.alphabet_offset(), ref.alphabet_size(), True))


def test_translation_records():
    dev, _ = build_and_check([[2 * x for x in p] for p in kat.TRANSLATION_PATHS])
    data, starts = dev.records()
    assert bytes(data).hex() == kat.TRANSLATION_DATA_HEX
    assert list(starts) == kat.TRANSLATION_STARTS


# ---- 2. the smallest shapes at which each stage can go wrong ---------------------------------------------------------------------------------

@pytest.mark.parametrize("length", [300, 4096])
def test_one_long_run(length):
    """One node visited `length` times in a row: a run with a multi-byte tail, and as many doubling rounds as a path of that length can need."""
    paths = [[2] * length]
    dev, _ = build_and_check(paths)
    info = dev.last_build_info()
    assert (length, info["rounds"]) in ((300, 9), (4096, 12)) and info["rounds"] <= rounds_bound(paths)


def test_ties_down_to_the_sequence_id():
    build_and_check([[2, 4, 6, 8, 10] * 8] * 200)


def test_path_that_is_its_own_reverse():
    build_and_check([[2, 3], [4, 6, 7, 5]])


def test_empty_records_and_long_deltas():
    dev, _ = build_and_check([[2, 2 * 100001, 2 * 100001 + 1, 2]])
    assert dev.stats.records == 200003                # nodes 2 .. 200003 and the endmarker; four of them are visited


@pytest.mark.parametrize("k", [128, 129, 254, 255, 256, 300])
def test_hub_outdegrees_around_the_run_encodings(k):
    """Node 2 has k successors; the endmarker one more: node 2 and the k flipped ends, where the reverse sequences start."""
    dev, _ = build_and_check([[2, 2 * (2 + i)] for i in range(k) for _ in range(2)])
    assert dev.stats.max_outdegree == k + 1


def test_unidirectional():
    build_and_check([[2, 4, 2, 4, 2, 6]], bidirectional=False)


@pytest.mark.parametrize("paths", [[[], []], []], ids=["empty-paths", "no-paths"])
@pytest.mark.parametrize("bidirectional", [True, False])
def test_sets_without_visits(paths, bidirectional):
    dev, witness = build_and_check(paths, bidirectional)
    assert (dev.alphabet_offset(), dev.alphabet_size(), dev.stats.records) == (0, 1, 1)
    assert dev.last_build_info()["built"] == 1 and dev.last_build_info()["visits"] == 0


@pytest.mark.parametrize("seed,cyclic", [(1, False), (2, True), (3, True), (4, False)])
def test_random_paths(seed, cyclic):
    rng = random.Random(seed)
    paths = random_paths(rng, n_paths=12, n_nodes=9, max_len=14, cyclic=cyclic)
    if not any(paths):
        paths[0] = [2, 4]
    build_and_check(paths)


# ---- 3. the tangled graphs, at reduced sizes ---------------------------------------------------------------------------------------------------

TANGLED = {
    "permuted-path": lambda: TG.permuted_path(20000),
    "zigzag": lambda: TG.zigzag(20000),
    "interleaved": lambda: TG.interleaved(20000),
    "reverse-joins": lambda: TG.reverse_joins(20000),
    "permuted-path-unidirectional": lambda: TG.permuted_path_unidirectional(20000),
    "tree-with-hub": lambda: TG.tree_with_hub(n=20000, hub_edges=2000, leaves=1000),
    "grid": lambda: TG.grid(60, 60),
}


@pytest.mark.parametrize("name", sorted(TANGLED))
def test_tangled_graphs(name):
    paths, bidirectional = TANGLED[name]()
    build_and_check(paths, bidirectional)


# ---- 4. the sweep generator as a second witness --------------------------------------------------------------------------------------------------

def assert_chain(s):
    paths = [s.path(h) for h in range(s.paths)]
    dev = G.GBWT.from_paths(paths, bidirectional=True)
    assert_same_index(dev, s.data(), s.starts(), header(s))
    return dev


@pytest.mark.parametrize("sites,haplotypes,alleles,model", [(2000, 500, 2, S.MOSAIC), (300, 100, 5, S.MOSAIC), (300, 100, 300, S.IID)])
def test_chain_generator(sites, haplotypes, alleles, model):
    dev = assert_chain(S.Synth.chain(sites=sites, haplotypes=haplotypes, alleles=alleles, model=model))
    info = dev.last_build_info()
    assert info["visits"] == 2 * 2 * sites * haplotypes and info["rounds"] <= int(np.ceil(np.log2(2 * sites + 1)))


@pytest.mark.parametrize("alleles,model,extra,every", [(2, S.MOSAIC, 1, 1), (2, S.IID, 3, 1), (5, S.MOSAIC, 2, 1), (40, S.IID, 1, 1),
                                                       (2, S.MOSAIC, 2, 3), (4, S.IID, 1, 4), (2, S.IID, 1, 9)])
def test_indel_chain(alleles, model, extra, every):
    assert_chain(S.Synth.chain(sites=9, haplotypes=21, alleles=alleles, model=model, founders=4, switch_rate=0.2, seed=8, extra=extra, indel_every=every))


@pytest.mark.parametrize("alleles,model,extra,every,chop", [(2, S.MOSAIC, 0, 1, 2), (2, S.IID, 1, 1, 3), (3, S.MOSAIC, 2, 2, 2), (5, S.IID, 0, 1, 4),
                                                            (2, S.MOSAIC, 1, 5, 5)])
def test_chopped_chain(alleles, model, extra, every, chop):
    assert_chain(S.Synth.chain(sites=7, haplotypes=19, alleles=alleles, model=model, founders=4, switch_rate=0.2, seed=12, extra=extra, indel_every=every, chop=chop))


# ---- 5. the handle works -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built():
    rng = random.Random(3)
    paths = random_paths(rng, n_paths=12, n_nodes=9, max_len=14, cyclic=True)
    dev, witness = build_and_check(paths)
    oracle = O.OracleGBWT.from_bwt(O.OracleBWT.from_parts(bytes(witness.data()), witness.starts()), witness.sequences, witness.size, witness.alphabet_offset,
                                   witness.alphabet_size, True)
    return paths, dev, oracle


def test_built_handle_extracts_its_input(built):
    paths, dev, _ = built
    offsets, nodes = dev.sequences_csr(np.arange(dev.sequences(), dtype=np.uint64))
    assert dev.sequences() == 2 * len(paths)
    for k, p in enumerate(paths):
        assert nodes[int(offsets[2 * k]):int(offsets[2 * k + 1])].tolist() == list(p)
        assert nodes[int(offsets[2 * k + 1]):int(offsets[2 * k + 2])].tolist() == kat.reverse_path(list(p))


def test_built_handle_finds_and_locates(built):
    paths, dev, oracle = built
    node = next(p[0] for p in paths if len(p))
    states, valid = dev.find([node])
    assert valid[0] and tuple(int(x) for x in states[0]) == oracle.find(node)
    assert dev.locate(states[0], unique=True).tolist() == LX.row(LX.owners(oracle), states[0], True)


def test_build_info(built):
    paths, dev, _ = built
    info = dev.last_build_info()
    visits = 2 * sum(len(p) for p in paths)
    assert (info["built"], info["visits"], info["sequences"], info["records"]) == (1, visits, 2 * len(paths), dev.stats.records)
    assert info["data_bytes"] == dev.stats.data_bytes and info["peak_scratch_bytes"] > 0
    assert 1 <= info["rounds"] <= rounds_bound(paths)
    assert min(info["expand_ms"], info["rank_ms"], info["edges_ms"], info["encode_ms"], info["open_ms"]) > 0
    loaded = G.GBWT.load(os.path.join(O.GOLDEN, "example.gbwt"))
    assert set(loaded.last_build_info().values()) == {0}             # a handle that was not built


def test_same_input_same_bytes():
    paths, bidirectional = TG.grid(60, 60)
    first, second = G.GBWT.from_paths(paths, bidirectional), G.GBWT.from_paths(paths, bidirectional)
    (d1, s1), (d2, s2) = first.records(), second.records()
    assert bytes(d1) == bytes(d2) and np.array_equal(s1, s2)


# ---- 6. composition: extracted rows become an index -----------------------------------------------------------------------------------------------

def test_extracted_rows_become_the_index_they_came_from():
    path = os.path.join(O.GOLDEN, "example.gbwt")
    ref = O.OracleGBWT.load(path)
    loaded = G.GBWT.load(path)
    even = np.arange(0, loaded.sequences(), 2, dtype=np.uint64)
    rows = loaded.extract_device(even)
    dev = G.GBWT.from_rows_device(rows, even.size, bidirectional=True)
    assert_same_index(dev, ref.bwt().data(), ref.bwt().starts(), (ref.sequences(), ref.len(), ref.alphabet_offset(), ref.alphabet_size(), True))
    offsets, nodes = loaded.sequences_csr(even)                       # the rows were only read
    assert [nodes[int(a):int(b)].tolist() for a, b in zip(offsets[:-1], offsets[1:])] == kat.true_paths(False)


# ---- 7. save -----------------------------------------------------------------------------------------------------------------------------

def test_saved_index_loads_in_the_oracle(tmp_path):
    dev, witness = build_and_check(kat.true_paths(True))
    out = tmp_path / "built.gbwt"
    dev.save(str(out))
    ref = O.OracleGBWT.load(str(out))
    assert ref.bwt().data() == bytes(witness.data()) and ref.bwt().starts() == list(witness.starts())
    assert (ref.sequences(), ref.len(), ref.alphabet_offset(), ref.alphabet_size()) == header(witness)[:4]


@pytest.mark.parametrize("name,cls", [("example.gbwt", G.GBWT), ("example-v1.gbz", G.GBZ)])
def test_loaded_file_is_saved_unchanged(tmp_path, name, cls):
    src = os.path.join(O.GOLDEN, name)
    out = tmp_path / name
    cls.load(src).save(str(out))
    assert out.read_bytes() == open(src, "rb").read()
