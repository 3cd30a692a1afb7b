"""GBWT / GBZ merging on the device against the host builder over the concatenated paths (Synth.from_paths, pinned on the reference's
fixtures by tests/test_synth.py).  Every comparison is exact: the record stream, the record starts and the header fields.  The recurrence
itself is held against the same builder, step by step, in tests/test_merge_cpu.py."""
import os
import random

import numpy as np
import pytest

import gbwt_rs_amd as G
import kat
import merge_expect as MX
import oracle_lib as O
import tangled_graphs as TG
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S
from test_synth import random_paths

pytestmark = pytest.mark.gpu

EXAMPLE_GFA = os.path.join(O.GOLDEN, "example.gfa")
TRANSLATION_GFA = os.path.join(O.GOLDEN, "translation.gfa")


def header(x):
    if isinstance(x, S.Synth):
        return x.sequences, x.size, x.alphabet_offset, x.alphabet_size, x.bidirectional
    return x.sequences(), x.len(), x.alphabet_offset(), x.alphabet_size(), x.is_bidirectional()


def assert_same_index(dev, data, starts, hdr):
    got_data, got_starts = dev.records()
    assert np.array_equal(got_starts, np.asarray(starts, dtype=np.uint64))
    assert bytes(got_data) == bytes(data)
    assert header(dev) == tuple(hdr)


def merge_and_check(paths_a, paths_b, algorithm="insert", bidirectional=True, flags=_lib.OPEN_ALL):
    """The device's merge of the two indexes equals the brute-force builder's index of all paths; returns (merged, a, b, witness).  The
    insertion is asked for by name where the inputs are bidirectional: AUTO takes the rebuild for handles that are open for extraction."""
    if algorithm == "insert":
        algorithm = G.MERGE_INSERT if bidirectional else None
    witness = S.Synth.from_paths(list(paths_a) + list(paths_b), bidirectional=bidirectional)
    a = G.GBWT.from_paths(paths_a, bidirectional=bidirectional, flags=flags)
    b = G.GBWT.from_paths(paths_b, bidirectional=bidirectional, flags=flags)
    merged = G.GBWT.merge(a, b, algorithm=algorithm)
    assert_same_index(merged, witness.data(), witness.starts(), header(witness))
    return merged, a, b, witness


# ---- 1. the reference's fixtures, split at every index -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,with_empty", [("example.gbwt", False), ("with-empty.gbwt", True)])
def test_fixtures_split_at_every_index(name, with_empty):
    ref = O.OracleGBWT.load(os.path.join(O.GOLDEN, name))
    paths = kat.true_paths(with_empty)
    for k in range(len(paths) + 1):
        merged, _, _, _ = merge_and_check(paths[:k], paths[k:])
        assert_same_index(merged, ref.bwt().data(), ref.bwt().starts(), (ref.sequences(), ref.len(), ref.alphabet_offset(), ref.alphabet_size(), True))


# ---- 2. the smallest shapes at which each stage can go wrong ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [name for name, _, _ in MX.special_pairs()])
def test_special_shapes(name):
    _, pa, pb = next(p for p in MX.special_pairs() if p[0] == name)
    merged, _, _, _ = merge_and_check(pa, pb)
    if name.startswith("long-deltas"):
        assert merged.stats.records == 200003


@pytest.mark.parametrize("k", [128, 129, 254, 255, 256, 300])
def test_hubs_around_the_run_encodings(k):
    merged, _, _, _ = merge_and_check(*MX.hub_pair(k))
    assert merged.stats.max_outdegree == k + 1


@pytest.mark.parametrize("pa,pb", [([], []), ([[]], []), ([], [[], []]), ([[2, 4]], []), ([], [[2, 4]]), ([[]], [[2, 5]]), ([[3, 2]], [[], []])])
def test_sets_without_visits(pa, pb):
    merged, a, b, _ = merge_and_check(pa, pb)
    assert merged.sequences() == a.sequences() + b.sequences()
    assert merged.last_merge_info()["merged"] == 1


RANDOM = [(seed, seed % 2 == 1) for seed in range(20)]


def random_pair(seed, cyclic):
    rng = random.Random(seed)
    paths = random_paths(rng, n_paths=12, n_nodes=9, max_len=14, cyclic=cyclic)
    k = rng.randrange(len(paths) + 1)
    return paths[:k], paths[k:]


@pytest.mark.parametrize("seed,cyclic", RANDOM)
def test_random_pairs(seed, cyclic):
    pa, pb = random_pair(seed, cyclic)
    merged, _, _, witness = merge_and_check(pa, pb)
    rebuilt = G.GBWT.merge(G.GBWT.from_paths(pa), G.GBWT.from_paths(pb), algorithm=G.MERGE_REBUILD)       # rebuild equals insertion
    assert_same_index(rebuilt, witness.data(), witness.starts(), header(witness))
    assert rebuilt.last_merge_info()["algorithm_used"] == G.MERGE_REBUILD and merged.last_merge_info()["algorithm_used"] == G.MERGE_INSERT


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
def test_tangled_graphs_split_by_path_parity(name):
    paths, bidirectional = TANGLED[name]()
    merged, _, _, _ = merge_and_check(paths[0::2], paths[1::2], bidirectional=bidirectional)
    assert merged.last_merge_info()["algorithm_used"] == (G.MERGE_INSERT if bidirectional else G.MERGE_REBUILD)


# ---- 3. a chain ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain():
    s = S.Synth.chain(sites=2000, haplotypes=64)
    return s, [s.path(h) for h in range(s.paths)]


@pytest.mark.parametrize("cut,walked", [(32, 1), (62, 1), (2, 0)])
def test_chain(chain, cut, walked):
    s, paths = chain
    a, b = G.GBWT.from_paths(paths[:cut]), G.GBWT.from_paths(paths[cut:])
    merged = G.GBWT.merge(a, b, algorithm=G.MERGE_INSERT)
    assert_same_index(merged, s.data(), s.starts(), header(s))
    info = merged.last_merge_info()
    assert info["walked_input"] == walked and info["algorithm_used"] == G.MERGE_INSERT
    walked_handle = b if walked else a
    assert info["walked_steps"] == walked_handle.len() - walked_handle.sequences() and info["walked_sequences"] == walked_handle.sequences()
    if cut == 32:
        rebuilt = G.GBWT.merge(a, b, algorithm=G.MERGE_REBUILD)
        assert_same_index(rebuilt, s.data(), s.starts(), header(s))
        assert rebuilt.last_merge_info()["rounds"] >= 1
        again = G.GBWT.merge(a, b, algorithm=G.MERGE_INSERT)      # the same inputs give the same bytes
        assert bytes(again.records()[0]) == bytes(merged.records()[0])


def test_more_than_two_handles_fold_left(chain):
    s, paths = chain
    parts = [G.GBWT.from_paths(paths[lo:hi]) for lo, hi in ((0, 10), (10, 11), (11, 40), (40, 64))]
    merged = G.GBWT.merge(parts)
    assert_same_index(merged, s.data(), s.starts(), header(s))
    assert merged.last_merge_info()["algorithm_used"] == G.MERGE_REBUILD      # AUTO over handles that are open for extraction
    by_insertion = G.GBWT.merge(parts, algorithm=G.MERGE_INSERT)
    assert_same_index(by_insertion, s.data(), s.starts(), header(s))


def test_auto_inserts_where_the_inputs_cannot_be_extracted():
    pa, pb = random_pair(5, True)
    witness = S.Synth.from_paths(list(pa) + list(pb))
    a, b = G.GBWT.from_paths(pa, flags=_lib.OPEN_SEARCH), G.GBWT.from_paths(pb, flags=_lib.OPEN_SEARCH)
    merged = G.GBWT.merge(a, b)
    assert_same_index(merged, witness.data(), witness.starts(), header(witness))
    assert merged.last_merge_info()["algorithm_used"] == G.MERGE_INSERT


# ---- 4. unidirectional inputs and mixed ones ----------------------------------------------------------------------------------------------------

def test_unidirectional_inputs_are_rebuilt():
    merged, _, _, _ = merge_and_check([[2, 4, 2, 4, 2, 6]], [[4, 2]], bidirectional=False)
    assert merged.last_merge_info()["algorithm_used"] == G.MERGE_REBUILD and not merged.is_bidirectional()
    a, b = G.GBWT.from_paths([[2, 4]], bidirectional=False), G.GBWT.from_paths([[4, 2]], bidirectional=False)
    with pytest.raises(G.GbwtHipError) as e:
        G.GBWT.merge(a, b, algorithm=G.MERGE_INSERT)
    assert e.value.status == _lib.BAD_ARGUMENT


def test_mixed_directionality_is_refused():
    a, b = G.GBWT.from_paths([[2, 4]], bidirectional=True), G.GBWT.from_paths([[2, 4]], bidirectional=False)
    for x, y in ((a, b), (b, a)):
        with pytest.raises(G.GbwtHipError) as e:
            G.GBWT.merge(x, y)
        assert e.value.status == _lib.BAD_ARGUMENT and "bidirectional" in str(e.value)


# ---- 5. the result is a handle like any other -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def merged_pair():
    pa, pb = random_pair(7, True)
    merged, a, b, witness = merge_and_check(pa, pb)
    return pa, pb, merged, a, b, witness


def test_sequences_are_those_of_a_then_b(merged_pair):
    pa, pb, merged, a, b, _ = merged_pair
    want = []
    for p in list(pa) + list(pb):
        want += [list(p), kat.reverse_path(list(p))]
    assert merged.sequences() == len(want)
    assert [merged.sequence(i) for i in range(merged.sequences())] == want


def counts(dev, first, second):
    states, valid = dev.find([first])
    if not valid[0]:
        return 0, 0
    found = int(states[0][2]) - int(states[0][1])
    states, valid = dev.extend(states, [second])
    return found, (int(states[0][2]) - int(states[0][1]) if valid[0] else 0)


def test_find_extend_and_locate_add_up(merged_pair):
    pa, pb, merged, a, b, _ = merged_pair
    nodes = sorted({v for p in list(pa) + list(pb) for v in p})
    pairs = [(p[i], p[i + 1]) for p in list(pa) + list(pb) for i in range(len(p) - 1)][:6] + [(nodes[0], nodes[-1])]
    for first, second in pairs:
        assert counts(merged, first, second) == tuple(x + y for x, y in zip(counts(a, first, second), counts(b, first, second)))
    for node in nodes[:4]:
        ids = []
        for dev, shift in ((a, 0), (b, a.sequences())):
            states, valid = dev.find([node])
            if valid[0]:
                ids += [int(x) + shift for x in dev.locate(states[0], unique=True)]
        states, valid = merged.find([node])
        assert valid[0] and sorted(int(x) for x in merged.locate(states[0], unique=True)) == sorted(ids)


def test_saved_merge_loads_in_the_oracle_and_the_inputs_still_answer(tmp_path, merged_pair):
    pa, pb, _, a, b, witness = merged_pair
    merged = G.GBWT.merge(a, b)
    out = tmp_path / "merged.gbwt"
    merged.save(str(out))
    ref = O.OracleGBWT.load(str(out))
    assert ref.bwt().data() == bytes(witness.data()) and ref.bwt().starts() == list(witness.starts())
    assert [ref.sequence(i) for i in range(ref.sequences())] == [merged.sequence(i) for i in range(merged.sequences())]
    merged.close()
    for dev, paths in ((a, pa), (b, pb)):                         # the inputs were only read
        assert [dev.sequence(2 * k) for k in range(len(paths))] == [list(p) for p in paths]


def test_lean_and_built_inputs(tmp_path):
    pa, pb = random_pair(11, False)
    merge_and_check(pa, pb, flags=_lib.OPEN_EXTRACT)              # built handles that were opened for extraction only
    files = []
    for k, paths in enumerate((pa, pb)):
        files.append(str(tmp_path / f"part{k}.gbwt"))
        S.Synth.from_paths(paths).save(files[-1])
    witness = S.Synth.from_paths(list(pa) + list(pb))
    for flags in (_lib.OPEN_EXTRACT, _lib.OPEN_ALL):                # loaded handles, lean and not
        a, b = G.GBWT.load(files[0], flags=flags), G.GBWT.load(files[1], flags=flags)
        for algorithm in (G.MERGE_INSERT, None):
            assert_same_index(G.GBWT.merge(a, b, algorithm=algorithm), witness.data(), witness.starts(), header(witness))
        assert set(a.last_merge_info().values()) == {0}           # a handle that was not merged


def test_last_merge_info(merged_pair):
    pa, pb, merged, a, b, _ = merged_pair
    info = merged.last_merge_info()
    visits = 2 * sum(len(p) for p in list(pa) + list(pb))
    assert (info["merged"], info["visits"], info["sequences"], info["records"]) == (1, visits, 2 * (len(pa) + len(pb)), merged.stats.records)
    assert info["data_bytes"] == merged.stats.data_bytes and info["peak_scratch_bytes"] > 0
    walked = b if b.len() - b.sequences() <= a.len() - a.sequences() else a
    assert info["walked_input"] == (1 if walked is b else 0) and info["walked_steps"] == walked.len() - walked.sequences()
    assert min(info["walk_ms"], info["decode_ms"], info["interleave_ms"], info["edges_ms"], info["encode_ms"], info["open_ms"]) > 0


# ---- 6. metadata and graph, end to end ----------------------------------------------------------------------------------------------------------

def split_gfa(path, change=None):
    """Two texts that both keep the H- and S-lines: text 1 with all P-lines and the first half of the W-lines, text 2 with the other W-lines."""
    lines = open(path, "rb").read().splitlines(keepends=True)
    walks = [k for k, line in enumerate(lines) if line.startswith(b"W")]
    second = set(walks[len(walks) // 2:])
    first = set(walks) - second | {k for k, line in enumerate(lines) if line.startswith(b"P")}
    common = [k for k, line in enumerate(lines) if line[:1] in (b"H", b"S", b"L")]
    t1 = b"".join(lines[k] for k in range(len(lines)) if k in first or k in common)
    t2 = b"".join((change(lines[k]) if change else lines[k]) for k in range(len(lines)) if k in second or k in common)
    return t1, t2


@pytest.mark.parametrize("algorithm", [G.MERGE_INSERT, G.MERGE_AUTO], ids=["insert", "auto"])
def test_gbz_merge_equals_the_whole_build(tmp_path, algorithm):
    t1, t2 = split_gfa(EXAMPLE_GFA)
    a, b = G.GBZ.from_gfa_text(t1), G.GBZ.from_gfa_text(t2)
    merged, whole = G.GBZ.merge(a, b, algorithm=algorithm), G.GBZ.from_gfa(EXAMPLE_GFA)
    merged.save(str(tmp_path / "merged.gbz"))
    whole.save(str(tmp_path / "whole.gbz"))
    assert (tmp_path / "merged.gbz").read_bytes() == (tmp_path / "whole.gbz").read_bytes()
    merged.write_gfa(str(tmp_path / "merged.gfa"))
    whole.write_gfa(str(tmp_path / "whole.gfa"))
    assert (tmp_path / "merged.gfa").read_bytes() == (tmp_path / "whole.gfa").read_bytes()
    assert merged.node_sequence(23) == whole.node_sequence(23) and merged.paths() == whole.paths() == 6
    assert merged.stats.is_gbz == 1 and merged.stats.has_metadata == 1


def test_translated_graphs_are_unsupported():
    t1, t2 = split_gfa(TRANSLATION_GFA)
    a, b = G.GBZ.from_gfa_text(t1, max_node=2), G.GBZ.from_gfa_text(t2, max_node=2)
    with pytest.raises(G.GbwtHipError) as e:
        G.GBZ.merge(a, b)
    assert e.value.status == _lib.UNSUPPORTED and "translation" in str(e.value)


def test_refusals_with_their_messages():
    t1, t2 = split_gfa(EXAMPLE_GFA)
    a = G.GBZ.from_gfa_text(t1)
    # a duplicated path name: text 2 with the W-line that is path 2 of text 1 put behind its own
    twin = next(line for line in t1.splitlines(keepends=True) if line.startswith(b"W"))
    with pytest.raises(G.GbwtHipError) as e:
        G.GBZ.merge(a, G.GBZ.from_gfa_text(t2 + twin))
    assert e.value.status == _lib.INVALID_DATA and "path 2 of b" in str(e.value)
    # a label conflict: one S-line changed in text 2
    _, changed = split_gfa(EXAMPLE_GFA, change=lambda line: b"S\t24\tC\n" if line.startswith(b"S\t24\t") else line)
    with pytest.raises(G.GbwtHipError) as e:
        G.GBZ.merge(a, G.GBZ.from_gfa_text(changed))
    assert e.value.status == _lib.INVALID_DATA and "node 24" in str(e.value)
    # GBZ + GBWT
    bare = G.GBWT.from_paths([[22, 24]])
    for x, y in ((a, bare), (bare, a)):
        with pytest.raises(G.GbwtHipError) as e:
            G.GBWT.merge(x, y)
        assert e.value.status == _lib.BAD_ARGUMENT and "GBZ" in str(e.value)
    # metadata on one side only
    with_metadata = G.GBWT.load(os.path.join(O.GOLDEN, "example.gbwt"))
    assert with_metadata.has_metadata()
    with pytest.raises(G.GbwtHipError) as e:
        G.GBWT.merge(with_metadata, bare)
    assert e.value.status == _lib.UNSUPPORTED and "metadata" in str(e.value)
