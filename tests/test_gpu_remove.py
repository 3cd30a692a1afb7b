"""GBWT / GBZ path removal on the device against the host builder over the kept paths (Synth.from_paths, pinned on the reference's fixtures
by tests/test_synth.py).  Every comparison is exact: the record stream, the record starts and the header fields.  The deletion itself is
held against the same builder, step by step, in tests/test_remove_cpu.py.  The deletion is asked for by name where the handle is open for
extraction: AUTO takes the rebuild there."""
import itertools
import os
import random

import numpy as np
import pytest

import gbwt_rs_amd as G
import kat
import oracle_lib as O
import remove_expect as RX
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


def kept_paths(paths, removed):
    gone = set(int(r) for r in removed)
    return [p for k, p in enumerate(paths) if k not in gone]


def remove_and_check(paths, removed, algorithm=G.REMOVE_DELETE, bidirectional=True, flags=_lib.OPEN_ALL, source=None):
    """The device's removal equals the brute-force builder's index of the kept paths; returns (result, input, witness)."""
    witness = S.Synth.from_paths(kept_paths(paths, removed), bidirectional=bidirectional)
    x = source if source is not None else G.GBWT.from_paths(paths, bidirectional=bidirectional, flags=flags)
    out = x.remove_paths(removed, algorithm=algorithm)
    assert_same_index(out, witness.data(), witness.starts(), header(witness))
    info = out.last_remove_info()
    assert info["removed"] == 1 and info["removed_sequences"] == (2 if bidirectional else 1) * len(removed)
    assert info["removed_steps"] == (2 if bidirectional else 1) * sum(len(paths[k]) for k in removed)
    if algorithm is not None and algorithm != G.REMOVE_AUTO:
        assert info["algorithm_used"] == algorithm
    return out, x, witness


def subsets(n):
    return [list(c) for k in range(n + 1) for c in itertools.combinations(range(n), k)]


# ---- 1. the reference's fixtures --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loaded", [False, True], ids=["built", "loaded"])
def test_every_subset_of_the_fixture(loaded):
    paths = kat.true_paths(False)
    source = G.GBWT.load(os.path.join(O.GOLDEN, "example.gbwt")) if loaded else G.GBWT.from_paths(paths)
    for removed in subsets(len(paths)):
        remove_and_check(paths, removed, source=source)


@pytest.mark.parametrize("loaded", [False, True], ids=["built", "loaded"])
def test_singletons_of_the_fixture_with_an_empty_path(loaded):
    paths = kat.true_paths(True)
    source = G.GBWT.load(os.path.join(O.GOLDEN, "with-empty.gbwt")) if loaded else G.GBWT.from_paths(paths)
    for removed in range(len(paths)):
        remove_and_check(paths, [removed], source=source)


@pytest.mark.parametrize("algorithm", [G.REMOVE_DELETE, G.REMOVE_REBUILD, None], ids=["delete", "rebuild", "auto"])
def test_removing_nothing_from_the_loaded_fixture_gives_its_own_bytes(algorithm):
    ref = O.OracleGBWT.load(os.path.join(O.GOLDEN, "example.gbwt"))
    x = G.GBWT.load(os.path.join(O.GOLDEN, "example.gbwt"))
    out = x.remove_paths([], algorithm=algorithm)
    assert_same_index(out, ref.bwt().data(), ref.bwt().starts(), (ref.sequences(), ref.len(), ref.alphabet_offset(), ref.alphabet_size(), True))
    assert out.last_remove_info()["removed"] == 1 and out.last_remove_info()["removed_sequences"] == 0


# ---- 2. the smallest shapes at which each stage can go wrong ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [name for name, _, _, _ in RX.special_removals()])
def test_special_shapes(name):
    _, paths, removed, bidirectional = next(s for s in RX.special_removals() if s[0] == name)
    out, x, _ = remove_and_check(paths, removed, bidirectional=bidirectional)
    assert out.is_bidirectional() == bidirectional
    if name == "alone-on-the-smallest":
        assert out.alphabet_offset() > x.alphabet_offset() and out.alphabet_size() == x.alphabet_size()
    if name == "alone-on-the-largest":
        assert out.alphabet_offset() == x.alphabet_offset() and out.alphabet_size() < x.alphabet_size()
    if name == "interior-record-emptied":
        assert (out.alphabet_offset(), out.alphabet_size()) == (x.alphabet_offset(), x.alphabet_size())
        assert out.find([8])[1][0] == 0 and x.find([8])[1][0] == 1
    if name == "all":
        assert (out.sequences(), out.len(), out.alphabet_size()) == (0, 0, 1)
    if name.startswith("only-empty"):
        rebuilt, _, _ = remove_and_check(paths, removed, algorithm=G.REMOVE_REBUILD)
        assert rebuilt.sequences() == out.sequences()


@pytest.mark.parametrize("k", [128, 129, 254, 255, 256, 300])
def test_hubs_around_the_run_encodings(k):
    paths, removed = RX.hub(k)
    out, x, _ = remove_and_check(paths, removed)
    assert x.stats.max_outdegree == k + 1 and out.stats.max_outdegree == k


# ---- 3. random sets ---------------------------------------------------------------------------------------------------------------------------

def random_removal(seed):
    rng = random.Random(seed)
    paths = random_paths(rng, n_paths=12, n_nodes=9, max_len=14, cyclic=seed % 2 == 1)
    removed = sorted(rng.sample(range(len(paths)), rng.randrange(len(paths) + 1)))
    return paths, removed


@pytest.mark.parametrize("seed", range(20))
def test_random_sets(seed):
    paths, removed = random_removal(seed)
    deleted, x, witness = remove_and_check(paths, removed)
    rebuilt, _, _ = remove_and_check(paths, removed, algorithm=G.REMOVE_REBUILD, source=x)      # rebuild equals deletion equals the witness
    assert deleted.last_remove_info()["algorithm_used"] == G.REMOVE_DELETE and rebuilt.last_remove_info()["algorithm_used"] == G.REMOVE_REBUILD


# ---- 4. tangled graphs --------------------------------------------------------------------------------------------------------------------------

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
def test_tangled_graphs_without_their_odd_paths(name):
    paths, bidirectional = TANGLED[name]()
    out, _, _ = remove_and_check(paths, list(range(1, len(paths), 2)), bidirectional=bidirectional)
    assert out.last_remove_info()["algorithm_used"] == G.REMOVE_DELETE


# ---- 5. a chain ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain():
    s = S.Synth.chain(sites=2000, haplotypes=64)
    paths = [s.path(h) for h in range(s.paths)]
    return s, paths, G.GBWT.from_paths(paths)


@pytest.mark.parametrize("removed", [[17], list(range(0, 64, 2)), [h for h in range(64) if h != 40]], ids=["1", "32", "63"])
def test_chain(chain, removed):
    s, paths, x = chain
    out, _, _ = remove_and_check(paths, removed, source=x)
    visits = 2 * sum(len(paths[k]) for k in removed)
    info = out.last_remove_info()
    assert info["removed_steps"] == visits and info["visits"] == x.len() - x.sequences() - visits
    again = x.remove_paths(removed, algorithm=G.REMOVE_DELETE)   # the same call gives the same bytes
    assert bytes(again.records()[0]) == bytes(out.records()[0]) and np.array_equal(again.records()[1], out.records()[1])


# ---- 6. the inverse of merging ------------------------------------------------------------------------------------------------------------------

def check_inverse(x, paths, k):
    tail = list(range(len(paths) - k, len(paths)))
    head = x.remove_paths(tail, algorithm=G.REMOVE_DELETE)
    back = G.GBWT.from_paths([paths[t] for t in tail])
    data, starts = x.records()
    for algorithm in (G.MERGE_INSERT, G.MERGE_REBUILD):
        assert_same_index(G.GBWT.merge(head, back, algorithm=algorithm), data, starts, header(x))


def test_merging_the_removed_tail_back_gives_the_chain(chain):
    _, paths, x = chain
    check_inverse(x, paths, 10)


@pytest.mark.parametrize("seed", range(5))
def test_merging_the_removed_tail_back_gives_the_input(seed):
    paths, _ = random_removal(seed)
    check_inverse(G.GBWT.from_paths(paths), paths, 1 + random.Random(seed).randrange(len(paths) - 1))


# ---- 7. where it can run ------------------------------------------------------------------------------------------------------------------------

def auto_choice(flags):
    """The rule include/gbwt_hip.h states: the rebuild where the handle is open for extraction, else the deletion."""
    return G.REMOVE_REBUILD if flags & _lib.OPEN_EXTRACT else G.REMOVE_DELETE


@pytest.mark.parametrize("flags", [_lib.OPEN_SEARCH, _lib.OPEN_EXTRACT, _lib.OPEN_ALL], ids=["search", "extract", "all"])
@pytest.mark.parametrize("loaded", [False, True], ids=["built", "loaded"])
def test_lean_built_and_loaded_handles(tmp_path, flags, loaded):
    paths, removed = random_removal(11)
    if loaded:
        S.Synth.from_paths(paths).save(str(tmp_path / "x.gbwt"))
        x = G.GBWT.load(str(tmp_path / "x.gbwt"), flags=flags)
    else:
        x = G.GBWT.from_paths(paths, flags=flags)
    remove_and_check(paths, removed, source=x)
    out, _, _ = remove_and_check(paths, removed, algorithm=None, source=x)
    assert out.last_remove_info()["algorithm_used"] == auto_choice(flags)
    if flags == _lib.OPEN_SEARCH:
        with pytest.raises(G.GbwtHipError) as e:
            x.remove_paths(removed, algorithm=G.REMOVE_REBUILD)
        assert e.value.status == _lib.BAD_ARGUMENT and "extraction" in str(e.value)
    assert set(x.last_remove_info().values()) == {0}             # a handle that was not made by a removal


def test_a_merged_handle():
    paths, removed = random_removal(13)
    merged = G.GBWT.merge(G.GBWT.from_paths(paths[:5]), G.GBWT.from_paths(paths[5:]), algorithm=G.MERGE_INSERT)
    remove_and_check(paths, removed, source=merged)
    out, _, _ = remove_and_check(paths, removed, algorithm=None, source=merged)
    assert out.last_remove_info()["algorithm_used"] == auto_choice(_lib.OPEN_ALL)


def test_bad_path_ids_are_refused_with_their_ids():
    x = G.GBWT.from_paths([[2, 4], [4, 6], [2, 6]])
    for ids, what in (([0, 3], "path id 3 "), ([7], "path id 7 "), ([1, 2, 1], "path id 1 appears twice")):
        with pytest.raises(G.GbwtHipError) as e:
            x.remove_paths(ids)
        assert e.value.status == _lib.BAD_ARGUMENT and what in str(e.value)
    one_way = G.GBWT.from_paths([[2, 4], [4, 6]], bidirectional=False)
    with pytest.raises(G.GbwtHipError) as e:
        one_way.remove_paths([2])                                # two sequences are two paths there
    assert e.value.status == _lib.BAD_ARGUMENT and "path id 2 " in str(e.value)
    assert x.sequence(2) == [4, 6]                               # the handle is as it was


def test_a_damaged_index_is_refused_not_rewritten():
    """The stored offset of edge 2 -> 6 is put beyond the record of 6: the kept path takes that edge, the offsets kernel raises the error
    word, and the call answers INVALID_DATA where it would have written a plausible record."""
    paths = [[2, 4, 6], [2, 6]]
    witness = S.Synth.from_paths(paths)
    data, starts = np.array(witness.data()), witness.starts()
    at = int(starts[2 - witness.alphabet_offset])                # the record of node 2: sigma, (delta 4, offset), (delta 2, offset)
    assert list(data[at:at + 5]) == [2, 4, 0, 2, 0]
    data[at + 4] = 100
    x = G.GBWT.from_records(data, starts, witness.alphabet_offset, witness.alphabet_size, witness.sequences, witness.size, flags=_lib.OPEN_SEARCH)
    with pytest.raises(G.GbwtHipError) as e:
        x.remove_paths([0], algorithm=G.REMOVE_DELETE)
    assert e.value.status == _lib.INVALID_DATA and "not consistent" in str(e.value)


# ---- 8. the result is a handle like any other ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def removed_set():
    paths, _ = random_removal(7)
    removed = [1, 4, 5, 10]
    out, x, witness = remove_and_check(paths, removed)
    return paths, removed, out, x, witness


def test_sequences_are_the_kept_ones(removed_set):
    paths, removed, out, _, _ = removed_set
    want = []
    for p in kept_paths(paths, removed):
        want += [list(p), kat.reverse_path(list(p))]
    assert out.sequences() == len(want)
    assert [out.sequence(i) for i in range(out.sequences())] == want
    kept = out.keep_paths([0, 2])                                # the complement: paths 0 and 2 of the result
    assert [kept.sequence(i) for i in range(kept.sequences())] == want[0:2] + want[4:6]


def counts(dev, first, second):
    states, valid = dev.find([first])
    if not valid[0]:
        return 0, 0
    found = int(states[0][2]) - int(states[0][1])
    states, valid = dev.extend(states, [second])
    return found, (int(states[0][2]) - int(states[0][1]) if valid[0] else 0)


def test_find_extend_and_locate_subtract(removed_set):
    paths, removed, out, x, _ = removed_set
    gone = G.GBWT.from_paths([paths[k] for k in removed])
    nodes = sorted({v for p in paths for v in p})
    pairs = [(p[i], p[i + 1]) for p in paths for i in range(len(p) - 1)][:8] + [(nodes[0], nodes[-1])]
    for first, second in pairs:
        assert counts(out, first, second) == tuple(a - b for a, b in zip(counts(x, first, second), counts(gone, first, second)))
    renumbered, nxt = {}, 0
    for s in range(x.sequences()):
        if s // 2 not in removed:
            renumbered[s], nxt = nxt, nxt + 1
    for node in nodes[:4]:
        states, valid = x.find([node])
        want = sorted(renumbered[int(s)] for s in x.locate(states[0], unique=True) if int(s) in renumbered) if valid[0] else []
        states, valid = out.find([node])
        got = sorted(int(s) for s in out.locate(states[0], unique=True)) if valid[0] else []
        assert got == want


def test_saved_result_loads_in_the_oracle_and_the_input_still_answers(tmp_path, removed_set):
    paths, removed, _, x, witness = removed_set
    out = x.remove_paths(removed, algorithm=G.REMOVE_DELETE)
    path = tmp_path / "removed.gbwt"
    out.save(str(path))
    ref = O.OracleGBWT.load(str(path))
    assert ref.bwt().data() == bytes(witness.data()) and ref.bwt().starts() == list(witness.starts())
    assert [ref.sequence(i) for i in range(ref.sequences())] == [out.sequence(i) for i in range(out.sequences())]
    out.close()
    assert [x.sequence(2 * k) for k in range(len(paths))] == [list(p) for p in paths]      # the input was only read


def test_last_remove_info(removed_set):
    paths, removed, out, x, _ = removed_set
    info = out.last_remove_info()
    visits = 2 * sum(len(p) for p in kept_paths(paths, removed))
    assert (info["removed"], info["visits"], info["sequences"], info["records"]) == (1, visits, 2 * (len(paths) - len(removed)), out.stats.records)
    assert info["data_bytes"] == out.stats.data_bytes and info["peak_scratch_bytes"] > 0
    assert info["removed_sequences"] == 2 * len(removed) and info["removed_steps"] == 2 * sum(len(paths[k]) for k in removed)
    assert info["algorithm_used"] == G.REMOVE_DELETE and info["rounds"] == 0
    assert min(info["walk_ms"], info["decode_ms"], info["compact_ms"], info["edges_ms"], info["encode_ms"], info["open_ms"]) > 0
    assert set(x.last_remove_info().values()) == {0}
    rebuilt = x.remove_paths(removed, algorithm=G.REMOVE_REBUILD)
    assert rebuilt.last_remove_info()["rounds"] >= 1 and rebuilt.last_remove_info()["walk_ms"] == 0


# ---- 9. metadata and graph, end to end ------------------------------------------------------------------------------------------------------------

def gfa_without(path, removed):
    """The text without the P- / W-lines of the paths: path ids count the P-lines in file order, then the W-lines."""
    lines = open(path, "rb").read().splitlines(keepends=True)
    order = [k for k, line in enumerate(lines) if line.startswith(b"P")] + [k for k, line in enumerate(lines) if line.startswith(b"W")]
    gone = {order[p] for p in removed}
    return b"".join(line for k, line in enumerate(lines) if k not in gone)


@pytest.mark.parametrize("algorithm", [G.REMOVE_DELETE, G.REMOVE_AUTO], ids=["delete", "auto"])
@pytest.mark.parametrize("what", ["contig-B", "haplotype-2"])
def test_gbz_removal_equals_the_build_without_those_lines(tmp_path, what, algorithm):
    x = G.GBZ.from_gfa(EXAMPLE_GFA)
    if what == "contig-B":
        removed = [1, 4, 5]
        assert [int(p) for p in x.select_paths(contig="B")] == removed
        out = x.remove_contig("B", algorithm=algorithm)
    else:
        removed = [3, 5]
        out = x.remove_paths(removed, algorithm=algorithm)
    assert isinstance(out, G.GBZ)
    whole = G.GBZ.from_gfa_text(gfa_without(EXAMPLE_GFA, removed))
    out.save(str(tmp_path / "removed.gbz"))
    whole.save(str(tmp_path / "whole.gbz"))
    assert (tmp_path / "removed.gbz").read_bytes() == (tmp_path / "whole.gbz").read_bytes()
    out.write_gfa(str(tmp_path / "removed.gfa"))
    whole.write_gfa(str(tmp_path / "whole.gfa"))
    text = (tmp_path / "removed.gfa").read_bytes()
    assert text == (tmp_path / "whole.gfa").read_bytes()
    assert out.stats.is_gbz == 1 and out.stats.has_metadata == 1
    if what == "contig-B":
        assert out.paths() == 3
        assert out.node_sequence(11) == x.node_sequence(11) == b"G"
        assert not out.has_node(2 * 21) and out.successors(21, G.FORWARD) is None and out.node_sequence(21) is None
        assert b"S\t21\t" not in text and b"S\t11\t" in text
        assert out.alphabet_size() == whole.alphabet_size() == 2 * 17 + 2
    assert x.paths() == 6 and x.node_sequence(21) == b"G"       # the input was only read


def test_translated_graphs_are_unsupported():
    x = G.GBZ.from_gfa(TRANSLATION_GFA, max_node=2)
    with pytest.raises(G.GbwtHipError) as e:
        x.remove_paths([0])
    assert e.value.status == _lib.UNSUPPORTED and "translation" in str(e.value)


def test_metadata_of_a_loaded_gbwt_is_kept(tmp_path):
    x = G.GBWT.load(os.path.join(O.GOLDEN, "example.gbwt"))
    assert x.has_metadata()
    out = x.remove_paths([1, 4], algorithm=G.REMOVE_DELETE)
    assert out.has_metadata() and out.sequences() == x.sequences() - 4
    out.save(str(tmp_path / "removed.gbwt"))
    ref = O.OracleGBWT.load(str(tmp_path / "removed.gbwt"))
    witness = S.Synth.from_paths(kept_paths(kat.true_paths(False), [1, 4]))
    assert ref.bwt().data() == bytes(witness.data()) and ref.sequences() == out.sequences()
