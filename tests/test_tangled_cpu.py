"""The yardstick of tests/tangled_graphs.py pinned without a GPU: its path union-find against components_expect over the CPU oracle's records
for every topology, and for the long-label graphs what tests/test_gpu_tangled.py relies on -- the generator gives the requested label
lengths, the two expectations of the tag array agree, and the inputs really hold the cases they are there for."""
import numpy as np
import pytest

import components_expect as X
import oracle_lib as O
import seq_expect as E
import tags_expect as T
import tangled_graphs as TG
from gbwt_rs_amd import synth as S


def oracle_of(tmp_path, paths, bidirectional, label_lengths=None):
    """The CPU oracle's GBWT of a path set (through a GBZ file where the index is bidirectional), and the OracleGBZ or None."""
    s = S.Synth.from_paths(paths, bidirectional=bidirectional)
    if not bidirectional:
        bwt = O.OracleBWT.from_parts(bytes(s.data()), s.starts())
        return O.OracleGBWT.from_bwt(bwt, s.sequences, s.size, s.alphabet_offset, s.alphabet_size, False), None
    path = str(tmp_path / "graph.gbz")
    s.attach_gbz(seed=3, label_lengths=label_lengths).save(path, as_gbz=True)
    gbz = O.OracleGBZ(path)
    return gbz.gbwt(), gbz


@pytest.mark.parametrize("name", sorted(TG.COMPONENT_BUILDERS))
def test_path_union_find_equals_the_oracle_components(tmp_path, name):
    paths, bidirectional = TG.COMPONENT_BUILDERS[name]()
    want = TG.Expected(paths)
    gbwt, _ = oracle_of(tmp_path, paths, bidirectional)
    assert gbwt.is_bidirectional() == bidirectional
    assert X.geometry(gbwt) == (want.min_node, want.slots)
    comps = X.components(gbwt)
    assert comps == want.lists()
    assert len(comps) == want.components and sum(len(c) for c in comps) == want.nodes
    stride = 2 if bidirectional else 1
    assert gbwt.sequences() // stride == len(paths) == want.paths
    assert X.path_components(comps, X.first_nodes(gbwt, len(paths), stride)) == want.path_component.tolist()


def test_topologies_hold_what_they_are_for():
    """Properties of the inputs the GPU test leans on, from the yardstick alone."""
    sizes = {}
    for name, build in TG.COMPONENT_BUILDERS.items():
        paths, _ = build()
        sizes[name] = want = TG.Expected(paths)
        assert want.slots >= 90000 and 2 * want.slots // 256 >= 700, name            # hundreds of workgroups of one lane per record
    assert [sizes[n].components for n in ("permuted-path", "descending-path", "zigzag", "grid", "tree-with-hub", "permuted-path-unidirectional")] == [1] * 6
    assert sizes["tree-with-hub"].ids[-1] == sizes["tree-with-hub"].min_node + sizes["tree-with-hub"].slots - 1     # the hub is the largest id
    hub = 2 * int(sizes["tree-with-hub"].ids[-1])
    assert sum(1 for p in TG.tree_with_hub()[0] if int(p[0]) == hub) == 5000
    inter = sizes["interleaved"]
    singles = int(np.count_nonzero(np.diff(inter.offsets) == 1))
    assert inter.components == 997 + singles and 200 <= singles <= 1000
    assert inter.nodes < inter.slots - 5000                                            # slots without nodes
    assert int(np.count_nonzero(inter.path_component == TG.NONE)) == 5                 # the empty paths
    joins = sizes["reverse-joins"]
    assert int(np.diff(joins.offsets).max()) == 2 * (100000 // 3) and joins.components > 200
    sparse = sizes["sparse-random"]
    assert sparse.components >= 1 << 16                                                # component numbers of 17 bits
    assert sparse.nodes < 0.75 * sparse.slots and len(np.unique(np.diff(sparse.offsets))) > 20


@pytest.fixture(scope="module")
def tangle(tmp_path_factory):
    lengths = TG.tangle_label_lengths()
    paths, _ = TG.tangle(lengths=lengths)
    gbwt, gbz = oracle_of(tmp_path_factory.mktemp("tangle"), paths, True, lengths)
    return lengths, paths, gbz


def test_tangle_labels_have_the_requested_lengths(tangle):
    lengths, paths, gbz = tangle
    visited = np.unique(np.concatenate(paths) >> np.uint64(1)).astype(np.int64)
    got = {int(k): len(v) for k, v in E.s_lines(gbz.gfa()).items()}
    assert sorted(got) == visited.tolist()                                             # nodes without a record have no S-line
    assert [got[v] for v in visited.tolist()] == lengths[visited - 1].tolist()
    assert set(b"".join(E.s_lines(gbz.gfa()).values())) == set(b"ACGT")
    assert {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2048, 5000, TG.TANGLE_GIANT} <= set(got.values())
    assert [len(p) for p in paths] == TG.TANGLE_PATH_LENGTHS
    rows = T.rows_of(gbz.gbwt().extract(2 * np.arange(len(paths), dtype=np.uint64)), len(paths))
    assert all(np.array_equal(a, b) for a, b in zip(rows, paths))                      # the oracle walks what was asked for


def test_tangle_text_and_preconditions(tangle):
    lengths, paths, gbz = tangle
    table = E.LabelTable.from_gfa(gbz.gfa())
    ids = np.arange(len(paths), dtype=np.uint64)
    text, offsets = T.oracle_text(gbz, ids, table.len)
    assert 5000000 <= text.size <= 10000000                                            # more than the 2 M entries of one tile per workgroup
    sa = np.random.default_rng(12).permutation(text.size).astype(np.uint64)
    assert np.array_equal(T.two_sorts(text, sa), T.gather(text, sa))
    # a node longer than 1 024 bases in both orientations
    nodes = np.concatenate(paths)
    long_ids = np.flatnonzero(lengths > 1024) + 1
    both = [v for v in long_ids.tolist() if (nodes == 2 * v).any() and (nodes == 2 * v + 1).any()]
    assert both and lengths[np.array(both) - 1].max() == TG.TANGLE_GIANT
    # the carry: bit 10 of a tag that is not the orientation of its node
    orientation = np.concatenate([np.r_[np.repeat(p & np.uint64(1), table.len[(p >> np.uint64(1)).astype(np.int64)]), np.uint64(0)] for p in paths])
    assert orientation.size == text.size
    carried = ((text >> np.uint64(10)) & np.uint64(1)) != orientation
    assert carried.any() and not carried.all()
    # a 16-byte unit of the output across a forward / reverse boundary with labels of at least 1 024 bases on both sides (all paths in one
    # request with an endmarker each: the byte offsets of the text)
    found = 0
    for p, start in zip(paths, offsets[:-1].tolist()):
        lens = table.len[(p >> np.uint64(1)).astype(np.int64)]
        at = start + np.cumsum(lens)[:-1]                                              # first byte of visit k + 1
        o = (p & np.uint64(1)).astype(np.int64)
        found += int(np.count_nonzero((o[:-1] != o[1:]) & (lens[:-1] >= 1024) & (lens[1:] >= 1024) & (at % 16 != 0)))
    assert found >= 4


@pytest.mark.parametrize("length", [1025, 70000])
def test_long_label_and_self_loop_builders(tmp_path, length):
    lengths, paths = TG.long_label(length)
    _, gbz = oracle_of(tmp_path, paths, True, lengths)
    labels = E.s_lines(gbz.gfa())
    assert [len(labels[k]) for k in (b"1", b"2", b"3")] == [1, length, 1]
    text, offsets = T.oracle_text(gbz, [0])
    assert text.size == 3 * length + 3 and offsets.tolist() == [0, 3 * length + 3]
    assert text[1 + length - 1] == (2 << 11) + length - 1                              # the last base of the first visit: a plain addition
    assert text[1 + 2 * length] == ((2 << 11) | (1 << 10)) and text[-1] == 0
    lengths, paths = TG.self_loop(length, 6)
    assert lengths.tolist() == [1, length, 1] and (paths[0] & np.uint64(1)).tolist() == [0, 0, 1, 0, 1, 0, 1, 0]


def test_generator_refuses_bad_label_lengths():
    paths, _ = TG.long_label(5)[1], True
    s = S.Synth.from_paths(paths)
    with pytest.raises(ValueError):
        s.attach_gbz(label_lengths=[1, 5])                                             # one entry per potential node
    with pytest.raises(ValueError):
        S.Synth.from_paths(paths).attach_gbz(label_lengths=[1, 0, 1])                  # a node with a record has bases
    gaps = S.Synth.from_paths([[TG.fwd(1), TG.fwd(4)]]).attach_gbz(label_lengths=[2, 9, 9, 3])
    assert gaps.sequences == 2                                                         # ids 2 and 3 have no record: their entries are ignored
