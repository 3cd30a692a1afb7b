"""Every request family on graphs whose node ids start far from 1: the tangle, four component topologies, two chains and a cyclic random
set, each moved up the id range by the three shifts of tests/shifted_graphs.py -- seven-digit ids, GBWT nodes on both sides of 2^31, and the
largest id the library accepts (2^31 - 1: alphabet_size 2^32, bit 31 of every node word set, ten-digit ids in the text).  The expectations
are the existing helpers' over the UNSHIFTED oracle file, moved by the shift (pinned on the CPU in tests/test_shifted_cpu.py); text is also
compared with the oracle's text of the shifted file.  Everything is integer or byte equality."""
import random

import numpy as np
import pytest

import components_expect as X_components
import gbwt_rs_amd as G
import graph_expect as X
import locate_expect as LX
import oracle_lib as O
import refpos_expect as R
import seq_expect as E
import shifted_graphs as SG
import tags_expect as T
import tangled_graphs as TG
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S
from search_checks import check_all_positions, check_follow, check_search
from test_gpu_build import assert_same_index, header
from test_gpu_tangled import check_components

pytestmark = pytest.mark.gpu

SHIFTS = list(SG.SHIFT_NAMES)
TOO_MANY_RECORDS = "more than 2^30 records are not supported"


def bare(s, flags=_lib.OPEN_ALL):
    return G.GBWT.from_records(s.data(), s.starts(), s.alphabet_offset, s.alphabet_size, s.sequences, s.size, s.bidirectional, flags=flags)


def oracle_of(s):
    bwt = O.OracleBWT.from_parts(bytes(s.data()), s.starts())
    return O.OracleGBWT.from_bwt(bwt, s.sequences, s.size, s.alphabet_offset, s.alphabet_size, s.bidirectional)


def sparse_graph(gbwt, node_ids):
    """A graph_expect.Graph that holds the records of these node ids alone (both orientations): enough for Graph.edges of them."""
    graph = X.Graph.__new__(X.Graph)
    graph.offset, graph.size = gbwt.alphabet_offset(), gbwt.alphabet_size()
    graph.min_node, graph.max_node = (graph.offset + 1) // 2, graph.size // 2 - 1
    graph.rows = {}
    bwt = gbwt.bwt()
    for node in {2 * int(v) + o for v in node_ids for o in (0, 1)}:
        if graph.offset < node < graph.size:
            rec = bwt.record(node - graph.offset)
            if rec is not None:
                graph.rows[node] = [int(succ) for succ, _ in rec.edges()]
    return graph


def moved_edges(graph, d, node_id, orientation, predecessors):
    """Graph.edges of the unshifted graph for a shifted id: None for an id the shift does not reach, the rows plus d otherwise."""
    plain = int(node_id) - d
    if not graph.min_node <= plain <= graph.max_node:
        return None
    rows = graph.edges(plain, int(orientation), predecessors)
    return None if rows is None else [(v + d, o) for v, o in rows]


def check_edge_rows(dev, graph, d, ids, orient):
    for predecessors in (False, True):
        rows = [moved_edges(graph, d, i, o, predecessors) for i, o in zip(ids, orient)]
        offsets, flat, valid = dev.edges_csr(ids, orient, predecessors)
        e_off, e_flat, e_valid = X.csr(rows)
        assert offsets.dtype == np.uint64 and flat.dtype == np.uint64
        assert np.array_equal(valid, e_valid)
        assert np.array_equal(offsets, e_off)
        assert np.array_equal(flat, e_flat)
    return rows


# ---- the tangle -----------------------------------------------------------------------------------------------------------------------------

class TangleBase:
    """The unshifted tangle and everything the helpers say about it: computed once, moved for every shift."""

    def __init__(self, directory):
        self.directory = directory
        self.lengths = TG.tangle_label_lengths()
        self.paths, _ = TG.tangle(lengths=self.lengths)
        self.n = len(self.paths)
        self.max_id = SG.max_id_of(self.paths)
        gbz = str(directory / "plain.gbz")
        S.Synth.from_paths(self.paths).attach_gbz(seed=3, label_lengths=self.lengths).save(gbz, as_gbz=True)
        self.oracle = O.OracleGBZ(gbz)
        gbwt = self.oracle.gbwt()
        self.gfa = [self.oracle.gfa(mode) for mode in (0, 1, 2)]
        self.table = E.LabelTable.from_gfa(self.gfa[0])
        ids = np.arange(self.n, dtype=np.uint64)
        self.csr = gbwt.extract(np.arange(2 * self.n, dtype=np.uint64))
        self.bases = []                                                  # [orientation][path]: bytes
        for o in (0, 1):
            seq_ids = [2 * p + o for p in range(self.n)]
            offsets, data = E.expected_rows(self.table, E.node_rows(gbwt.extract(2 * ids + np.uint64(o)), seq_ids, 2 * self.n))
            self.bases.append([data[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])])
        self.rows = T.rows_of(gbwt.extract(2 * ids), self.n)
        self.text, self.text_offsets = T.tag_text(self.table.len, self.rows)
        self.graph = X.Graph(gbwt)
        self.components = TG.Expected(self.paths)
        self.starts = {p: R.node_starts(gbwt, p, self.table.len) for p in range(self.n)}

    def expected_bases(self, order, reverse, endmarker):
        tail = b"" if endmarker is None else bytes([endmarker])
        parts = [self.bases[reverse][p] + tail for p in order]
        return np.cumsum([0] + [len(x) for x in parts]).astype(np.uint64), b"".join(parts)


class ShiftedTangle:
    def __init__(self, base, shift):
        self.base, self.shift = base, shift
        self.d = d = SG.SHIFTS(base.max_id)[shift]
        self.paths = SG.shift_paths(base.paths, d)
        self.synth = S.Synth.from_paths(self.paths)
        self.gbz = str(base.directory / f"{shift}.gbz")
        self.synth.attach_gbz(seed=3, label_lengths=base.lengths).save(self.gbz, as_gbz=True)
        self.oracle = O.OracleGBZ(self.gbz)
        self.dev = G.GBZ.load(self.gbz)

    def handles(self):
        return [self.dev, G.GBZ.load(self.gbz, flags=_lib.OPEN_EXTRACT), bare(self.synth)]


@pytest.fixture(scope="module")
def tangle_base(tmp_path_factory):
    return TangleBase(tmp_path_factory.mktemp("shifted-tangle"))


@pytest.fixture(scope="module", params=SHIFTS)
def tangle(request, tangle_base):
    return ShiftedTangle(tangle_base, request.param)


def test_tangle_header_and_limits(tangle):
    dev, d = tangle.dev, tangle.d
    assert dev.alphabet_offset() == 1 + 2 * d and dev.alphabet_size() == 2 * (tangle.base.max_id + d) + 2
    if tangle.shift == "top":
        assert dev.alphabet_size() == 1 << 32
    if tangle.shift == "straddle":
        assert dev.alphabet_offset() < (1 << 31) < dev.alphabet_size()


def test_tangle_all_sequences_from_three_handles(tangle):
    base = tangle.base
    ids = np.arange(2 * base.n, dtype=np.uint64)
    want = SG.move_nodes(base.csr[1], tangle.d)
    for dev in tangle.handles():
        offsets, nodes = dev.sequences_csr(ids)
        assert np.array_equal(offsets, base.csr[0])
        assert np.array_equal(np.asarray(nodes).astype(np.uint64), want)
    for p in (1, 5, base.n - 1):                                       # ... which are the paths that went in, and their reverses
        assert np.array_equal(want[int(base.csr[0][2 * p]):int(base.csr[0][2 * p + 1])], tangle.paths[p])
        assert np.array_equal(want[int(base.csr[0][2 * p + 1]):int(base.csr[0][2 * p + 2])], tangle.paths[p][::-1] ^ np.uint64(1))


def test_tangle_bases_orders_orientations_endmarkers(tangle):
    dev, n = tangle.dev, tangle.base.n
    ids = list(range(n))
    shuffled = np.random.default_rng(21).permutation(n).tolist()
    shuffled = shuffled + shuffled[:3] + [shuffled[0]]
    for order, reverse, endmarker in ((ids, 0, 0), (ids, 1, None), (shuffled, 0, 255), (shuffled, 1, 0), (shuffled, 0, None), (shuffled, 1, None)):
        offsets, data = dev.path_sequences(order, G.REVERSE if reverse else G.FORWARD, endmarker)
        e_off, e_data = tangle.base.expected_bases(order, reverse, endmarker)
        assert np.array_equal(offsets, e_off), (reverse, endmarker)
        assert data == e_data, (reverse, endmarker)


def test_tangle_write_sequences(tangle, tmp_path):
    out = tmp_path / "tangle.seq"
    tangle.dev.write_sequences(str(out))
    e_off, e_data = tangle.base.expected_bases(range(tangle.base.n), 0, 0)
    assert out.read_bytes() == e_data
    lines = out.with_name(out.name + ".names").read_text().splitlines()
    assert [int(l.split("\t")[0]) for l in lines] == list(range(tangle.base.n))
    assert [int(l.split("\t")[5]) for l in lines] == [len(b) for b in tangle.base.bases[0]]


def test_tangle_text_length_and_tags(tangle, monkeypatch):
    dev, base = tangle.dev, tangle.base
    ids = np.arange(base.n, dtype=np.uint64)
    text = SG.move_tags(base.text, tangle.d)
    assert int(np.count_nonzero(text == 0)) == base.n
    if tangle.shift == "top":
        assert int(text.max()) >> 11 >= SG.MAX_NODE_ID                 # tags of 42 bits and more (the offset inside a long node carries)
    assert dev.text_length(ids) == text.size == int(base.text_offsets[-1])
    sas = [np.random.default_rng(22).permutation(text.size).astype(np.uint64), np.arange(text.size, dtype=np.uint64)]
    for sa in sas:
        tags, runs = dev.tag_array(ids, sa, return_runs=True)
        want = T.gather(text, sa)
        assert np.array_equal(tags, want)
        assert runs == T.runs(want)
    if tangle.shift == "top":                                          # the plan with 64-bit hints, on a workspace of its own
        monkeypatch.setenv("GBWT_HIP_TAG_WIDE", "1")
        other = dev.another_workspace()
        tags, runs = other.tag_array(ids, sas[0], return_runs=True)
        want = T.gather(text, sas[0])
        assert np.array_equal(tags, want) and runs == T.runs(want)


@pytest.mark.parametrize("mode", [G.PATHS_DEFAULT, G.PATHS_PAN_SN, G.PATHS_REF_ONLY])
def test_tangle_gfa_equals_the_oracle(tangle, tmp_path, mode):
    out = tmp_path / "tangle.gfa"
    tangle.dev.write_gfa(str(out), mode)
    got = out.read_bytes()
    assert got == tangle.oracle.gfa(mode)
    assert got == SG.shift_gfa(tangle.base.gfa[mode], tangle.d)


def test_tangle_graph_lines_and_node_ids(tangle):
    want = X.graph_text(SG.shift_gfa(tangle.base.gfa[0], tangle.d))
    assert want == X.graph_text(tangle.oracle.gfa())
    got = tangle.dev.graph_lines()
    assert len(got) == len(want) and got == want
    ids = tangle.dev.node_iter()
    assert np.array_equal(np.asarray(ids).astype(np.uint64), SG.move_ids(tangle.base.graph.node_ids(), tangle.d))
    for v in (tangle.base.graph.node_ids()[0], tangle.base.graph.node_ids()[-1]):
        label = tangle.base.table.bytes[tangle.base.table.start[v]:tangle.base.table.start[v + 1]].tobytes()
        assert tangle.dev.node_sequence(v + tangle.d) == label


def test_tangle_edges_of_every_node_and_of_no_node(tangle):
    base, d = tangle.base, tangle.d
    graph = base.graph
    real = SG.move_ids(np.arange(graph.min_node, graph.max_node + 1), d)     # every slot: nodes and slots without one
    lo, hi = graph.min_node + d, graph.max_node + d
    no_node = np.array([0, 1, base.max_id, lo - 1, hi + 1, hi + 2, 1 << 31, (1 << 31) + 1, 1 << 32, 1 << 40, (1 << 62) - 1, 1 << 62, (1 << 64) - 1], dtype=np.uint64)
    rng = np.random.default_rng(25)
    ids = np.concatenate([real, no_node, rng.choice(real, size=50).repeat(3)])
    ids = ids[rng.permutation(ids.size)]
    for handle in (tangle.dev, bare(tangle.synth)):
        for o in (0, 1):
            check_edge_rows(handle, graph, d, ids, np.full(ids.size, o, dtype=np.uint8))
    for o in (0, 1):                                                     # the ids of no node come back not valid
        for predecessors in (False, True):
            offsets, flat, valid = tangle.dev.edges_csr(no_node, np.full(no_node.size, o, dtype=np.uint8), predecessors)
            assert not valid.any() and flat.size == 0 and not offsets.any()


@pytest.mark.parametrize("interval", [1, 37, 1000])
def test_tangle_path_and_reference_positions(tangle, interval):
    base, d = tangle.base, tangle.d

    def want(ids):
        out = []
        for p in ids:
            path_id, length, offsets, positions = R.positions_of(base.starts[p], p, interval)
            out.append((path_id, length, offsets, SG.move_positions(positions, d)))
        return out

    every = list(range(base.n))
    assert R.same(tangle.dev.path_positions(every, interval), want(every))
    ref = tangle.dev.reference_paths().tolist()
    assert ref == [0]                                                    # the generator's one generic path
    assert R.same(tangle.dev.reference_positions(interval), want(ref))
    longest = tangle.dev.path_positions([base.n - 1], interval)
    assert R.same(longest, want([base.n - 1])) and longest[0][3][:, 0].min() > 2 * d


def test_tangle_components_from_three_handles(tangle):
    want = SG.move_expected(tangle.base.components, tangle.d)
    assert want.min_node == 1 + tangle.d
    for dev in tangle.handles():
        check_components(dev, want)


# ---- construction from the tangle: paths and GFA text --------------------------------------------------------------------------------------------

def test_tangle_built_from_its_paths(tangle):
    dev = G.GBWT.from_paths(tangle.paths)
    assert_same_index(dev, tangle.synth.data(), tangle.synth.starts(), header(tangle.synth))
    data, starts = tangle.dev.records()
    assert bytes(data) == bytes(tangle.synth.data()) and np.array_equal(starts, tangle.synth.starts())


def test_tangle_built_from_its_gfa_text(tangle, tmp_path):
    text = SG.shift_gfa(tangle.base.gfa[0], tangle.d)                    # gbunzip's text of the shifted file (test_tangle_gfa_equals_the_oracle)
    built = G.GBZ.from_gfa_text(text)
    loaded = tangle.dev
    assert_same_index(built, *loaded.records(), header(loaded))
    out = tmp_path / "built.gfa"
    built.write_gfa(str(out))
    assert out.read_bytes() == text                                      # gbunzip o build
    kept = tmp_path / "loaded.gbz"
    loaded.save(str(kept))
    assert kept.read_bytes() == open(tangle.gbz, "rb").read()            # the loaded file is saved unchanged
    saved = tmp_path / "built.gbz"                                       # (the built one differs from it in the tags: the generator's `source`)
    built.save(str(saved))
    assert O.OracleGBZ(str(saved)).gfa() == text                         # the saved file, read by the oracle
    again = G.GBZ.load(str(saved))
    assert_same_index(again, *loaded.records(), header(loaded))
    resaved = tmp_path / "again.gbz"
    again.save(str(resaved))
    assert resaved.read_bytes() == saved.read_bytes()
    rebuilt = G.GBZ.from_gfa(str(out))                                   # ... and the fixed point
    assert_same_index(rebuilt, *loaded.records(), header(loaded))
    rebuilt.write_gfa(str(out))
    assert out.read_bytes() == text
    ids = np.arange(tangle.base.n, dtype=np.uint64)
    o1, b1 = built.path_sequences(ids)
    e_off, e_data = tangle.base.expected_bases(range(tangle.base.n), 0, None)
    assert np.array_equal(o1, e_off) and bytes(b1) == e_data


# ---- topologies -------------------------------------------------------------------------------------------------------------------------------

TOPOLOGIES = ["interleaved", "tree-with-hub", "reverse-joins", "permuted-path-unidirectional"]
LOCATE_SAMPLE = 64


class TopologyBase:
    def __init__(self, name):
        self.name = name
        self.paths, self.bidirectional = TG.COMPONENT_BUILDERS[name]()
        self.max_id = SG.max_id_of(self.paths)
        self.components = TG.Expected(self.paths)
        self.synth = S.Synth.from_paths(self.paths, bidirectional=self.bidirectional)
        self.oracle = oracle_of(self.synth)
        self.hub = self.max_id if name == "tree-with-hub" else None
        rng = np.random.default_rng(26)
        stride = 2 if self.bidirectional else 1
        picked = rng.choice(self.components.ids, size=LOCATE_SAMPLE, replace=False).astype(np.int64)
        nodes = [2 * int(v) + int(o) * (stride - 1) for v, o in zip(picked, rng.integers(0, 2, size=LOCATE_SAMPLE))]
        if self.hub is not None:
            nodes += [2 * self.hub, 2 * self.hub + 1]
        self.states = [self.oracle.find(node) or (node, 0, 1) for node in nodes]       # whole records; (node, 0, 1) where there is none
        self._own = None

    def own(self):
        if self._own is None:
            self._own = LX.owners(self.oracle)
        return self._own


_topology_bases = {}


@pytest.fixture(scope="module", params=[(name, shift) for name in TOPOLOGIES for shift in SHIFTS], ids=lambda p: f"{p[0]}-{p[1]}")
def topology(request, tmp_path_factory):
    name, shift = request.param
    if name not in _topology_bases:
        _topology_bases.clear()                                          # one unshifted topology at a time
        _topology_bases[name] = TopologyBase(name)
    base = _topology_bases[name]
    d = SG.SHIFTS(base.max_id)[shift]
    s = S.Synth.from_paths(SG.shift_paths(base.paths, d), bidirectional=base.bidirectional)
    handles = [bare(s)]
    if base.bidirectional:
        gbz = str(tmp_path_factory.mktemp("shifted-topology") / "graph.gbz")
        s.attach_gbz(seed=3).save(gbz, as_gbz=True)
        handles.insert(0, G.GBZ.load(gbz))
    return base, d, s, handles


def test_topology_components_from_the_gbz_and_the_bare_handle(topology):
    base, d, s, handles = topology
    want = SG.move_expected(base.components, d)
    for dev in handles:
        assert dev.alphabet_size() == s.alphabet_size and dev.alphabet_offset() == s.alphabet_offset
        check_components(dev, want)


def test_topology_edges_of_the_hub(topology):
    base, d, s, handles = topology
    if base.hub is None:
        return                                                           # (the one record of 5 000 edges is tree-with-hub's)
    graph = sparse_graph(base.oracle, [base.hub, base.hub - 1])
    ids = np.array([base.hub + d, base.hub + d - 1, base.hub + d + 1, base.hub], dtype=np.uint64)
    for dev in handles:
        for o in (0, 1):
            rows = check_edge_rows(dev, graph, d, ids, np.full(ids.size, o, dtype=np.uint8))
        assert len(rows[0]) == 5000 and rows[2] is None and rows[3] is None


def test_topology_locate_both_modes(topology):
    base, d, s, handles = topology
    own = base.own()
    states = np.zeros(len(base.states), dtype=G.STATE_DTYPE)
    for k, (node, start, end) in enumerate(base.states):
        states[k] = (node + 2 * d, start, end)
    dev = handles[-1]
    for unique in (False, True):
        rows = [LX.row(own, st, unique) for st in base.states]
        assert sum(r is not None for r in rows) >= LOCATE_SAMPLE // 2
        offsets, ids, valid = dev.locate_csr(states, unique)
        e_off, e_ids, e_valid = LX.csr(rows)
        assert offsets.dtype == np.uint64 and ids.dtype == np.uint64 and valid.dtype == bool
        assert np.array_equal(valid, e_valid)
        assert np.array_equal(offsets, e_off)
        assert np.array_equal(ids, e_ids)
    unshifted = np.zeros(2, dtype=G.STATE_DTYPE)                          # the same states without the shift name no record of this index
    unshifted[0], unshifted[1] = base.states[0], base.states[-1]
    offsets, ids, valid = dev.locate_csr(unshifted, False)
    assert not valid.any() and ids.size == 0


def components_by_the_reference_rule(gbwt, paths):
    """What check_components takes, from components_expect over the oracle's records: a node exists where its FORWARD record holds an edge
    (GBZ::has_node), which the path union-find of tangled_graphs does not know -- it differs where a node is visited in reverse alone."""
    comps = X_components.components(gbwt)
    want = TG.Expected([])
    want.paths = paths
    want.min_node, want.slots = X_components.geometry(gbwt)
    want.offsets = np.cumsum([0] + [len(c) for c in comps]).astype(np.uint64)
    want.ids = np.array([v for c in comps for v in c], dtype=np.uint64)
    where = {node: k for k, c in enumerate(comps) for node in c}
    firsts = X_components.first_nodes(gbwt, paths, 1)
    want.path_component = np.array([TG.NONE if f is None else where.get(f, TG.NONE) for f in firsts], dtype=np.uint32)
    return want


@pytest.mark.parametrize("share", [1.0, 0.5], ids=["all-reverse", "half-reverse"])
def test_even_alphabet_offset_extraction_and_components(share):
    """A unidirectional set whose smallest node is a reverse visit: that node is odd and alphabet_offset even.  With all visits reverse (the
    first case) no forward record holds an edge, so by the reference's rule the graph has no node at all; the second case has nodes in
    components.  At `straddle` only."""
    paths, bidirectional = TG.permuted_path(n=20000 if share < 1 else 100000, share=share, bidirectional=False)
    at = int(np.flatnonzero(paths[0] >> np.uint64(1) == 1)[0])
    paths[0][at] |= np.uint64(1)                                         # the visit of id 1 is reverse
    d = SG.SHIFTS(SG.max_id_of(paths))["straddle"]
    shifted = SG.shift_paths(paths, d)
    s = S.Synth.from_paths(shifted, bidirectional=False)
    assert s.alphabet_offset % 2 == 0 and s.alphabet_offset == 2 * (1 + d) and s.alphabet_offset < (1 << 31) < s.alphabet_size
    want = components_by_the_reference_rule(oracle_of(s), len(paths))
    assert want.min_node == 1 + d and (want.components == 0 if share == 1.0 else want.nodes > 5000)
    for flags in (_lib.OPEN_ALL, _lib.OPEN_EXTRACT):
        dev = bare(s, flags)
        offsets, nodes = dev.sequences_csr([0])
        assert offsets.tolist() == [0, shifted[0].size] and np.array_equal(np.asarray(nodes).astype(np.uint64), shifted[0])
        check_components(dev, want)


# ---- walks ----------------------------------------------------------------------------------------------------------------------------------------

CHAINS = {
    "main": dict(sites=800, haplotypes=64, alleles=2, extra=2, indel_every=2, chop=3),
    "high-degree": dict(sites=300, haplotypes=100, alleles=5),
}
WALK_ENVS = [{}, {"GBWT_HIP_CHAINS": "0"}, {"GBWT_HIP_CHAINS": "6"}, {"GBWT_HIP_SAMPLE_INTERVAL": "8"}, {"GBWT_HIP_SEGMENTS": "0"},
             {"GBWT_HIP_WIDE_ADDRESSES": "1"}, {"GBWT_HIP_DIRECT": "0"}]


class Walk:
    """A chain rebuilt from its own paths, shifted; the expected rows of all sequences and the oracle's checksums of them."""

    def __init__(self, name, shift):
        chain = S.Synth.chain(**CHAINS[name])
        plain = [chain.path(h).astype(np.uint64) for h in range(chain.paths)]
        self.d = SG.SHIFTS(SG.max_id_of(plain))[shift]
        self.paths = SG.shift_paths(plain, self.d)
        self.synth = S.Synth.from_paths(self.paths)
        self.oracle = oracle_of(self.synth)
        self.ids = np.arange(self.synth.sequences, dtype=np.uint64)
        rows = [r for p in self.paths for r in (p, p[::-1] ^ np.uint64(1))]
        self.offsets = np.cumsum([0] + [r.size for r in rows]).astype(np.uint64)
        self.nodes = np.concatenate(rows)
        self.steps, self.lengths, self.sums, self.hashes = self.oracle.extract_checksums(self.ids, 8)

    def check(self, dev):
        offsets, nodes = dev.sequences_csr(self.ids)
        assert np.array_equal(offsets, self.offsets)
        assert np.array_equal(np.asarray(nodes).astype(np.uint64), self.nodes)
        rows = dev.extract_device(self.ids)
        assert int(rows.total) == self.steps == self.nodes.size
        n = self.ids.size
        assert np.array_equal(np.diff(dev.last_offsets(n)), self.lengths)
        assert np.array_equal(dev.path_sums(n), self.sums) and np.array_equal(dev.path_hashes(n), self.hashes)
        return rows


_walks = {}


def walk_of(name, shift):
    if (name, shift) not in _walks:
        _walks[(name, shift)] = Walk(name, shift)
    return _walks[(name, shift)]


def test_chain_rebuilt_from_its_paths_has_the_chain_records():
    for name, visits in (("main", 383118), ("high-degree", None)):
        chain = S.Synth.chain(**CHAINS[name])
        again = S.Synth.from_paths([chain.path(h) for h in range(chain.paths)])
        assert bytes(again.data()) == bytes(chain.data()) and np.array_equal(again.starts(), chain.starts()) and header(again) == header(chain)
        if visits is not None:
            assert (chain.size - chain.sequences) // 2 == visits and max(len(chain.path(h)) for h in range(chain.paths)) == 6108


@pytest.mark.parametrize("env", WALK_ENVS, ids=lambda e: ",".join(f"{k[9:]}={v}" for k, v in e.items()) or "defaults")
@pytest.mark.parametrize("name", sorted(CHAINS))
@pytest.mark.parametrize("shift", SHIFTS)
def test_walks_under_every_knob(monkeypatch, shift, name, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    walk = walk_of(name, shift)
    if shift == "top":
        assert walk.synth.alphabet_size == 1 << 32 and int(walk.nodes.min()) >= 1 << 31
    walk.check(bare(walk.synth))


@pytest.mark.parametrize("shift", SHIFTS)
def test_walks_lean_handle_and_rows_back_to_the_index(shift):
    walk = walk_of("main", shift)
    lean = bare(walk.synth, _lib.OPEN_EXTRACT)
    walk.check(lean)
    full = bare(walk.synth)
    even = walk.ids[0::2]
    rows = full.extract_device(even)
    built = G.GBWT.from_rows_device(rows, even.size, bidirectional=True)
    assert_same_index(built, walk.synth.data(), walk.synth.starts(), header(walk.synth))
    from_host = G.GBWT.from_paths(walk.paths)                            # ... and the same from the host's paths
    assert_same_index(from_host, walk.synth.data(), walk.synth.starts(), header(walk.synth))


# ---- search -----------------------------------------------------------------------------------------------------------------------------------------

def cyclic_random_paths(seed=12):
    """The cyclic set of tests/test_gpu_parity.py::test_random_path_sets."""
    rng = random.Random(seed)
    paths = []
    for _ in range(40):
        ln = rng.randint(0, 30)
        paths.append([2 * rng.randint(1, 12) + rng.randint(0, 1) for _ in range(ln)])
    paths[0] = [2, 4, 6]
    return [np.array(p, dtype=np.uint64) for p in paths]


def search_domain(s, own_nodes):
    """The nodes the checks go through: these nodes of the index, the ones around both ends of its alphabet -- alphabet_offset and
    alphabet_size (2^32 at `top`: a 64-bit value) among them --, the endmarker, and unshifted nodes."""
    lo, hi = s.alphabet_offset, s.alphabet_size
    return sorted(set(int(v) for v in own_nodes) | {0, 1, 2, 3, 24, lo - 1, lo, lo + 1, lo + 2, hi - 2, hi - 1, hi, hi + 1})


@pytest.mark.parametrize("shift", SHIFTS)
def test_search_cyclic_random_set(shift):
    plain = cyclic_random_paths()
    d = SG.SHIFTS(SG.max_id_of(plain))[shift]
    paths = SG.shift_paths(plain, d)
    s = S.Synth.from_paths(paths)
    dev, oracle = bare(s), oracle_of(s)
    nodes_used = sorted({int(x) for p in paths for x in p} | {int(x) ^ 1 for p in paths for x in p})
    domain = search_domain(s, range(s.alphabet_offset + 1, s.alphabet_size))
    assert {s.alphabet_offset, s.alphabet_size, 2} <= set(domain)
    check_all_positions(dev, oracle, nodes=domain)
    check_search(dev, oracle, nodes_used[:24], nodes=domain)
    check_follow(dev, oracle, nodes=domain, bogus_nodes=(s.alphabet_offset, 2, 3))


@pytest.mark.parametrize("shift", SHIFTS)
def test_search_main_chain(shift):
    walk = walk_of("main", shift)
    s, oracle = walk.synth, walk.oracle
    dev = bare(s)
    rng = np.random.default_rng(27)
    sample = rng.choice(np.unique(walk.nodes), size=48, replace=False).tolist() + [s.alphabet_offset + 1, s.alphabet_size - 1]
    domain = search_domain(s, sample)
    assert {s.alphabet_offset, s.alphabet_size, 2} <= set(domain)
    check_all_positions(dev, oracle, nodes=domain)
    check_search(dev, oracle, sample[:8], nodes=domain)
    check_follow(dev, oracle, limit=128, nodes=domain, bogus_nodes=(s.alphabet_offset, 2, 3))


# ---- merging and removal ----------------------------------------------------------------------------------------------------------------------------

def merge_cases(tangle_paths):
    joins, _ = TG.reverse_joins()
    return {"tangle-even-odd": (tangle_paths[0::2], tangle_paths[1::2]), "reverse-joins-long-paths": ([joins[0]], [joins[1]])}


@pytest.mark.parametrize("algorithm", [G.MERGE_INSERT, G.MERGE_REBUILD], ids=["insert", "rebuild"])
@pytest.mark.parametrize("case", ["tangle-even-odd", "reverse-joins-long-paths"])
@pytest.mark.parametrize("shift", SHIFTS)
def test_merge_is_the_construction_over_both(tangle_base, shift, case, algorithm):
    plain_a, plain_b = merge_cases(tangle_base.paths)[case]
    d = SG.SHIFTS(SG.max_id_of(list(plain_a) + list(plain_b)))[shift]
    paths_a, paths_b = SG.shift_paths(plain_a, d), SG.shift_paths(plain_b, d)
    witness = S.Synth.from_paths(paths_a + paths_b)
    a, b = G.GBWT.from_paths(paths_a), G.GBWT.from_paths(paths_b)
    if case == "reverse-joins-long-paths":
        assert b.alphabet_offset() - a.alphabet_offset() == 2 * (100000 // 3)       # the inputs' offsets differ by a third of the graph
    merged = G.GBWT.merge(a, b, algorithm=algorithm)
    assert_same_index(merged, witness.data(), witness.starts(), header(witness))
    assert merged.last_merge_info()["algorithm_used"] == algorithm


@pytest.mark.parametrize("algorithm", [G.MERGE_INSERT, G.MERGE_REBUILD], ids=["insert", "rebuild"])
def test_merge_across_the_whole_id_range_is_refused(algorithm):
    """An input at d = 0 and one at `top`: 2^32 - 2 records between them.  Refused, not wrapped."""
    plain = [np.array([TG.fwd(1), TG.rev(2), TG.fwd(3)], dtype=np.uint64)]
    low = G.GBWT.from_paths(plain)
    high = G.GBWT.from_paths(SG.shift_paths(plain, SG.SHIFTS(3)["top"]))
    assert high.alphabet_size() == 1 << 32
    for a, b in ((low, high), (high, low)):
        with pytest.raises(G.GbwtHipError) as e:
            G.GBWT.merge(a, b, algorithm=algorithm)
        assert e.value.status == _lib.UNSUPPORTED and TOO_MANY_RECORDS in str(e.value)
    offsets, nodes = high.sequences_csr([0])                              # the inputs still answer
    assert np.asarray(nodes).astype(np.uint64).tolist() == SG.shift_paths(plain, SG.SHIFTS(3)["top"])[0].tolist()


@pytest.mark.parametrize("algorithm", [G.REMOVE_DELETE, G.REMOVE_REBUILD], ids=["delete", "rebuild"])
@pytest.mark.parametrize("shift", SHIFTS)
def test_removing_the_path_of_the_smallest_ids_moves_the_offset(shift, algorithm):
    joins, _ = TG.reverse_joins()
    plain = joins[1:] + joins[:1]                                         # the descending path over ids 1 .. n / 3 last: merging it back restores the order
    d = SG.SHIFTS(SG.max_id_of(plain))[shift]
    paths = SG.shift_paths(plain, d)
    others = np.unique(np.concatenate(plain[:-1]) >> np.uint64(1))
    smallest_kept = int(others[0])
    assert smallest_kept == 3333 and int(plain[-1].min()) >> 1 == 1       # ids 1 .. 3332 are on that path alone
    x = G.GBWT.from_paths(paths)
    whole = S.Synth.from_paths(paths)
    assert_same_index(x, whole.data(), whole.starts(), header(whole))
    last = len(paths) - 1
    head = x.remove_paths([last], algorithm=algorithm)
    witness = S.Synth.from_paths(paths[:-1])
    assert_same_index(head, witness.data(), witness.starts(), header(witness))
    assert head.alphabet_offset() == 2 * (smallest_kept + d) - 1 and x.alphabet_offset() == 2 * (1 + d) - 1
    assert head.last_remove_info()["algorithm_used"] == algorithm
    back = G.GBWT.from_paths(paths[-1:])
    for merge_algorithm in (G.MERGE_INSERT, G.MERGE_REBUILD):
        assert_same_index(G.GBWT.merge(head, back, algorithm=merge_algorithm), whole.data(), whole.starts(), header(whole))
