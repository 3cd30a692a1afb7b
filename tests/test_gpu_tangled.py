"""Components, bases and tags through the device on the graphs of tests/tangled_graphs.py: topologies whose node ids run against their
edges across hundreds of workgroups, thousands of components with slots without nodes among them, a record of 5 000 edges -- against the
path union-find of that module (pinned to the oracle in tests/test_tangled_cpu.py) -- and labels of 1 to 70 000 bases on walks with mixed
orientation, repeats and revisits, a label of the largest accepted length, one base more, and 64 MiB out of one batch -- against
seq_expect / tags_expect over the oracle's S-lines and walks."""
import os

import numpy as np
import pytest

import gbwt_rs_amd as G
import oracle_lib as O
import seq_expect as E
import tags_expect as T
import tangled_graphs as TG
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S

pytestmark = pytest.mark.gpu

LARGEST_LABEL = 4194299                          # 1 024 * L + 16 * 256 + 16 <= 0xFFFFFFFF (sequences_compute)
TOO_LONG = "node labels too long for the bases kernel"


# ---- components -----------------------------------------------------------------------------------------------------------------------------

def check_components(dev, want):
    """The lists, the CSR, the counts of the device view and the component of every path, as numpy arrays."""
    offsets, ids = dev.components_csr()
    assert offsets.dtype == np.uint64 and ids.dtype == np.uint64
    assert np.array_equal(offsets, want.offsets) and np.array_equal(ids, want.ids)
    lists = dev.weakly_connected_components()
    assert len(lists) == want.components
    assert np.array_equal(np.array([c.size for c in lists], dtype=np.uint64), np.diff(want.offsets))
    assert np.array_equal(np.concatenate(lists) if lists else np.zeros(0, np.uint64), want.ids)
    view = dev.components_device()
    assert (view.min_node, view.slots, view.components, view.nodes, view.paths) == (want.min_node, want.slots, want.components, want.nodes, want.paths)
    got = dev.path_components(np.arange(want.paths, dtype=np.uint64))
    assert got.dtype == np.uint32 and np.array_equal(got, want.path_component)


@pytest.mark.parametrize("name", sorted(TG.COMPONENT_BUILDERS))
def test_components_of_every_topology_from_three_handles(tmp_path, name):
    paths, bidirectional = TG.COMPONENT_BUILDERS[name]()
    want = TG.Expected(paths)
    s = S.Synth.from_paths(paths, bidirectional=bidirectional)
    bare = lambda flags: G.GBWT.from_records(s.data(), s.starts(), s.alphabet_offset, s.alphabet_size, s.sequences, s.size, bidirectional, flags=flags)
    if bidirectional:
        path = str(tmp_path / "graph.gbz")
        s.attach_gbz(seed=3).save(path, as_gbz=True)
        handles = [G.GBZ.load(path), G.GBZ.load(path, flags=_lib.OPEN_EXTRACT), bare(_lib.OPEN_ALL)]
    else:                                        # (no GBZ of a unidirectional index: the bare handle, opened both ways)
        handles = [bare(_lib.OPEN_ALL), bare(_lib.OPEN_EXTRACT)]
    for dev in handles:
        check_components(dev, want)
    t = handles[0].last_components_ms()
    # what the build took, for the record (pytest -s): no bound on the launches is asserted
    print(f"\ncomponents[{name}]: slots={want.slots} records={2 * want.slots if bidirectional else want.slots} components={want.components} "
          f"hook_workgroups={(handles[0].alphabet_size() - handles[0].alphabet_offset() - 1 + 255) // 256} hook_launches={t['hook_launches']} "
          f"jump_launches={t['jump_launches']} hook_ms={t['hook_ms']:.3f} jump_ms={t['jump_ms']:.3f} shape_ms={t['shape_ms']:.3f}")
    assert t["hook_launches"] >= 2 and t["jump_launches"] >= 1
    if name in ("permuted-path", "zigzag", "grid"):
        assert t["hook_launches"] >= 3           # two passes that changed labels and the final one: links were lost or undone and repaired


# ---- the tangle: long labels on walks with mixed orientation --------------------------------------------------------------------------------------

class Tangle:
    def __init__(self, directory):
        self.lengths = TG.tangle_label_lengths()
        self.paths, _ = TG.tangle(lengths=self.lengths)
        self.n = len(self.paths)
        self.gbz = str(directory / "tangle.gbz")
        S.Synth.from_paths(self.paths).attach_gbz(seed=3, label_lengths=self.lengths).save(self.gbz, as_gbz=True)
        self.oracle = O.OracleGBZ(self.gbz)
        self.table = E.LabelTable.from_gfa(self.oracle.gfa())            # labels from the oracle's S-lines
        ids = np.arange(self.n, dtype=np.uint64)
        self.bases = []                                                  # [orientation][path]: bytes, rows from the oracle's walk
        for o in (0, 1):
            seq_ids = [2 * p + o for p in range(self.n)]
            offsets, data = E.expected_rows(self.table, E.node_rows(self.oracle.gbwt().extract(2 * ids + np.uint64(o)), seq_ids, 2 * self.n))
            self.bases.append([data[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])])
        self.rows = T.rows_of(self.oracle.gbwt().extract(2 * ids), self.n)
        self.dev = G.GBZ.load(self.gbz)

    def expected(self, order, reverse, endmarker):
        tail = b"" if endmarker is None else bytes([endmarker])
        parts = [self.bases[reverse][p] + tail for p in order]
        return np.cumsum([0] + [len(x) for x in parts]).astype(np.uint64), b"".join(parts)

    def tags(self, order):
        return T.tag_text(self.table.len, [self.rows[p] for p in order])


@pytest.fixture(scope="module")
def tangle(tmp_path_factory):
    return Tangle(tmp_path_factory.mktemp("tangle"))


def test_tangle_bases_all_paths_orders_orientations_endmarkers(tangle):
    dev, n = tangle.dev, tangle.n
    ids = list(range(n))
    shuffled = np.random.default_rng(21).permutation(n).tolist()
    shuffled = shuffled + shuffled[:3] + [shuffled[0]]
    for order, reverse, endmarker in ((ids, 0, 0), (ids, 1, None), (shuffled, 0, 255), (shuffled, 1, 0), (ids[::-1], 0, None)):
        offsets, data = dev.path_sequences(order, G.REVERSE if reverse else G.FORWARD, endmarker)
        e_off, e_data = tangle.expected(order, reverse, endmarker)
        assert np.array_equal(offsets, e_off), (reverse, endmarker)
        assert data == e_data, (reverse, endmarker)


@pytest.mark.parametrize("p", [k for k, length in enumerate(TG.TANGLE_PATH_LENGTHS) if length <= 4097])
def test_tangle_bases_of_every_boundary_length_path_alone(tangle, p):
    """Paths of 0, 1, 2 nodes and around the batch (1 024) and chunk (4 096) sizes of k_bases, each as a request of its own."""
    for reverse in (0, 1):
        for endmarker in (None, 0):
            offsets, data = tangle.dev.path_sequences([p], reverse, endmarker)
            e_off, e_data = tangle.expected([p], reverse, endmarker)
            assert np.array_equal(offsets, e_off) and data == e_data, (p, reverse, endmarker)


def test_tangle_write_sequences_and_names(tangle, tmp_path):
    out = tmp_path / "tangle.seq"
    tangle.dev.write_sequences(str(out))
    e_off, e_data = tangle.expected(range(tangle.n), 0, 0)
    assert out.read_bytes() == e_data
    lines = out.with_name(out.name + ".names").read_text().splitlines()
    assert [int(l.split("\t")[0]) for l in lines] == list(range(tangle.n))
    assert [int(l.split("\t")[5]) for l in lines] == [len(b) for b in tangle.bases[0]]


@pytest.mark.parametrize("mode", [G.PATHS_DEFAULT, G.PATHS_PAN_SN, G.PATHS_REF_ONLY])
def test_tangle_gfa_equals_the_oracle(tangle, tmp_path, mode):
    """The W-line end coordinates come from the summed label lengths of the line cache: here with labels of up to 70 000 bases."""
    out = tmp_path / "tangle.gfa"
    tangle.dev.write_gfa(str(out), mode)
    assert out.read_bytes() == tangle.oracle.gfa(mode)


@pytest.mark.parametrize("order_name", ["forward", "reversed", "duplicate"])
def test_tangle_tags_orders_and_suffix_arrays(tangle, order_name):
    dev, n = tangle.dev, tangle.n
    ids = list(range(n))
    order = {"forward": ids, "reversed": ids[::-1], "duplicate": ids + [n - 1]}[order_name]
    text, offsets = tangle.tags(order)
    assert dev.text_length(order) == text.size == int(offsets[-1])
    for sa in (np.random.default_rng(22).permutation(text.size).astype(np.uint64), np.arange(text.size, dtype=np.uint64)):
        tags, runs = dev.tag_array(order, sa, return_runs=True)
        want = T.gather(text, sa)
        assert np.array_equal(tags, want)
        assert np.array_equal(want, T.two_sorts(text, sa))
        assert runs == T.runs(want)


def write_sa(path, sa, lead=1):
    with open(path, "wb") as f:
        f.write(np.full(lead, 0xFFFFFFFFFFFFFFFF, dtype="<u8").tobytes())
        f.write(np.asarray(sa, dtype="<u8").tobytes())


def test_tangle_tag_files_batches_and_wide_plan(tangle, tmp_path, monkeypatch):
    dev, n = tangle.dev, tangle.n
    ids = np.arange(n, dtype=np.uint64)
    text, _ = tangle.tags(range(n))
    sa = np.random.default_rng(23).permutation(text.size).astype(np.uint64)
    want = T.gather(text, sa)
    base = str(tmp_path / "tangle")
    dev.write_sequences(base)
    write_sa(base + ".sa", sa)
    monkeypatch.delenv("GBWT_HIP_TAG_BATCH_MIB", raising=False)
    assert dev.write_tag_array(base) == T.runs(want)
    assert np.array_equal(np.fromfile(base + ".tags", dtype="<u8"), want)
    os.remove(base + ".tags")
    monkeypatch.setenv("GBWT_HIP_TAG_BATCH_MIB", "1")
    assert 8 * text.size > 32 << 20
    assert dev.write_tag_array(base) == T.runs(want)
    assert np.array_equal(np.fromfile(base + ".tags", dtype="<u8"), want)
    # the plan scanned in pieces and with 64-bit hints, on a workspace of its own
    monkeypatch.setenv("GBWT_HIP_SCAN_PIECE", "4096")
    monkeypatch.setenv("GBWT_HIP_TAG_WIDE", "1")
    other = dev.another_workspace()
    assert sum(TG.TANGLE_PATH_LENGTHS) > 8 * 4096
    tags, runs = other.tag_array(ids, sa, return_runs=True)
    assert np.array_equal(tags, want) and runs == T.runs(want)


# ---- labels at and past the limit of the bases kernel ------------------------------------------------------------------------------------------

def labelled(tmp_path, lengths, paths, name):
    gbz = str(tmp_path / name)
    S.Synth.from_paths(paths).attach_gbz(seed=5, label_lengths=lengths).save(gbz, as_gbz=True)
    return gbz, O.OracleGBZ(gbz)


def test_largest_accepted_label(tmp_path):
    lengths, paths = TG.long_label(LARGEST_LABEL)
    gbz, oracle = labelled(tmp_path, lengths, paths, "largest.gbz")
    dev = G.GBZ.load(gbz)
    table = E.LabelTable.from_gfa(oracle.gfa())
    assert table.len.tolist() == [0, 1, LARGEST_LABEL, 1]
    for reverse in (0, 1):
        rows = E.node_rows(oracle.gbwt().extract([reverse]), [reverse], 2)
        e_off, e_data = E.expected_rows(table, rows, 0)
        offsets, data = dev.path_sequences([0], reverse, 0)
        assert np.array_equal(offsets, e_off) and len(data) == 3 * LARGEST_LABEL + 3
        assert data == e_data
    text, offsets = T.oracle_text(oracle, [0], table.len)
    assert dev.text_length([0]) == text.size == 3 * LARGEST_LABEL + 3
    tags, runs = dev.tag_array([0], np.arange(text.size, dtype=np.uint64), return_runs=True)
    assert np.array_equal(tags, text) and runs == T.runs(text)
    assert int(tags[LARGEST_LABEL]) == (2 << 11) + LARGEST_LABEL - 1 and int(tags[3 * LARGEST_LABEL]) == ((2 << 11) | (1 << 10)) + LARGEST_LABEL - 1


def test_one_base_more_is_refused_and_the_handle_stays_good(tmp_path):
    lengths, paths = TG.long_label(LARGEST_LABEL + 1)
    gbz, oracle = labelled(tmp_path, lengths, paths, "toolong.gbz")
    dev = G.GBZ.load(gbz)
    for reverse in (0, 1):
        with pytest.raises(G.GbwtHipError) as e:
            dev.path_sequences([0], reverse)
        assert e.value.status == _lib.UNSUPPORTED and TOO_LONG in str(e.value)
    out = tmp_path / "refused.seq"
    with pytest.raises(G.GbwtHipError) as e:
        dev.write_sequences(str(out))
    assert e.value.status == _lib.UNSUPPORTED and TOO_LONG in str(e.value)
    assert not out.exists() and not out.with_name(out.name + ".names").exists()
    # the same handle afterwards: the walk, the tags (a plain addition, whatever the length) and the components
    o_off, o_nodes = oracle.gbwt().extract([0, 1])
    offsets, nodes = dev.sequences_csr([0, 1])
    assert np.array_equal(offsets, o_off) and np.array_equal(nodes, o_nodes) and nodes.tolist()[:5] == paths[0].tolist()
    text, _ = T.oracle_text(oracle, [0], np.array([0, 1, LARGEST_LABEL + 1, 1]))
    assert dev.text_length([0]) == text.size == 3 * (LARGEST_LABEL + 1) + 3
    sa = np.random.default_rng(24).integers(0, text.size, size=1 << 20).astype(np.uint64)
    sa[:4] = [0, LARGEST_LABEL + 1, 3 * (LARGEST_LABEL + 1), text.size - 1]
    assert np.array_equal(dev.tag_array([0], sa), T.gather(text, sa))
    want = TG.Expected(paths)
    check_components(dev, want)
    assert want.lists() == [[1, 2, 3]]


def test_sixty_four_mebibytes_out_of_one_batch(tmp_path):
    """One node of 1 MiB visited 64 times in a row in alternating orientation: the byte offsets inside one batch of k_bases reach 2^26.  Compared
    on the device; the host sees the label and a few sums."""
    import torch
    from gbwt_rs_amd import dist
    length, visits = 1 << 20, 64
    lengths, paths = TG.self_loop(length, visits)
    gbz, oracle = labelled(tmp_path, lengths, paths, "loop.gbz")
    labels = {int(k): v for k, v in E.s_lines(oracle.gfa()).items()}
    assert [len(labels[k]) for k in (1, 2, 3)] == [1, length, 1]
    table = E.LabelTable(labels)
    device = torch.device("cuda", 0)
    forward = torch.from_numpy(table.bases([2], [False])).to(device)
    backward = torch.from_numpy(table.bases([2], [True])).to(device)
    dev = G.GBZ.load(gbz)
    for reverse in (0, 1):
        lines = dev.path_sequences_device([0], reverse, 0)
        assert lines.n == 1 and lines.total == visits * length + 3
        offsets, text = dist.lines_tensors(lines, device)
        assert offsets.tolist() == [0, visits * length + 3]
        ends = (labels[3], labels[1]) if reverse else (labels[1], labels[3])
        if reverse:
            ends = tuple(bytes(E.COMPLEMENT[list(x)]) for x in ends)
        assert bytes(text[:1].tolist()) == ends[0] and bytes(text[-2:].tolist()) == ends[1] + b"\0"
        body = text[1:1 + visits * length].view(visits, length)
        # forward path: fwd, rev, fwd, ...; reverse path: the visits backwards and flipped -- fwd, rev, ... again
        assert torch.equal(body[0::2], forward.expand(visits // 2, length))
        assert torch.equal(body[1::2], backward.expand(visits // 2, length))
