"""The bases of GBZ paths (gbz-extract's `sequences` mode, src/bin/gbz-extract.rs:173-194, 266-294) through the device against values built
without the library: node labels from the S-lines of the oracle's GFA, paths from the oracle's walk, bytes put together in numpy
(tests/seq_expect.py)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import gbwt_rs_amd as G
import oracle_lib as O
import seq_expect as E
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S

pytestmark = pytest.mark.gpu

FIXTURES = ["example.gbz", "example-v1.gbz", "translation.gbz", "translation-v1.gbz"]


def expected_for_fixture(oracle, n_paths, reverse, endmarker, ids=None, translated=False):
    """Expected rows of a golden GBZ: node labels for plain graphs; segment labels along GBZ::segment_path for translation graphs."""
    gfa = oracle.gfa()
    ids = list(range(n_paths)) if ids is None else ids
    n_seq = 2 * n_paths
    seq_ids = [2 * p + int(reverse) for p in ids]
    if translated:
        # segments by name: the S-lines, and the segments of every forward path from its W-line (the oracle's segment_path as text); the
        # reverse path is the same segments backwards, each the other way round
        labels = E.s_lines(gfa)
        index = {name: j for j, name in enumerate(labels)}
        table = E.LabelTable({j: labels[name] for name, j in index.items()})
        rows = []
        for p, s in zip(ids, seq_ids):
            if s >= n_seq:
                rows.append(None)
                continue
            walk = oracle.path_lines([p], 1).rstrip(b"\n").split(b"\t")[6].replace(b">", b" >").replace(b"<", b" <").split()
            toks = [(index[t[1:]], t[:1] == b"<") for t in walk]
            if reverse:
                toks = [(j, not r) for j, r in toks[::-1]]
            rows.append(([j for j, _ in toks], [r for _, r in toks]))
    else:
        table = E.LabelTable.from_gfa(gfa)
        csr = oracle.gbwt().extract(np.array([min(s, n_seq - 1) for s in seq_ids], dtype=np.uint64))
        rows = E.node_rows(csr, seq_ids, n_seq)
    return E.expected_rows(table, rows, endmarker)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_every_path_both_orientations(name):
    path = os.path.join(O.GOLDEN, name)
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    translated = bool(G.parse_file(path).has_translation)
    ids = list(range(dev.paths()))
    for reverse in (False, True):
        for endmarker in (None, 0, ord("$")):
            offsets, data = dev.path_sequences(ids, G.REVERSE if reverse else G.FORWARD, endmarker)
            e_off, e_data = expected_for_fixture(oracle, dev.paths(), reverse, endmarker, translated=translated)
            assert offsets.tolist() == e_off.tolist(), (reverse, endmarker)
            assert data == e_data, (reverse, endmarker)
    # the paths in another order, one of them twice
    order = ids[::-1] + ids[:1]
    assert dev.path_sequences(order)[1] == expected_for_fixture(oracle, dev.paths(), False, None, order, translated)[1]


def test_example_gbz_against_golden_gfa():
    dev = G.GBZ.load(os.path.join(O.GOLDEN, "example.gbz"))
    gfa = open(os.path.join(O.GOLDEN, "example.gfa"), "rb").read()
    table = E.LabelTable.from_gfa(gfa)
    rows = []
    for line in gfa.split(b"\n"):                       # every P- and W-line of the golden file, in file order = path id order
        f = line.split(b"\t")
        if line.startswith(b"P\t"):
            steps = f[2].split(b",")
            rows.append(([int(s[:-1]) for s in steps], [s.endswith(b"-") for s in steps]))
        elif line.startswith(b"W\t"):
            walk = f[6].replace(b">", b" >").replace(b"<", b" <").split()
            rows.append(([int(s[1:]) for s in walk], [s[:1] == b"<" for s in walk]))
    assert len(rows) == dev.paths()
    offsets, data = dev.path_sequences(range(dev.paths()), endmarker=0)
    e_off, e_data = E.expected_rows(table, rows, 0)
    assert offsets.tolist() == e_off.tolist() and data == e_data
    for node, label in E.s_lines(gfa).items():
        assert dev.node_sequence(int(node)) == label
    assert dev.node_sequence(0) is None and dev.node_sequence(10) is None and dev.node_sequence(1 << 40) is None


def test_complement_table_with_a_rewritten_alphabet(tmp_path):
    """example-v1.gbz with its label alphabet ACGT (the 4-byte Vec<u8> at offset 1 696, behind its length word) rewritten to aCnR: lower
    case is kept forwards and complemented backwards, N and IUPAC codes become N."""
    raw = bytearray(open(os.path.join(O.GOLDEN, "example-v1.gbz"), "rb").read())
    assert raw[1688:1700] == (4).to_bytes(8, "little") + b"ACGT"
    raw[1696:1700] = b"aCnR"
    path = tmp_path / "alphabet.gbz"
    path.write_bytes(bytes(raw))
    dev, oracle = G.GBZ.load(str(path)), O.OracleGBZ(str(path))
    assert set(b"".join(E.s_lines(oracle.gfa()).values())) <= set(b"aCnR")
    ids = list(range(dev.paths()))
    fwd = dev.path_sequences(ids)[1]
    rev = dev.path_sequences(ids, G.REVERSE)[1]
    assert fwd == expected_for_fixture(oracle, dev.paths(), False, None)[1]
    assert rev == expected_for_fixture(oracle, dev.paths(), True, None)[1]
    # path 0 has forward nodes only (P-line A of example.gfa): its bases keep the rewritten alphabet, its reverse is T, G and N
    p_fwd, p_rev = dev.path_sequences([0])[1], dev.path_sequences([0], G.REVERSE)[1]
    assert set(p_fwd) <= set(b"aCnR") and b"a" in p_fwd and (b"n" in p_fwd or b"R" in p_fwd)
    assert set(p_rev) <= set(b"TGN") and b"T" in p_rev and b"N" in p_rev
    assert set(fwd) | set(rev) <= set(b"aCnRTGN")


def synthetic(tmp_path, name, make):
    path = str(tmp_path / name)
    make().save(path, as_gbz=True)
    oracle = O.OracleGBZ(path)
    return path, oracle, E.LabelTable.from_gfa(oracle.gfa())


def expected_synthetic(oracle, table, n_seq, seq_ids, endmarker):
    ids = np.array([min(s, n_seq - 1) for s in seq_ids], dtype=np.uint64)
    return E.expected_rows(table, E.node_rows(oracle.gbwt().extract(ids), seq_ids, n_seq), endmarker)


def test_synthetic_genome_every_byte_and_cached_sizes(tmp_path, monkeypatch):
    path, oracle, table = synthetic(tmp_path, "genome.gbz", lambda: S.Synth.genome(contigs=8, fragments=6, haplotypes=64, sites=40, labels=1))
    dev = G.GBZ.load(path)
    n = dev.paths()
    assert n >= 2000 and table.len.max() == 1024
    ids = np.arange(n, dtype=np.uint64)
    f_off, f_data = dev.path_sequences(ids, endmarker=0)                 # forward: sizes from the line cache of the index
    e_off, e_data = expected_synthetic(oracle, table, 2 * n, 2 * ids, 0)
    assert f_off.tolist() == e_off.tolist() and f_data == e_data
    r_off, r_data = dev.path_sequences(ids, G.REVERSE)                   # reverse: sizes from the pass over the label lengths
    e_off, e_data = expected_synthetic(oracle, table, 2 * n, 2 * ids + 1, None)
    assert r_off.tolist() == e_off.tolist() and r_data == e_data
    assert np.array_equal(np.diff(f_off) - 1, np.diff(r_off))
    monkeypatch.setenv("GBWT_HIP_LINE_CACHE", "0")                       # (read at open) a handle without the line cache sizes every row itself
    plain = G.GBZ.load(path)
    p_off, p_data = plain.path_sequences(ids, endmarker=0)
    assert np.array_equal(p_off, f_off) and p_data == f_data
    # a shuffled sample through the device-resident form and the copy-out of the same request
    rng = np.random.default_rng(7)
    sample = rng.permutation(n)[:300].astype(np.uint64)
    lines = dev.path_sequences_device(sample)
    s_off, s_data = dev.path_sequences(sample)
    assert lines.n == sample.size and lines.total == len(s_data)
    assert s_data == expected_synthetic(oracle, table, 2 * n, 2 * sample, None)[1]
    walk_ms, sizes_ms, bases_ms = dev.last_sequences_ms()
    assert walk_ms > 0 and bases_ms > 0


def test_long_rows_cross_chunks_and_batches(tmp_path):
    """Rows of 12 000 positions (three chunks of 4 096, twelve batches of 1 024 in the bases kernel), labels of 1 .. 1 024 bases."""
    path, oracle, table = synthetic(tmp_path, "chain.gbz", lambda: S.Synth.chain(sites=2000, haplotypes=6, labels=1, chop=3, seed=3))
    dev = G.GBZ.load(path)
    n = dev.paths()
    for reverse in (0, 1):
        ids = list(range(n)) + [0]
        offsets, data = dev.path_sequences(ids, reverse, endmarker=255)
        e_off, e_data = expected_synthetic(oracle, table, 2 * n, [2 * p + reverse for p in ids], 255)
        assert offsets.tolist() == e_off.tolist() and data == e_data
        # one path at a time: every 16-byte alignment of a row start the batch above did not give
        for p in range(n):
            assert dev.path_sequences([p], reverse)[1] == e_data[int(e_off[p]):int(e_off[p + 1]) - 1]


def test_edge_cases(tmp_path):
    path = os.path.join(O.GOLDEN, "example.gbz")
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    n = dev.paths()
    # out-of-range ids: empty rows without endmarker, next to real ones
    offsets, data = dev.path_sequences([n, 0, 1 << 62, n - 1], endmarker=0)
    e_off, e_data = expected_for_fixture(oracle, n, False, 0, [n, 0, 1 << 62, n - 1])
    assert offsets.tolist() == e_off.tolist() and data == e_data and offsets[1] == 0 and offsets[3] == offsets[2]
    # empty batch
    offsets, data = dev.path_sequences([])
    assert offsets.tolist() == [0] and data == b""
    assert dev.path_sequences_device([]).total == 0
    # a bad endmarker
    for bad in (-2, 256):
        with pytest.raises(ValueError):
            dev.path_sequences([0], endmarker=bad)
        with pytest.raises(G.GbwtHipError) as e:
            ids, total = np.zeros(1, dtype=np.uint64), C.c_uint64(0)
            _lib.check(dev._L.gbwt_hip_path_sequences(dev._h, dev._ws, ids.ctypes.data, 1, 0, bad, None, None, 0, C.byref(total)))
        assert e.value.status == _lib.BAD_ARGUMENT
    # out= must be a writable contiguous uint8 array
    with pytest.raises(TypeError):
        dev.path_sequences([0], out=np.zeros(64, dtype=np.int32))
    frozen = np.zeros(64, dtype=np.uint8)
    frozen.flags.writeable = False
    with pytest.raises(TypeError):
        dev.path_sequences([0], out=frozen)
    buf = np.zeros(4096, dtype=np.uint8)
    offsets, view = dev.path_sequences([0, 1], out=buf)
    assert view.base is buf and view.tobytes() == dev.path_sequences([0, 1])[1]
    # a bare GBWT, a GBZ handle without EXTRACT
    gbwt = G.GBWT.load(os.path.join(O.GOLDEN, "example.gbwt"))
    total, ids = C.c_uint64(0), np.zeros(1, dtype=np.uint64)
    assert gbwt._L.gbwt_hip_path_sequences(gbwt._h, gbwt._ws, ids.ctypes.data, 1, 0, -1, None, None, 0, C.byref(total)) == _lib.BAD_ARGUMENT
    length, found = C.c_uint64(0), C.c_uint8(0)
    assert gbwt._L.gbwt_hip_node_sequence(gbwt._h, 12, None, 0, C.byref(length), C.byref(found)) == _lib.BAD_ARGUMENT
    search_only = G.GBZ.load(path, flags=_lib.OPEN_SEARCH)
    with pytest.raises(G.GbwtHipError) as e:
        search_only.path_sequences([0])
    assert e.value.status == _lib.BAD_ARGUMENT
    assert search_only.node_sequence(11) == dev.node_sequence(11)       # (host image: no extraction needed)
    # size query, then the fill call: one walk
    em = 0
    assert dev._L.gbwt_hip_path_sequences(dev._h, dev._ws, np.array([2, 3], dtype=np.uint64).ctypes.data, 2, 1, em, None, None, 0, C.byref(total)) == 0
    want = total.value
    walk_before = dev.last_sequences_ms()
    out = np.zeros(want, dtype=np.uint8)
    small = np.zeros(max(want - 1, 1), dtype=np.uint8)
    ids2 = np.array([2, 3], dtype=np.uint64)
    assert dev._L.gbwt_hip_path_sequences(dev._h, dev._ws, ids2.ctypes.data, 2, 1, em, small.ctypes.data, None, small.size, C.byref(total)) == _lib.CAPACITY
    assert dev._L.gbwt_hip_path_sequences(dev._h, dev._ws, ids2.ctypes.data, 2, 1, em, out.ctypes.data, None, out.size, C.byref(total)) == 0
    assert dev.last_sequences_ms() == walk_before                       # the same events: nothing was launched again
    assert out.tobytes() == expected_for_fixture(oracle, n, True, 0, [2, 3])[1]


def test_labels_made_once_on_first_request(tmp_path):
    """The labels reach HBM with the first request for bases, not at open; two workspaces asking at once see one upload."""
    path, oracle, table = synthetic(tmp_path, "genome.gbz", lambda: S.Synth.genome(contigs=4, fragments=3, haplotypes=16, sites=30, labels=1, seed=4))
    dev = G.GBZ.load(path)
    other = dev.another_workspace()
    before = dev.memory_usage()
    results, errors = [None, None], []
    ids = np.arange(dev.paths(), dtype=np.uint64)
    barrier = threading.Barrier(2)

    def ask(k, handle):
        try:
            barrier.wait()
            results[k] = handle.path_sequences(ids, endmarker=0)
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append(e)

    threads = [threading.Thread(target=ask, args=(0, dev)), threading.Thread(target=ask, args=(1, other))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    after = dev.memory_usage()
    e_off, e_data = expected_synthetic(oracle, table, 2 * dev.paths(), 2 * ids, 0)
    for off, data in results:
        assert off.tolist() == e_off.tolist() and data == e_data
    grown = after["index_device_bytes"] - before["index_device_bytes"]
    n_labels, n_bytes = table.len.size, int(table.len.sum())           # (the S-lines hold the labels of the nodes that exist; the handle uploads every potential one)
    assert grown >= n_bytes + 8 * n_labels
    assert grown < 2 * (n_bytes + 8 * n_labels) + (1 << 16)
    dev.path_sequences(ids[:3])
    assert dev.memory_usage()["index_device_bytes"] == after["index_device_bytes"]


def test_write_sequences_one_and_many_batches(tmp_path, monkeypatch):
    path, oracle, table = synthetic(tmp_path, "genome.gbz", lambda: S.Synth.genome(contigs=6, fragments=4, haplotypes=24, sites=150, labels=1, seed=9))
    dev = G.GBZ.load(path)
    n = dev.paths()
    ids = np.arange(n, dtype=np.uint64)
    e_off, e_data = expected_synthetic(oracle, table, 2 * n, 2 * ids, 0)
    for budget in (None, "1"):                                         # default: one batch; 1 MiB: many batches
        if budget is None:
            monkeypatch.delenv("GBWT_HIP_SEQ_BATCH_MIB", raising=False)
        else:
            monkeypatch.setenv("GBWT_HIP_SEQ_BATCH_MIB", budget)
        out = tmp_path / f"out{budget}"
        dev.write_sequences(str(out))
        assert out.read_bytes() == e_data
        lines = out.with_name(out.name + ".names").read_bytes().decode().splitlines()
        assert len(lines) == n
        for p, line in enumerate(lines):
            f = line.split("\t")
            assert f[0] == str(p) and int(f[5]) == int(e_off[p + 1] - e_off[p]) - 1
    assert len(e_data) > 3 << 20                                        # (so that 1 MiB batches are several)
    # a subset in the given order, another endmarker
    sub = [5, 1, 3]
    dev.write_sequences(str(tmp_path / "sub"), sub, endmarker=ord("#"))
    assert (tmp_path / "sub").read_bytes() == expected_synthetic(oracle, table, 2 * n, [2 * p for p in sub], ord("#"))[1]
    assert [l.split("\t")[0] for l in (tmp_path / "sub.names").read_text().splitlines()] == ["5", "1", "3"]
    with pytest.raises(G.GbwtHipError) as e:
        dev.write_sequences(str(tmp_path / "bad"), [n])
    assert e.value.status == _lib.BAD_ARGUMENT


def test_write_sequences_names_match_the_reference_format(tmp_path):
    """example.gbz: path_name_as_line (src/bin/gbz-extract.rs:191-194) -- sample and contig names, phase, fragment, bases."""
    path = os.path.join(O.GOLDEN, "example.gbz")
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    out = tmp_path / "example.seq"
    dev.write_sequences(str(out))
    e_off, e_data = expected_for_fixture(oracle, dev.paths(), False, 0)
    assert out.read_bytes() == e_data
    # the W-lines of the golden GFA carry sample, phase, contig, fragment of paths 2..5 (P-lines: the generic sample)
    gfa = open(os.path.join(O.GOLDEN, "example.gfa"), "rb").read().decode()
    walks = [l.split("\t") for l in gfa.splitlines() if l.startswith("W\t")]
    names = (tmp_path / "example.seq.names").read_text().splitlines()
    assert len(names) == dev.paths()
    for p, line in enumerate(names):
        f = line.split("\t")
        assert len(f) == 6 and f[0] == str(p) and int(f[5]) == int(e_off[p + 1] - e_off[p]) - 1
    for w, line in zip(walks, names[2:]):
        f = line.split("\t")
        assert (f[1], f[3], f[2], f[4]) == (w[1], w[2], w[3], w[4])
