"""gbz-extract's `tag-array` mode (src/bin/gbz-extract.rs:296-482) through the device, every tag compared with values built without the
library (tests/tags_expect.py): paths from the oracle's walk, label lengths from the S-lines of the oracle's GFA, the tag formula in numpy."""
import ctypes as C
import os

import numpy as np
import pytest

import gbwt_rs_amd as G
import oracle_lib as O
import seq_expect as E
import tags_expect as T
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S

pytestmark = pytest.mark.gpu

FIXTURES = ["example.gbz", "example-v1.gbz", "translation.gbz", "translation-v1.gbz"]
SKIPPED = np.uint64(0xFFFFFFFFFFFFFFFF)                # the value in front of a suffix array file (sa_skip = 1): never read


def fixture_text(dev, oracle, translated):
    """(node label lengths, bases of every path with an endmarker 0 each: offsets and bytes) of a golden GBZ.  Plain graphs: both from the
    S-lines of the oracle's GFA.  Translation graphs: the GFA has segments, so the NODE lengths come from the host image (GBZ.node_sequence)
    and the bases from the segment labels along the W-lines; the two are cross-checked path by path in the caller."""
    gfa = oracle.gfa()
    n = dev.paths()
    if not translated:
        table = E.LabelTable.from_gfa(gfa)
        rows = E.node_rows(oracle.gbwt().extract(2 * np.arange(n, dtype=np.uint64)), [2 * p for p in range(n)], 2 * n)
        return table.len, E.expected_rows(table, rows, 0)
    lengths = np.zeros(dev.alphabet_size() // 2 + 1, dtype=np.int64)
    for v in range(1, lengths.size):
        label = dev.node_sequence(v)
        lengths[v] = 0 if label is None else len(label)
    labels = E.s_lines(gfa)
    index = {name: j for j, name in enumerate(labels)}
    table = E.LabelTable({j: labels[name] for name, j in index.items()})
    rows = []
    for p in range(n):
        walk = oracle.path_lines([p], 1).rstrip(b"\n").split(b"\t")[6].replace(b">", b" >").replace(b"<", b" <").split()
        rows.append(([index[t[1:]] for t in walk], [t[:1] == b"<" for t in walk]))
    return lengths, E.expected_rows(table, rows, 0)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_true_suffix_array_and_permutations(name):
    path = os.path.join(O.GOLDEN, name)
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    translated = bool(G.parse_file(path).has_translation)
    n = dev.paths()
    lengths, (b_off, b_data) = fixture_text(dev, oracle, translated)
    ids = list(range(n))
    rng = np.random.default_rng(11)
    for order in (ids, ids[::-1], ids[::-1] + ids[:1]):
        text, offsets = T.oracle_text(oracle, order, lengths)
        # the bases of every row, derived from the oracle's GFA alone, have the lengths the tags were laid out with
        assert np.diff(offsets).tolist() == [int(b_off[p + 1] - b_off[p]) for p in order], order
        assert dev.text_length(order) == int(offsets[-1]) == text.size
        data = b"".join(b_data[int(b_off[p]):int(b_off[p + 1])] for p in order)
        for sa in (T.suffix_array(data), rng.permutation(text.size).astype(np.uint64), np.arange(text.size, dtype=np.uint64)):
            tags, runs = dev.tag_array(order, sa, return_runs=True)
            want = T.gather(text, sa)
            assert tags.dtype == np.uint64 and np.array_equal(tags, want), (order, sa[:8])
            assert np.array_equal(want, T.two_sorts(text, sa))
            assert runs == T.runs(want)
    if name == "example.gbz":                                                     # the known answer (tests/test_tags_cpu.py)
        text = dev.tag_array(ids, np.arange(34))
        assert text[0:6].tolist() == [22528, 24576, 28672, 30720, 34816, 0] and text[23:29].tolist() == [43008, 45056, 49152, 48128, 44032, 0]
        gfa = open(os.path.join(O.GOLDEN, "example.gfa"), "rb").read()
        assert np.array_equal(text, T.tag_text(E.LabelTable.from_gfa(gfa).len, T.gfa_rows(gfa))[0])


def write_sa(path, sa, lead=1):
    with open(path, "wb") as f:
        f.write(np.full(lead, SKIPPED, dtype="<u8").tobytes())
        f.write(np.asarray(sa, dtype="<u8").tobytes())


def test_synthetic_genome_host_device_and_file_forms(tmp_path, monkeypatch):
    gbz = str(tmp_path / "genome.gbz")
    S.Synth.genome(contigs=8, fragments=6, haplotypes=64, sites=40, labels=1).save(gbz, as_gbz=True)
    dev, oracle = G.GBZ.load(gbz), O.OracleGBZ(gbz)
    n = dev.paths()
    ids = np.arange(n, dtype=np.uint64)
    table = E.LabelTable.from_gfa(oracle.gfa())
    text, offsets = T.oracle_text(oracle, ids, table.len)
    assert n >= 2000 and table.len.max() == 1024 and text.size > 3000000
    # the two modes chained as a user chains them: `sequences` writes base and base.names, an external tool the suffix array
    base = str(tmp_path / "out")
    dev.write_sequences(base)
    assert os.path.getsize(base) == text.size == dev.text_length(ids)
    before = dev.memory_usage()["workspace_device_bytes"]
    sa = np.random.default_rng(2024).permutation(text.size).astype(np.uint64)
    want = T.gather(text, sa)
    want_runs = T.runs(want)
    # host pointers
    tags, runs = dev.tag_array(ids, sa, return_runs=True)
    assert np.array_equal(tags, want) and runs == want_runs
    positions = int(oracle.gbwt().extract(2 * ids)[0][-1]) + n
    assert dev.memory_usage()["workspace_device_bytes"] - before >= 12 * positions + text.size // 8
    # device pointers: slices that start and end inside rows, of the permutation and of the text order
    import torch
    device = torch.device("cuda", 0)
    a, b = int(offsets[3]) + 2, int(offsets[n - 5]) - 3
    assert offsets[3] < a < offsets[4] and offsets[n - 6] < b < offsets[n - 5]
    for values in (sa, np.arange(text.size, dtype=np.uint64)):
        d_sa = torch.from_numpy(values.view(np.int64)).to(device)
        d_tags = torch.full((b - a + 2,), -1, dtype=torch.int64, device=device)
        runs = dev.tags_device(ids, d_sa.data_ptr() + 8 * a, b - a, d_tags.data_ptr() + 8)
        got = d_tags.cpu().numpy().view(np.uint64)
        part = T.gather(text, values[a:b])
        assert got[0] == SKIPPED and got[-1] == SKIPPED                          # nothing outside the slice
        assert np.array_equal(got[1:-1], part) and runs == T.runs(part)
    # files: one batch (the default), many batches of 1 MiB, sa_skip 1 and 0
    write_sa(base + ".sa", sa)
    monkeypatch.delenv("GBWT_HIP_TAG_BATCH_MIB", raising=False)
    assert dev.write_tag_array(base) == want_runs
    assert open(base + ".tags", "rb").read() == want.astype("<u8").tobytes()
    os.remove(base + ".tags")
    monkeypatch.setenv("GBWT_HIP_TAG_BATCH_MIB", "1")
    assert 8 * text.size > 16 << 20                                              # (more than sixteen batches)
    assert dev.write_tag_array(base, sa_skip=1) == want_runs
    assert open(base + ".tags", "rb").read() == want.astype("<u8").tobytes()
    write_sa(base + ".sa", sa, lead=0)
    assert dev.write_tag_array(base, sa_skip=0) == want_runs
    assert open(base + ".tags", "rb").read() == want.astype("<u8").tobytes()
    walk_ms, plan_ms, gather_ms = dev.last_tags_ms()
    assert walk_ms > 0 and plan_ms > 0 and gather_ms > 0
    # the same plan scanned in pieces and with 64-bit hints (what plans of 2^30 and 2^32 positions get)
    monkeypatch.setenv("GBWT_HIP_SCAN_PIECE", "4096")
    monkeypatch.setenv("GBWT_HIP_TAG_WIDE", "1")
    other = dev.another_workspace()
    assert positions > 8 * 4096
    tags, runs = other.tag_array(ids, sa, return_runs=True)
    assert np.array_equal(tags, want) and runs == want_runs


def test_long_rows(tmp_path):
    """Rows of 12 000 positions with labels of 1 .. 1 024 bases: rows cross the tiles of the gather, the windows of the top level and the
    launches of the plan many times over."""
    gbz = str(tmp_path / "chain.gbz")
    S.Synth.chain(sites=2000, haplotypes=6, labels=1, chop=3, seed=3).save(gbz, as_gbz=True)
    dev, oracle = G.GBZ.load(gbz), O.OracleGBZ(gbz)
    n = dev.paths()
    order = list(range(n)) + [0]
    text, offsets = T.oracle_text(oracle, order)
    assert dev.text_length(order) == text.size
    for sa in (np.random.default_rng(8).permutation(text.size).astype(np.uint64), np.arange(text.size, dtype=np.uint64)):
        tags, runs = dev.tag_array(order, sa, return_runs=True)
        want = T.gather(text, sa)
        assert np.array_equal(tags, want) and runs == T.runs(want)
    # one path, and entries that repeat (not a permutation: the gather is still defined)
    one, _ = T.oracle_text(oracle, [n - 1])
    sa = np.random.default_rng(9).integers(0, one.size, size=5000).astype(np.uint64)
    sa[100:200] = sa[100]
    tags, runs = dev.tag_array([n - 1], sa, return_runs=True)
    assert np.array_equal(tags, T.gather(one, sa)) and runs == T.runs(T.gather(one, sa))


def test_plan_is_kept_while_the_paths_stay_the_same():
    path = os.path.join(O.GOLDEN, "example.gbz")
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    ids = list(range(dev.paths()))
    text, _ = T.oracle_text(oracle, ids)
    assert dev.text_length(ids) == 34
    first = dev.last_tags_ms()
    assert first[0] > 0 and first[1] > 0 and first[2] == 0
    held = dev.memory_usage()["workspace_device_bytes"]
    tags = dev.tag_array(ids, np.arange(34)[::-1].copy())
    assert np.array_equal(tags, text[::-1])
    second = dev.last_tags_ms()
    assert second[:2] == first[:2] and second[2] > 0                           # the same walk and plan: only the gather ran
    assert dev.text_length(ids) == 34 and dev.last_tags_ms()[:2] == first[:2]
    assert dev.memory_usage()["workspace_device_bytes"] >= held
    # another list is another plan; an extraction in between does not disturb a plan that is kept
    assert dev.text_length(ids[:2]) == 11
    dev.sequences_csr([0, 1, 2])
    assert np.array_equal(dev.tag_array(ids[:2], np.arange(11)), text[:11])
    assert dev.text_length(ids) == 34


def call_tags(h, ids, sa, tags):
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    expected, runs = C.c_uint64(0), C.c_uint64(0)
    st = h._L.gbwt_hip_tags(h._h, h._ws, ids.ctypes.data if ids.size else None, ids.size, None if sa is None else sa.ctypes.data, 0 if sa is None else sa.size,
                            None if tags is None else tags.ctypes.data, C.byref(expected), C.byref(runs))
    return st, expected.value, runs.value


def test_errors_and_edges(tmp_path):
    path = os.path.join(O.GOLDEN, "example.gbz")
    dev, oracle = G.GBZ.load(path), O.OracleGBZ(path)
    n = dev.paths()
    ids = list(range(n))
    text, offsets = T.oracle_text(oracle, ids)
    # a value equal to expected_len: INVALID_DATA, the output untouched
    sa = np.arange(34, dtype=np.uint64)
    sa[17] = 34
    out = np.full(34, 0xABABABABABABABAB, dtype=np.uint64)
    st, expected, runs = call_tags(dev, ids, sa, out)
    assert st == _lib.INVALID_DATA and expected == 34 and runs == 0 and (out == 0xABABABABABABABAB).all()
    with pytest.raises(G.GbwtHipError) as e:
        dev.tag_array(ids, [1 << 63])
    assert e.value.status == _lib.INVALID_DATA and "out of range" in str(e.value)
    import torch
    d_sa = torch.from_numpy(sa.view(np.int64)).to("cuda:0")
    d_tags = torch.zeros(34, dtype=torch.int64, device="cuda:0")
    with pytest.raises(G.GbwtHipError) as e:
        dev.tags_device(ids, d_sa.data_ptr(), 34, d_tags.data_ptr())
    assert e.value.status == _lib.INVALID_DATA
    assert dev.tags_device(ids, d_sa.data_ptr(), 17, d_tags.data_ptr()) == T.runs(text[:17]) == 17      # (the entries in front of it)
    assert np.array_equal(d_tags.cpu().numpy().view(np.uint64)[:17], text[:17])
    # a path id that is no path; null pointers with a count
    for bad in ([n], [0, 1 << 62], [1 << 63]):
        with pytest.raises(G.GbwtHipError) as e:
            dev.text_length(bad)
        assert e.value.status == _lib.BAD_ARGUMENT
    assert call_tags(dev, ids, sa, None)[0] == _lib.BAD_ARGUMENT
    # n = 0: an empty text; count = 0: nothing to do
    assert dev.text_length([]) == 0 and dev.tag_array([], []).size == 0
    with pytest.raises(G.GbwtHipError) as e:
        dev.tag_array([], [0])
    assert e.value.status == _lib.INVALID_DATA
    tags, runs = dev.tag_array(ids, [], return_runs=True)
    assert tags.size == 0 and runs == 0
    assert dev.tags_device(ids, 0, 0, 0) == 0
    # a bare GBWT, a GBZ handle without EXTRACT
    gbwt = G.GBWT.load(os.path.join(O.GOLDEN, "example.gbwt"))
    assert call_tags(gbwt, [0], None, None)[0] == _lib.BAD_ARGUMENT
    runs = C.c_uint64(0)
    assert gbwt._L.gbwt_hip_write_tag_array(gbwt._h, gbwt._ws, os.fsencode(str(tmp_path / "bare")), 1, C.byref(runs)) == _lib.BAD_ARGUMENT
    search_only = G.GBZ.load(path, flags=_lib.OPEN_SEARCH)
    with pytest.raises(G.GbwtHipError) as e:
        search_only.text_length([0])
    assert e.value.status == _lib.BAD_ARGUMENT
    with pytest.raises(G.GbwtHipError) as e:
        search_only.last_tags_ms()
    assert e.value.status == _lib.BAD_ARGUMENT
    # files
    base = str(tmp_path / "example")
    dev.write_sequences(base)
    names = open(base + ".names").read()
    sa = np.random.default_rng(1).permutation(34).astype(np.uint64)

    def failing(status, message=None):
        with pytest.raises(G.GbwtHipError) as e:
            dev.write_tag_array(base)
        assert e.value.status == status, str(e.value)
        assert message is None or message in str(e.value), str(e.value)
        assert not os.path.exists(base + ".tags")

    failing(_lib.IO_ERROR)                                                         # no .sa at all
    write_sa(base + ".sa", sa[:33])                                                # one value short
    failing(_lib.IO_ERROR, "too short")
    write_sa(base + ".sa", sa)
    assert dev.write_tag_array(base) == T.runs(T.gather(text, sa))
    assert open(base + ".tags", "rb").read() == T.gather(text, sa).astype("<u8").tobytes()
    os.remove(base + ".tags")
    bad = sa.copy()
    bad[33] = 34
    write_sa(base + ".sa", bad)
    failing(_lib.INVALID_DATA, "out of range")
    write_sa(base + ".sa", np.concatenate([sa, sa]))                               # (long enough for the wrong lengths below)
    lines = names.splitlines()
    f = lines[2].split("\t")
    for delta in (1, -1):
        wrong = lines[:2] + ["\t".join(f[:5] + [str(int(f[5]) + delta)])] + lines[3:]
        open(base + ".names", "w").write("\n".join(wrong) + "\n")
        failing(_lib.INVALID_DATA, f"Invalid length for path 2: expected {int(f[5]) + delta}, got {int(f[5])}")
    open(base + ".names", "w").write("")
    failing(_lib.INVALID_DATA, "No path names found")
    open(base + ".names", "w").write(names.replace("\t", " "))
    failing(_lib.INVALID_DATA)
    open(base + ".names", "w").write(f"{n}\tx\ty\t0\t0\t5\n")                       # a path the graph does not have
    failing(_lib.INVALID_DATA, f"Invalid length for path {n}: expected 5, got 0")
    os.remove(base + ".names")
    failing(_lib.IO_ERROR)
    # the names alone decide: ids in another order, fields in between ignored
    open(base + ".names", "w").write("5\t4\n0\tanything\t5\n")
    part, _ = T.oracle_text(oracle, [5, 0])
    write_sa(base + ".sa", np.arange(part.size)[::-1], lead=3)
    assert dev.write_tag_array(base, sa_skip=3) == T.runs(part[::-1])
    assert open(base + ".tags", "rb").read() == part[::-1].astype("<u8").tobytes()
