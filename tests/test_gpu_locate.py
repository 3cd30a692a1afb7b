"""Locate queries on the device -- the sequences behind search states and positions -- against tests/locate_expect.py (the oracle's own walk of
every sequence; pinned on the CPU in tests/test_locate_cpu.py): the golden files with every kind of invalid state, sub-ranges from searches
(host and device forms), rows wider than a wave with revisits, the three ways a lane can end (a sampled record at once, after steps, at the end
of its sequence), every kind of handle, the index built once and shared, the device rows and the C ABI's protocol.  Every comparison is exact."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import gbwt_rs_amd as G
import locate_expect as LX
import oracle_lib as O
import tangled_graphs as TG
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S

pytestmark = pytest.mark.gpu

GOLDEN = ["example.gbwt", "example.gbz", "example-v1.gbz", "translation.gbz", "with-empty.gbwt"]


def golden(name):
    path = os.path.join(O.GOLDEN, name)
    return path, (O.OracleGBZ(path).gbwt() if name.endswith(".gbz") else O.OracleGBWT.load(path))


def load(path, flags=_lib.OPEN_ALL):
    return (G.GBZ if path.endswith(".gbz") else G.GBWT).load(path, flags=flags)


def synth_pair(paths, bidirectional=True, flags=_lib.OPEN_ALL):
    s = S.Synth.from_paths(paths, bidirectional=bidirectional)
    dev = G.GBWT.from_records(s.data(), s.starts(), s.alphabet_offset, s.alphabet_size, s.sequences, s.size, bidirectional, flags=flags)
    oracle = O.OracleGBWT.from_bwt(O.OracleBWT.from_parts(s.data(), s.starts()), s.sequences, s.size, s.alphabet_offset, s.alphabet_size, bidirectional)
    return dev, oracle


def as_states(tuples):
    out = np.zeros(len(tuples), dtype=G.STATE_DTYPE)
    for k, t in enumerate(tuples):
        out[k] = tuple(int(x) for x in t)
    return out


def assert_rows(got, rows):
    offsets, ids, valid = got
    e_off, e_ids, e_valid = LX.csr(rows)
    assert offsets.dtype == np.uint64 and ids.dtype == np.uint64 and valid.dtype == bool
    assert np.array_equal(valid, e_valid)
    assert np.array_equal(offsets, e_off)
    assert np.array_equal(ids, e_ids)


def check_states(dev, own, states):
    """Both modes of one batch against the truth; returns the expected plain and unique rows."""
    states = as_states(states) if not isinstance(states, np.ndarray) else states
    expected = []
    for unique in (False, True):
        rows = [LX.row(own, (s["node"], s["start"], s["end"]), unique) for s in states]
        assert_rows(dev.locate_csr(states, unique), rows)
        expected.append(rows)
    return expected


def check_positions(dev, own, positions):
    ids, valid = dev.locate_positions(np.array(positions, dtype=np.uint64).reshape(-1, 2))
    want = [LX.position(own, p) for p in positions]
    assert ids.dtype == np.uint64 and valid.tolist() == [w is not None for w in want]
    assert ids.tolist() == [0 if w is None else w for w in want]


def whole_records(oracle, own, hi=None):
    """find(node) of every node in 0 .. alphabet_size + 2 -- (node, 0, 1) where there is nothing to find -- and hand-made invalid states."""
    states = []
    for node in range(0, (oracle.alphabet_size() + 3) if hi is None else hi):
        st = oracle.find(node)
        states.append(st if st is not None else (node, 0, 1))
        n = own.lengths.of(node)
        if n is not None:
            states += [(node, 1, 1), (node, 2, 1), (node, 0, n + 1), (node, n, n + 1), (node, n - 1, n)]
    states += [(0, 0, 1), (1 << 40, 0, 1), ((1 << 64) - 1, 0, 1), (oracle.alphabet_offset(), 0, 1), (oracle.alphabet_size(), 0, 1)]
    return states


def all_positions(oracle, own):
    """Every visit, one offset past every record, and nodes without a record."""
    nodes = sorted({node for node, _ in own})
    return list(own) + [(node, own.lengths.of(node)) for node in nodes] + [(0, 0), (oracle.alphabet_offset(), 0), (oracle.alphabet_size(), 0), (1 << 50, 0), (nodes[0], (1 << 64) - 1)]


def windows(oracle, width):
    """Every window of `width` nodes of every sequence, and as many that are no stretch of any path (a window with its last node doubled)."""
    rows = []
    for seq in range(oracle.sequences()):
        nodes = oracle.sequence(seq)
        for a in range(0, len(nodes) - width + 1):
            rows.append(nodes[a:a + width])
            rows.append(nodes[a:a + width - 1] + [nodes[a]])
    return np.array(rows, dtype=np.uint64).reshape(-1, width)


# ---- the golden files ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GOLDEN)
def test_golden_states_positions_and_single_calls(name):
    path, oracle = golden(name)
    dev, own = load(path), LX.owners(oracle)
    states = whole_records(oracle, own)
    plain, unique = check_states(dev, own, states)
    assert any(r is None for r in plain) and any(r is not None and len(r) > 1 for r in plain)
    check_positions(dev, own, all_positions(oracle, own))
    for st, want in list(zip(states, unique))[:40]:
        got = dev.locate(st)
        assert (got is None) == (want is None) and (want is None or (got.dtype == np.uint64 and got.tolist() == want))
    real = next(st for st, r in zip(states, plain) if r is not None)
    assert dev.locate(real, unique=False).tolist() == LX.row(own, real, False)
    for empty in (np.zeros(0, dtype=G.STATE_DTYPE), []):
        for unique_mode in (False, True):
            offsets, ids, valid = dev.locate_csr(empty, unique_mode)
            assert offsets.tolist() == [0] and ids.size == 0 and valid.size == 0
    ids, valid = dev.locate_positions(np.zeros((0, 2), dtype=np.uint64))
    assert ids.size == 0 and valid.size == 0


def test_sub_ranges_from_searches_host_and_device_forms():
    import torch
    path, oracle = golden("example.gbz")
    dev, own = load(path), LX.owners(oracle)
    for width in (2, 3):
        q = windows(oracle, width)
        states, found = dev.search(q)
        assert found.any() and not found.all()
        assert any(int(s["end"]) - int(s["start"]) < own.lengths.of(int(s["node"])) for s, ok in zip(states, found) if ok)      # real sub-ranges
        check_states(dev, own, states)                # the host form: a failed search is whatever state it left, judged by its content
        d_q = torch.from_numpy(q.view(np.int64)).cuda()
        for unique in (False, True):
            result = dev.search_device(d_q.data_ptr(), q.shape[0], width)
            rows = [LX.row(own, (s["node"], s["start"], s["end"]), unique) if ok else None for s, ok in zip(states, found)]
            assert_rows(dev.located_to_host(dev.locate_states_device(result, unique)), rows)
        # without the validity bytes the states are judged by their content, as the host form does
        result = dev.search_device(d_q.data_ptr(), q.shape[0], width)
        bare = _lib.States(result.d_states, None, result.n)
        assert_rows(dev.located_to_host(dev.locate_states_device(bare, False)), [LX.row(own, (s["node"], s["start"], s["end"]), False) for s in states])
        del d_q


# ---- rows wider than a wave ---------------------------------------------------------------------------------------------------------------

def wide_paths():
    """Node 10 is visited by 260 paths that leave it to five nodes, and four times (once reversed) by one more."""
    fwd, rev = TG.fwd, TG.rev
    paths = [[fwd(1 + k % 3), fwd(10), fwd(20 + k % 5), fwd(30)] for k in range(260)]
    paths.append([fwd(2), fwd(10), fwd(21), fwd(10), fwd(22), fwd(10), rev(10), fwd(30), fwd(10)])
    return [np.array(p, dtype=np.uint64) for p in paths]


def test_wide_rows_revisits_and_sort_pieces(monkeypatch):
    dev, oracle = synth_pair(wide_paths())
    own = LX.owners(oracle)
    assert dev.stats.max_record_len > 130 and dev.stats.max_outdegree > 2 and len(own) < 100000
    hub = TG.fwd(10)
    n = own.lengths.of(hub)
    assert n > 130
    q = windows(oracle, 3)[::7]
    searched, _ = dev.search(q)
    states = whole_records(oracle, own) + [(hub, i, i + 1) for i in range(n)] + [(hub, 3, n - 2), (hub, 63, 65), (hub, 64, 129)]
    batch = np.concatenate([as_states(states), searched])
    plain, unique = check_states(dev, own, batch)
    whole = states.index(oracle.find(hub))
    assert len(plain[whole]) == n and len(unique[whole]) < n          # the path that comes back to the node is there once
    # a unique request sorted in pieces cut at row boundaries: the same rows; a row longer than a piece is refused, a plain one is not
    monkeypatch.setenv("GBWT_HIP_LOCATE_SORT_PIECE", "100")
    pieces = dev.another_workspace()
    small = np.array([s for s in batch if int(s["end"]) - int(s["start"]) <= 100 or int(s["start"]) >= int(s["end"])], dtype=G.STATE_DTYPE)
    assert small.size > 200 and sum(max(0, int(s["end"]) - int(s["start"])) for s in small) > 300
    check_states(pieces, own, small)
    with pytest.raises(G.GbwtHipError) as e:
        pieces.locate_csr(batch, unique=True)
    assert e.value.status == _lib.UNSUPPORTED and "row" in str(e.value)
    assert_rows(pieces.locate_csr(batch, unique=False), plain)


def test_rows_and_ids_scanned_in_pieces(monkeypatch):
    """The scans of a request -- the rows' offsets over the states, the ranks of a unique request over the ids -- in pieces of 4 096 items, on a
    workspace of its own (GBWT_HIP_SCAN_PIECE is read when a workspace is made): what only requests of more than 2^30 states or ids get otherwise."""
    dev, oracle = synth_pair(wide_paths())
    own = LX.owners(oracle)
    hub = TG.fwd(10)
    n = own.lengths.of(hub)
    states = [(hub, i % n, i % n + 1) for i in range(4200)] + [(hub, 7, 3), (hub, 0, n + 1)] + [oracle.find(hub)] * 130 + [(hub, 5, 60)]
    assert len(states) > 4096                             # more than one piece of rows; more than eight of ids (below)
    monkeypatch.setenv("GBWT_HIP_SCAN_PIECE", "4096")
    pieces = dev.another_workspace()
    plain, unique = check_states(pieces, own, states)
    assert sum(len(r) for r in plain if r is not None) > 8 * 4096 and any(r is None for r in plain)
    assert sum(len(r) for r in unique if r is not None) < sum(len(r) for r in plain if r is not None)


# ---- the three ways a lane can end --------------------------------------------------------------------------------------------------------

def test_interval_one_default_and_none_agree(monkeypatch):
    path, oracle = golden("example.gbz")
    own = LX.owners(oracle)
    states = as_states(whole_records(oracle, own))
    positions = all_positions(oracle, own)
    records = len({node for node, _ in own})
    sequences = sum(1 for k in range(oracle.sequences()) if oracle.start(k) is not None)
    results = []
    for interval in ("1", None, "0"):
        if interval is None:
            monkeypatch.delenv("GBWT_HIP_LOCATE_INTERVAL", raising=False)
        else:
            monkeypatch.setenv("GBWT_HIP_LOCATE_INTERVAL", interval)
        dev = load(path)
        results.append((dev.locate_csr(states, False), dev.locate_csr(states, True), dev.locate_positions(np.array(positions, dtype=np.uint64))))
        check_states(dev, own, states)
        check_positions(dev, own, positions)
        info = dev.locate_index_info()
        steps, located = dev.locate_count_steps(states)
        assert located == int(results[-1][0][0][-1]) and info["built"] == 1 and info["end_entries"] == sequences
        if interval == "1":
            assert (info["interval"], info["table_positions"], info["sampled_records"], steps) == (1, len(own), records, 0)
        elif interval == "0":
            assert (info["interval"], info["table_positions"], info["sampled_records"]) == (0, 0, 0) and steps >= located
        else:
            assert info["interval"] == 64 and info["table_positions"] <= len(own)
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_one_lane_walks_a_whole_path_to_its_end(monkeypatch):
    monkeypatch.setenv("GBWT_HIP_LOCATE_INTERVAL", "0")
    paths, bidirectional = TG.permuted_path(n=3000)
    dev, oracle = synth_pair(paths, bidirectional)
    own = LX.owners(oracle)
    assert len(own) == 6000
    first = oracle.start(0)
    steps, located = dev.locate_count_steps(as_states([(first[0], first[1], first[1] + 1)]))
    assert (steps, located) == (3000, 1)              # 2 999 steps to the last node and the one that leaves to the endmarker
    check_positions(dev, own, all_positions(oracle, own))
    check_states(dev, own, whole_records(oracle, own, hi=400))
    assert dev.locate_index_info()["end_entries"] == 2 and dev.locate_index_info()["table_positions"] == 0


# ---- every kind of handle -----------------------------------------------------------------------------------------------------------------

def test_every_kind_of_handle_gives_the_same_rows(monkeypatch, tmp_path):
    path, oracle = golden("example.gbz")
    own = LX.owners(oracle)
    states = as_states(whole_records(oracle, own))
    positions = all_positions(oracle, own)
    for flags in (_lib.OPEN_EXTRACT, _lib.OPEN_SEARCH, _lib.OPEN_GFA, _lib.OPEN_ALL):
        dev = load(path, flags)
        check_states(dev, own, states)
        check_positions(dev, own, positions)
    bare = load(os.path.join(O.GOLDEN, "example.gbwt"))
    check_states(bare, own, states)
    # a chain of biallelic sites: a handle opened for extraction alone gives its raw descriptors back and steps on the record bytes
    chain = str(tmp_path / "chain.gbz")
    S.Synth.chain(sites=150, haplotypes=24, alleles=2, founders=8, seed=5).save(chain, as_gbz=True)
    chain_oracle = O.OracleGBZ(chain).gbwt()
    chain_own = LX.owners(chain_oracle)
    chain_states = as_states(whole_records(chain_oracle, chain_own))
    for flags in (_lib.OPEN_EXTRACT, _lib.OPEN_ALL):
        dev = load(chain, flags)
        check_states(dev, chain_own, chain_states)
        check_positions(dev, chain_own, all_positions(chain_oracle, chain_own))
    monkeypatch.setenv("GBWT_HIP_SAMPLE_INTERVAL", "0")                     # no samples: one lane per sequence builds
    for p, o, st in ((path, own, states), (chain, chain_own, chain_states)):
        dev = load(p)
        check_states(dev, o, st)
    monkeypatch.delenv("GBWT_HIP_SAMPLE_INTERVAL")
    monkeypatch.setenv("GBWT_HIP_SAMPLE_INTERVAL", "16")                    # several segments per sequence
    dev = load(chain)
    check_states(dev, chain_own, chain_states)
    monkeypatch.delenv("GBWT_HIP_SAMPLE_INTERVAL")
    paths, bidirectional = TG.permuted_path_unidirectional(n=2000)
    dev, uni = synth_pair(paths, bidirectional)
    uni_own = LX.owners(uni)
    assert len(uni_own) == 2000
    check_states(dev, uni_own, whole_records(uni, uni_own, hi=300))
    check_positions(dev, uni_own, all_positions(uni, uni_own))


# ---- built once, shared -------------------------------------------------------------------------------------------------------------------

def test_index_is_built_once_and_shared_between_workspaces_and_threads():
    path, oracle = golden("translation.gbz")
    own = LX.owners(oracle)
    states = as_states(whole_records(oracle, own))
    dev = load(path)
    zeros = dev.locate_index_info()
    assert set(zeros) == {"built", "interval", "sampled_records", "table_positions", "end_entries", "device_bytes", "build_ms", "build_launches"}
    assert not any(zeros.values())
    before = dev.memory_usage()["index_device_bytes"]
    check_states(dev, own, states)
    info = dev.locate_index_info()
    assert info["built"] == 1 and info["device_bytes"] > 0 and info["build_launches"] > 0 and info["build_ms"] >= 0
    assert dev.memory_usage()["index_device_bytes"] == before + info["device_bytes"]
    check_states(dev, own, states)
    view = dev.another_workspace()
    check_states(view, own, states)
    assert dev.locate_index_info() == info and view.locate_index_info() == info
    assert dev.memory_usage()["index_device_bytes"] == before + info["device_bytes"]
    # two threads, a workspace each, first call together
    fresh = load(path)
    views = [fresh.another_workspace(), fresh.another_workspace()]
    gate, got, errors = threading.Barrier(2), [None, None], []

    def first_call(k):
        try:
            gate.wait()
            got[k] = (views[k].locate_csr(states, False), views[k].locate_csr(states, True))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=first_call, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for plain, unique in got:
        assert_rows(plain, [LX.row(own, (s["node"], s["start"], s["end"]), False) for s in states])
        assert_rows(unique, [LX.row(own, (s["node"], s["start"], s["end"]), True) for s in states])
    assert fresh.locate_index_info()["build_launches"] == info["build_launches"]


def test_located_rows_and_edge_rows_leave_each_other_alone():
    path, oracle = golden("example.gbz")
    own = LX.owners(oracle)
    states = as_states(whole_records(oracle, own))
    dev = load(path)
    ids = np.arange(0, oracle.alphabet_size() // 2 + 2, dtype=np.uint64)
    orient = np.zeros(ids.size, dtype=np.uint8)
    edges = dev.another_workspace().edges_csr(ids, orient)
    want = [LX.row(own, (s["node"], s["start"], s["end"]), False) for s in states]
    located = dev.locate_device(states, False)
    edge_rows = dev.edges_device(ids, orient)
    assert_rows(dev.located_to_host(located), want)
    located = dev.locate_device(states, True)
    assert all(np.array_equal(a, b) for a, b in zip(dev.rows_to_host(edge_rows), edges))
    assert_rows(dev.located_to_host(located), [LX.row(own, (s["node"], s["start"], s["end"]), True) for s in states])


# ---- device rows and times ----------------------------------------------------------------------------------------------------------------

def test_device_rows_equal_host_rows_and_times():
    path, oracle = golden("example.gbz")
    own = LX.owners(oracle)
    states = as_states(whole_records(oracle, own))
    dev = load(path)
    with pytest.raises(G.GbwtHipError) as e:
        dev.last_locate_ms()
    assert e.value.status == _lib.BAD_ARGUMENT
    for unique in (False, True):
        host = dev.locate_csr(states, unique)
        rows = dev.locate_device(states, unique)
        assert rows.n == states.size and rows.total == host[1].size
        assert all(np.array_equal(a, b) for a, b in zip(dev.located_to_host(rows), host))
        walk_ms, sort_ms = dev.last_locate_ms()
        assert walk_ms >= 0 and (sort_ms >= 0 if unique else sort_ms == 0)
    rows = dev.locate_device([], True)
    assert (rows.n, rows.total) == (0, 0) and dev.located_to_host(rows)[0].tolist() == [0]


# ---- the C ABI's protocol -----------------------------------------------------------------------------------------------------------------

def test_capacity_and_null_states():
    path, oracle = golden("example.gbz")
    own = LX.owners(oracle)
    states = as_states(whole_records(oracle, own))
    dev, L = load(path), _lib.lib()
    for unique in (0, 1):
        e_off, e_ids, e_valid = LX.csr([LX.row(own, (s["node"], s["start"], s["end"]), bool(unique)) for s in states])
        offsets, valid, total = np.zeros(states.size + 1, dtype=np.uint64), np.zeros(states.size, dtype=np.uint8), C.c_uint64(0)
        assert L.gbwt_hip_locate(dev._h, dev._ws, states.ctypes.data, states.size, unique, offsets.ctypes.data, None, 0, C.byref(total), valid.ctypes.data) == _lib.OK
        assert total.value == e_ids.size > 1 and np.array_equal(offsets, e_off) and np.array_equal(valid.astype(bool), e_valid)
        ids = np.zeros(total.value, dtype=np.uint64)
        total.value = 0
        assert L.gbwt_hip_locate(dev._h, dev._ws, states.ctypes.data, states.size, unique, offsets.ctypes.data, ids.ctypes.data, e_ids.size - 1, C.byref(total),
                                 valid.ctypes.data) == _lib.CAPACITY
        assert total.value == e_ids.size and not ids.any()
        assert L.gbwt_hip_locate(dev._h, dev._ws, states.ctypes.data, states.size, unique, offsets.ctypes.data, ids.ctypes.data, e_ids.size, C.byref(total),
                                 valid.ctypes.data) == _lib.OK
        assert np.array_equal(ids, e_ids)
        assert L.gbwt_hip_locate(dev._h, dev._ws, None, states.size, unique, offsets.ctypes.data, ids.ctypes.data, ids.size, C.byref(total), valid.ctypes.data) == _lib.BAD_ARGUMENT
    rows = _lib.Located()
    assert L.gbwt_hip_locate_device(dev._h, dev._ws, None, 3, 0, C.byref(rows)) == _lib.BAD_ARGUMENT
    assert L.gbwt_hip_locate_states_device(dev._h, dev._ws, None, None, 3, 0, C.byref(rows)) == _lib.BAD_ARGUMENT
    assert L.gbwt_hip_locate_positions(dev._h, dev._ws, None, 3, offsets.ctypes.data, valid.ctypes.data) == _lib.BAD_ARGUMENT
    assert L.gbwt_hip_locate(dev._h, dev._ws, states.ctypes.data, states.size, 2, offsets.ctypes.data, None, 0, C.byref(total), valid.ctypes.data) == _lib.BAD_ARGUMENT
    other = load(path)
    assert L.gbwt_hip_locate_device(dev._h, other._ws, states.ctypes.data, states.size, 0, C.byref(rows)) == _lib.BAD_ARGUMENT     # a workspace of another handle
