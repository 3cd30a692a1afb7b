"""What one workspace keeps apart, through the C ABI (include/gbwt_hip.h): every request family with the idiom "size query, then the same call
with a buffer" -- extract, follow, path lines, path sequences, path positions, edges, links, locate -- is interrupted between its two calls by
a complete, different request of every other family on the same workspace, and is asked to fill with one parameter changed; the answer is
always that of the request run alone on a fresh workspace.  And what gbwt_hip_memory_usage counts of a workspace after the smallest request
of a family.  (The parts of a handle that a first request makes -- labels, components, the locate index -- have their accounting checked in
test_gpu_sequences.py, test_gpu_components.py and test_gpu_locate.py, the scratch of positions and tags in test_gpu_refpos.py and
test_gpu_tags.py.)  The calls go through _lib.lib(): the Python mirror never leaves a size query and its fill call apart."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
from gbwt_rs_amd import _lib
from gbwt_rs_amd.api import BD_DTYPE, REFPATH_DTYPE, REFPOS_DTYPE, STATE_DTYPE

pytestmark = pytest.mark.gpu


def ptr(a):
    return a.ctypes.data if a is not None and a.size else None


class Graph:
    """A golden GBZ on the device and the two lists (x: the request under test, y: the one that interrupts it) every family asks about."""

    def __init__(self, name):
        self.L = _lib.lib()
        self.h = C.c_void_p()
        _lib.check(self.L.gbwt_hip_open_file_flags(os.fsencode(os.path.join(O.GOLDEN, name)), 0, _lib.OPEN_ALL, C.byref(self.h)))
        stats = _lib.Stats()
        _lib.check(self.L.gbwt_hip_get_stats(self.h, C.byref(stats)))
        paths = stats.paths
        assert paths >= 3
        total = C.c_uint64(0)
        _lib.check(self.L.gbwt_hip_node_ids(self.h, None, 0, C.byref(total)))
        nodes = np.zeros(total.value, dtype=np.uint64)
        _lib.check(self.L.gbwt_hip_node_ids(self.h, ptr(nodes), nodes.size, C.byref(total)))
        assert nodes.size >= 8
        self.paths = {"x": np.array([0, 2 % paths, paths - 1], dtype=np.uint64), "y": np.array([1, 1, paths - 2, 0], dtype=np.uint64), "one": np.array([0], dtype=np.uint64)}
        self.nodes = {"x": nodes[0::3][:5].copy(), "y": nodes[1::3][:4].copy(), "one": nodes[:1].copy()}
        # segment ids are 0, 1, ... where the graph has a translation; without one every row of a links request is empty and not valid
        self.segments = {"x": np.array([0, 1, 2, 1], dtype=np.uint64), "y": np.array([3, 0], dtype=np.uint64), "one": np.array([0], dtype=np.uint64)}
        self.orient = {k: (np.arange(v.size) % 2).astype(np.uint8) for k, v in self.nodes.items()}
        self.seg_orient = {k: (np.arange(v.size) % 2).astype(np.uint8) for k, v in self.segments.items()}
        ws = self.workspace()
        self.states, self.bd_states = {}, {}
        for which, ids in self.nodes.items():
            gbwt_nodes = 2 * ids + self.orient[which]
            for fn, dtype, keep in ((self.L.gbwt_hip_find, STATE_DTYPE, self.states), (self.L.gbwt_hip_bd_find, BD_DTYPE, self.bd_states)):
                out, valid = np.zeros(ids.size, dtype=dtype), np.zeros(ids.size, dtype=np.uint8)
                _lib.check(fn(self.h, ws, ptr(gbwt_nodes), ids.size, ptr(out), ptr(valid)))
                assert valid.all()
                keep[which] = out
        self.L.gbwt_hip_workspace_destroy(ws)
        self.alone = {}

    def workspace(self):
        ws = C.c_void_p()
        _lib.check(self.L.gbwt_hip_workspace_create(self.h, C.byref(ws)))
        return ws

    def memory(self, ws):
        m = _lib.Memory()
        _lib.check(self.L.gbwt_hip_memory_usage(self.h, ws, C.byref(m)))
        return m

    def close(self):
        self.L.gbwt_hip_close(self.h)


# One call of a family with the size-query / fill idiom: call(g, ws, which, param, capacity) -> (total, arrays).  capacity None: the size query
# (no buffer for the sized output); else the fill call, with every output the call can write.

def _rows(total, *arrays):
    return total.value, tuple(a[: total.value] if k == len(arrays) - 1 else a for k, a in enumerate(arrays))


def call_extract(g, ws, which, reverse, capacity):
    ids, total = g.paths[which], C.c_uint64(0)
    offsets, nodes = np.zeros(ids.size + 1, dtype=np.uint64), np.zeros(max(1, capacity or 0), dtype=np.uint32)
    _lib.check(g.L.gbwt_hip_extract_paths(g.h, ws, ptr(ids), ids.size, reverse, ptr(offsets), None if capacity is None else ptr(nodes), capacity or 0, C.byref(total)))
    return _rows(total, offsets, nodes)


def call_follow(g, ws, which, backward, capacity):
    st, total = g.bd_states[which], C.c_uint64(0)
    offsets, valid, out = np.zeros(st.size + 1, dtype=np.uint64), np.zeros(st.size, dtype=np.uint8), np.zeros(max(1, capacity or 0), dtype=BD_DTYPE)
    _lib.check(g.L.gbwt_hip_follow(g.h, ws, ptr(st), st.size, backward, ptr(offsets), None if capacity is None else ptr(out), capacity or 0, C.byref(total), ptr(valid)))
    return _rows(total, offsets, valid, out)


def call_lines(g, ws, which, mode, capacity):
    ids, total = g.paths[which], C.c_uint64(0)
    out = np.zeros(max(1, capacity or 0), dtype=np.uint8)
    _lib.check(g.L.gbwt_hip_path_lines(g.h, ws, ptr(ids), ids.size, mode, None if capacity is None else ptr(out), capacity or 0, C.byref(total)))
    return _rows(total, out)


def call_bases(g, ws, which, reverse, capacity):
    ids, total = g.paths[which], C.c_uint64(0)
    offsets, out = np.zeros(ids.size + 1, dtype=np.uint64), np.zeros(max(1, capacity or 0), dtype=np.uint8)
    _lib.check(g.L.gbwt_hip_path_sequences(g.h, ws, ptr(ids), ids.size, reverse, ord("$"), None if capacity is None else ptr(out), ptr(offsets), capacity or 0, C.byref(total)))
    return _rows(total, offsets, out)


def call_positions(g, ws, which, interval, capacity):
    ids, total = g.paths[which], C.c_uint64(0)
    paths, out = np.zeros(ids.size, dtype=REFPATH_DTYPE), np.zeros(max(1, capacity or 0), dtype=REFPOS_DTYPE)
    _lib.check(g.L.gbwt_hip_path_positions(g.h, ws, ptr(ids), ids.size, interval, ptr(paths), None if capacity is None else ptr(out), capacity or 0, C.byref(total)))
    return _rows(total, paths, out)


def _call_rows(fn, g, ws, ids, orient, predecessors, capacity):
    total = C.c_uint64(0)
    offsets, valid, out = np.zeros(ids.size + 1, dtype=np.uint64), np.zeros(ids.size, dtype=np.uint8), np.zeros(max(1, capacity or 0), dtype=np.uint64)
    _lib.check(fn(g.h, ws, ptr(ids), ptr(orient), ids.size, predecessors, ptr(offsets), None if capacity is None else ptr(out), capacity or 0, C.byref(total), ptr(valid)))
    return _rows(total, offsets, valid, out)


def call_edges(g, ws, which, predecessors, capacity):
    return _call_rows(g.L.gbwt_hip_edges, g, ws, g.nodes[which], g.orient[which], predecessors, capacity)


def call_links(g, ws, which, predecessors, capacity):
    return _call_rows(g.L.gbwt_hip_links, g, ws, g.segments[which], g.seg_orient[which], predecessors, capacity)


def call_locate(g, ws, which, unique, capacity):
    st, total = g.states[which], C.c_uint64(0)
    offsets, valid, out = np.zeros(st.size + 1, dtype=np.uint64), np.zeros(st.size, dtype=np.uint8), np.zeros(max(1, capacity or 0), dtype=np.uint64)
    _lib.check(g.L.gbwt_hip_locate(g.h, ws, ptr(st), st.size, unique, ptr(offsets), None if capacity is None else ptr(out), capacity or 0, C.byref(total), ptr(valid)))
    return _rows(total, offsets, valid, out)


# family: (call, the parameter of the request, the parameter of the changed request)
SIZED = {"extract": (call_extract, 0, 1), "follow": (call_follow, 0, 1), "lines": (call_lines, 1, 0), "bases": (call_bases, 0, 1),
         "positions": (call_positions, 3, 1), "edges": (call_edges, 0, 1), "links": (call_links, 0, 1), "locate": (call_locate, 0, 1)}


def complete_sized(family):
    def run(g, ws, which):
        call, param, _ = SIZED[family]
        total, _ = call(g, ws, which, param, None)
        return call(g, ws, which, param, total)[1]
    return run


def complete_find(g, ws, which):
    nodes = 2 * g.nodes[which] + 1 - g.orient[which]
    out, valid = np.zeros(nodes.size, dtype=STATE_DTYPE), np.zeros(nodes.size, dtype=np.uint8)
    _lib.check(g.L.gbwt_hip_find(g.h, ws, ptr(nodes), nodes.size, ptr(out), ptr(valid)))
    return out, valid


def complete_tags(g, ws, which):
    ids, expected, runs = g.paths[which], C.c_uint64(0), C.c_uint64(0)
    _lib.check(g.L.gbwt_hip_tags(g.h, ws, ptr(ids), ids.size, None, 0, None, C.byref(expected), None))
    sa = np.arange(expected.value, dtype=np.uint64)[::-1].copy()
    tags = np.zeros(sa.size, dtype=np.uint64)
    _lib.check(g.L.gbwt_hip_tags(g.h, ws, ptr(ids), ids.size, ptr(sa), sa.size, ptr(tags), None, C.byref(runs)))
    return tags, runs.value


def complete_graph_text(g, ws, which):
    total = C.c_uint64(0)
    _lib.check(g.L.gbwt_hip_graph_lines(g.h, ws, None, 0, C.byref(total)))
    out = np.zeros(max(1, total.value), dtype=np.uint8)
    _lib.check(g.L.gbwt_hip_graph_lines(g.h, ws, ptr(out), out.size, C.byref(total)))
    return (out[: total.value],)


COMPLETE = {**{family: complete_sized(family) for family in SIZED}, "find": complete_find, "tags": complete_tags, "graph_text": complete_graph_text}
# (links has rows to mix up only where the graph has a translation: those pairs run on translation.gbz as well)
PAIRS = [("example.gbz", a, b) for a in SIZED for b in COMPLETE if a != b] + \
        [("translation.gbz", a, b) for a in SIZED for b in COMPLETE if a != b and "links" in (a, b)]


@pytest.fixture(scope="module")
def graphs():
    made = {}
    yield lambda name: made[name] if name in made else made.setdefault(name, Graph(name))
    for g in made.values():
        g.close()


def alone(g, family, param):
    """The request on a fresh workspace, size query and fill call back to back: (total, arrays).  Computed once."""
    if (family, param) not in g.alone:
        call, ws = SIZED[family][0], g.workspace()
        total, _ = call(g, ws, "x", param, None)
        g.alone[family, param] = call(g, ws, "x", param, total)
        g.L.gbwt_hip_workspace_destroy(ws)
    return g.alone[family, param]


def same(got, want):
    return got[0] == want[0] and len(got[1]) == len(want[1]) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got[1], want[1]))


@pytest.mark.parametrize("name,family,other", PAIRS, ids=["-".join(p) for p in PAIRS])
def test_another_family_between_size_query_and_fill_call(graphs, name, family, other):
    g = graphs(name)
    call, param, _ = SIZED[family]
    want = alone(g, family, param)
    ws = g.workspace()
    total, _ = call(g, ws, "x", param, None)
    assert total == want[0]
    COMPLETE[other](g, ws, "y")
    assert same(call(g, ws, "x", param, total), want)
    g.L.gbwt_hip_workspace_destroy(ws)


@pytest.mark.parametrize("name,family", [("example.gbz", f) for f in SIZED] + [("translation.gbz", "links")])
def test_fill_call_with_one_parameter_changed(graphs, name, family):
    """Same ids, another reverse / backward / mode / interval / predecessors / unique: the rows in the workspace do not answer it."""
    g = graphs(name)
    call, param, changed = SIZED[family]
    first, want = alone(g, family, param), alone(g, family, changed)
    # (the two answers differ, except: links of a graph without translation are empty rows either way, and the records of these graphs
    # hold their sequence ids ascending and once each, which is what unique = 1 makes of them)
    if family != "locate" and (name == "translation.gbz" or family != "links"):
        assert not same(first, want)
    ws = g.workspace()
    assert call(g, ws, "x", param, None)[0] == first[0]
    assert same(call(g, ws, "x", changed, want[0]), want)
    assert same(call(g, ws, "x", param, first[0]), first)             # ... and back
    g.L.gbwt_hip_workspace_destroy(ws)


@pytest.mark.parametrize("family", [f for f in COMPLETE if f not in ("positions", "tags")])
def test_smallest_request_is_counted(graphs, family):
    g = graphs("example.gbz")
    ws = g.workspace()
    before = g.memory(ws)
    COMPLETE[family](g, ws, "one")
    after = g.memory(ws)
    assert after.workspace_device_bytes > before.workspace_device_bytes
    if family in ("lines", "bases", "graph_text"):
        assert after.text_bytes > before.text_bytes
        assert after.workspace_device_bytes - before.workspace_device_bytes >= after.text_bytes - before.text_bytes
    else:
        assert after.text_bytes == before.text_bytes
    if family == "extract":
        assert after.rows_bytes > before.rows_bytes
    g.L.gbwt_hip_workspace_destroy(ws)
