"""The exhaustive position / search / follow checks of a device index against an OracleGBWT, shared by tests/test_gpu_parity.py (small
indexes: every node 0 .. alphabet_size + 1) and tests/test_gpu_shifted.py (indexes moved up the id range, where that range has 2^32 nodes:
`nodes` names the nodes to go through instead -- the index's own, and the bogus ones around and far below them).  The assertions are
the same for both."""
import random

import numpy as np

import gbwt_rs_amd as G


def states(rows):
    return np.array(rows, dtype=G.STATE_DTYPE)


def bd_states(rows):
    return np.array(rows, dtype=G.BD_DTYPE)


def bd_tuple(x):
    return (tuple(int(v) for v in x["forward"]), tuple(int(v) for v in x["reverse"]))


def _domain(oracle, nodes):
    """The nodes a check goes through: all of 0 .. alphabet_size + 1, or the caller's list."""
    return list(range(0, oracle.alphabet_size() + 2)) if nodes is None else [int(x) for x in nodes]


def check_all_positions(dev, oracle, nodes=None):
    """start + forward for every position of every record, find/extend/bd for every state the oracle can reach."""
    n_seq = oracle.sequences()
    pos, ok = dev.start(np.arange(n_seq + 2))
    for i in range(n_seq + 2):
        exp = oracle.start(i)
        assert bool(ok[i]) == (exp is not None)
        if exp is not None:
            assert tuple(int(v) for v in pos[i]) == exp
    # every (node, offset) incl. one past the end of each record and nodes outside the alphabet
    queries = []
    for node in _domain(oracle, nodes):
        st = oracle.find(node)
        ln = (st[2] - st[1]) if st else 0
        for off in range(ln + 2):
            queries.append((node, off))
    out, ok = dev.forward(np.array(queries, dtype=G.POS_DTYPE))
    for q, r, v in zip(queries, out, ok):
        exp = oracle.forward(q)
        assert bool(v) == (exp is not None), q
        if exp is not None:
            assert tuple(int(x) for x in r) == exp, q
    if oracle.is_bidirectional():
        # GBWT::backward for the same positions (src/gbwt/tests.rs:191-214 walks every sequence backward)
        out, ok = dev.backward(np.array(queries, dtype=G.POS_DTYPE))
        for q, r, v in zip(queries, out, ok):
            exp = oracle.backward(q)
            assert bool(v) == (exp is not None), q
            if exp is not None:
                assert tuple(int(x) for x in r) == exp, q


def check_search(dev, oracle, nodes_of_interest, nodes=None):
    domain = _domain(oracle, nodes)
    nodes = np.array(domain, dtype=np.uint64)
    st, ok = dev.find(nodes)
    for node, s, v in zip(nodes, st, ok):
        exp = oracle.find(int(node))
        assert bool(v) == (exp is not None)
        if exp:
            assert tuple(int(x) for x in s) == exp
    # extend: every sub-range of every record x every destination
    q_states, q_nodes = [], []
    for node in nodes_of_interest:
        f = oracle.find(node)
        if f is None:
            continue
        ln = f[2]
        ranges = [(a, b) for a in range(ln + 1) for b in range(a, ln + 2)] if ln <= 6 else \
                 [(0, ln), (0, 1), (ln - 1, ln), (1, ln - 1), (ln // 2, ln // 2), (ln, ln + 3)]
        for (a, b) in ranges:
            for dest in domain:
                q_states.append((node, a, b))
                q_nodes.append(dest)
    out, ok = dev.extend(states(q_states), q_nodes)
    for s, d, r, v in zip(q_states, q_nodes, out, ok):
        exp = oracle.extend(s, d)
        assert bool(v) == (exp is not None), (s, d)
        if exp:
            assert tuple(int(x) for x in r) == exp, (s, d)
    if not oracle.is_bidirectional():
        return
    bst, ok = dev.bd_find(nodes)
    for node, s, v in zip(nodes, bst, ok):
        exp = oracle.bd_find(int(node))
        assert bool(v) == (exp is not None)
        if exp:
            assert bd_tuple(s) == exp
    # bidirectional extension: forward range from the extend cases, arbitrary reverse range of the same length
    q_bd = []
    for (node, a, b) in q_states[::2]:
        for rev_start in (0, 2):
            q_bd.append(((node, a, b), (node ^ 1, rev_start, rev_start + max(0, b - a))))
    dests = domain
    rng = random.Random(7)
    q_nodes = [rng.choice(dests) for _ in q_bd]
    for fn, ofn in ((dev.extend_forward, oracle.extend_forward), (dev.extend_backward, oracle.extend_backward)):
        out, ok = fn(bd_states(q_bd), q_nodes)
        for s, d, r, v in zip(q_bd, q_nodes, out, ok):
            exp = ofn(s, d)
            assert bool(v) == (exp is not None), (s, d)
            if exp:
                assert bd_tuple(r) == exp, (s, d)


def check_follow(dev, oracle, limit=400, nodes=None, bogus_nodes=()):
    """GBZ::follow_forward / follow_backward the way src/gbz/tests.rs:100-168 exercises them: breadth-first over every
    state reachable from every node, device extensions against the oracle's, in edge order."""
    if not oracle.is_bidirectional():
        return
    nodes = _domain(oracle, nodes)
    frontier, seen = [], set()
    for node in nodes:
        st = oracle.bd_find(node)
        if st is not None and st not in seen:
            seen.add(st)
            frontier.append(st)
    # states for nodes that do not exist must give "no iterator"
    bogus = [((n, 0, 1), (n ^ 1, 0, 1)) for n in (0, 1, oracle.alphabet_size(), oracle.alphabet_size() + 1) + tuple(bogus_nodes)]
    checked = 0
    while frontier and checked < limit:
        batch, frontier = frontier[:128], frontier[128:]
        queries = batch + (bogus if checked == 0 else [])
        checked += len(batch)
        for backward in (False, True):
            offsets, ext, ok = dev.follow(bd_states(queries), backward)
            for k, st in enumerate(queries):
                exp = oracle.follow(st, backward)
                assert bool(ok[k]) == (exp is not None), (st, backward)
                got = [bd_tuple(e) for e in ext[int(offsets[k]):int(offsets[k + 1])]]
                assert got == (exp or []), (st, backward)
                for e in exp or []:
                    if e not in seen:
                        seen.add(e)
                        frontier.append(e)
