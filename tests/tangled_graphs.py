"""Seeded path sets on which components, bases and tags can go wrong -- node ids that run against the edges, thousands of components with
slots without nodes among them, edge lists thousands of entries long, long labels visited in both orientations -- and their own yardstick
for the components: a union-find over the consecutive node ids of the paths, which uses neither the library nor the oracle's records
(tests/test_tangled_cpu.py pins it against components_expect on the CPU).  Plain Python and numpy: shared by the CPU and the GPU tests.

Every builder returns (paths, bidirectional): paths = a list of numpy uint64 arrays of GBWT-encoded nodes (2 * id + orientation), made for
gbwt_rs_amd.synth.Synth.from_paths.  Node id 1 is on a path of every bidirectional set (attach_gbz needs that)."""
import numpy as np

NONE = 0xFFFFFFFF
REVERSE_SHARE = 0.3


def fwd(n):
    return 2 * int(n)


def rev(n):
    return 2 * int(n) + 1


def _oriented(ids, rng, share=REVERSE_SHARE):
    """ids as GBWT-encoded nodes, about `share` of the visits reverse."""
    ids = np.asarray(ids, dtype=np.uint64)
    return 2 * ids + (rng.random(ids.size) < share).astype(np.uint64)


def _pairs(a, b):
    """Two-node forward paths a[k] -> b[k]."""
    both = np.stack([2 * np.asarray(a, dtype=np.uint64), 2 * np.asarray(b, dtype=np.uint64)], axis=1)
    return list(both)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------

class Expected:
    """Components of a path set: geometry (min_node, slots), the CSR (offsets uint64[components + 1], ids uint64[nodes]; sets in order of their
    smallest id, ids ascending inside: the order of components_expect.components), and the component of the first node of every path
    (uint32, NONE for an empty path)."""

    def __init__(self, paths):
        used = np.unique(np.concatenate([np.asarray(p, dtype=np.uint64) >> np.uint64(1) for p in paths] + [np.zeros(0, np.uint64)])).astype(np.int64)
        self.paths = len(paths)
        if used.size == 0:
            self.min_node, self.slots = 0, 0
            self.offsets, self.ids = np.zeros(1, np.uint64), np.zeros(0, np.uint64)
            self.path_component = np.full(self.paths, NONE, dtype=np.uint32)
            return
        self.min_node, self.slots = int(used[0]), int(used[-1] - used[0] + 1)
        parent = list(range(int(used[-1]) + 1))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for p in paths:
            ids = (np.asarray(p, dtype=np.uint64) >> np.uint64(1)).tolist()
            for a, b in zip(ids, ids[1:]):
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)          # the root of a set is its smallest id
        root = np.array([find(int(x)) for x in used], dtype=np.int64)
        order = np.lexsort((used, root))                       # by smallest id of the set, then by id
        self.ids = used[order].astype(np.uint64)
        starts = np.flatnonzero(np.r_[True, root[order][1:] != root[order][:-1]])
        self.offsets = np.r_[starts, used.size].astype(np.uint64)
        number = np.full(int(used[-1]) + 1, NONE, dtype=np.uint32)
        number[used[order]] = np.repeat(np.arange(starts.size, dtype=np.uint32), np.diff(np.r_[starts, used.size]))
        self.path_component = np.array([NONE if len(p) == 0 else number[int(p[0]) >> 1] for p in paths], dtype=np.uint32)

    @property
    def components(self):
        return self.offsets.size - 1

    @property
    def nodes(self):
        return self.ids.size

    def lists(self):
        return [self.ids[int(a):int(b)].tolist() for a, b in zip(self.offsets[:-1], self.offsets[1:])]


# ---- topologies for the components ------------------------------------------------------------------------------------------------------------

def permuted_path(n=100000, seed=1, share=REVERSE_SHARE, bidirectional=True):
    """One path over ids 1 .. n in a random permutation."""
    rng = np.random.default_rng(seed)
    return [_oriented(rng.permutation(n) + 1, rng, share)], bidirectional


def descending_path(n=100000):
    """n, n - 1, ..., 1: the ids run against every edge."""
    return [2 * np.arange(n, 0, -1, dtype=np.uint64)], True


def zigzag(n=100000):
    """1, n, 2, n - 1, 3, ...: every edge joins a small id and a large one."""
    ids = np.empty(n, dtype=np.uint64)
    ids[0::2] = np.arange(1, (n + 1) // 2 + 1)
    ids[1::2] = np.arange(n, (n + 1) // 2, -1)
    return [2 * ids], True


def interleaved(n=100000, seed=2, classes=997, hole=13, single_every=20, empty=5):
    """`classes` components: component c holds the ids = c (mod classes), each a permuted path with reverse visits.  Every `hole`-th id is on
    none of them: slots without nodes inside and between the components -- but for every `single_every`-th of those, which is a path of one
    node (a component of its own).  `empty` empty paths in between."""
    rng = np.random.default_rng(seed)
    ids = np.arange(1, n + 1)
    paths = []
    for c in range(classes):
        member = ids[(ids % classes == c) & (ids % hole != 0)]
        paths.append(_oriented(rng.permutation(member), rng))
    holes = ids[ids % hole == 0]
    paths += [_oriented([x], rng) for x in holes[::single_every]]
    order = rng.permutation(len(paths))
    paths = [paths[k] for k in order]
    for k in range(empty):
        paths.insert((k * len(paths)) // empty, np.zeros(0, dtype=np.uint64))
    return paths, True


def tree_with_hub(n=100000, seed=3, hub_edges=5000, leaves=3000):
    """Two-node paths along the edges of a random recursive tree over permuted ids 1 .. n - 1 - leaves, and the hub -- id n, the largest --
    joined to `hub_edges` nodes: one record with that many edges.  `leaves` of them hang on the hub alone."""
    rng = np.random.default_rng(seed)
    m = n - 1 - leaves
    ids = rng.permutation(m) + 1
    child = np.arange(1, m)
    parent = (rng.random(m - 1) * child).astype(np.int64)            # node k hangs under one of the k nodes before it
    paths = _pairs(ids[child], ids[parent])
    flip = rng.random(len(paths)) < 0.5                               # (the edge in either direction)
    paths = [p[::-1].copy() if f else p for p, f in zip(paths, flip)]
    joined = np.r_[rng.choice(ids, hub_edges - leaves, replace=False), np.arange(m + 1, n)]
    paths += _pairs(np.full(joined.size, n), joined)
    return [paths[k] for k in rng.permutation(len(paths))], True


def grid(rows=300, cols=300, seed=4):
    """rows x cols nodes with permuted ids, a path along every row and one along every column (the columns with reverse visits)."""
    rng = np.random.default_rng(seed)
    ids = (rng.permutation(rows * cols) + 1).reshape(rows, cols)
    paths = [2 * ids[r].astype(np.uint64) for r in range(rows)] + [_oriented(ids[:, c], rng) for c in range(cols)]
    return paths, True


def reverse_joins(n=100000, seed=5):
    """Two long forward paths (ids descending / permuted) that meet only in one edge fwd(a) -> rev(b); a third long path on its own; hairpins
    fwd(x) rev(x) and self-loops in both orientations, on nodes of the long paths and on nodes of their own."""
    rng = np.random.default_rng(seed)
    third = n // 3
    a = np.arange(third, 0, -1)                                       # 1 .. third, descending
    b = rng.permutation(third) + third + 1
    c = rng.permutation(third - 300) + 2 * third + 1
    paths = [2 * a.astype(np.uint64), 2 * b.astype(np.uint64), 2 * c.astype(np.uint64)]
    paths.append(np.array([fwd(a[third // 2]), rev(b[third // 2])], dtype=np.uint64))
    own = np.arange(3 * third - 299, 3 * third + 1)                   # 300 ids on no long path
    for k, x in enumerate(np.r_[own, a[::5000], c[::5000]]):
        form = ([fwd(x), rev(x)], [fwd(x), fwd(x)], [rev(x), rev(x)], [rev(x), fwd(x), fwd(x)])[k % 4]
        paths.append(np.array(form, dtype=np.uint64))
    return paths, True


def sparse_random(n=580000, seed=6, share=0.55):
    """About share * n random two-node paths over ids 1 .. n: tens of thousands of components of every size, many ids on no path."""
    rng = np.random.default_rng(seed)
    m = int(share * n)
    a, b = rng.integers(1, n + 1, size=m), rng.integers(1, n + 1, size=m)
    a[0] = 1
    paths = list(np.stack([_oriented(a, rng), _oriented(b, rng)], axis=1))
    return paths, True


def permuted_path_unidirectional(n=100000, seed=7):
    """permuted_path, forward visits only, as a unidirectional index: half of the records are empty."""
    return permuted_path(n, seed, share=0.0, bidirectional=False)


COMPONENT_BUILDERS = {
    "permuted-path": permuted_path,
    "descending-path": descending_path,
    "zigzag": zigzag,
    "interleaved": interleaved,
    "tree-with-hub": tree_with_hub,
    "grid": grid,
    "reverse-joins": reverse_joins,
    "sparse-random": sparse_random,
    "permuted-path-unidirectional": permuted_path_unidirectional,
}


# ---- long labels --------------------------------------------------------------------------------------------------------------------------

TANGLE_NODES = 3000
TANGLE_PATH_LENGTHS = [0, 1, 2, 1023, 1024, 1025, 4095, 4096, 4097, 9000, 20000]
TANGLE_GIANT = 70000


def tangle_label_lengths(seed=8, nodes=TANGLE_NODES):
    """lengths[q] for node id q + 1: most nodes one base, the rest around the unit (16), batch-offset (1 024) and much longer sizes, one node
    of TANGLE_GIANT bases."""
    rng = np.random.default_rng(seed)
    lengths = np.ones(nodes, dtype=np.uint64)
    special = rng.permutation(nodes)
    at = 0
    for values, count in (((2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15), 420), ((16, 17), 120), ((31, 32, 33), 120), ((63, 64, 65), 120),
                          ((1023, 1024, 1025), 150), ((2048,), 60), ((5000,), 30), ((TANGLE_GIANT,), 1)):
        lengths[special[at:at + count]] = rng.choice(np.array(values, dtype=np.uint64), size=count)
        at += count
    return lengths


def tangle(seed=9, nodes=TANGLE_NODES, lengths=None):
    """Random walks over ids 1 .. nodes with mixed orientation, immediate repeats (x x, x rev(x)) and revisits (the next node is mostly a
    near neighbour by id), of TANGLE_PATH_LENGTHS nodes; the longest path also visits the giant node and the longest other labels in both
    orientations next to each other."""
    rng = np.random.default_rng(seed)
    lengths = tangle_label_lengths() if lengths is None else lengths
    longest = np.argsort(lengths, kind="stable")[::-1][:6] + 1        # ids of the six longest labels, the giant first
    paths = []
    for n in TANGLE_PATH_LENGTHS:
        walk = np.zeros(n, dtype=np.uint64)
        x = int(rng.integers(1, nodes + 1))
        o = 0
        for k in range(n):
            u = rng.random()
            if k == 0 or u >= 0.15:                                   # somewhere else: mostly nearby, sometimes anywhere
                x = int(rng.integers(1, nodes + 1)) if rng.random() < 0.2 else min(nodes, max(1, x + int(rng.integers(-40, 41))))
                o = int(rng.random() < REVERSE_SHARE)
            elif u >= 0.08:                                           # x rev(x)
                o ^= 1
            walk[k] = 2 * x + o                                        # (u < 0.08: x x)
        paths.append(walk)
    g, others = int(longest[0]), [int(v) for v in longest[1:]]
    forced = [fwd(g), rev(g), rev(others[0]), fwd(others[1]), fwd(g), fwd(others[2]), rev(others[2]), rev(g), fwd(others[3]), rev(others[4]), rev(g), fwd(1)]
    paths[-1][5000:5000 + len(forced)] = forced
    paths[1][0] = fwd(1)                                              # node id 1 is on a path
    return paths, True


def long_label(length):
    """Three nodes, the middle one with `length` bases: (label lengths, paths).  Text = 1 + 3 * length + 1 bases."""
    return np.array([1, length, 1], dtype=np.uint64), [np.array([fwd(1), fwd(2), fwd(2), rev(2), fwd(3)], dtype=np.uint64)]


def self_loop(length=1 << 20, visits=64):
    """One node of `length` bases visited `visits` times in a row in alternating orientation, between two one-base nodes."""
    middle = [fwd(2) if k % 2 == 0 else rev(2) for k in range(visits)]
    return np.array([1, length, 1], dtype=np.uint64), [np.array([fwd(1)] + middle + [fwd(3)], dtype=np.uint64)]
