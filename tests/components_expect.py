"""Expected weakly connected components and contig path selections, built without the library: a plain union-find over the edges of the CPU
oracle's records with the reference's has_node rule and output order (GBZ::weakly_connected_components, src/gbz.rs:570-598;
DisjointSets::extract, src/support.rs:1551-1576), and select_paths of gbz-extract restated over a components list (src/bin/gbz-extract.rs:196-264)."""

NONE = 0xFFFFFFFF


def records_of(gbwt):
    """The oracle's records by record index (None for an empty one); record i belongs to GBWT node alphabet_offset + i."""
    bwt = gbwt.bwt()
    return [bwt.record(i) for i in range(len(bwt))]


def geometry(gbwt):
    """(min_node, slots): node ids min_node .. min_node + slots - 1 (GBZ::min_node / max_node, src/gbz.rs:274-282)."""
    if gbwt.alphabet_size() <= gbwt.first_node():
        return 0, 0
    min_node = gbwt.first_node() // 2
    return min_node, (gbwt.alphabet_size() - 1) // 2 - min_node + 1


def has_node(gbwt, records, node_id):
    """GBZ::has_node (src/gbz.rs:286-289): the forward record is non-empty and holds an edge."""
    rec = 2 * node_id - gbwt.alphabet_offset()
    return 1 <= rec < len(records) and records[rec] is not None and records[rec].outdegree > 0


def components(gbwt):
    """[[node ids ascending], ...] in order of the smallest node id."""
    records = records_of(gbwt)
    offset = gbwt.alphabet_offset()
    parent = {}

    def find(x):
        root = x
        while parent.setdefault(root, root) != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for i in range(1, len(records)):
        if records[i] is None:
            continue
        node_id = (offset + i) // 2
        for successor, _ in records[i].edges():
            if successor == 0:                                   # EdgeIter::new skips the ENDMARKER (src/gbz.rs:834-836)
                continue
            j = successor - offset
            if j < 1 or j >= len(records) or records[j] is None:  # outside the alphabet / without a record
                continue
            a, b = find(node_id), find(successor // 2)
            if a != b:
                parent[max(a, b)] = min(a, b)
    min_node, slots = geometry(gbwt)
    out, index = [], {}
    for node_id in range(min_node, min_node + slots):            # DisjointSets::extract: sets in order of first appearance
        if not has_node(gbwt, records, node_id):
            continue
        root = find(node_id)
        if root not in index:
            index[root] = len(out)
            out.append([])
        out[index[root]].append(node_id)
    return out


def first_nodes(gbwt, paths, stride=2):
    """Node id of the first node of every path (sequence stride * p), None for an empty path."""
    out = []
    for p in range(paths):
        start = gbwt.start(stride * p)
        out.append(None if start is None or start[0] == 0 else start[0] // 2)
    return out


def path_components(comps, firsts):
    where = {node: c for c, nodes in enumerate(comps) for node in nodes}
    return [NONE if f is None else where[f] for f in firsts]


def select_paths(comps, firsts, path_contigs, contig_names, contig):
    """select_paths: `path_contigs` = contig id of every path, `contig_names` = the metadata's contig names or None (no names).
    Raises ValueError with the reference's message."""
    if contig is None:
        return list(range(len(path_contigs)))
    if contig_names is None:
        raise ValueError("Cannot select a contig without contig names")
    if contig not in contig_names:
        raise ValueError(f"The graph does not contain contig {contig}")
    contig_id = contig_names.index(contig)
    initial = [p for p, c in enumerate(path_contigs) if c == contig_id]
    if not initial:
        raise ValueError(f"The graph does not contain any paths for contig {contig}")
    of = path_components(comps, firsts)
    wanted = {of[p] for p in initial if of[p] != NONE}
    return [p for p in range(len(firsts)) if of[p] != NONE and of[p] in wanted]
