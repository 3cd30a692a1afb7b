"""Expected tags of a suffix array (gbz-extract's `tag-array` mode, src/bin/gbz-extract.rs:296-482), built without the library: paths from the
oracle's walk (or a golden GFA), label lengths from S-lines (seq_expect.LabelTable), the tag formula in numpy, and the reference's
two-sort procedure written out with argsort.

The text of paths p_0 .. p_{n-1} is the bases of p_0, an endmarker, the bases of p_1, an endmarker, ...; the tag of a text position is 0 for an
endmarker and ((node id << 11) | (orientation << 10)) + offset inside the node otherwise (extract_path / encode_start, :346-371)."""
import numpy as np

import seq_expect as E


def tag_text(lengths, rows):
    """lengths[node id] = label length; rows = one array of GBWT-encoded nodes (2 id + orientation) per path, in text order.
    Returns (tags of every text position uint64, text offset of every row + the text length: uint64[n + 1])."""
    lengths = np.asarray(lengths, dtype=np.int64)
    parts, offsets = [], [0]
    for row in rows:
        v = np.asarray(row, dtype=np.uint64)
        ids, orientation = v >> np.uint64(1), v & np.uint64(1)
        lens = lengths[ids.astype(np.int64)]
        total = int(lens.sum())
        at = np.zeros(v.size, dtype=np.int64)
        if v.size:
            np.cumsum(lens[:-1], out=at[1:])
        within = (np.arange(total, dtype=np.int64) - np.repeat(at, lens)).astype(np.uint64)
        start = (ids << np.uint64(11)) | (orientation << np.uint64(10))          # encode_start
        parts.append(np.repeat(start, lens) + within)                            # pos += 1 for every base: a plain addition
        parts.append(np.zeros(1, dtype=np.uint64))                               # the endmarker
        offsets.append(offsets[-1] + total + 1)
    text = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)
    return text, np.array(offsets, dtype=np.uint64)


def gather(text, sa):
    """TAG[i] = tag(SA[i])."""
    return text[np.asarray(sa, dtype=np.int64)]


def two_sorts(text, sa):
    """extract_tag_array (:408-444) literally: (i, SA[i]) sorted by the second field, the second field of the pair at place offset + j replaced
    by the tag of position j of every path, sorted back by the first field.  Needs len(sa) == len(text), as the reference does."""
    sa = np.asarray(sa, dtype=np.uint64)
    assert sa.size == text.size
    first = np.arange(sa.size, dtype=np.int64)
    by_value = np.argsort(sa, kind="stable")
    first, second = first[by_value], sa[by_value]
    second = second.copy()
    second[:] = text                                                             # values[offset + i].1 = path[i] over all paths
    by_index = np.argsort(first, kind="stable")
    return second[by_index]


def runs(tags):
    """The reference's "Tag array runs" (:455-467): entries that differ from the one in front, the first counting as one."""
    tags = np.asarray(tags)
    return 0 if tags.size == 0 else 1 + int(np.count_nonzero(tags[1:] != tags[:-1]))


def rows_of(csr, n):
    """The rows of an oracle extraction (offsets, GBWT-encoded nodes)."""
    offsets, nodes = csr
    return [np.asarray(nodes[int(offsets[k]):int(offsets[k + 1])], dtype=np.uint64) for k in range(n)]


def oracle_text(oracle, path_ids, lengths=None):
    """Tags of the text of these paths of an OracleGBZ: rows from the oracle's walk of sequences 2 p, label lengths from the S-lines of its GFA
    (a graph without a node-to-segment translation) unless `lengths` (per node id) is given."""
    ids = np.asarray(path_ids, dtype=np.uint64)
    if lengths is None:
        lengths = E.LabelTable.from_gfa(oracle.gfa()).len
    return tag_text(lengths, rows_of(oracle.gbwt().extract(2 * ids), ids.size))


def gfa_rows(gfa):
    """GBWT-encoded rows of the P- and W-lines of a GFA text, in file order."""
    rows = []
    for line in gfa.split(b"\n"):
        f = line.split(b"\t")
        if line.startswith(b"P\t"):
            rows.append(np.array([2 * int(s[:-1]) + (1 if s.endswith(b"-") else 0) for s in f[2].split(b",")], dtype=np.uint64))
        elif line.startswith(b"W\t"):
            walk = f[6].replace(b">", b" >").replace(b"<", b" <").split()
            rows.append(np.array([2 * int(s[1:]) + (1 if s[:1] == b"<" else 0) for s in walk], dtype=np.uint64))
    return rows


def suffix_array(text_bytes):
    """The suffix array of a short text by sorting its suffixes as byte strings (the endmarker 0 sorts first; equal suffixes -- there are none
    when they are compared to the end of the text -- by position)."""
    return np.array(sorted(range(len(text_bytes)), key=lambda i: (text_bytes[i:], i)), dtype=np.uint64)
