"""Expected bases of GBZ paths, built without the library: node labels from the S-lines of a GFA (the oracle's gbunzip restatement, or a
golden file), paths from the oracle, the bytes put together in numpy (gbz-extract's extract_sequence, src/bin/gbz-extract.rs:173-189;
support::reverse_complement, src/support.rs:87-110)."""
import numpy as np

COMPLEMENT = np.full(256, ord("N"), dtype=np.uint8)
for a, b in zip(b"ACGTacgt", b"TGCATGCA"):
    COMPLEMENT[a] = b


def s_lines(gfa):
    """{name (bytes): label (bytes)} of the S-lines of a GFA text, in file order."""
    out = {}
    for line in gfa.split(b"\n"):
        if line.startswith(b"S\t"):
            _, name, seq = line.split(b"\t")[:3]
            out[name] = seq
    return out


class LabelTable:
    """Labels indexed by integer id (node id, or segment index): a byte array and offsets; ids without a label have none."""

    def __init__(self, labels):
        ids = np.array(sorted(labels), dtype=np.int64)
        size = int(ids.max()) + 1 if ids.size else 1
        lens = np.zeros(size, dtype=np.int64)
        for k in ids:
            lens[k] = len(labels[int(k)])
        self.start = np.zeros(size + 1, dtype=np.int64)
        np.cumsum(lens, out=self.start[1:])
        self.bytes = np.frombuffer(b"".join(labels[int(k)] for k in ids), dtype=np.uint8) if ids.size else np.zeros(0, np.uint8)
        self.len = lens

    @classmethod
    def from_gfa(cls, gfa):
        """Node ids = the S-line names (a graph without a node-to-segment translation)."""
        return cls({int(k): v for k, v in s_lines(gfa).items()})

    def bases(self, ids, reverse):
        """Labels of ids[k] joined, those with reverse[k] reverse-complemented: one numpy uint8 array."""
        ids = np.asarray(ids, dtype=np.int64)
        reverse = np.asarray(reverse, dtype=bool)
        lens = self.len[ids]
        total = int(lens.sum())
        if total == 0:
            return np.zeros(0, dtype=np.uint8)
        at = np.zeros(ids.size, dtype=np.int64)
        np.cumsum(lens[:-1], out=at[1:])
        within = np.arange(total, dtype=np.int64) - np.repeat(at, lens)
        start, rev, length = np.repeat(self.start[ids], lens), np.repeat(reverse, lens), np.repeat(lens, lens)
        src = np.where(rev, start + length - 1 - within, start + within)
        out = self.bytes[src]
        return np.where(rev, COMPLEMENT[out], out).astype(np.uint8)


def expected_rows(table, rows, endmarker=None):
    """rows: one (ids, reverse flags) pair per path, or None for a path that does not exist (an empty row without endmarker).
    Returns (offsets[n + 1] uint64, bytes)."""
    parts, offsets = [], [0]
    for row in rows:
        if row is None:
            offsets.append(offsets[-1])
            continue
        b = table.bases(*row)
        if endmarker is not None:
            b = np.append(b, np.uint8(endmarker))
        parts.append(b)
        offsets.append(offsets[-1] + b.size)
    data = np.concatenate(parts).tobytes() if parts else b""
    return np.array(offsets, dtype=np.uint64), data


def node_rows(gbwt_nodes_csr, seq_ids, n_sequences):
    """(ids, reverse) rows from a CSR of GBWT-encoded nodes (2 id + o) of the oracle's extraction; None where seq_ids[k] >= n_sequences."""
    offsets, nodes = gbwt_nodes_csr
    nodes = np.asarray(nodes, dtype=np.int64)
    out = []
    for k, s in enumerate(seq_ids):
        if s >= n_sequences:
            out.append(None)
            continue
        v = nodes[int(offsets[k]):int(offsets[k + 1])]
        out.append((v >> 1, (v & 1).astype(bool)))
    return out
