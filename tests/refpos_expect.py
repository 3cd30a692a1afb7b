"""Expected results of GBZ::reference_positions (src/gbz.rs:600-657) and of its reference-sample rule (src/gbz.rs:146-196), built without the
library: the walk is OracleGBWT.start / forward, one call per step, as the reference's loop; label lengths are passed in by the caller (the
generator's label_lengths, or the S-lines of a GFA), and so is the metadata, as the caller built it.

For a forward path p (sequence 2 p) with nodes v_0 .. v_{m-1}: off_0 = 0, off_{k+1} = off_k + len(node id of v_k); a visit is kept when its
offset has reached `next`, which then becomes its offset + interval (saturating at 2^64 - 1): the reference's loop, literally."""
import os

import numpy as np

import seq_expect as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GENERIC_SAMPLE = "_gbwt_ref"
U64_MAX = 2 ** 64 - 1


def golden(name):
    """(node label lengths by node id, sample names, sample id of every path) of a golden GBZ, read off its GFA source (tests/golden/
    example.gfa, translation.gfa): the P-lines are paths of the generic sample, the W-lines of `sample`.  The translation graphs hold the
    segments of translation.gfa, in file order, chopped into nodes of at most two bases with consecutive ids from 1 (tests/golden/README.md)."""
    translated = name.startswith("translation")
    gfa = open(os.path.join(GOLDEN, "translation.gfa" if translated else "example.gfa"), "rb").read()
    if translated:
        lengths = [0]
        for label in E.s_lines(gfa).values():
            lengths += [min(2, len(label) - at) for at in range(0, len(label), 2)]
        lengths = np.array(lengths, dtype=np.int64)
    else:
        lengths = E.LabelTable.from_gfa(gfa).len
    kinds = [line[:1] for line in gfa.split(b"\n") if line[:2] in (b"P\t", b"W\t")]
    return lengths, [GENERIC_SAMPLE, "sample"], [0 if k == b"P" else 1 for k in kinds]


def reference_sample_names(sample_names, tag, also_generic):
    """sample_names: the metadata's sample dictionary (a list); tag: the value of the GBWT tag `reference_samples`, or None.  The names of the
    tag split at ' ', then the generic sample, those that the dictionary holds (reference_samples_impl + reference_sample_names)."""
    names = [] if tag is None else tag.split(" ")
    if also_generic:
        names.append(GENERIC_SAMPLE)
    return [name for name in names if name in sample_names]


def reference_paths(sample_names, path_samples, tag, also_generic=True):
    """path_samples[p] = the sample id of path p.  The ids of the paths whose sample is a reference sample, ascending."""
    ids = {sample_names.index(name) for name in reference_sample_names(sample_names, tag, also_generic)}
    return [p for p, sample in enumerate(path_samples) if int(sample) in ids]


def node_starts(gbwt, path_id, lengths):
    """Every visit of path `path_id`: (len, offsets uint64[m], positions uint64[m, 2]) with positions[k] = Pos of visit k; lengths[node id]."""
    offsets, positions = [], []
    at = 0
    pos = gbwt.start(2 * path_id)
    while pos is not None:
        offsets.append(at)
        positions.append(pos)
        at += int(lengths[pos[0] // 2])
        pos = gbwt.forward(pos)
    return at, np.array(offsets, dtype=np.uint64), np.array(positions, dtype=np.uint64).reshape(-1, 2)


def kept(offsets, interval):
    """Indices of the visits the reference's loop keeps: `if path_offset >= next { push; next = path_offset + interval }`."""
    out, nxt = [], 0
    for k, off in enumerate(offsets.tolist()):
        if off >= nxt:
            out.append(k)
            nxt = min(off + interval, U64_MAX)
    return np.array(out, dtype=np.int64)


def positions_of(starts, path_id, interval):
    """(id, len, offsets, positions) of one path from its node_starts."""
    length, offsets, positions = starts
    keep = kept(offsets, interval)
    return path_id, length, offsets[keep], positions[keep]


def same(got, want):
    """Exact equality of two lists of (id, len, offsets, positions)."""
    if len(got) != len(want):
        return False
    for a, b in zip(got, want):
        if a[0] != b[0] or a[1] != b[1] or a[2].dtype != np.uint64 or a[3].dtype != np.uint64:
            return False
        if a[3].shape != (a[2].size, 2) or not np.array_equal(a[2], b[2]) or not np.array_equal(a[3], b[3]):
            return False
    return True
