"""The host's side of the GFA text (csrc/gfa_host.cpp: the H-, S- and L-lines of a whole file, the replay of the reference's SegmentPathIter)
without a GPU: tests/cpp/gfa_host.cpp as a program of its own under ASan + UBSan, linked with gfa_host.cpp and host_index.cpp only,
against the oracle."""
import os

import numpy as np

import oracle_lib as O
from gbwt_rs_amd import _lib
from gbwt_rs_amd import synth as S
from test_merge_cpu import sanitized_program


def broken_paths_graph(tmp_path):
    """The graph of test_synthetic_translation_broken_paths (tests/test_gpu_gfa.py): paths that are not concatenations of whole segments."""
    starts = [1, 4, 5, 7, 8, 12]                   # segments: [1,2,3] [4] [5,6] [7] [8,9,10,11] [12]
    fwd = lambda a, b: [2 * v for v in range(a, b + 1)]
    rev = lambda a, b: [2 * v + 1 for v in range(b, a - 1, -1)]
    paths = [fwd(1, 3) + fwd(4, 4),                # valid
             fwd(2, 3) + fwd(4, 4),                # enters segment [1,2,3] at its second node
             fwd(1, 2) + fwd(4, 4),                # leaves segment [1,2,3] early: the row is cut in the middle of a segment
             fwd(1, 3) + rev(5, 5) + fwd(7, 7),    # enters [5,6] reversed at the wrong end
             fwd(4, 4) + fwd(9, 9),                # ends inside a segment entered in the middle
             fwd(8, 9) + rev(9, 9),                # turns around inside a segment
             fwd(1, 3) + fwd(1, 3),                # valid: the same segment twice
             fwd(12, 12)]                          # (makes node 12 exist)
    path = tmp_path / "broken.gbz"
    S.Synth.from_paths(paths, bidirectional=True).attach_gbz(starts, seed=5).save(str(path), as_gbz=True)
    return str(path)


def test_host_graph_lines_and_segment_paths_under_sanitizers(tmp_path, monkeypatch):
    """host_graph_lines on example.gbz and translation.gbz: byte for byte the H-, S- and L-lines of the oracle's file (every line that is no
    P- or W-line, in order).  host_segment_path on every sequence of translation.gbz and of the broken-paths graph -- the oracle's
    segment_path takes a sequence id, not a row, so the rows that stop inside a segment come from that generator -- fed the node rows the
    oracle extracts: the oracle's tokens, and for forward sequences the summed segment lengths the oracle's W-line ends on."""
    files = {"example": os.path.join(O.GOLDEN, "example.gbz"), "translation": os.path.join(O.GOLDEN, "translation.gbz"), "broken": broken_paths_graph(tmp_path)}
    oracles = {name: O.OracleGBZ(path) for name, path in files.items()}
    job, rows = [], {}
    for name in ("example", "translation", "broken"):
        job += ["file " + files[name], "lines " + name + ".gfa"]
        if name == "example":
            continue                               # (no node-to-segment translation)
        gbwt = oracles[name].gbwt()
        offsets, nodes = gbwt.extract(np.arange(gbwt.sequences(), dtype=np.uint64))
        for seq in range(gbwt.sequences()):
            rows[f"{name}{seq}"] = (name, seq)
            job.append(f"row {name}{seq} " + " ".join(str(int(v)) for v in nodes[int(offsets[seq]):int(offsets[seq + 1])]))
    (tmp_path / "job.txt").write_text("\n".join(job) + "\n")
    monkeypatch.setenv("GFA_HOST_JOB", str(tmp_path / "job.txt"))
    monkeypatch.setenv("GFA_HOST_OUT", str(tmp_path))
    got, _ = sanitized_program(tmp_path, "gfa_host", os.path.join(_lib.CSRC, "gfa_host.cpp"), os.path.join(_lib.CSRC, "host_index.cpp"))
    for name, oracle in oracles.items():
        graph_lines = b"".join(l for l in oracle.gfa().splitlines(keepends=True) if l[:1] not in (b"P", b"W"))
        assert graph_lines.startswith(b"H\t") and b"\nS\t" in graph_lines and b"\nL\t" in graph_lines
        assert bytes.fromhex(got[f"lines.{name}.gfa"]) == graph_lines, name
    stopped_inside = 0
    for key, (name, seq) in rows.items():
        fields = got["row." + key].split()
        want = oracles[name].segment_path(seq)
        assert [tuple(int(x) for x in f.split(":")) for f in fields[1:]] == want, key
        if seq % 2 == 0:                           # W-line: ... <fragment> <fragment + summed segment lengths> <walk>
            w = oracles[name].path_lines([seq // 2], 1).split(b"\t")
            assert int(fields[0]) == int(w[5]) - int(w[4]), key
        if name == "broken":                       # the nodes its tokens stand for are not the row: the iterator has stopped inside it
            segments = ([1, 2, 3], [4], [5, 6], [7], [8, 9, 10, 11], [12])
            whole = [2 * v + o for s, o in want for v in (segments[s][::-1] if o else segments[s])]
            stopped_inside += len(want) > 0 and whole != list(oracles[name].gbwt().sequence(seq))
    assert len(rows) == 2 * oracles["translation"].paths() + 16 and 3 <= stopped_inside <= 10      # (rows that yield some tokens and then stop: among the five broken paths and their reverses)
