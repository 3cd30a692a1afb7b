"""Weakly connected components and contig path selection without a GPU: the expected-value helper of tests/test_gpu_components.py
reproduces the reference's own known answer, its select_paths restatement a hand-made case, and the C ABI declares, exports and types
the entry points."""
import os
import re

import pytest

import components_expect as X
import oracle_lib as O
from gbwt_rs_amd import _lib

NEW_SYMBOLS = ["gbwt_hip_components_device", "gbwt_hip_weakly_connected_components", "gbwt_hip_path_components", "gbwt_hip_last_components_ms",
               "gbwt_hip_select_paths", "gbwt_hip_write_sequences_contig"]


def test_helper_reproduces_the_reference_vector():
    """src/gbz/tests.rs:503-518 (and the doc test of GBZ::weakly_connected_components, src/gbz.rs:565-568) on example.gbz."""
    gbwt = O.OracleGBZ(os.path.join(O.GOLDEN, "example.gbz")).gbwt()
    assert X.components(gbwt) == [[11, 12, 13, 14, 15, 16, 17], [21, 22, 23, 24, 25]]
    assert X.geometry(gbwt) == (11, 15)
    # the bare GBWT of the same graph gives the same components
    assert X.components(O.OracleGBWT.load(os.path.join(O.GOLDEN, "example.gbwt"))) == [[11, 12, 13, 14, 15, 16, 17], [21, 22, 23, 24, 25]]
    firsts = X.first_nodes(gbwt, 6)
    assert firsts[:2] == [11, 21] and X.path_components(X.components(gbwt), firsts)[:2] == [0, 1]


def test_select_paths_restatement_by_hand():
    """Three components; paths 0-6 start in components 0, 0, 1, 1, 2, -, 2 (path 5 is empty) and carry contigs a, u, b, b, c, u, u
    (u = "unplaced", z = a contig name no path carries)."""
    comps = [[1, 2, 3], [5, 6], [8]]
    firsts = [1, 3, 5, 6, 8, None, 8]
    names = ["a", "b", "c", "u", "z"]
    contigs = [0, 3, 1, 1, 2, 3, 3]
    assert X.path_components(comps, firsts) == [0, 0, 1, 1, 2, X.NONE, 2]
    assert X.select_paths(comps, firsts, contigs, names, None) == [0, 1, 2, 3, 4, 5, 6]
    assert X.select_paths(comps, firsts, contigs, names, "a") == [0, 1]            # the unplaced path of a's component comes along
    assert X.select_paths(comps, firsts, contigs, names, "b") == [2, 3]
    assert X.select_paths(comps, firsts, contigs, names, "c") == [4, 6]
    assert X.select_paths(comps, firsts, contigs, names, "u") == [0, 1, 4, 6]      # every component an unplaced path starts in; never the empty path
    for contig, message in (("q", "The graph does not contain contig q"), ("z", "The graph does not contain any paths for contig z")):
        with pytest.raises(ValueError, match=message):
            X.select_paths(comps, firsts, contigs, names, contig)
    with pytest.raises(ValueError, match="Cannot select a contig without contig names"):
        X.select_paths(comps, firsts, contigs, None, "a")


def test_entry_points_declared_exported_and_typed():
    header = open(_lib.HEADER).read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"gbwt_hip_status\s+" + name + r"\(", header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
