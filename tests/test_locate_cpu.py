"""tests/locate_expect.py, the truth of the GPU locate tests, against the oracle's GBWT::sequence on the golden files and on a path that
visits one node again and again (no GPU)."""
import os
from collections import Counter

import numpy as np
import pytest

import locate_expect as LX
import oracle_lib as O
import tangled_graphs as TG
from gbwt_rs_amd import synth as S


def load(name):
    path = os.path.join(O.GOLDEN, name)
    if name.endswith(".gbz"):
        return O.OracleGBZ(path).gbwt()
    return O.OracleGBWT.load(path)


def synth_oracle(paths, bidirectional=True):
    s = S.Synth.from_paths(paths, bidirectional=bidirectional)
    bwt = O.OracleBWT.from_parts(s.data(), s.starts())
    return s, O.OracleGBWT.from_bwt(bwt, s.sequences, s.size, s.alphabet_offset, s.alphabet_size, bidirectional)


@pytest.mark.parametrize("name", ["example.gbwt", "example.gbz", "translation.gbz", "with-empty.gbwt"])
def test_rows_hold_the_sequences_that_contain_the_node(name):
    g = load(name)
    own = LX.owners(g)
    sequences = [g.sequence(i) for i in range(g.sequences())]
    assert len(own) == sum(len(s) for s in sequences)
    visits = Counter((node, i) for i, s in enumerate(sequences) for node in s)
    with_record = 0
    for node in range(0, g.alphabet_size() + 3):
        state = g.find(node)
        if state is None:
            assert LX.row(own, (node, 0, 1), False) is None and LX.position(own, (node, 0)) is None
            continue
        with_record += 1
        plain = LX.row(own, state, False)
        assert len(plain) == state[2] - state[1] == own.lengths.of(node)
        assert Counter((node, i) for i in plain) == Counter({k: v for k, v in visits.items() if k[0] == node})
        assert LX.row(own, state, True) == sorted(set(plain))
        assert LX.row(own, (node, 0, state[2] + 1), False) is None and LX.row(own, (node, 1, 1), True) is None
        assert LX.position(own, (node, state[2])) is None and LX.position(own, (node, 0)) == plain[0]
    assert with_record == len({node for s in sequences for node in s})
    if name == "with-empty.gbwt":
        assert any(len(s) == 0 for s in sequences)


def test_a_sequence_that_revisits_a_node_owns_all_of_its_positions():
    _, paths = TG.self_loop(length=8, visits=10)
    _, g = synth_oracle(paths)
    own = LX.owners(g)
    for node, visits in ((TG.fwd(2), 5), (TG.rev(2), 5)):
        state = g.find(node)
        assert state[2] - state[1] == 10                # five forward visits of sequence 0 and five reverse visits of sequence 1, or the other way round
        plain = LX.row(own, state, False)
        assert sorted(Counter(plain).values()) == [visits, visits] and set(plain) == {0, 1}
    # every position of the node of a one-orientation loop belongs to the one sequence
    loop = [np.array([TG.fwd(1)] + [TG.fwd(2)] * 7 + [TG.fwd(3)], dtype=np.uint64)]
    _, g = synth_oracle(loop, bidirectional=False)
    own = LX.owners(g)
    state = g.find(TG.fwd(2))
    assert LX.row(own, state, False) == [0] * 7 and LX.row(own, state, True) == [0]
    csr = LX.csr([LX.row(own, state, True), None, LX.row(own, state, False)])
    assert csr[0].tolist() == [0, 1, 1, 8] and csr[1].tolist() == [0] * 8 and csr[2].tolist() == [True, False, True]
