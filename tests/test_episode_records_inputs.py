"""CPU checks of the inputs of tests/test_episode_records_gpu.py: the oracle's
expectation must exercise the cases the GPU tests are about (terminated and
truncated ends, several ends inside one fused launch, every room drawn), so
an input that stops doing so fails here, without a GPU."""
import numpy as np

import episode_helpers as eh


def test_cubic_fused_case_exercises_every_kind_of_end():
    eo, snaps, first = eh.cubic_expectation(64)
    assert (eo.n_term, eo.n_trunc, eo.n_both) == (3, 431, 1)
    assert (int(eo.rec[:, 0].min()), int(eo.rec[:, 0].max())) == (2, 15)
    assert int((first >= 2).sum()) == 58
    assert len(snaps) == len(eh.CUBIC_LAUNCHES)
    # the totals are the rows' sums, and the four sums really need their width of the row
    assert snaps[-1][1].tolist() == eo.rec[:, :6].sum(0).tolist()
    assert int(eo.totals()[0]) == 435


def test_partial_wave_and_ph16_cases():
    eo, _, first = eh.cubic_expectation(50)
    assert eo.n_term + eo.n_both >= 1 and eo.n_trunc >= 1 and int((first >= 2).sum()) >= 25
    eo, _, first = eh.cubic_expectation(64, boxes=eh.PH16_BOXES, policy_seed=eh.PH16_POLICY_SEED)
    assert eo.n_trunc >= 1 and int((first >= 2).sum()) >= 1
    assert sorted(set(eo.rec[:, 10].tolist())) == [0, 1]


def test_simple_case_has_goals_truncations_and_repeated_ends():
    eo, _, first = eh.simple_expectation()
    assert eo.n_term >= 1 and eo.n_trunc >= 1 and int((first >= 2).sum()) >= 1
    assert int(eo.rec[:, 1].sum()) == eo.n_term + eo.n_both      # finished = goal reached


def test_latch_counts_one_episode_without_autoreset():
    N = 8
    eo = eh.EpisodeOracle(eh.oracle_boxes([(4, 4, 3)], N), 42 + np.arange(N), N, 5, autoreset=False)
    for K in (40, 1, 1):
        eo.run(K)
    assert (eo.rec[:, 0] == 1).all() and (eo.rec[:, 9] == 4).all()
