"""The frontier planner's rule on the CPU: the NumPy restatement (tests/route_helpers.py, the
reference every GPU test of vn_plan_frontier compares with) against answers derived by hand, and
its invariants when it drives the per-agent CPU oracle (oracle/py_cubic.py) to the end of an episode.
"""
import numpy as np
import pytest

import route_helpers as rh
from helpers import box_text


@pytest.mark.parametrize("case", rh.hand_cases(), ids=[c[0] for c in rh.hand_cases()])
def test_restatement_gives_the_hand_derived_answer(case):
    _, belief, pos, facing, want = case
    action, dist, _ = rh.plan(belief, pos, facing)
    assert (action, dist) == want


def test_moves_are_do_actions_table():
    # directions_relative_to_facing, written out: rows forward, right, backward, left; columns facing 0..3
    table = [[(0, 1, 0), (1, 0, 0), (0, -1, 0), (-1, 0, 0)],
             [(1, 0, 0), (0, -1, 0), (-1, 0, 0), (0, 1, 0)],
             [(0, -1, 0), (-1, 0, 0), (0, 1, 0), (1, 0, 0)],
             [(-1, 0, 0), (0, 1, 0), (1, 0, 0), (0, -1, 0)]]
    for k in range(4):
        for f in range(4):
            assert rh.move(k, f) == table[k][f]
    for f in range(4):
        assert rh.move(4, f) == (0, 0, 1) and rh.move(5, f) == (0, 0, -1)


def test_ties_are_reported():
    by_name = {c[0]: c for c in rh.hand_cases()}
    assert rh.plan(*by_name["tie-f0"][1:4])[2] and rh.plan(*by_name["detour"][1:4])[2]
    assert rh.plan(*by_name["enclosed"][1:4])[2]
    assert not rh.plan(*by_name["corridor-f1"][1:4])[2]


@pytest.mark.parametrize("whd,L", [((8, 8, 4), 4), ((16, 16, 8), 10)], ids=["8x8x4", "16x16x8"])
@pytest.mark.parametrize("seed", [1, 2])
def test_closed_loop_never_bumps_and_walks_towards_its_target(whd, L, seed):
    """The planner driving the CPU oracle: no bump ever (it only moves into cells it knows to be
    free), and after a step planned with dist = d >= 2 the next dist is in 1..d-1 -- the planned
    path stays valid, a target changes only when stepped on, and sensing can only bring one closer.
    Every episode finishes."""
    from oracle.oracle import parse_room_text
    from oracle.py_cubic import PyCubicAgent
    env = PyCubicAgent([parse_room_text(box_text(*whd), "box")], local_map_length=L)
    env.reset(seed)
    prev = None
    for _ in range(env.max_steps):
        action, dist, _ = rh.plan(env.belief, (env.x, env.y, env.z), env.facing)
        if prev is not None and prev >= 2:
            assert 1 <= dist <= prev - 1, (prev, dist)
        prev = dist
        _, _, done, truncated = env.step(action)
        assert env.bump_count == 0
        if done or truncated:
            break
    assert env.done and env.bump_count == 0
