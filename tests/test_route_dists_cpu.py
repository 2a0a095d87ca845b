"""The frontier planner's per-action rule on the CPU (include/voxnav.h, vn_plan_frontier_dists): the
NumPy restatement (tests/route_dists_helpers.py, the reference the GPU tests compare with) against
the hand-derived table, and tied to the restatement of vn_plan_frontier on crafted maps and along
closed loops on the per-agent CPU oracle.
"""
import numpy as np
import pytest

import route_dists_helpers as rd
import route_helpers as rh
from helpers import box_text, product_room_set

BY_NAME = {c[0]: c for c in rh.hand_cases()}


@pytest.mark.parametrize("row", rd.hand_table(), ids=[r[0] for r in rd.hand_table()])
def test_restatement_gives_the_hand_derived_table(row):
    name, want_dists, want_best = row
    _, belief, pos, facing, (action, dist) = BY_NAME[name]
    dists, best, _ = rd.plan_dists(belief, pos, facing)
    assert dists == want_dists
    if want_best is not None:
        assert best == want_best
    rd.check_against_plan(dists, best, action, dist, rh.plan(belief, pos, facing)[2])


def test_flood_flag_of_the_hand_cases():
    """Answered by the neighbour test: no passable neighbour (boxed-in).  Every other hand case
    has its targets further away and floods."""
    for name, belief, pos, facing, _ in rh.hand_cases():
        assert rd.plan_dists(belief, pos, facing)[2] == (name != "boxed-in"), name


@pytest.mark.parametrize("src,L,seed", [("box:16x16x8", 2, 101), ("box:9x9x20", 1, 103), ("set:P2_training", 10, 104),
                                        ("box:4x4x3", 1, 107)])
def test_crafted_maps_agree_with_plan(src, L, seed):
    walls = [r.walls for r in product_room_set(src).rooms]
    pads = tuple(max(w.shape[k] for w in walls) for k in range(3))
    state, belief = rh.crafted_agents(walls, L, 48, pads, seed)
    shapes = [w.shape for w in walls]
    act, dist, tie = rh.plan_batch(state, belief, shapes)
    dists, best, _ = rd.plan_dists_batch(state, belief, shapes)
    for i in range(len(state)):
        rd.check_against_plan([int(v) for v in dists[i]], int(best[i]), int(act[i]), int(dist[i]), bool(tie[i]))


@pytest.mark.parametrize("whd,L", [((8, 8, 4), 4), ((16, 16, 8), 10)], ids=["8x8x4", "16x16x8"])
def test_closed_loop_agrees_with_plan(whd, L):
    """The planner driving the CPU oracle for a whole episode: at every step the per-action rule
    and plan() agree, and the sets hold singletons as well as ties."""
    from oracle.oracle import parse_room_text
    from oracle.py_cubic import PyCubicAgent
    env = PyCubicAgent([parse_room_text(box_text(*whd), "box")], local_map_length=L)
    env.reset(3)
    sizes = set()
    for _ in range(env.max_steps):
        pos = (env.x, env.y, env.z)
        action, dist, tie = rh.plan(env.belief, pos, env.facing)
        dists, best, _ = rd.plan_dists(env.belief, pos, env.facing)
        rd.check_against_plan(dists, best, action, dist, tie)
        sizes.add(bin(best).count("1"))
        _, _, done, truncated = env.step(action)
        if done or truncated:
            break
    assert env.done and {1, 2, 3} <= sizes
