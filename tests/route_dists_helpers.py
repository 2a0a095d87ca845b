"""The per-action rule of the frontier planner (include/voxnav.h, vn_plan_frontier_dists) restated
in NumPy on a dense belief array -- TEST INFRASTRUCTURE ONLY; the product path is the HIP kernel.

``plan_dists(belief, pos, facing)`` takes what ``route_helpers.plan`` takes and returns
``(dists, best, flooded)``: the six distances (-1: passable and never reached, -2: not passable),
the bit set of the smallest positive ones, and whether the answer needed the flood (False where a
neighbour is itself a target and the agent's own cell is passable: the kernel's 36-lane shortcut,
or where no neighbour is passable).  The flood here runs to its fixpoint for every neighbour; it
shares ``grow`` and ``neighbours`` with the restatement of ``vn_plan_frontier`` and nothing else.
"""
from __future__ import annotations

import numpy as np

import route_helpers as rh

UNREACHED, BLOCKED = -1, -2


def plan_dists(belief, pos, facing):
    b = np.asarray(belief)
    passable = b >= 0
    R = b == 0
    cells = rh.neighbours(pos, facing, b.shape)
    dists = [UNREACHED if c is not None and passable[c] else BLOCKED for _, c in cells]
    open_ = [k for k in range(6) if dists[k] == UNREACHED]
    near = any(R[cells[k][1]] for k in open_)
    flooded = bool(open_) and not (near and passable[tuple(pos)])
    j = 0
    while True:
        for k in open_:
            if dists[k] == UNREACHED and R[cells[k][1]]:
                dists[k] = j + 1
        if all(dists[k] != UNREACHED for k in open_):
            break
        G = rh.grow(R) & passable
        if (G == R).all():
            break
        R = G
        j += 1
    pos_d = [d for d in dists if d > 0]
    best = sum(1 << k for k in range(6) if pos_d and dists[k] == min(pos_d))
    return dists, best, flooded


def plan_dists_batch(state, belief, shapes):
    """The rule for every agent of an exported env (``route_helpers.plan_batch``'s arguments)
    -> (dists int32 [N, 6], best uint8 [N], flooded bool [N])."""
    N = len(state)
    dists, best, flooded = np.zeros((N, 6), np.int32), np.zeros(N, np.uint8), np.zeros(N, bool)
    for i in range(N):
        W, D, H = shapes[int(state[i, 13])]
        dists[i], best[i], flooded[i] = plan_dists(belief[i, :W, :D, :H], tuple(int(v) for v in state[i, :3]),
                                                   int(state[i, 3]))
    return dists, best, flooded


def popcount(best):
    return np.array([bin(int(v)).count("1") for v in np.asarray(best).ravel()]).reshape(np.shape(best))


def check_against_plan(dists, best, action, dist, tie):
    """What ties the per-action rule to ``route_helpers.plan``'s answer for one agent."""
    pos_d = [d for d in dists if d > 0]
    assert (min(pos_d) if pos_d else -1) == dist
    assert (best == 0) == (dist == -1)
    assert all(d - min(pos_d) <= 2 for d in pos_d)       # one step back and on through the best neighbour
    if best:
        assert (best & -best) == 1 << action
        assert tie == (bin(best).count("1") > 1)


# the hand-derived table: (case name of route_helpers.hand_cases(), dists, best or None)
def hand_table():
    """Every row worked out by hand from the rule; the reasoning is beside each case."""
    rows = []
    # corridor-f1: facing +x at x = 1 of the corridor y = 1, z = 1; forward (2,1,1) is five steps
    # from the target at x = 6 (the (0, 5) of the existing case).  Backward is (0,1,1), a wall
    # (the corridor is x = 1..6), right/left leave y = 1 into walls, up/down are walls: all -2.
    rows.append(("corridor-f1", [5, -2, -2, -2, -2, -2], 0b000001))
    # tie-f0: facing +y in the middle (3,3,1) of a visited 7 x 7 plane, targets at (5,3) and (1,3).
    # k = 1 is +x: (4,3) touches the target (5,3): j = 1, dist 2; k = 3 is -x: (2,3), the same.
    # k = 0 is +y: (3,4); the nearest target is |dx| + |dy| = 2 + 1 = 3 flood steps away, dist 4; k = 2
    # (-y, (3,2)) mirrors it.  Up and down are the wall layers.
    rows.append(("tie-f0", [4, 2, 4, 2, -2, -2], 0b001010))
    # tie-f1: the same place facing +x: forward and backward are now the +-x moves.
    rows.append(("tie-f1", [2, 4, 2, 4, -2, -2], 0b000101))
    # detour: facing +x at (1,2); the slab x = 3, y = 0..3 is unknown, its gap at y = 4, the target
    # (5,2).  From a cell (x <= 2, y) the way is to (2,4), through (3,4), (4,4), down to (4,2), then
    # (5,2): |2 - x| + |4 - y| + 2 + 2 + 1 steps.  k = 0 (2,2): 0 + 2 + 5 = 7, dist 8.  k = 3 is +y
    # under facing 1 (heading (1 + 3) % 4 = 0): (1,3): 1 + 1 + 5 = 7, dist 8.  k = 1 is -y (heading 2):
    # (1,1): 1 + 3 + 5 = 9, dist 10.  k = 2 is -x: (0,2): 2 + 2 + 5 = 9, dist 10.
    rows.append(("detour", [8, 10, 10, 8, -2, -2], 0b001001))
    # enclosed: the only target's neighbours are unknown, R_1 = R_0: the four visited neighbours are
    # passable and unreached, up and down are walls.
    rows.append(("enclosed", [-1, -1, -1, -1, -2, -2], 0))
    # boxed-in: every neighbour unknown.
    rows.append(("boxed-in", [-2] * 6, 0))
    # x0-from-32: facing -x at x = 32 of the 64-wide corridor, the target at x = 0.  Forward (31,1,1):
    # 31 flood steps, dist 32 (the existing case); backward (33,1,1): 33 steps, dist 34; the rest walls.
    rows.append(("x0-from-32", [32, -2, 34, -2, -2, -2], None))
    # x63-from-0: facing +x at x = 0, the target at x = 63: forward (1,1,1) is 62 steps away, dist 63;
    # backward is outside the room.
    rows.append(("x63-from-0", [63, -2, -2, -2, -2, -2], None))
    # shaft-up: at z = 2 of the shaft z = 0..5, the target at z = 5: up (z = 3) is 2 steps away, dist 3;
    # down (z = 1) is 4 away, dist 5; the four sides are walls.
    rows.append(("shaft-up", [-2, -2, -2, -2, 3, 5], None))
    # shaft-down: the target at z = 0: down (z = 1) touches it, dist 2; up (z = 3) is 3 away, dist 4.
    rows.append(("shaft-down", [-2, -2, -2, -2, 4, 2], None))
    return rows
