"""The frontier planner's rule (include/voxnav.h, vn_plan_frontier) restated in NumPy on a dense
belief array -- TEST INFRASTRUCTURE ONLY; the product path is the HIP kernel.

``plan(belief, pos, facing)`` takes one agent's map cut to its room (int [W, D, H]: -2 wall,
-1 unknown, 0 known free and unvisited, n >= 1 visited), its cell and its facing, and returns
``(action, dist, tie)``: the action and distance of the rule, and whether more than one action
reached the flood at that distance (the tie the rule breaks towards the lowest k).
"""
from __future__ import annotations

import numpy as np

# the cell action k moves to under facing f (do_action): heading (f + k) % 4 with 0 = +y, 1 = +x,
# 2 = -y, 3 = -x for k < 4; 4 is +z, 5 is -z
HEADINGS = ((0, 1, 0), (1, 0, 0), (0, -1, 0), (-1, 0, 0))


def move(k: int, f: int):
    if k == 4:
        return (0, 0, 1)
    if k == 5:
        return (0, 0, -1)
    return HEADINGS[(f + k) % 4]


def neighbours(pos, facing, shape):
    """[(k, cell or None)]: None when n_k is outside the room."""
    out = []
    for k in range(6):
        c = tuple(int(p + d) for p, d in zip(pos, move(k, facing)))
        out.append((k, c if all(0 <= c[i] < shape[i] for i in range(3)) else None))
    return out


def grow(R):
    """R and the six-neighbours of its cells."""
    G = R.copy()
    G[1:] |= R[:-1]
    G[:-1] |= R[1:]
    G[:, 1:] |= R[:, :-1]
    G[:, :-1] |= R[:, 1:]
    G[:, :, 1:] |= R[:, :, :-1]
    G[:, :, :-1] |= R[:, :, 1:]
    return G


def plan(belief, pos, facing):
    b = np.asarray(belief)
    passable = b >= 0
    R = b == 0
    nb = [(k, c) for k, c in neighbours(pos, facing, b.shape) if c is not None and passable[c]]
    j = 0
    while True:
        hit = [k for k, c in nb if R[c]]
        if hit:
            return hit[0], j + 1, len(hit) > 1
        G = grow(R) & passable
        if (G == R).all():
            break
        R = G
        j += 1
    if not nb:
        return 0, -1, False
    lo = min(int(b[c]) for _, c in nb)
    ks = [k for k, c in nb if int(b[c]) == lo]
    return ks[0], -1, len(ks) > 1


def plan_batch(state, belief, shapes):
    """The rule for every agent of an exported env: ``state`` int [N, 16] (vn_export_state),
    ``belief`` int8 [N, pw, pd, ph] (vn_export_belief), ``shapes[r]`` the size of room r.
    -> (actions, dist, tie) arrays."""
    N = len(state)
    act, dist, tie = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, bool)
    for i in range(N):
        W, D, H = shapes[int(state[i, 13])]
        act[i], dist[i], tie[i] = plan(belief[i, :W, :D, :H], tuple(int(v) for v in state[i, :3]), int(state[i, 3]))
    return act, dist, tie


# ------------------------------------------------------------------------------------ crafted maps
STEPS6 = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


def _ball(free, centre, radius):
    """Cells within ``radius`` breadth-first steps of ``centre`` through free cells."""
    R = np.zeros(free.shape, bool)
    R[centre] = True
    for _ in range(radius):
        R = grow(R) & free
    return R


def crafted_agents(walls_by_room, L, N, pads, seed):
    """Importable agents (vn_import_state) whose maps make the planner work: per agent a
    random-walk trail of 10-200 moves through its room with visit counts 1-5, for two agents in
    three united with a breadth-first ball of radius 1-4 around the agent; every other free cell
    known and unvisited with probability p in {0, 0.05, 0.5} (cycling per agent); walls known with
    probability 0.5; a random facing; and the sensing marks of the agent's own cell (get_obs marks
    them in any state an env can be in).  A trail with a ball and few known cells gives far targets
    and fallbacks; the dense ones give ties.  -> state int64 [N, 16], belief int8 [N, *pads]
    (-128 outside the agent's room)."""
    rng = np.random.default_rng(seed)
    state = np.zeros((N, 16), np.int64)
    belief = np.full((N, *pads), -128, np.int8)
    for i in range(N):
        r = int(rng.integers(0, len(walls_by_room)))
        walls = walls_by_room[r]
        free = ~walls
        W, D, H = walls.shape
        cells = np.argwhere(free)
        pos = tuple(int(v) for v in cells[rng.integers(0, len(cells))])
        b = np.full(walls.shape, -1, np.int64)
        b[pos] = int(rng.integers(1, 6))
        for _ in range(int(rng.integers(10, 201))):
            d = STEPS6[int(rng.integers(0, 6))]
            c = (pos[0] + d[0], pos[1] + d[1], pos[2] + d[2])
            if all(0 <= c[k] < walls.shape[k] for k in range(3)) and free[c]:
                pos = c
                if b[pos] < 0:
                    b[pos] = int(rng.integers(1, 6))
        if (i // 3) % 3 != 0:
            ball =_ball(free, pos, int(rng.integers(1, 5))) & (b < 0)
            b[ball] = rng.integers(1, 6, size=int(ball.sum()))
        p = (0.0, 0.05, 0.5)[i % 3]
        b[(b < 0) & free & (rng.random(walls.shape) < p)] = 0
        b[walls & (rng.random(walls.shape) < 0.5)] = -2
        for d in STEPS6:                                 # the rays of get_obs from the agent's cell
            c = pos
            for _ in range(L):
                c = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
                if not all(0 <= c[k] < walls.shape[k] for k in range(3)):
                    break
                if walls[c]:
                    b[c] = -2
                    break
                if b[c] == -1:
                    b[c] = 0
        belief[i, :W, :D, :H] = b
        visited = int((b >= 1).sum())
        state[i, :8] = (*pos, int(rng.integers(0, 4)), int(rng.integers(0, 6)), visited, visited, 0)
        state[i, 13] = r
        state[i, 14] = int(free[1:-1, 1:-1, 1:-1].sum())
        state[i, 15] = int(rng.integers(0, 2 ** 32))
    return state, belief


# ------------------------------------------------------------------------------ hand-derived cases
def _plane(W, D, fill=1):
    """A W x D x 3 map whose middle layer z = 1 is visited (count ``fill``); the layers above
    and below it are walls."""
    b = np.full((W, D, 3), -2, np.int64)
    b[:, :, 1] = fill
    return b


def hand_cases():
    """[(name, belief [W, D, H], pos, facing, (action, dist))], every answer worked out by hand
    from the rule; the reasoning is beside each case."""
    cases = []

    # a corridor along x (y = 1, z = 1), the agent at x = 1, one target at x = 6: five steps in +x.
    # +x is heading 1, so the action is (1 - f) mod 4: forward when facing +x, right when facing +y.
    b = np.full((8, 3, 3), -2, np.int64)
    b[1:7, 1, 1] = 1
    b[6, 1, 1] = 0
    cases.append(("corridor-f1", b, (1, 1, 1), 1, (0, 5)))
    cases.append(("corridor-f0", b, (1, 1, 1), 0, (1, 5)))

    # two targets two cells away in +x and in -x (headings 1 and 3; every other neighbour is at
    # least 1 + 3 steps from either): actions (1 - f) mod 4 and (3 - f) mod 4 tie, the lower wins.
    b = _plane(7, 7)
    b[5, 3, 1] = b[1, 3, 1] = 0
    for f, k in ((0, 1), (1, 0), (2, 1), (3, 0)):
        cases.append((f"tie-f{f}", b, (3, 3, 1), f, (k, 2)))

    # a target four cells away in +x behind an unknown slab x = 3, y = 0..3 with its only gap at
    # y = 4: (1,2) -> (2,2) (2,3) (2,4) (3,4) (4,4) (4,3) (4,2) (5,2), eight steps; starting in +y
    # is as short ((1,3) (1,4) (2,4) ...).  Facing +x, +x is action 0 and +y action 3: 0 wins.
    b = _plane(7, 5)
    b[3, 0:4, 1] = -1
    b[5, 2, 1] = 0
    cases.append(("detour", b, (1, 2, 1), 1, (0, 8)))

    # the only target enclosed by unknown cells: the flood never grows.  Fallback, facing +y:
    # n_0 = (1,2) count 3, n_1 = (2,1) count 2, n_2 = (1,0) count 2, n_3 = (0,1) count 5, n_4 and
    # n_5 walls: the smallest count is 2, at actions 1 and 2, the lower wins.
    b = _plane(5, 5, fill=4)
    b[4, 4, 1] = 0
    b[3, 4, 1] = b[4, 3, 1] = -1
    b[1, 2, 1], b[2, 1, 1], b[1, 0, 1], b[0, 1, 1] = 3, 2, 2, 5
    cases.append(("enclosed", b, (1, 1, 1), 0, (1, -1)))

    # no neighbour passable at all: action 0
    b = np.full((3, 3, 3), -1, np.int64)
    b[1, 1, 1] = 1
    cases.append(("boxed-in", b, (1, 1, 1), 2, (0, -1)))

    # a 64-wide corridor: bit 0 and bit 63 of a row.  Facing -x (3): -x is forward, +x backward.
    b = np.full((64, 3, 3), -2, np.int64)
    b[:, 1, 1] = 1
    lo, hi = b.copy(), b.copy()
    lo[0, 1, 1] = 0
    hi[63, 1, 1] = 0
    cases.append(("x0-from-32", lo, (32, 1, 1), 3, (0, 32)))
    cases.append(("x63-from-32", hi, (32, 1, 1), 3, (2, 31)))
    # from one end to the other, 63 steps; the neighbour beyond the agent's end is outside the room
    cases.append(("x63-from-0", hi, (0, 1, 1), 1, (0, 63)))
    cases.append(("x0-from-63", lo, (63, 1, 1), 1, (2, 63)))

    # up and down: a shaft along z, the target above (action 4) or below (action 5)
    b = np.full((3, 3, 6), -2, np.int64)
    b[1, 1, :] = 1
    up, down = b.copy(), b.copy()
    up[1, 1, 5] = 0
    down[1, 1, 0] = 0
    cases.append(("shaft-up", up, (1, 1, 2), 0, (4, 3)))
    cases.append(("shaft-down", down, (1, 1, 2), 0, (5, 2)))
    return cases
