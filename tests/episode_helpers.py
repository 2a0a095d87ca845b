"""The episode records the device keeps (vn_episode_records), restated on
the CPU oracle: per agent ``OracleEnv.step`` / ``state`` / ``reset`` with
``random_action(policy_seed, gid, t)`` (or given actions) and the pinned seed
schedule ``seed += stride`` at every auto-reset.  Shared by the CPU checks of
the test inputs (tests/test_episode_records_inputs.py) and the GPU tests."""
from __future__ import annotations

import numpy as np

from helpers import box_text

SEED_MOD = 2 ** 32

# the fused auto-reset cases (CubicEnv): walled boxes drawn per episode
CUBIC_BOXES = [(4, 4, 3), (5, 4, 3), (5, 5, 4), (8, 8, 4)]
CUBIC_LAUNCHES = (128, 1, 16, 15)
CUBIC_POLICY_SEED = 7
PH16_BOXES = [(4, 4, 3), (5, 5, 10)]
PH16_POLICY_SEED = 7
# simpleEnv: tiny boxes (goal drawn per episode)
SIMPLE_BOXES = [(4, 4, 3), (5, 4, 4), (6, 5, 4)]
SIMPLE_LAUNCHES = (96, 1, 16, 15)
SIMPLE_POLICY_SEED = 11
SIMPLE_N = 64


def box_texts(boxes):
    return [(f"box{w}x{d}x{h}.txt", box_text(w, d, h)) for (w, d, h) in boxes]


def oracle_boxes(boxes, N, L=4, variant=0):
    from oracle.oracle import OracleEnv, parse_room_text
    return OracleEnv([parse_room_text(t, n) for n, t in box_texts(boxes)], n_agents=N, local_map_length=L,
                     use_room_draw=True, variant=variant)


def product_boxes(boxes):
    from voxnav.rooms import RoomSet, parse_room
    return RoomSet([parse_room(t, n) for n, t in box_texts(boxes)], use_room_draw=True, source="boxes")


class EpisodeOracle:
    """The expected [N, 12] records of an env driven like the oracle."""

    def __init__(self, orc, seeds, stride, policy_seed=0, autoreset=True, gid_base=0):
        self.orc, self.N = orc, orc.n_agents
        self.stride, self.policy_seed, self.autoreset, self.gid_base = int(stride), int(policy_seed), autoreset, gid_base
        self.rec = np.zeros((self.N, 12), np.int64)
        self.next_seed = [0] * self.N
        self.over = [False] * self.N          # without auto-reset: ended, stepped on
        self.t = 0
        self.n_term = self.n_trunc = self.n_both = 0
        for i, s in enumerate(seeds):
            self.reset(i, int(s))

    def reset(self, i, seed):
        """A (manual or auto) reset: a running episode is abandoned, nothing counted."""
        self.orc.reset(i, seed % SEED_MOD)
        self.next_seed[i] = (seed + self.stride) % SEED_MOD
        self.over[i] = False

    def _end(self, i, te, tr):
        st = self.orc.state(i)
        r = self.rec[i]
        r[0] += 1
        r[1] += int(bool(st["done"]))
        r[2] += st["step_count"]
        r[3] += st["bump_count"]
        r[4] += st["visited_count"]
        r[5] += st["max_steps"]
        r[6:] = (st["step_count"], st["bump_count"], st["visited_count"], st["max_steps"], st["room"],
                 int(te) | (int(tr) << 1))
        self.n_term += int(te and not tr)
        self.n_trunc += int(tr and not te)
        self.n_both += int(te and tr)

    def run(self, K, actions=None):
        """K steps of every agent; returns the episode ends per agent in this launch."""
        from oracle.oracle import random_action
        ends = np.zeros(self.N, np.int64)
        self.step_rewards = np.zeros((K, self.N), np.float64)      # this launch's f64 rewards
        for i in range(self.N):
            for k in range(K):
                a = int(actions[k][i]) if actions is not None else \
                    random_action(self.policy_seed, self.gid_base + i, self.t + k)
                _, self.step_rewards[k, i], te, tr = self.orc.step(i, a)
                if (te or tr) and not self.over[i]:
                    self._end(i, te, tr)
                    ends[i] += 1
                    if self.autoreset:
                        self.reset(i, self.next_seed[i])
                    else:
                        self.over[i] = True
        self.t += K
        return ends

    def totals(self):
        return self.rec[:, :6].sum(0)


def expectation(N, boxes, launches, policy_seed, variant=0, L=4):
    """The oracle's (records, totals) after each fused launch of an
    auto-resetting env (seeds 42 + i, stride N), the EpisodeOracle itself and
    the episode ends per agent inside the first launch."""
    eo = EpisodeOracle(oracle_boxes(boxes, N, L, variant=variant), 42 + np.arange(N), N, policy_seed)
    snaps, first_ends = [], None
    for K in launches:
        ends = eo.run(K)
        first_ends = ends if first_ends is None else first_ends
        snaps.append((eo.rec.copy(), eo.totals().copy()))
    return eo, snaps, first_ends


def cubic_expectation(N, boxes=CUBIC_BOXES, policy_seed=CUBIC_POLICY_SEED):
    return expectation(N, boxes, CUBIC_LAUNCHES, policy_seed)


def simple_expectation():
    return expectation(SIMPLE_N, SIMPLE_BOXES, SIMPLE_LAUNCHES, SIMPLE_POLICY_SEED, variant=1)
