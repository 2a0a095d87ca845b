"""Float64 restatement of the return-based reward normalisation (the rule in
include/voxnav.h, "Return-based reward normalisation"; SB3 VecNormalize with
norm_reward=True), shared by tests/test_reward_norm_{cpu,host,gpu}.py.
Importing this module needs no GPU.

Every operation below is one IEEE float64 + - * / sqrt on numpy float64
scalars or arrays, in the order the rule states, so the C++ of
csrc/ret_rms.h and the kernels of csrc/voxnav_rnorm.hip (built without
contraction) must reproduce these numbers bit for bit.

The bound of `sb3_rel_bound` (the restatement against the straightforward
np.mean / np.var form of SB3's update).  u = 2^-53.  Both forms compute the
same real-valued function of the same f64 returns, so they differ by rounding
only, and the bound counts the roundings on each path and adds the two:

  batch mean, this rule: the butterfly is 6 levels of additions (any one lane's
  value passes through 6), the division by m one more, and each of the
  ceil(log2 C) tree levels puts a value through one merge, whose mean costs 4
  roundings (d, d * n_b, / n, +):  6 + 1 + 4 L roundings deep, L = ceil(log2 C).
  Each rounding perturbs the result by at most u relative to the magnitudes it
  adds; with R = max |ret| / |mean_B| as the condition number of the sum (the
  additions are of numbers as large as max |ret|, the result as small as the
  mean), the relative error is at most (7 + 4 L) u R (1 + small).
  batch mean, np.mean: pairwise summation of N terms, ceil(log2 N) + 1 <=
  6 + L + 1 roundings deep, and the division: (8 + L) u R.

  batch variance: the deviations (ret - mean)^2 carry 2 roundings and twice the
  relative error of the mean scaled by |mean| / |ret - mean|; M2 adds 6
  butterfly levels and per tree level 7 roundings (the M2 line of merge) plus
  twice the mean's error.  All M2 terms are non-negative, so their sum is
  perfectly conditioned with respect to its own roundings; the only
  cancellation is in ret - mean, and since squared deviations are summed the
  bound uses R2 = max (ret - mean)^2 / var_B >= 1 for the propagated mean error.
  The count: (2 + 6 + 7 L + 1) u for M2's own roundings and
  2 (7 + 4 L) u R R2^(1/2) for the mean's; np.var likewise with its own
  (8 + L) u R R2^(1/2) and (3 + 6 + L + 1) u.

  the T running updates: each is one merge plus var * count, var_B * n_B and
  M2 / n: 4 roundings on the mean and 7 + 3 on the variance, added per step,
  and the straightforward form spends the same number in its own order; the
  running mean is again a cancelling sum (condition Rm = max_t |mean_B,t| /
  |mean_T|), the running M2 is a sum of non-negative terms.

Collected (both paths, so each count doubled, and a factor 2 for the
second-order terms the counts ignore):
  rel(mean) <= 4 u [(15 + 5 L) R + 4 T] Rm
  rel(var)  <= 4 u [(28 + 8 L) + 2 (15 + 5 L) R sqrt(R2) + 10 T] Rv
with Rv = max(1, max_t (mean_B,t - mean_t)^2 / var_T) for the mean-difference
term of the variance merge.  R, R2, Rm, Rv are computed from the data by
`sb3_rel_bound`, none of them from the difference under test.
"""
from __future__ import annotations

import math

import numpy as np

F64 = np.float64
CHUNK = 64
U53 = 2.0 ** -53


def new_state(n_agents: int, mean=0.0, var=1.0, count=1e-4):
    """{'rms': f64 [3] = (mean, var, count), 'ret': f64 [N]}; SB3's RunningMeanStd(epsilon=1e-4) by default."""
    return dict(rms=np.array([mean, var, count], F64), ret=np.zeros(n_agents, F64))


def merge(a, b):
    """(n, mean, M2) of the union, the rule's merge, on f64 scalars."""
    n_a, mean_a, m2_a = (F64(v) for v in a)
    n_b, mean_b, m2_b = (F64(v) for v in b)
    n = n_a + n_b
    d = mean_b - mean_a
    mean = mean_a + (d * n_b) / n
    m2 = (m2_a + m2_b) + (((d * d) * n_a) * n_b) / n
    return n, mean, m2


def butterfly(v):
    """v_j += v_{j xor s}, s = 1 .. 32, on a f64 [64] vector; lane 0's sum."""
    v = np.asarray(v, F64).copy()
    j = np.arange(CHUNK)
    s = 1
    while s < CHUNK:
        v = v + v[j ^ s]
        s <<= 1
    return v[0]


def chunk_triples(ret, agent_id_base: int = 0):
    """The chunk triples [C][3] of one shard's returns (global id = agent_id_base + i)."""
    if agent_id_base % CHUNK:
        raise ValueError("agent_id_base must be a multiple of 64")
    ret = np.asarray(ret, F64)
    out = []
    for c0 in range(0, len(ret), CHUNK):
        part = ret[c0:c0 + CHUNK]
        m = len(part)
        v = np.zeros(CHUNK, F64)
        v[:m] = part
        n = F64(m)
        mean = butterfly(v) / n
        sq = np.zeros(CHUNK, F64)
        dev = part - mean
        sq[:m] = dev * dev
        out.append((n, mean, butterfly(sq)))
    return np.array(out, F64).reshape(-1, 3)


def tree(triples):
    """The binary tree over the chunk triples [C][3] -> the root (n, mean, M2)."""
    nodes = [tuple(F64(v) for v in t) for t in np.asarray(triples, F64)]
    while len(nodes) > 1:
        nodes = [merge(nodes[k], nodes[k + 1]) if k + 1 < len(nodes) else nodes[k] for k in range(0, len(nodes), 2)]
    return nodes[0]


def update(rms, root):
    """Step 3 on rms = (mean, var, count) -> the new (mean, var, count), f64 [3]."""
    mean, var, count = (F64(v) for v in rms)
    n_b, mean_b, m2_b = root
    var_b = m2_b / n_b
    n, mean, m2 = merge((count, mean, var * count), (n_b, mean_b, var_b * n_b))
    return np.array([mean, m2 / n, n], F64)


def scale(var, epsilon=1e-8):
    return np.sqrt(F64(var) + F64(epsilon))


def normalize_rewards(r, sc, clip=10.0):
    """Step 4: f32 rewards r by the f64 scale sc, clipped in f64, rounded once to f32."""
    x = np.asarray(r, np.float32).astype(F64) / F64(sc)
    return np.clip(x, -F64(clip), F64(clip)).astype(np.float32)


def moments(state, rewards, dones, t0, t1, gamma, agent_id_base=0):
    """vn_return_moments restated: steps [t0, t1) of rewards / dones [T][N] for one shard; carries
    state['ret'] and returns the chunk triples f64 [t1 - t0][C][3]."""
    ret = state["ret"]
    out = []
    for t in range(t0, t1):
        ret[:] = ret * F64(gamma) + np.asarray(rewards[t], np.float32).astype(F64)
        out.append(chunk_triples(ret, agent_id_base))
        ret[np.asarray(dones[t]) != 0] = 0.0
    return np.stack(out)


def normalize(state, rewards, t0, t1, partials, epsilon=1e-8, clip=10.0, training=True):
    """vn_reward_normalize restated: rewards [T][N] f32 normalised in place over [t0, t1) from the
    (concatenated) chunk triples; updates state['rms']; returns the per-step scales f64 [t1 - t0]."""
    scales = np.zeros(t1 - t0, F64)
    for t in range(t0, t1):
        if training:
            state["rms"] = update(state["rms"], tree(partials[t - t0]))
        scales[t - t0] = scale(state["rms"][1], epsilon)
        rewards[t] = normalize_rewards(rewards[t], scales[t - t0], clip)
    return scales


def run(state, rewards, dones, t0, t1, gamma, epsilon=1e-8, clip=10.0, training=True, shards=None):
    """Both calls on steps [t0, t1).  `shards`: the shard sizes (their sum N), each shard's triples
    computed on its own and concatenated in order; None: one shard.  rewards [T][N] f32 is
    normalised in place; returns the per-step scales."""
    N = rewards.shape[1]
    if not training:
        return normalize(state, rewards, t0, t1, None, epsilon, clip, training=False)
    sizes = [N] if shards is None else list(shards)
    assert sum(sizes) == N and all(s % CHUNK == 0 for s in sizes[:-1])
    parts, base = [], 0
    for s in sizes:
        sub = dict(ret=state["ret"][base:base + s])         # a view: the shard's slice is carried in place
        parts.append(moments(sub, rewards[:, base:base + s], dones[:, base:base + s], t0, t1, gamma, base))
        base += s
    return normalize(state, rewards, t0, t1, np.concatenate(parts, axis=1), epsilon, clip)


# --------------------------------------------------------------- the straightforward form
def sb3_update(rms, batch):
    """RunningMeanStd.update as SB3 writes it (np.mean / np.var, update_from_moments)."""
    mean, var, count = rms
    batch_mean, batch_var, batch_count = np.mean(batch), np.var(batch), batch.shape[0]
    delta = batch_mean - mean
    tot = count + batch_count
    new_mean = mean + delta * batch_count / tot
    m2 = var * count + batch_var * batch_count + np.square(delta) * count * batch_count / tot
    return np.array([new_mean, m2 / tot, tot], F64)


def sb3_run(rms, rewards, dones, gamma):
    """VecNormalize._update_reward over rewards [T][N] (f64 here) -> (rms, the per-step returns [T][N])."""
    T, N = rewards.shape
    ret = np.zeros(N, F64)
    rets = np.zeros((T, N), F64)
    for t in range(T):
        ret = ret * gamma + rewards[t]
        rets[t] = ret
        rms = sb3_update(rms, ret)
        ret[dones[t] != 0] = 0.0
    return rms, rets


def sb3_rel_bound(rms0, rets, rms_steps):
    """(bound on rel(mean), bound on rel(var)) of the module docstring for returns rets [T][N] and the
    restatement's statistics after each step rms_steps [T][3] (the data's condition numbers only)."""
    T, N = rets.shape
    L = max(0, math.ceil(math.log2(max(1, -(-N // CHUNK)))))
    bm = rets.mean(axis=1)
    bv = rets.var(axis=1)
    R = float(np.max(np.abs(rets).max(axis=1) / np.abs(bm)))
    R2 = float(np.max(((rets - bm[:, None]) ** 2).max(axis=1) / bv))
    mean_T, var_T = rms_steps[-1][0], rms_steps[-1][1]
    prev = np.vstack([np.asarray(rms0, F64)[None], rms_steps[:-1]])
    Rm = max(1.0, float(np.max(np.abs(bm)) / abs(mean_T)))
    Rv = max(1.0, float(np.max((bm - prev[:, 0]) ** 2) / var_T), float(np.max(bv) / var_T))
    mean_b = 4 * U53 * ((15 + 5 * L) * R + 4 * T) * Rm
    var_b = 4 * U53 * ((28 + 8 * L) + 2 * (15 + 5 * L) * R * math.sqrt(R2) + 10 * T) * Rv
    return mean_b, var_b


# --------------------------------------------------------------- shared cases
def random_case(seed, T, N, p_done=0.1, lo=-1.0, hi=2.0):
    rng = np.random.default_rng(seed)
    rew = rng.uniform(lo, hi, size=(T, N)).astype(np.float32)
    dones = (rng.random((T, N)) < p_done).astype(np.float32)
    return rew, dones


def standard_cases():
    """The cases tests/test_reward_norm_cpu.py works by hand or by property, as data: dicts of
    name, rewards f32 [T][N], dones f32 [T][N], gamma, clip, training, shards (or None) and the
    initial (mean, var, count) and ret."""
    def case(name, rew, dones, gamma, clip=10.0, training=True, shards=None, rms=(0.0, 1.0, 1e-4), ret=None):
        rew = np.asarray(rew, np.float32)
        ret = np.zeros(rew.shape[1], F64) if ret is None else np.asarray(ret, F64)
        return dict(name=name, rewards=rew, dones=np.asarray(dones, np.float32), gamma=gamma, clip=clip,
                    training=training, shards=shards, rms=np.array(rms, F64), ret=ret)
    out = [
        case("one-agent", np.ones((3, 1)), np.zeros((3, 1)), 0.5),
        case("episode-end", [[1.0, 0.5], [2.0, -1.0], [3.0, 4.0]], [[1, 0], [0, 0], [0, 0]], 0.5),
        case("clip-10", [[100.0, -100.0, 1.5]], np.zeros((1, 3)), 0.99, rms=(0.0, 1.0, 1e6)),
        case("clip-2.5", [[100.0, -100.0, 1.5]], np.zeros((1, 3)), 0.99, clip=2.5, rms=(0.0, 1.0, 1e6)),
        case("not-training", [[1.0, -3.0, 50.0, 0.0, 2.0], [2.0, 2.0, 2.0, 2.0, -50.0]], np.ones((2, 5)), 0.9,
             training=False, rms=(0.25, 4.0, 37.0), ret=[1.0, -2.0, 3.5, 0.0, 7.0]),
    ]
    for seed, T, N in ((1, 12, 193), (2, 40, 64), (3, 5, 1000), (4, 25, 7)):
        out.append(case(f"random-T{T}-N{N}", *random_case(seed, T, N), 0.99))
    for shards in ((128, 65), (64, 64, 2)):
        N = sum(shards)
        rew, dones = random_case(10 + N, 9, N, p_done=0.2)
        out.append(case(f"unsharded-N{N}", rew, dones, 0.99))
        out.append(case("shards-" + "+".join(map(str, shards)), rew, dones, 0.99, shards=shards))
    return out


def run_case(c, t0=0, t1=None):
    """A standard case through the restatement -> dict(rms, ret, scales, rewards)."""
    st = dict(rms=c["rms"].copy(), ret=c["ret"].copy())
    rew = c["rewards"].copy()
    t1 = rew.shape[0] if t1 is None else t1
    sc = run(st, rew, c["dones"], t0, t1, c["gamma"], clip=c["clip"], training=c["training"], shards=c["shards"])
    return dict(rms=st["rms"], ret=st["ret"], scales=sc, rewards=rew)
