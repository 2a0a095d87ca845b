"""Shared helpers for the parity tests (golden fixtures, room sources)."""
from __future__ import annotations

import hashlib
import tarfile
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / "tests" / "golden"
ARCHIVE = REPO / "rooms" / "reference_rooms.tar.xz"

STATE13 = ("x", "y", "z", "facing", "last_action", "step_count", "visited_count", "bump_count",
           "done", "last_bump", "near_wall", "was_near_wall", "cells_insight_down")


def grid_hash(a: np.ndarray) -> int:
    h = hashlib.blake2b(np.ascontiguousarray(a, dtype=np.int64).tobytes(), digest_size=8).digest()
    return int(np.frombuffer(h, dtype=np.uint64)[0])


_ARCH_CACHE = {}


def archive_texts() -> dict:
    """{'P2_training/kitchen2.txt': text, ...} from the committed room archive."""
    if not _ARCH_CACHE:
        with tarfile.open(ARCHIVE) as tf:
            for m in tf.getmembers():
                if m.isfile():
                    rel = str(Path(m.name).relative_to("rooms"))
                    _ARCH_CACHE[rel] = tf.extractfile(m).read().decode()
    return _ARCH_CACHE


def set_members(setname: str):
    """Sorted (name, text) of a room set, the glob('*.txt') of that directory."""
    texts = archive_texts()
    out = [(Path(k).name, v) for k, v in texts.items() if Path(k).parent.name == setname and k.endswith(".txt")]
    return sorted(out, key=lambda t: t[0])


def box_text(W, D, H) -> str:
    lines = [f"Size={W},{D},{H}"]
    for z in range(H):
        lines.append(f"Layer z={z}")
        for y in range(D):
            lines.append(" ".join("2" if (x in (0, W - 1) or y in (0, D - 1) or z in (0, H - 1)) else "0"
                                  for x in range(W)))
    return "\n".join(lines) + "\n"


def source_texts(src: str):
    """room_source string of a golden file -> ([(name, text)], use_room_draw, ctor_whd)."""
    kind, arg = src.split(":", 1)
    if kind == "ctor":
        return [], False, tuple(int(v) for v in arg.split("x"))
    if kind == "box":
        W, D, H = (int(v) for v in arg.split("x"))
        return [(f"box_{arg}.txt", box_text(W, D, H))], True, None
    if kind == "file":
        return [(Path(arg).name, archive_texts()[arg])], True, None
    if kind == "set":
        return set_members(arg), True, None
    raise ValueError(src)


def oracle_env(src: str, L: int, n_agents: int = 1, crash_penalty: float = -2.0, variant: int = 0):
    from oracle.oracle import OracleEnv, parse_room_text, walled_box
    texts, draw, whd = source_texts(src)
    rooms = [walled_box(*whd)] if whd else [parse_room_text(t, n) for n, t in texts]
    return OracleEnv(rooms, n_agents=n_agents, local_map_length=L, crash_penalty=crash_penalty, use_room_draw=draw,
                     variant=variant)


# The collector's policy paths ("Collector paths"):
#   id -> (lstm_hidden_size or None for the MLP policy, net_arch widths (pi = vf), policy_dtype,
#          voxnav.collector._Weights' (recurrent, fused, fused32, f32mlp, mlp_head))
# tests/test_collector_paths.py pins the flags on the CPU; the GPU cases of
# tests/test_collector_gpu.py build their policies from the same rows.
COLLECTOR_PATHS = {
    # the reference's shapes: vn_lstm_fused_f32 + vn_mlp_head_f32
    "P0": (256, [256, 256, 128], "f32", (True, False, True, True, True)),
    # vn_lstm_fused_f32 + vn_linear_f32 per layer + vn_policy_head
    "P1": (64, [384, 128], "f32", (True, False, True, True, False)),
    # torch.mm + vn_lstm_cell[_masked] + addmm + vn_policy_head (SB3's default net_arch)
    "P2": (48, [64, 64], "f32", (True, False, False, False, False)),
    # torch.mm + vn_lstm_cell_masked + vn_mlp_head_f32 with K0 = 48; _critic: addmm + vn_policy_head
    "P3": (48, [128, 128], "f32", (True, False, False, True, True)),
    # addmm + vn_policy_head
    "P4": (None, [64, 64], "f32", (False, False, False, False, False)),
    # vn_linear_f32 per layer + vn_policy_head
    "P5": (None, [384, 128], "f32", (False, False, False, True, False)),
    # torch.mm + vn_lstm_cell_bf16 + addmm + vn_policy_head_bf16
    "P6": (48, [64, 64], "bf16", (True, False, False, False, False)),
    # vn_lstm_fused_bf16[_masked] + addmm + vn_policy_head_bf16
    "P7": (256, [256, 256, 128], "bf16", (True, True, False, False, False)),
    # the reference's MLP policy (BASELINE C3): vn_mlp_head_f32 with K0 = 80, and its bf16 option
    "M0": (None, [256, 256, 128], "f32", (False, False, False, True, True)),
    "M1": (None, [256, 256, 128], "bf16", (False, False, False, False, False)),
}


def path_policy(pid: str, n_actions: int = 6):
    """The (CPU, f32) policy module of a COLLECTOR_PATHS row."""
    from voxnav.policy import ActorCriticPolicy, RecurrentActorCriticPolicy
    H, widths, _, _ = COLLECTOR_PATHS[pid]
    arch = dict(pi=list(widths), vf=list(widths))
    if H is None:
        return ActorCriticPolicy(n_actions=n_actions, net_arch=arch)
    return RecurrentActorCriticPolicy(n_actions=n_actions, lstm_hidden_size=H, net_arch=arch)


def path_flags(w):
    """(recurrent, fused, fused32, f32mlp, mlp_head) of a voxnav.collector._Weights."""
    return (w.recurrent, w.fused, w.fused32, w.f32mlp, w.mlp_head)


def philox_uniform(seed, gids, t):
    """The sampler's uniform (collector_oracle.sample_uniform) for many agents at once (numpy)."""
    m = np.uint64(0xFFFFFFFF)
    gids = np.asarray(gids, np.uint64)
    hi = (int(t) | (1 << 63)) & ((1 << 64) - 1)
    c0, c1 = gids & m, gids >> np.uint64(32)
    c2 = np.full_like(gids, hi & 0xFFFFFFFF)
    c3 = np.full_like(gids, hi >> 32)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(0x9E3779B9)) & m
            k1 = (k1 + np.uint64(0xBB67AE85)) & m
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m
    return (c0 >> np.uint64(8)).astype(np.float64) / 16777216.0


# vn_policy_head[_bf16] alone (tests/test_collector_kernels_gpu.py): (N, P, A) and the draws'
# (sample_seed, t, agent_id_base) -- the second with the counter's high words in use
HEAD_CASES = [(4099, 128, 6), (1, 4, 1), (17, 68, 8), (300, 4096, 8)]
HEAD_DRAWS = [(1234, 77, 1000), (0x1234567890ABCDEF, (1 << 33) + 5, (1 << 32) + 12345)]


def head_case_data(N, P, A):
    """Latents in multiples of 1/8 (|x| <= 1/2), head weights in multiples of
    1/16 (|w| <= 3/16), biases in multiples of 1/8 -- f32 and bf16 hold them
    exactly and, with P <= 4096, every partial sum of a logit or value in any
    order (units of 1/128, below 2^24 of them).  Action a's bias also carries
    a / 1024, so two logits of a row never tie.  -> dict of float64 arrays
    with the exact logits / values and the float64 log-softmax."""
    rng = np.random.default_rng(1000 * N + P + A)
    lat_pi = rng.integers(-4, 5, size=(N, P)) / 8.0
    lat_vf = rng.integers(-4, 5, size=(N, P)) / 8.0
    wa = rng.integers(-3, 4, size=(A, P)) / 16.0
    wv = rng.integers(-3, 4, size=P) / 16.0
    ba = rng.integers(-8, 9, size=A) / 8.0 + np.arange(A) / 1024.0
    bv = np.array([rng.integers(-8, 9) / 8.0])
    logits = lat_pi @ wa.T + ba
    values = lat_vf @ wv + bv[0]
    m = logits.max(axis=1, keepdims=True)
    lsm = logits - (m + np.log(np.exp(logits - m).sum(axis=1, keepdims=True)))
    return dict(lat_pi=lat_pi, lat_vf=lat_vf, wa=wa, wv=wv, ba=ba, bv=bv, logits=logits, values=values, lsm=lsm)


def head_draws64(lsm, u):
    """The Categorical draw of float64 log-probs lsm [N, A] for the uniforms
    u [N]: first a with u < cdf[a] (the last action if none), and u's distance
    to the nearest CDF boundary (1 when there is none)."""
    N, A = lsm.shape
    if A == 1:
        return np.zeros(N, np.int64), np.ones(N)
    cdf = np.cumsum(np.exp(lsm), axis=1)[:, :A - 1]
    hit = u[:, None] < cdf
    act = np.where(hit.any(1), hit.argmax(1), A - 1)
    return act, np.abs(cdf - u[:, None]).min(1)


def head_draws32(logits32, u):
    """vn_policy_head's draw restated in numpy f32, step by step as the
    kernel does it (max, sum of exp, lse, running CDF of exp(logit - lse),
    u = (w >> 8) * 2^-24 as f32); numpy's expf / logf may differ from the
    device's in the last bit."""
    f = np.float32
    lg = np.asarray(logits32, f)
    N, A = lg.shape
    mx = lg.max(1)
    se = np.zeros(N, f)
    for a in range(A):
        se = (se + np.exp((lg[:, a] - mx).astype(f)).astype(f)).astype(f)
    lse = (mx + np.log(se).astype(f)).astype(f)
    u32 = np.asarray(u, f)          # (w >> 8) / 2^24 is exact in f32
    act = np.full(N, A - 1, np.int64)
    cdf = np.zeros(N, f)
    for a in range(A - 1):
        cdf = (cdf + np.exp((lg[:, a] - lse).astype(f)).astype(f)).astype(f)
        act = np.where((u32 < cdf) & (act == A - 1), a, act)
    return act


def simple_golden_trajectories():
    return sorted(GOLDEN.glob("simple_*.npz"))


def product_room_set(src: str):
    from voxnav.rooms import RoomSet, ctor_box_set, parse_room
    texts, draw, whd = source_texts(src)
    if whd:
        return ctor_box_set(*whd)
    return RoomSet([parse_room(t, n) for n, t in texts], use_room_draw=draw, source=src)


def golden_trajectories():
    return sorted(GOLDEN.glob("traj_*.npz"))


def load_golden(path) -> dict:
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
