"""The collector's kernel dispatch (voxnav.collector._Weights) pinned on the CPU.

INTEGRATION.md ("Collector paths") states which kernels a policy's shapes
select; ``helpers.COLLECTOR_PATHS`` is that table as data, and the GPU cases
of tests/test_collector_gpu.py run one collector per row.  Here the flags
are asserted without a GPU (the packing functions are plain torch), so a
change of the dispatch shows up as a failure instead of moving a GPU case
onto another kernel.

Also on the CPU: the construction-time refusal of shapes no head kernel
takes, and the seeds of the direct vn_policy_head tests
(tests/test_collector_kernels_gpu.py) checked against a numpy f32
restatement of the kernel's draw.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from helpers import (COLLECTOR_PATHS, HEAD_CASES, HEAD_DRAWS, head_case_data, head_draws32, head_draws64,  # noqa: E402
                     path_flags, path_policy, philox_uniform)

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _weights(pid):
    from voxnav.collector import _Weights
    torch.manual_seed(7)
    return _Weights(path_policy(pid), "cpu", DTYPES[COLLECTOR_PATHS[pid][2]])


@pytest.mark.parametrize("pid", sorted(COLLECTOR_PATHS))
def test_dispatch_table(pid, monkeypatch):
    monkeypatch.delenv("VOXNAV_MLP_HEAD", raising=False)
    H, widths, _, flags = COLLECTOR_PATHS[pid]
    w = _weights(pid)
    assert path_flags(w) == flags
    assert (w.A, w.P) == (6, widths[-1])
    if H is not None:
        assert w.H == H
    # what each flag promises the kernels it selects
    if w.fused32:
        assert w.lstm_packed.shape == (2, H // 64, 80 + H, 4, 64) and w.Kp32 == 80 + H
    if w.fused:
        assert w.w_cat.dtype == torch.bfloat16 and w.w_cat.shape == (2, 4 * H, w.Kp) and w.Kp % 64 == 0
    if w.f32mlp:
        k = H if H is not None else 80
        for n, wp in zip(widths, w.pi_packed):
            assert wp.shape == (n // 128, k, 128)
            k = n
    if w.mlp_head:
        k0 = H if H is not None else 80
        assert w.widths == widths and len(w.mh_wt) == 2 * len(widths)
        assert w.mh_wt[0].shape == (widths[0] // 32, k0 // 8, 2, 32, 4)       # [N/32][K/8][64 lanes][4]
    gemm = DTYPES[COLLECTOR_PATHS[pid][2]]
    assert all(wt.dtype == gemm and b.dtype == gemm for wt, b in w.pi + w.vf)
    assert w.wa.dtype == w.wv.dtype == torch.float32         # the heads stay f32 on every path


def test_mlp_head_knob_gives_the_per_layer_path(monkeypatch):
    """VOXNAV_MLP_HEAD=0 on the reference's shapes: P1's MLP path
    (vn_linear_f32 per layer + vn_policy_head) behind the same fused LSTM."""
    monkeypatch.setenv("VOXNAV_MLP_HEAD", "0")
    assert path_flags(_weights("P0")) == (True, False, True, True, False) == COLLECTOR_PATHS["P1"][3]
    assert path_flags(_weights("M0")) == (False, False, False, True, False) == COLLECTOR_PATHS["P5"][3]
    monkeypatch.setenv("VOXNAV_MLP_HEAD", "1")
    assert path_flags(_weights("P0")) == COLLECTOR_PATHS["P0"][3]


@pytest.mark.parametrize("pid", ["P0", "P2", "P4", "P5", "P6"])
def test_more_than_8_actions_is_refused_at_construction(pid):
    """No head kernel takes more than 8 actions (HEAD_MAX_A): such a policy
    is refused when its weights are laid out, not at the first step."""
    from voxnav.collector import MAX_ACTIONS, _Weights
    assert MAX_ACTIONS == 8
    dt = DTYPES[COLLECTOR_PATHS[pid][2]]
    torch.manual_seed(7)
    _Weights(path_policy(pid, n_actions=8), "cpu", dt)
    with pytest.raises(ValueError, match="at most 8 actions"):
        _Weights(path_policy(pid, n_actions=9), "cpu", dt)


def test_latent_width_no_head_kernel_takes_is_refused():
    from voxnav.collector import MAX_LATENT, _Weights
    from voxnav.policy import ActorCriticPolicy
    torch.manual_seed(7)
    for p in (6, MAX_LATENT + 4):
        with pytest.raises(ValueError, match="latent width"):
            _Weights(ActorCriticPolicy(net_arch=dict(pi=[p], vf=[p])), "cpu")
    _Weights(ActorCriticPolicy(net_arch=dict(pi=[8], vf=[8])), "cpu")


@pytest.mark.parametrize("N,P,A", HEAD_CASES, ids=[f"N{n}-P{p}-A{a}" for n, p, a in HEAD_CASES])
def test_head_case_data_is_exact_and_draws_are_clear(N, P, A):
    """The direct head tests' data: logits / values are exactly representable
    in f32 (so the kernel's sums must equal them bitwise), no two logits of a
    row tie, and for the tests' (seed, t, agent_id_base) a numpy f32
    restatement of the kernel's draw differs from the float64 draw in at most
    2 rows, each within 1e-5 of a CDF boundary -- the allowance the GPU test
    gives."""
    d = head_case_data(N, P, A)
    for k in ("lat_pi", "lat_vf", "wa", "wv", "ba", "bv", "logits", "values"):
        assert np.array_equal(d[k].astype(np.float32).astype(np.float64), d[k]), k
    assert np.abs(d["lat_pi"]).max() <= 0.5 and np.abs(d["wa"]).max() <= 3 / 16
    # f32 sums in the kernel's order (16 lanes x float4 strides, then a butterfly) are
    # exact because every partial sum is: |sum| * 1024 stays below 2^24
    assert ((np.abs(d["lat_pi"]) @ np.abs(d["wa"]).T).max() + np.abs(d["ba"]).max()) * 1024 < 2 ** 24
    if A > 1:
        srt = np.sort(d["logits"], axis=1)
        assert (srt[:, 1:] - srt[:, :-1]).min() > 0.0
    for seed, t, base in HEAD_DRAWS:
        u = philox_uniform(seed, base + np.arange(N, dtype=np.uint64), t)
        a64, margin = head_draws64(d["lsm"], u)
        a32 = head_draws32(d["logits"], u)
        diff = a32 != a64
        assert diff.sum() <= 2 and np.all(margin[diff] < 1e-5)
        if N > 1000:
            assert len(set(a64.tolist())) == A          # every action is drawn


def test_philox_uniform_matches_the_oracle():
    from oracle.collector_oracle import sample_uniform
    for seed, t, base in HEAD_DRAWS:
        u = philox_uniform(seed, base + np.arange(5, dtype=np.uint64), t)
        assert [sample_uniform(seed, base + i, t) for i in range(5)] == u.tolist()
