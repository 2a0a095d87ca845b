"""The learner's matrix-core products (voxnav/learn_ops.py over
csrc/voxnav_gemm_f32.hip) against plain PyTorch fp32 on the same device:
the paired Linear+Tanh layers (forward and every gradient), the heads'
plain Linear, and the split-K weight-gradient product with column sums, at
the learner's minibatch size and at ragged / odd shapes.  Tolerances are
relative to each tensor's scale: f32 sums over up to 65,536 samples in a
different order."""
import pytest
import torch

from ppo_loss_helpers import _ppo_loss_reference

pytestmark = pytest.mark.gpu


def _close(got, ref, rel=2e-5, floor=1e-6):
    err = (got - ref).abs().max().item()
    assert err <= rel * ref.abs().max().item() + floor, err


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("M,K,N,shared", [(65536 + 333, 256, 128, False), (65536, 80, 256, True), (77, 40, 6, False)])
def test_linear_tanh_pair_matches_torch(M, K, N, shared):
    from voxnav.learn_ops import linear_tanh_pair
    dev = "cuda:0"
    torch.manual_seed(M + K + N)
    la, lb = torch.nn.Linear(K, N).to(dev), torch.nn.Linear(K, N).to(dev)
    xa = torch.randn((M, K), device=dev, requires_grad=not shared)
    xb = xa if shared else torch.randn((M, K), device=dev, requires_grad=True)
    dy = torch.randn((2, M, N), device=dev)
    w = torch.stack([la.weight, lb.weight])
    b = torch.stack([la.bias, lb.bias])
    y = linear_tanh_pair(xa if shared else torch.stack([xa, xb]), w, b)
    (y * dy).sum().backward()
    got = [la.weight.grad.clone(), la.bias.grad.clone(), lb.weight.grad.clone(), lb.bias.grad.clone()]
    if not shared:
        got += [xa.grad.clone(), xb.grad.clone()]
    for p in [la.weight, la.bias, lb.weight, lb.bias, xa, xb]:
        p.grad = None
    ya, yb = torch.tanh(la(xa)), torch.tanh(lb(xb))
    ((ya * dy[0]).sum() + (yb * dy[1]).sum()).backward()
    _close(y[0], ya)
    _close(y[1], yb)
    ref = [la.weight.grad, la.bias.grad, lb.weight.grad, lb.bias.grad]
    if not shared:
        ref += [xa.grad, xb.grad]
    for g, r in zip(got, ref):
        _close(g, r)


@pytest.mark.parametrize("N", [6, 1, 130])
def test_head_linear_matches_torch(N):
    from voxnav.learn_ops import linear
    dev = "cuda:0"
    torch.manual_seed(N)
    lin = torch.nn.Linear(128, N).to(dev)
    x = torch.randn((4099, 128), device=dev, requires_grad=True)
    dy = torch.randn((4099, N), device=dev)
    y = linear(x, lin)
    (y * dy).sum().backward()
    got = [x.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone()]
    x.grad = lin.weight.grad = lin.bias.grad = None
    y2 = lin(x)
    (y2 * dy).sum().backward()
    _close(y, y2)
    for g, r in zip(got, [x.grad, lin.weight.grad, lin.bias.grad]):
        _close(g, r)


@pytest.mark.parametrize("K,M,N,bt", [(65536, 1024, 256, 2), (65536 + 777, 1024, 80, 2), (1000, 6, 128, 1),
                                      (17, 33, 5, 1)])
def test_mm_tn_matches_torch(K, M, N, bt):
    from voxnav.learn_ops import mm_tn
    dev = "cuda:0"
    torch.manual_seed(K + M)
    a = torch.randn((bt, K, M), device=dev)
    y = 0.9 * torch.tanh(torch.randn((bt, K, M), device=dev))
    b = torch.randn((bt, K, N), device=dev)
    out, cs = mm_tn(a, b, colsum=True)
    _close(out, a.transpose(1, 2) @ b)
    _close(cs, a.sum(1))
    z = a * (1 - y * y)
    out2, cs2 = mm_tn(a, b, y=y, colsum=True)
    _close(out2, z.transpose(1, 2) @ b)
    _close(cs2, z.sum(1))
    # a batch-shared B (stride 0) and a strided batch of A
    bs = b[:1].expand(bt, K, N)
    out3, _ = mm_tn(a, bs)
    _close(out3, a.transpose(1, 2) @ bs)


@pytest.mark.parametrize("D,H,L,B", [(80, 256, 8, 512), (31, 64, 5, 300), (67, 16, 3, 70)])
def test_dual_lstm_matches_torch(D, H, L, B):
    """The learner's LSTM re-run (voxnav/lstm_seq.py over the fused per-step
    kernels of csrc/voxnav_learn_f32.hip) against two torch nn.LSTMs: outputs
    and every parameter / initial-state gradient, including input widths that
    are not multiples of 4 (simpleEnv's 6L + 7 observation, zero-padded)."""
    from types import SimpleNamespace
    from voxnav.lstm_seq import dual_lstm
    dev = "cuda:0"
    torch.manual_seed(D * H + L)
    la, lc = torch.nn.LSTM(D, H).to(dev), torch.nn.LSTM(D, H).to(dev)
    pol = SimpleNamespace(lstm_actor=la, lstm_critic=lc)
    x = torch.randn((L, B, D), device=dev)
    h0 = torch.randn((2, B, H), device=dev, requires_grad=True)
    c0 = torch.randn((2, B, H), device=dev, requires_grad=True)
    dy = torch.randn((2, L, B, H), device=dev)
    oa, oc = dual_lstm(pol, x, h0, c0)
    ((oa * dy[0]).sum() + (oc * dy[1]).sum()).backward()
    params = list(la.parameters()) + list(lc.parameters())
    got = [p.grad.clone() for p in params] + [h0.grad.clone(), c0.grad.clone()]
    for p in params + [h0, c0]:
        p.grad = None
    ra, _ = la(x, (h0[0:1], c0[0:1]))
    rc, _ = lc(x, (h0[1:2], c0[1:2]))
    ((ra * dy[0]).sum() + (rc * dy[1]).sum()).backward()
    _close(oa, ra)
    _close(oc, rc)
    ref = [p.grad for p in params] + [h0.grad, c0.grad]
    for g, r in zip(got, ref):
        _close(g, r, rel=1e-4)


def _rows_reference(x, env, start, keep, hs, cs, lstm, l):
    """float64 restatement of one LSTM over the row layout: at a sequence start
    the state is the buffer's stored state x keep, else the row's previous."""
    L, B, _ = x.shape
    w_ih, w_hh = lstm.weight_ih_l0.double(), lstm.weight_hh_l0.double()
    b = (lstm.bias_ih_l0 + lstm.bias_hh_l0).double()
    h = torch.zeros((B, w_hh.shape[1]), dtype=torch.float64, device=x.device)
    c = torch.zeros_like(h)
    outs = []
    for t in range(L):
        st = start[t].bool().view(B, 1)
        k = keep[t].double().view(B, 1)
        h = torch.where(st, hs[t, l, env[t].long()].double() * k, h)
        c = torch.where(st, cs[t, l, env[t].long()].double() * k, c)
        gi, gf, gg, go = (x[t].double() @ w_ih.T + h @ w_hh.T + b).chunk(4, dim=1)
        c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        h = torch.sigmoid(go) * torch.tanh(c)
        outs.append(h)
    return torch.stack(outs)


@pytest.mark.parametrize("layout", ["auto", "units16", "units32"])
@pytest.mark.parametrize("L,B,N,p_start", [(24, 512, 600, 0.03), (9, 37, 40, 0.2), (128, 64, 64, 0.01),
                                           (128, 512, 512, 0.004), (1, 1, 4, 0.5), (2, 33, 8, 0.5),
                                           (5, 289, 300, 1.0)])
def test_dual_lstm_rows_matches_float64(L, B, N, p_start, layout):
    """The persistent row-layout LSTM (csrc/voxnav_learn_rows.hip: weights
    resident, in-launch h / partial-dh hand-offs between the unit blocks of a
    row tile) against a float64 restatement: outputs and the weight / bias
    gradients of both LSTMs, with sequence starts (stored states x keep) at t = 0,
    at random steps and mid-row; full 512-row tiles, a ragged last tile, a
    whole 128-step rollout, and the learner bench's own shape (512 rows x 128
    steps: every block of the launch resident, 128 hand-offs per direction);
    edge shapes: one step of one row, two steps of a 33-row batch (one full
    tile and a 1-row tile), and a batch where every row starts a sequence at
    every step (no state crosses a step: only the stored states).
    Both forward layouts, forced: 16 unit blocks of 16 units (option
    rows_layout 2; two blocks per CU at 512 rows) and 8 of 32 (rows_layout 1),
    and the default pick by grid size; the backward has one layout (16 units)
    and runs behind each."""
    from voxnav import _native
    with _native.option("rows_layout", {"auto": 0, "units32": 1, "units16": 2}[layout]):
        _dual_lstm_rows_vs_float64(L, B, N, p_start)


def _dual_lstm_rows_vs_float64(L, B, N, p_start):
    from types import SimpleNamespace
    from voxnav import lstm_seq
    dev = "cuda:0"
    D, H = 80, 256
    torch.manual_seed(L * B + N)
    la, lc = torch.nn.LSTM(D, H).to(dev), torch.nn.LSTM(D, H).to(dev)
    pol = SimpleNamespace(lstm_actor=la, lstm_critic=lc)
    if not lstm_seq.rows_supported(pol, D, B):
        pytest.skip("row-layout kernels not co-resident on this device")
    x = torch.randn((L, B, D), device=dev)
    env = torch.randint(0, N, (L, B), device=dev, dtype=torch.int32)
    start = (torch.rand((L, B), device=dev) < p_start).to(torch.uint8)
    start[0] = 1
    keep = (torch.rand((L, B), device=dev) > 0.3).float()
    hs = 0.5 * torch.randn((L, 2, N, H), device=dev)
    cs = 0.5 * torch.randn((L, 2, N, H), device=dev)
    dy = torch.randn((2, L, B, H), device=dev)
    oa, oc = lstm_seq.dual_lstm_rows(pol, x, env, start, keep, hs, cs)
    ((oa * dy[0]).sum() + (oc * dy[1]).sum()).backward()
    params = list(la.parameters()) + list(lc.parameters())
    got = [p.grad.clone() for p in params]
    lstm_seq.rows_check(torch.device(dev))
    for p in params:
        p.grad = None
    ra = _rows_reference(x, env, start, keep, hs, cs, la, 0)
    rc = _rows_reference(x, env, start, keep, hs, cs, lc, 1)
    ((ra * dy[0].double()).sum() + (rc * dy[1].double()).sum()).backward()
    _close(oa, ra.float())
    _close(oc, rc.float())
    for g, p in zip(got, params):
        _close(g, p.grad, rel=1e-4)


@pytest.mark.parametrize("layout", ["auto", "units16", "units32"])
@pytest.mark.parametrize("L,B,N,p_start", [(9, 37, 40, 0.2), (2, 33, 8, 0.5)])
def test_dual_lstm_rows_input_gradient_matches_float64(L, B, N, p_start, layout):
    """The row-layout backward (one layout, behind each forward layout) with an
    input that needs a gradient (dG is only allocated and written then): x.grad
    and the eight parameter gradients against float64 autograd, and the
    parameter gradients bit-identical to a run whose x needs none (the
    learner's own case)."""
    from types import SimpleNamespace
    from voxnav import _native, lstm_seq
    dev = "cuda:0"
    D, H = 80, 256
    torch.manual_seed(L * B + N + 1)
    la, lc = torch.nn.LSTM(D, H).to(dev), torch.nn.LSTM(D, H).to(dev)
    pol = SimpleNamespace(lstm_actor=la, lstm_critic=lc)
    if not lstm_seq.rows_supported(pol, D, B):
        pytest.skip("row-layout kernels not co-resident on this device")
    x = torch.randn((L, B, D), device=dev)
    env = torch.randint(0, N, (L, B), device=dev, dtype=torch.int32)
    start = (torch.rand((L, B), device=dev) < p_start).to(torch.uint8)
    start[0] = 1
    keep = (torch.rand((L, B), device=dev) > 0.3).float()
    hs = 0.5 * torch.randn((L, 2, N, H), device=dev)
    cs = 0.5 * torch.randn((L, 2, N, H), device=dev)
    dy = torch.randn((2, L, B, H), device=dev)
    params = list(la.parameters()) + list(lc.parameters())
    runs = []
    with _native.option("rows_layout", {"auto": 0, "units32": 1, "units16": 2}[layout]):
        for need_dx in (True, False):
            xin = x.clone().requires_grad_(need_dx)
            oa, oc = lstm_seq.dual_lstm_rows(pol, xin, env, start, keep, hs, cs)
            ((oa * dy[0]).sum() + (oc * dy[1]).sum()).backward()
            runs.append(([p.grad.clone() for p in params], xin.grad))
            lstm_seq.rows_check(torch.device(dev))
            for p in params:
                p.grad = None
    (got, dx), (got_no_dx, none) = runs
    assert none is None and dx.shape == x.shape
    for a, b in zip(got, got_no_dx):
        assert torch.equal(a, b)
    x64 = x.double().requires_grad_()
    ra = _rows_reference(x64, env, start, keep, hs, cs, la, 0)
    rc = _rows_reference(x64, env, start, keep, hs, cs, lc, 1)
    ((ra * dy[0].double()).sum() + (rc * dy[1].double()).sum()).backward()
    _close(dx, x64.grad, rel=1e-4)
    for g, p in zip(got, params):
        _close(g, p.grad, rel=1e-4)


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_rows_supported_up_to_the_co_residency_bound(layout):
    """Every block of a row-layout launch must be resident at once: 16 blocks
    per 32-row tile at one per CU (the 32-unit forward) or 32 at two per CU
    (the 16-unit kernels), so under every rows_layout the kernels take
    B = 32 * (ncu // 16) rows and refuse one row more.  Launches nothing."""
    from types import SimpleNamespace
    from voxnav import _native, lstm_seq
    D, H = 80, 256
    pol = SimpleNamespace(lstm_actor=torch.nn.LSTM(D, H), lstm_critic=torch.nn.LSTM(D, H))
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 32 * (ncu // 16)
    with _native.option("rows_layout", layout):
        assert lstm_seq.rows_supported(pol, D, B)
        assert not lstm_seq.rows_supported(pol, D, B + 1)


@pytest.mark.parametrize("M,F,A,gather,norm", [(65536, 128, 6, True, True), (77, 64, 3, False, True),
                                               (4099, 256, 8, True, False), (1, 128, 6, False, False)])
def test_ppo_loss_matches_float64(M, F, A, gather, norm):
    """The fused loss kernel (heads, advantage normalisation, clipped
    surrogate, value MSE, entropy; gradient to the latents and the head
    weights) against the same block in float64 autograd.  Old log-probs are
    spread so the ratio falls on both sides of the clip range and inside it
    (the min's tie, where torch splits the gradient)."""
    from voxnav.learn_ops import ppo_loss
    dev = "cuda:0"
    torch.manual_seed(M + F + A)
    an, vn = torch.nn.Linear(F, A).to(dev), torch.nn.Linear(F, 1).to(dev)
    h = torch.tanh(torch.randn((2, M, F), device=dev))
    R = M + 1000 if gather else M
    src = torch.randperm(R, device=dev)[:M].contiguous() if gather else None
    act = torch.randint(0, A, (R,), device=dev, dtype=torch.int32)
    adv = torch.randn(R, device=dev) * 3 + 0.5
    ret = torch.randn(R, device=dev)
    with torch.no_grad():
        lp_true = torch.log_softmax(h[0] @ an.weight.T + an.bias, -1)
    sel = src if gather else torch.arange(M, device=dev)
    olp = torch.randn(R, device=dev) - 1.5
    olp[sel] = lp_true.gather(1, act[sel].long().view(-1, 1)).flatten() + 0.3 * torch.randn(M, device=dev)
    clip, ent, vf = 0.2, 0.01, 0.5
    dh, grads, stats = ppo_loss(h, an, vn, src, act, adv, olp, ret, clip, ent, vf, norm)
    g = lambda t: t if src is None else t[src]  # noqa: E731
    rdh, rgrads, rstats = _ppo_loss_reference(h, an.weight, an.bias, vn.weight, vn.bias, g(act), g(adv), g(olp),
                                              g(ret), clip, ent, vf, norm)
    if M == 1 and norm:
        return
    _close(dh.double(), rdh, rel=2e-5, floor=1e-9)
    for a, b in zip(grads, rgrads):
        assert a.shape == b.shape
        _close(a.double(), b, rel=1e-4, floor=1e-9)
    _close(stats, rstats, rel=1e-5, floor=1e-7)


def test_grad_norm_scale_matches_clip_grad_norm():
    """The two-launch gradient norm (and the Adam grad_scale divisor) against
    torch.nn.utils.clip_grad_norm_ over tensors of ragged sizes and offsets;
    and the fused Adam step with that divisor against clip + step."""
    from voxnav.learn_ops import grad_norm_scale
    dev = "cuda:0"
    torch.manual_seed(3)
    shapes = [(1024, 256), (1024, 80), (1024,), (6, 128), (6,), (1, 128), (1,), (333, 7)]
    ps = [torch.nn.Parameter(torch.randn(s, device=dev)) for s in shapes]
    for p in ps:
        p.grad = torch.randn_like(p) * 0.05
    ref_ps = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    for r, p in zip(ref_ps, ps):
        r.grad = p.grad.clone()
    for max_norm in (0.5, 1e3):
        norm, scale = grad_norm_scale(ps, max_norm)
        ref = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad.double()) for p in ps])).float()
        _close(norm, ref, rel=1e-6)
        assert abs(scale.item() - max(1.0, (ref.item() + 1e-6) / max_norm)) <= 1e-6 * scale.item()
    opt = torch.optim.Adam(ps, lr=3e-4, eps=1e-5, fused=True)
    ref_opt = torch.optim.Adam(ref_ps, lr=3e-4, eps=1e-5, fused=True)
    norm, scale = grad_norm_scale(ps, 0.5)
    opt.grad_scale = scale
    opt.step()
    torch.nn.utils.clip_grad_norm_(ref_ps, 0.5)
    ref_opt.step()
    for p, r in zip(ps, ref_ps):
        _close(p.detach(), r.detach(), rel=1e-6, floor=1e-7)



def test_adam_step_matches_torch_fused_adam():
    """The library's Adam step (clip divisor applied on the way) against
    torch's fused Adam with the same grad_scale, over three steps from a
    fresh state, including a tensor whose size is not a multiple of 4; the
    optimizer state (step, moments) is torch's own."""
    from voxnav.learn_ops import adam_step, grad_norm_scale
    dev = "cuda:0"
    torch.manual_seed(5)
    shapes = [(1024, 336), (6, 128), (6,), (333, 7), (1,)]
    ps = [torch.nn.Parameter(torch.randn(s, device=dev)) for s in shapes]
    rs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = torch.optim.Adam(ps, lr=3e-4, eps=1e-5, fused=True)
    ref = torch.optim.Adam(rs, lr=3e-4, eps=1e-5, fused=True)
    for it in range(3):
        for p, r in zip(ps, rs):
            g = torch.randn_like(p) * 0.3
            p.grad, r.grad = g.clone(), g.clone()
        _, scale = grad_norm_scale(ps, 0.5)
        adam_step(opt, scale)
        ref.grad_scale = scale.clone()
        ref.step()
        ref.grad_scale = None
        for p, r in zip(ps, rs):
            _close(p.detach(), r.detach(), rel=1e-6, floor=1e-7)
            for k in ("exp_avg", "exp_avg_sq"):
                _close(opt.state[p][k], ref.state[r][k], rel=1e-5, floor=1e-12)
            assert float(opt.state[p]["step"]) == float(ref.state[r]["step"]) == it + 1


def test_minibatch_rows_matches_index_arithmetic():
    """The one-launch minibatch gather against the torch index arithmetic it
    replaces (env-major ids -> [T, N]-major rows), ragged M."""
    from voxnav.learn_ops import minibatch_rows
    dev = "cuda:0"
    T, N, D = 128, 1000, 80
    obs = torch.randn((T, N, D), device=dev)
    idx = torch.randperm(T * N, device=dev)[:4099].contiguous()
    src, rows = minibatch_rows(idx, T, N, obs)
    env = idx // T
    ref = (idx - env * T) * N + env
    assert torch.equal(src, ref)
    assert torch.equal(rows, obs.reshape(T * N, D)[ref])


# vn_adam_step takes its hyperparameters as f32 (include/voxnav.h), so the
# kernel's Adam is the one with the f32-rounded betas: 1 - beta2 is then
# 1 - f32(0.999) = 0.99998713e-3, 1.29e-5 (relative) below torch's 1 - 0.999,
# and with it every second moment -- more than the 1e-5 these tests allow,
# and not a rounding error of the kernel.  The torch optimizers compared
# against below are therefore built with the betas the kernel receives.
# (test_adam_step_matches_torch_fused_adam keeps torch's defaults: at its
# gradient scale the difference lies below its floor.)
F32_BETAS = tuple(float(torch.tensor(b, dtype=torch.float32)) for b in (0.9, 0.999))


def _adam_pair(shapes, dev, **kw):
    ps = [torch.nn.Parameter(torch.randn(s, device=dev)) for s in shapes]
    rs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    kw = dict(lr=3e-4, eps=1e-5, betas=F32_BETAS, **kw)
    return ps, rs, torch.optim.Adam(ps, **kw), torch.optim.Adam(rs, **kw)


def _adam_same(opt, ref, ps, rs, step):
    for p, r in zip(ps, rs):
        _close(p.detach(), r.detach(), rel=1e-6, floor=1e-7)
        for k in ("exp_avg", "exp_avg_sq"):
            _close(opt.state[p][k], ref.state[r][k], rel=1e-5, floor=1e-12)
        assert float(opt.state[p]["step"]) == float(ref.state[r]["step"]) == step


@pytest.mark.parametrize("pattern", [(1, 0, 0), (0, 1, 0, 1, 1, 0), (1, 1, 0)],
                         ids=lambda p: "".join("SA"[1 - s] for s in p))
def test_adam_step_skip_gate(pattern):
    """``adam_step(skip=word)``: with a nonzero word the parameters, both
    moments and ``state["step"]`` keep their bits; the applied steps before
    and after equal a torch fused Adam that took only those (bias corrections
    and ``step`` of the applied count, not of the attempts)."""
    from voxnav.learn_ops import adam_step, grad_norm_scale
    dev = "cuda:0"
    torch.manual_seed(7)
    ps, rs, opt, ref = _adam_pair([(129, 33), (6, 128), (6,), (333, 7), (1,)], dev, fused=True)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    applied = 0
    for skipped in pattern:
        for p, r in zip(ps, rs):
            g = torch.randn_like(p) * 0.3
            p.grad, r.grad = g.clone(), g.clone()
        _, scale = grad_norm_scale(ps, 0.5)
        word.fill_(3 if skipped else 0)
        before = [(p.detach().clone(), {k: v.clone() for k, v in opt.state[p].items()}) for p in ps]
        adam_step(opt, scale, skip=word)
        if skipped:
            for p, (p0, st0) in zip(ps, before):
                assert torch.equal(p.detach().view(torch.int32), p0.view(torch.int32))
                st = opt.state[p]
                assert float(st["step"]) == applied
                assert not st["exp_avg"].any() if not st0 else torch.equal(st["exp_avg"], st0["exp_avg"])
                assert not st["exp_avg_sq"].any() if not st0 else torch.equal(st["exp_avg_sq"], st0["exp_avg_sq"])
            continue
        applied += 1
        ref.grad_scale = scale.clone()
        ref.step()
        ref.grad_scale = None
        _adam_same(opt, ref, ps, rs, applied)
    assert applied == pattern.count(0)


def test_adam_step_gated_never_skipped_keeps_the_ungated_bits():
    """A gated step whose word stays 0 and an ungated step give the same bits
    (parameters, moments, step) over three steps."""
    from voxnav.learn_ops import adam_step
    dev = "cuda:0"
    torch.manual_seed(8)
    ps, rs, opt, ref = _adam_pair([(129, 33), (6,), (1,)], dev, fused=True)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    for it in range(3):
        for p, r in zip(ps, rs):
            g = torch.randn_like(p) * 0.3
            p.grad, r.grad = g.clone(), g.clone()
        adam_step(opt, None, skip=word)
        adam_step(ref, None)
        for p, r in zip(ps, rs):
            assert torch.equal(p.detach(), r.detach())
            for k in ("exp_avg", "exp_avg_sq", "step"):
                assert torch.equal(opt.state[p][k], ref.state[r][k])
            assert float(opt.state[p]["step"]) == it + 1


def test_adam_step_unaligned_tensors_take_the_scalar_path():
    """A parameter, a gradient and a moment that are views one float into
    their storage (not 16-B aligned: the kernel's scalar path), sizes that are
    no multiple of 4, against torch's fused Adam on aligned copies."""
    from voxnav.learn_ops import adam_step, grad_norm_scale
    dev = "cuda:0"
    torch.manual_seed(11)
    n = [1027, 515, 259, 1024]
    off1 = lambda t: torch.cat([t.new_zeros(1), t.flatten()])[1:]  # noqa: E731
    ps = [torch.nn.Parameter(off1(torch.randn(n[0], device=dev)))] + \
         [torch.nn.Parameter(torch.randn(k, device=dev)) for k in n[1:]]
    rs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = torch.optim.Adam(ps, lr=3e-4, eps=1e-5, betas=F32_BETAS, fused=True)
    ref = torch.optim.Adam(rs, lr=3e-4, eps=1e-5, betas=F32_BETAS, fused=True)
    opt.state[ps[2]] = {"step": torch.zeros((), dtype=torch.float32, device=dev),
                        "exp_avg": off1(torch.zeros(n[2], device=dev)),
                        "exp_avg_sq": torch.zeros(n[2], device=dev)}
    assert ps[0].data_ptr() % 16 == 4 and opt.state[ps[2]]["exp_avg"].data_ptr() % 16 == 4
    for it in range(2):
        for i, (p, r) in enumerate(zip(ps, rs)):
            g = torch.randn_like(r) * 0.3
            p.grad, r.grad = (off1(g) if i == 1 else g.clone()), g.clone()
        assert ps[1].grad.data_ptr() % 16 == 4 and ps[3].grad.data_ptr() % 16 == 0
        norm, scale = grad_norm_scale(ps, 0.5)
        _close(norm, torch.linalg.vector_norm(torch.cat([r.grad.double().flatten() for r in rs])).float(), rel=1e-6)
        adam_step(opt, scale)
        ref.grad_scale = scale.clone()
        ref.step()
        ref.grad_scale = None
        _adam_same(opt, ref, ps, rs, it + 1)


def test_adam_step_after_load_state_dict_with_cpu_step():
    """A state whose ``step`` is a CPU tensor (torch's default Adam, through a
    state_dict round trip): the next step continues the loaded count -- set on
    the host when ungated, moved to the device by a gated step."""
    import copy
    from voxnav.learn_ops import adam_step
    dev = "cuda:0"
    torch.manual_seed(12)
    ps, rs, first, ref = _adam_pair([(129, 33), (6,), (1,)], dev)

    def grads():
        for p, r in zip(ps, rs):
            g = torch.randn_like(p) * 0.3
            p.grad, r.grad = g.clone(), g.clone()

    grads()
    first.step()
    ref.step()
    opt = torch.optim.Adam(ps, lr=1.0)
    opt.load_state_dict(copy.deepcopy(first.state_dict()))
    assert all(opt.state[p]["step"].device.type == "cpu" for p in ps) and opt.param_groups[0]["lr"] == 3e-4
    grads()
    adam_step(opt)
    ref.step()
    assert all(opt.state[p]["step"].device.type == "cpu" for p in ps)
    _adam_same(opt, ref, ps, rs, 2)
    grads()
    adam_step(opt, skip=torch.zeros(1, dtype=torch.int32, device=dev))
    ref.step()
    assert all(opt.state[p]["step"].is_cuda for p in ps)
    _adam_same(opt, ref, ps, rs, 3)


def test_grad_norm_scale_edges():
    """All-zero gradients (norm 0, divisor 1), exactly 64 tensors, 65 refused,
    a zero-sized tensor in the list."""
    from voxnav import _native
    from voxnav.learn_ops import grad_norm_scale
    dev = "cuda:0"
    torch.manual_seed(13)

    def params(sizes, zero=False):
        ps = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in sizes]
        for p in ps:
            p.grad = torch.zeros_like(p) if zero else torch.randn_like(p) * 0.05
        return ps

    def ref_norm(ps):
        return torch.linalg.vector_norm(torch.cat([p.grad.double().flatten() for p in ps])).float()

    norm, scale = grad_norm_scale(params([(33, 7), (5,), (1,)], zero=True), 0.5)
    assert float(norm) == 0.0 and float(scale) == 1.0
    ps = params([(i % 7 + 1, i % 5 + 1) for i in range(64)])
    for max_norm in (0.05, 1e3):
        norm, scale = grad_norm_scale(ps, max_norm)
        _close(norm, ref_norm(ps), rel=1e-6)
        assert abs(scale.item() - max(1.0, (ref_norm(ps).item() + 1e-6) / max_norm)) <= 1e-6 * scale.item()
    with pytest.raises(_native.VoxnavError):
        grad_norm_scale(ps + params([(3,)]), 0.5)
    ps = params([(33, 7), (0,), (5,), (0, 4), (1,)])
    norm, scale = grad_norm_scale(ps, 0.05)
    _close(norm, ref_norm(ps), rel=1e-6)
    assert abs(scale.item() - max(1.0, (ref_norm(ps).item() + 1e-6) / 0.05)) <= 1e-6 * scale.item()
    norm, scale = grad_norm_scale(params([(0,)]), 0.5)
    assert float(norm) == 0.0 and float(scale) == 1.0


def test_mm_tn_refuses_a_y_of_other_shape_or_strides():
    """``mm_tn`` reads ``y`` with ``a``'s row and batch strides: any other
    layout is a ValueError before anything is launched."""
    from voxnav.learn_ops import mm_tn
    dev = "cuda:0"
    torch.manual_seed(14)
    bt, K, M, N = 2, 40, 12, 8
    a, b = torch.randn((bt, K, M), device=dev), torch.randn((bt, K, N), device=dev)
    y = 0.9 * torch.tanh(torch.randn((bt, K, M), device=dev))
    out = torch.full((bt, M, N), -7.0, device=dev)
    bad = [y[:, :K - 1], y[0], y[:1].expand(bt, K, M), torch.zeros((bt, K, M + 4), device=dev)[:, :, :M],
           y.transpose(1, 2).contiguous().transpose(1, 2), torch.zeros((bt, 2 * K, M), device=dev)[:, ::2],
           y.double(), y.cpu()]
    for yy in bad:
        with pytest.raises(ValueError):
            mm_tn(a, b, y=yy, colsum=True, out=out)
    torch.cuda.synchronize()
    assert float(out.min()) == -7.0 == float(out.max())
    got, _ = mm_tn(a, b, y=y, out=out)
    z = a.double() * (1 - y.double() ** 2)
    _close(got.double(), z.transpose(1, 2) @ b.double())
