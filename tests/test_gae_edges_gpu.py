"""``compute_gae`` (vn_gae: one lane per env, a reverse scan over T) against
the f32 oracle ``oracle.oracle.gae``, bit for bit, at the edges the collector
tests do not reach: one step, one env, env counts on either side of the
256-lane block, discount constants other than the defaults (1.0 and a zero
lambda), and every pattern of episode starts and final dones."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 257), (2, 256), (128, 255)]
CONSTANTS = [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)]
STARTS = ["all", "first", "random"]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("starts", STARTS)
@pytest.mark.parametrize("gamma,lam", CONSTANTS)
@pytest.mark.parametrize("T,N", SHAPES)
def test_gae_edges_match_oracle(T, N, gamma, lam, starts):
    from oracle.oracle import gae as oracle_gae
    from voxnav.gae import compute_gae
    rng = np.random.default_rng(1000 * T + N)
    r = rng.normal(size=(T, N)).astype(np.float32)
    v = rng.normal(size=(T, N)).astype(np.float32)
    lv = rng.normal(size=N).astype(np.float32)
    if starts == "all":
        s = np.ones((T, N), np.float32)
    elif starts == "first":
        s = np.zeros((T, N), np.float32)
        s[0] = 1
    else:
        s = (rng.random((T, N)) < 0.3).astype(np.float32)
    for done in (0.0, 1.0):
        dn = np.full(N, done, np.float32)
        adv, ret = compute_gae(*(torch.as_tensor(a, device="cuda:0") for a in (r, v, s, lv, dn)), gamma=gamma,
                               gae_lambda=lam)
        ea, er = oracle_gae(r, v, s, lv, dn, gamma=gamma, gae_lambda=lam)
        assert adv.shape == ret.shape == (T, N)
        np.testing.assert_array_equal(adv.cpu().numpy(), ea, err_msg=f"advantages, dones all {done}")
        np.testing.assert_array_equal(ret.cpu().numpy(), er, err_msg=f"returns, dones all {done}")
