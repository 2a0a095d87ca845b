"""Properties of ``learn_ops._splits``, the split count ``mm_tn`` asks
``vn_gemm_f32_tn`` for and sizes its workspaces by -- no GPU needed.  Over
every K < 600, a sampled grid of K up to 70,000 (the powers of two, the
multiples of SPLIT_ROWS and of 32 and their neighbours, pseudo-random fills)
and tile counts 1 .. 4096."""
import random

import pytest

from gemm_helpers import splits_recomputed, tn_plan

TILES = (1, 2, 8, 64, 512, 4096)


def _k_grid():
    ks = set(range(1, 600))
    for p in range(9, 17):
        ks.update((2 ** p - 1, 2 ** p, 2 ** p + 1))
    for m in range(2, 274):
        ks.update((256 * m - 1, 256 * m, 256 * m + 1, 256 * m + 31, 256 * m + 33))
    rng = random.Random(7)
    ks.update(rng.randrange(600, 70001) for _ in range(2000))
    ks.update((65536 + 333, 65536 + 777, 69999, 70000))
    return sorted(k for k in ks if 1 <= k <= 70000)


K_GRID = _k_grid()


@pytest.mark.parametrize("tiles", TILES)
def test_splits_bounds_and_workspace(tiles):
    from voxnav.learn_ops import SPLIT_ROWS, _splits
    assert SPLIT_ROWS == 256
    for K in K_GRID:
        sp = _splits(K, tiles)
        assert isinstance(sp, int), (K, tiles)
        assert sp >= 1, (K, tiles, sp)
        assert sp <= 256, (K, tiles, sp)
        assert sp <= max(1, K // 256), (K, tiles, sp)
        assert sp < 8 or sp % 8 == 0, (K, tiles, sp)
        # the entry point rounds K per split up to 32 and recomputes the count:
        # never more than mm_tn sized its workspaces for
        eff = splits_recomputed(K, sp)
        assert 1 <= eff <= sp, (K, tiles, sp, eff)
        assert tn_plan(K, sp)[1] == eff


def test_splits_fill_the_chip_when_k_allows():
    """With K long enough the count reaches the wanted ~512 blocks / tiles
    (rounded down to a multiple of 8), capped at 256."""
    from voxnav.learn_ops import _splits
    assert _splits(70000, 1) == 256
    assert _splits(70000, 2) == 256
    assert _splits(70000, 8) == 64
    assert _splits(70000, 64) == 8
    assert _splits(70000, 512) == 1
    assert _splits(70000, 4096) == 1
    assert _splits(255, 1) == 1 and _splits(256, 1) == 1 and _splits(512, 1) == 2 and _splits(2047, 1) == 7
    assert _splits(2048, 1) == 8 and _splits(15 * 256, 1) == 8 and _splits(16 * 256, 1) == 16
