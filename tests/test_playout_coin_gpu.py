"""hz_playout_coin (include/hz_abi.h; hzamd.selfplay.NoiseSource.coin): the
per-board, per-move uniform that playout-cap randomization tosses, from the
root noise's counter-based generator under its own salt."""
import numpy as np
import pytest
import torch

import hzamd._native as nat
from hzamd.selfplay import NoiseSource

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED_BASE = 1234


def test_coin_law_and_batch_independence():
    """64 boards x 64 moves: every coin lies in (0, 1]; the share below 0.25
    is within 5 binomial sigma of 0.25 (sqrt(0.25 * 0.75 / 4096) = 0.0068:
    +-0.034); a board's coin is a function of (seed, global board id, move)
    alone: one call over 64 boards equals two calls over 32 with board_base
    moved, and a call with another seed differs."""
    src = NoiseSource(SEED_BASE, DEV)
    lo, hi = NoiseSource(SEED_BASE, DEV), NoiseSource(SEED_BASE + 32, DEV)
    coins = torch.stack([src.coin(m, 64) for m in range(64)])
    halves = torch.stack([torch.cat([lo.coin(m, 32), hi.coin(m, 32)]) for m in range(64)])
    assert coins.dtype == torch.float64 and coins.shape == (64, 64) and coins.device.type == "cuda"
    assert torch.equal(coins, halves)
    c = coins.cpu().numpy()
    assert (c > 0).all() and (c <= 1).all()
    assert abs((c < 0.25).mean() - 0.25) <= 0.034, (c < 0.25).mean()
    assert len(np.unique(c)) == c.size          # 53-bit draws: no two of 4,096 alike
    other = NoiseSource(SEED_BASE, DEV, seed=1)
    assert (other.coin(0, 64).cpu().numpy() != c[0]).all()
    assert torch.equal(src.coin(5, 64), coins[5])   # stateless: the same key, the same coin


def test_coin_is_not_the_move_choice_uniform_and_leaves_the_noise_alone():
    """The coin has a salt of its own: it is not hz_root_noise's u of the same
    key, and drawing coins between two draw() calls changes neither the noise
    nor u (the generator keeps no state)."""
    src = NoiseSource(SEED_BASE, DEV)
    count = torch.full((64,), 7, dtype=torch.int32, device=DEV)
    noise, u = src.draw(3, count, 0.4)
    coin = src.coin(3, 64)
    assert (u != coin).all() and (u + 2.0 ** -53 != coin).all()   # (u is its draw minus 2^-53)
    noise2, u2 = src.draw(3, count, 0.4)
    assert torch.equal(noise, noise2) and torch.equal(u, u2)


def test_coin_arguments():
    L = nat.lib()
    out = torch.full((4,), -1.0, dtype=torch.float64, device=DEV)
    s = nat.stream_ptr(torch.device(DEV))
    assert L.hz_playout_coin(-1, 0, 0, 0, nat.ptr(out), s) == -1
    assert L.hz_playout_coin(4, 0, 0, 0, None, s) == -1
    assert L.hz_playout_coin(0, 0, 0, 0, nat.ptr(out), s) == 0
    assert L.hz_playout_coin(3, 0, 0, 0, nat.ptr(out), s) == 0      # a short call writes n entries only
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:3] > 0).all() and (got[:3] <= 1).all() and got[3] == -1.0
