"""k_play2's static draw windows with six draw stages: the replay of
tests/test_p2_windows_cpu.py (whose simulation is imported, and which keeps
mirroring the five-stage build) for the six-stage default cuts and for every
cut set the round-22 scan considered.  A cut set is benchmarked only if it
passes here: over 1,000,000 simulated streams no board starts a stage below
its window's first row and no stage's last draw ends past its window.

DCUT6 mirrors harmonies-alphazero_amd/csrc/hz_play2.hpp (HZ_P2_DCUT for
HZ_P2_NDRAW == 6); change them together."""
import numpy as np
import pytest

from test_p2_windows_cpu import K_AHEAD_DRAWS, K_P2_TWIST, K_P2_WIN, STREAMS, cursors_after_draws

DCUT6 = (0, 5, 9, 13, 17, 20)   # HZ_P2_DCUT, HZ_P2_NDRAW == 6
# the first draws of D1..D6 of every set the scan ran (profiles/r22/bench_ab.json, "parts")
SCANNED = [
    DCUT6,
    (0, 5, 9, 13, 16, 20),
    (0, 5, 9, 13, 17, 21),
    (0, 4, 9, 13, 17, 20),
    (0, 5, 10, 13, 17, 20),
    (0, 5, 9, 12, 16, 20),
    (0, 5, 10, 14, 17, 20),
    (0, 6, 10, 14, 17, 21),
    (0, 6, 11, 15, 19, 24),     # the five-stage cuts, D6 empty
]
K_P2_STAGE_DRAWS = 7            # kP2StageDraws


@pytest.fixture(scope="module")
def cur():
    c = cursors_after_draws(STREAMS, 20240614)
    c.setflags(write=False)
    return c


def test_draws_consume_three_words_or_more(cur):
    assert cur.shape == (K_AHEAD_DRAWS + 1, 1_000_000)
    assert (np.diff(cur, axis=0) >= 3).all()  # what a window's first row rests on


@pytest.mark.parametrize("dcut", SCANNED, ids=lambda c: ",".join(map(str, c)))
def test_static_windows_hold_every_stage(cur, dcut):
    assert len(dcut) == 6 and dcut[0] == 0
    cuts = tuple(dcut) + (K_AHEAD_DRAWS,)
    assert all(0 <= b - a <= K_P2_STAGE_DRAWS for a, b in zip(cuts[:-1], cuts[1:]))
    for k in range(6):
        d0, d1 = cuts[k], cuts[k + 1]
        if d0 == d1:
            continue  # an empty stage stages a window and reads nothing of it
        lo = (3 * d0) & ~3
        end = min(lo + K_P2_WIN, K_P2_TWIST)
        start_min, last_max = int(cur[d0].min()), int(cur[d1].max())
        print(f"D{k + 1}: draws [{d0}, {d1}) window rows [{lo}, {end}); lowest start cursor {start_min} "
              f"(margin {start_min - lo}), highest cursor after the last draw {last_max} (margin {end - last_max})")
        assert start_min >= lo, k
        assert last_max <= end, k
