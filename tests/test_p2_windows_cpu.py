"""k_play2's static draw windows against the stream words that pile draws
consume.  A draw stage k stages slot rows [L_k, L_k + 96), L_k = (3 dcut[k]) &
~3, before it knows its boards' cursors; this replays, with numpy, how many
words the 24 scripted draws of a game consume and checks that every board
starts every stage at or past L_k and ends the stage's last draw inside the
window.  (A draw that did not would be discarded and redone by a later stage:
time, never results.  So this pins the windows' cost, not their exactness.)

Draw d of a game is random.sample(range(n), 3) with n = 120 - 3 d tiles in the
bag, n > 21: the set method.  Each pick takes the top k = n.bit_length() bits
of a 32-bit word, rejects a value >= n (_randbelow) and a value already picked
in this draw, and takes the next word.

The constants below mirror harmonies-alphazero_amd/csrc/hz_play2.hpp (kP2Win,
HZ_P2_DCUT for five draw stages, HZ_P2_TWIST) and hz_chance.hpp (kAheadDraws);
change them together."""
import numpy as np

K_AHEAD_DRAWS = 24          # kAheadDraws
K_P2_TWIST = 160            # kP2Twist: next-generation rows a slot holds
K_P2_WIN = 96               # kP2Win
DCUT = (0, 6, 11, 15, 19)   # HZ_P2_DCUT, HZ_P2_NDRAW == 5
BAG = 120                   # tiles in a full bag (23 + 21 + 19 + 23 + 19 + 15)
STREAMS = 1_000_000


def cursors_after_draws(streams, seed):
    """[K_AHEAD_DRAWS + 1, streams] words consumed before draw 0 and after each draw."""
    rng = np.random.default_rng(seed)
    cur = np.zeros((K_AHEAD_DRAWS + 1, streams), np.int32)
    pos = np.zeros(streams, np.int32)
    for d in range(K_AHEAD_DRAWS):
        n = BAG - 3 * d
        bits = int(n).bit_length()
        picks = np.full((3, streams), -1, np.int32)
        got = np.zeros(streams, np.int32)
        todo = np.arange(streams)
        while todo.size:
            v = rng.integers(0, 1 << bits, size=todo.size, dtype=np.int32)
            pos[todo] += 1
            p = picks[:, todo]
            keep = (v < n) & (p[0] != v) & (p[1] != v)  # (unset picks are -1)
            t, g = todo[keep], got[todo[keep]]
            picks[g, t] = v[keep]
            got[t] = g + 1
            todo = todo[got[todo] < 3]
        cur[d + 1] = pos
    return cur


def test_static_windows_hold_every_stage():
    cur = cursors_after_draws(STREAMS, 20240614)
    cuts = DCUT + (K_AHEAD_DRAWS,)
    assert (np.diff(cur, axis=0) >= 3).all()  # what L_k rests on
    for k in range(len(DCUT)):
        d0, d1 = cuts[k], cuts[k + 1]
        lo = (3 * d0) & ~3
        end = min(lo + K_P2_WIN, K_P2_TWIST)
        start_min, last_max = int(cur[d0].min()), int(cur[d1].max())
        print(f"D{k + 1}: draws [{d0}, {d1}) window rows [{lo}, {end}); lowest start cursor {start_min} "
              f"(margin {start_min - lo}), highest cursor after the last draw {last_max} (margin {end - last_max})")
        assert start_min >= lo, k
        assert last_max <= end, k
    print(f"words after {K_AHEAD_DRAWS} draws: mean {cur[-1].mean():.1f}, max {int(cur[-1].max())} of {K_P2_TWIST}")
    assert int(cur[-1].max()) < K_P2_TWIST
