"""k_rollout's four variants against each other across a game boundary.

The recording auto-reset variant (auto_reset=True, record=True) is pinned
here: against the plain auto-reset variant (same states, counters, streams),
against the non-auto-reset recording of each episode (the same rows; that
variant is pinned to the reference by test_rollout_records_traces), and
against itself under call splitting.  130 boards are two full waves and a
ragged block of two; rule games end by ply 80, so with a 96-ply budget every
board ends its first game and starts its second inside the run."""
import numpy as np
import pytest
import torch

import oracle
from hzamd.state import unpack_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, BASE, PLIES = 130, 9091, 96
ONE = (PLIES,)
SPLITS = {"one": ONE, "eights": (8,) * 12, "sevens": (7,) * 13 + (5,)}  # 7s: calls end inside turn pairs
assert all(sum(s) == PLIES for s in SPLITS.values())


@pytest.fixture(scope="module")
def Env():
    from hzamd.env import BatchedEnv
    return BatchedEnv


_cache = {}


def frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def episode_plies():
    """The oracle's ply count of every board's episodes 0, 1, 2: [3, N]."""
    if "plies" not in _cache:
        L = np.stack([oracle.play_rule_games(N, BASE, nthreads=8, episode=e)[2] for e in range(3)])
        assert (L[0] < PLIES).all() and (L.sum(0) >= PLIES).all()  # every board crosses a boundary; three episodes cover the budget
        _cache["plies"] = frozen([L])[0]
    return _cache["plies"]


def auto_run(Env, record, ahead=None, via_play=False, split=ONE):
    """PLIES auto-reset plies from episode 0's reset, in calls of `split`
    plies: (state, stream words, stream indices, games, steps) summed over
    the calls, and the calls' recordings concatenated (or None).  Computed
    once per setting and shared."""
    key = ("auto", record, ahead, via_play, split)
    if key in _cache:
        return _cache[key]
    env = Env(N, seed_base=BASE, device=DEV)
    if ahead is not None:
        env.set_auto_ahead(ahead)
    if not via_play:
        env.reset()
    games = np.zeros(N, np.int64)
    steps = np.zeros(N, np.int64)
    recs = []
    for c, k in enumerate(split):
        g, s, tr = env.rollout(k, auto_reset=True, record=record, reset=via_play and c == 0)
        games += g.cpu().numpy()
        steps += s.cpu().numpy()
        if record:
            recs.append([t.cpu().numpy() for t in tr])
    st, mt, idx = (t.cpu().numpy() for t in env.export_state(with_mt=True))
    env.check_errors()
    env.close()
    rec = frozen([np.concatenate(x) for x in zip(*recs)]) if record else None
    _cache[key] = (frozen([st, mt, idx, games, steps]), rec)
    return _cache[key]


def episode_recording(Env, ep):
    """The non-auto-reset recording of episode `ep` alone."""
    key = ("episode", ep)
    if key not in _cache:
        env = Env(N, seed_base=BASE, device=DEV)
        for _ in range(ep + 1):
            env.reset()
        _, steps, tr = env.rollout(PLIES, record=True)
        assert (steps.cpu().numpy() == episode_plies()[ep]).all()
        _cache[key] = frozen([t.cpu().numpy() for t in tr])
        env.close()
    return _cache[key]


def assert_same(a, b):
    for x, y in zip(a, b):
        assert x.shape == y.shape and (x == y).all()


@pytest.mark.parametrize("via_play", [False, True], ids=["hz_rollout", "hz_play"])
@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "in_place"])
def test_recording_auto_reset_equals_plain(Env, via_play, ahead):
    """Final states, games_done, steps_done and every stream word and cursor
    of a recording auto-reset run equal the plain run's, with episodes
    prepared ahead and seeded in place, through hz_rollout after reset() and
    through hz_play; the counters are what the oracle's ply counts give, the
    states what its auto-reset restatement gives."""
    rec, _ = auto_run(Env, True, via_play=via_play)
    plain, _ = auto_run(Env, False, ahead=ahead, via_play=via_play)
    assert_same(rec, plain)
    ends = np.cumsum(episode_plies(), axis=0)
    st, _, _, games, steps = rec
    assert (games == (ends <= PLIES).sum(0)).all()
    assert (steps == np.minimum(ends[-1], PLIES)).all()
    total, finals, ref_games, _ = oracle.play_rule_auto(N, BASE, PLIES, ep0=0, nthreads=8)
    assert (np.stack([unpack_ref(st[:, b]) for b in range(N)]) == finals).all()
    assert (games == ref_games).all() and int(steps.sum()) == total


@pytest.mark.parametrize("via_play", [False, True], ids=["hz_rollout", "hz_play"])
def test_recorded_rows_are_the_episodes_rows(Env, via_play):
    """Rows [0, L0) of each board are the rows of episode 0 recorded alone,
    rows [L0, 96) the first rows of episode 1 recorded alone (and so on), and
    every recorded action is legal in the mask of its row."""
    _, (ts, tm, ta) = auto_run(Env, True, via_play=via_play)
    assert ts.shape == (PLIES, 6, N) and tm.shape == (PLIES, N, 3) and ta.shape == (PLIES, N)
    L = episode_plies()
    for b in range(N):
        row, ep = 0, 0
        while row < PLIES:
            k = min(int(L[ep, b]), PLIES - row)
            es, em, ea = episode_recording(Env, ep)
            assert (ts[row:row + k, :, b] == es[:k, :, b]).all(), (b, ep)
            assert (tm[row:row + k, b] == em[:k, b]).all(), (b, ep)
            assert (ta[row:row + k, b] == ea[:k, b]).all(), (b, ep)
            row, ep = row + k, ep + 1
    a = ta.astype(np.int64)
    assert (a >= 0).all()  # 96 plies played: every row holds a move
    word = np.take_along_axis(tm.view(np.uint64), (a >> 6)[..., None], axis=2)[..., 0]
    assert (((word >> (a & 63).astype(np.uint64)) & np.uint64(1)) == 1).all()


@pytest.mark.parametrize("record", [False, True], ids=["plain", "record"])
@pytest.mark.parametrize("split", ["eights", "sevens"])
def test_call_splitting_does_not_matter(Env, record, split):
    """96 auto-reset plies as one call, as 12 calls of 8 and as 13 of 7 plus
    one of 5 (calls that end inside a turn pair): the same final states,
    streams, cursors, summed counters and concatenated recordings."""
    one, one_rec = auto_run(Env, record)
    cut, cut_rec = auto_run(Env, record, split=SPLITS[split])
    assert_same(one, cut)
    if record:
        assert_same(one_rec, cut_rec)
