"""hz_play's pipeline 2 (k_play2) with seeding pass 1 kept in registers and
five draw and five play stages: the whole stream a board is left with, every
pipeline phase going stale once, and the stage cuts at their extremes.  Every
game, ply count and stream word bit-exact against the C oracle and pipeline 1."""
import numpy as np
import pytest
import torch

import oracle
from hzamd.state import unpack_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORDS = 700  # crosses a generation boundary: the twisted rows 0-223 and the untwisted rows 224-623


@pytest.fixture(scope="module")
def Env():
    from hzamd.env import BatchedEnv
    return BatchedEnv


_games = {}


def rule_games(n, base, ep):
    """The oracle's episode, computed once per (n, base, episode) and shared."""
    key = (n, base, ep)
    if key not in _games:
        _, finals, plies, nxt = oracle.play_rule_games(n, base, nthreads=8, episode=ep)
        for a in (finals, plies, nxt):
            a.setflags(write=False)
        _games[key] = (finals, plies, nxt)
    return _games[key]


def states_of(env):
    st = env.export_state().cpu().numpy()
    return np.stack([unpack_ref(st[:, b]) for b in range(env.n)])


def streams_of(env):
    _, mt, idx = env.export_state(with_mt=True)
    return mt.cpu().numpy().view(np.uint32), idx.cpu().numpy()


def draw_words(mt, idx, b, count):
    m = oracle.mt_from_words(mt[b], idx[b])
    return [oracle.mt_next32(m) for _ in range(count)]


def check_episode(env, base, ep, steps):
    """test_env_gpu's _check_episode on every board: states, plies, next word."""
    finals, plies, nxt = rule_games(env.n, base, ep)
    assert (states_of(env) == finals).all(), ep
    assert (steps.cpu().numpy() == plies).all(), ep
    mt, idx = streams_of(env)
    for b in range(env.n):
        assert oracle.mt_next32(oracle.mt_from_words(mt[b], idx[b])) == nxt[b], (ep, b)


@pytest.mark.parametrize("n", [1, 65, 130])
def test_whole_stream_equals_pipeline_1(Env, n):
    """Sixteen calls on pipeline 2 and on pipeline 1 from one seed base; after
    each of the last three (fully prepared episodes: every stream word came
    through P1's hand-off, the three pass-2 stages' recomputed pass-1 words
    and the twist) every board's next 700 words are the same in both, and the
    games are the oracle's."""
    base = 31337
    e2, e1 = Env(n, seed_base=base, device=DEV), Env(n, seed_base=base, device=DEV)
    e2.set_pipeline(2)
    e1.set_pipeline(1)
    for ep in range(16):
        _, s2, _ = e2.rollout(200, reset=True)
        _, s1, _ = e1.rollout(200, reset=True)
        if ep < 13:
            continue
        finals, plies, _ = rule_games(n, base, ep)
        assert (states_of(e2) == finals).all() and (states_of(e1) == finals).all(), ep
        assert (s2.cpu().numpy() == plies).all() and (s1.cpu().numpy() == plies).all(), ep
        (mt2, i2), (mt1, i1) = streams_of(e2), streams_of(e1)
        for b in range(n):
            assert draw_words(mt2, i2, b, WORDS) == draw_words(mt1, i1, b, WORDS), (ep, b)
    e2.check_errors()
    e1.check_errors()
    e2.close()
    e1.close()


@pytest.mark.parametrize("k", list(range(1, 15)))
def test_every_phase_goes_stale_once(Env, k):
    """k calls, an hz_reset + hz_rollout (the pipeline re-primes: every
    hand-off then holds an episode the stages no longer expect, with the
    fourteen stages k calls into their filling), then fifteen more calls."""
    n, base = 65, 2718
    env = Env(n, seed_base=base, device=DEV)
    env.set_pipeline(2)
    ep = 0
    for _ in range(k):
        _, steps, _ = env.rollout(200, reset=True)
        check_episode(env, base, ep, steps)
        ep += 1
    env.reset()
    _, steps, _ = env.rollout(200)
    check_episode(env, base, ep, steps)
    ep += 1
    for _ in range(15):
        _, steps, _ = env.rollout(200, reset=True)
        check_episode(env, base, ep, steps)
        ep += 1
    env.check_errors()
    env.close()


@pytest.mark.parametrize("cuts,dcuts", [("4,8,12,16", "1,3,10,17"), ("60,64,68,72", "7,14,21,23")])
def test_cuts_at_their_extremes(Env, monkeypatch, cuts, dcuts):
    """The play cuts (HZ_P2_CUTS5) and the draw cuts (HZ_P2_DCUTS) at their
    smallest and at a late valid setting (a draw stage takes at most seven
    draws: the earliest and the latest cuts that allows), read when the env
    is created: sixteen calls against the oracle, for scripts of 24, 19, 3
    and 0 draws."""
    monkeypatch.setenv("HZ_P2_CUTS5", cuts)
    monkeypatch.setenv("HZ_P2_DCUTS", dcuts)
    n, base = 130, 1618
    for draws in (24, 19, 3, 0):
        env = Env(n, seed_base=base, device=DEV)
        env.set_pipeline(2)
        env.set_seed_ahead(draws > 0, draws)
        for ep in range(16):
            _, steps, _ = env.rollout(200, reset=True)
            check_episode(env, base, ep, steps)
        env.check_errors()
        env.close()
