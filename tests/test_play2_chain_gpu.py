"""hz_play's pipeline 2 (k_play2) after its stage loops were stripped to their
chains: P1's table words in two alternating scalar register sets from the
padded table, pass 2's stores from addresses made once per stage, the twist
part in four operations, the draw stages' windows staged with 16-byte LDS
stores at their own row stride, and D1's window loaded before its tags return.
Every game, ply count and stream word bit-exact against the C oracle and
pipeline 1."""
import numpy as np
import pytest
import torch

import oracle
from hzamd.state import unpack_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# two generations and more: every seeded row (the table's last rows 617-623
# among them), the twisted rows 0-223 and the rows on both sides of every
# stage boundary (P2a / P2b / P2c, the twist's rows from HBM and from LDS)
# reach a compared word
WORDS = 1400


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
    """States, plies and the next stream word of every board against the oracle."""
    finals, plies, nxt = rule_games(env.n, base, ep)
    assert (states_of(env) == finals).all(), ep
    assert (steps.cpu().numpy() == plies).all(), ep
    mt, idx = streams_of(env)
    for b in range(env.n):
        assert oracle.mt_next32(oracle.mt_from_words(mt[b], idx[b])) == nxt[b], (ep, b)


@pytest.mark.parametrize("n", [1, 65, 130])
def test_whole_stream_equals_pipeline_1(Env, n):
    """A lone lane, a second wave with one board, three waves: seventeen calls
    on pipeline 2 and on pipeline 1 from one seed base; after each of the last
    three every board's next 1400 words are the same in both, and the games
    are the oracle's."""
    base = 27182
    e2, e1 = Env(n, seed_base=base, device=DEV), Env(n, seed_base=base, device=DEV)
    e2.set_pipeline(2)
    e1.set_pipeline(1)
    for ep in range(17):
        _, s2, _ = e2.rollout(200, reset=True)
        _, s1, _ = e1.rollout(200, reset=True)
        if ep < 14:
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


@pytest.mark.parametrize("dcuts", ["1,3,10,17", "7,14,21,23"])
def test_windows_at_their_extremes(Env, monkeypatch, dcuts):
    """The draw cuts (HZ_P2_DCUTS) early and late, read when the env is
    created: the late setting starts windows near row 224 and makes draws
    overrun them (discarded and redone by the next stage or the play stages);
    sixteen calls against the oracle, for scripts of 24, 19, 3 and 0 draws."""
    monkeypatch.setenv("HZ_P2_DCUTS", dcuts)
    n, base = 130, 5772
    for draws in (24, 19, 3, 0):
        env = Env(n, seed_base=base, device=DEV)
        env.set_pipeline(2)
        env.set_seed_ahead(draws > 0, draws)
        for ep in range(16):
            _, steps, _ = env.rollout(200, reset=True)
            check_episode(env, base, ep, steps)
        env.check_errors()
        env.close()


@pytest.mark.parametrize("k", list(range(1, 15)))
def test_stale_hand_off_at_every_stage(Env, k):
    """k calls, an hz_reset + hz_rollout (every hand-off then holds an episode
    the stages no longer expect, the fourteen stages k calls into their
    filling), then fifteen more calls."""
    n, base = 65, 1414
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
