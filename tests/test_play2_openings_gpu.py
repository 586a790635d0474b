"""k_play2's stage openings: every stage loads its episode counter, tags and
hand-off (and a play stage the first turn pair's hashes) in one batch, without
guards, from a clamped board index, and compares the tags afterwards.  Board
counts that exercise the clamp (a lone lane, a full block plus one lane, two
blocks plus two), hand-offs that are stale when they are loaded, and the guard
of the hashes loaded ahead; every game bit-exact against the C oracle."""
import numpy as np
import pytest
import torch

import oracle
from hzamd.state import unpack_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


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


def check_episode(env, base, ep, steps):
    """Every board: final state, ply count, and (cursor and stream together)
    the next stream word, against the oracle's episode."""
    finals, plies, nxt = rule_games(env.n, base, ep)
    assert (states_of(env) == finals).all(), ep
    assert (steps.cpu().numpy() == plies).all(), ep
    _, mt, idx = env.export_state(with_mt=True)
    mt, idx = mt.cpu().numpy().view(np.uint32), idx.cpu().numpy()
    for b in range(env.n):
        assert oracle.mt_next32(oracle.mt_from_words(mt[b], idx[b])) == nxt[b], (ep, b)
    return finals, plies, nxt


@pytest.mark.parametrize("n", [1, 65, 130])
def test_parity_at_sizes_that_exercise_the_clamp(Env, n):
    """Sixteen calls (the last three replay fully prepared episodes), an
    hz_reset + hz_rollout, sixteen more: lanes past n read board n - 1's
    hand-offs in every stage's opening and must discard them."""
    base = 4242
    env = Env(n, seed_base=base, device=DEV)
    env.set_pipeline(2)
    for ep in range(16):
        _, steps, _ = env.rollout(200, reset=True)
        check_episode(env, base, ep, steps)
    env.reset()
    _, steps, _ = env.rollout(200)
    check_episode(env, base, 16, steps)
    for ep in range(17, 33):
        _, steps, _ = env.rollout(200, reset=True)
        check_episode(env, base, ep, steps)
    env.check_errors()
    env.close()


def test_speculative_loads_are_discarded_when_stale(Env):
    """130 boards, pipeline 2 and 1 alternated (each one's hand-offs, scripts
    and hashes go stale while the other runs, and are loaded all the same by
    the next opening), then an auto-reset call that moves the episode counters
    board by board, then one more call."""
    n, base = 130, 99
    env = Env(n, seed_base=base, device=DEV)
    ep = 0
    for pipe, calls in ((2, 15), (1, 2), (2, 15)):
        env.set_pipeline(pipe)
        for _ in range(calls):
            _, steps, _ = env.rollout(200, reset=True)
            check_episode(env, base, ep, steps)
            ep += 1
    games, _, _ = env.rollout(64, auto_reset=True, reset=True)  # episode ep, then maybe ep + 1
    resets = games.cpu().numpy() - env.done().cpu().numpy().astype(np.int64)
    nxt_ep = ep + 1 + resets
    _, steps, _ = env.rollout(200, reset=True)
    st = states_of(env)
    steps = steps.cpu().numpy()
    for e in sorted(set(nxt_ep.tolist())):
        finals, plies, _ = rule_games(n, base, int(e))
        sel = nxt_ep == e
        assert (st[sel] == finals[sel]).all(), e
        assert (steps[sel] == plies[sel]).all(), e
    env.check_errors()
    env.close()


def _run16(Env, n, base):
    env = Env(n, seed_base=base, device=DEV)
    env.set_pipeline(2)
    out = []
    for ep in range(16):
        _, steps, _ = env.rollout(200, reset=True)
        check_episode(env, base, ep, steps)
        _, mt, idx = env.export_state(with_mt=True)
        mt, idx = mt.cpu().numpy().view(np.uint32), idx.cpu().numpy()
        words = []
        for b in range(n):
            m = oracle.mt_from_words(mt[b], idx[b])
            words.append([oracle.mt_next32(m) for _ in range(32)])
        out.append((states_of(env), steps.cpu().numpy().copy(), np.array(words, dtype=np.uint64)))
    env.check_errors()
    env.close()
    return out


@pytest.fixture(scope="module")
def default_cuts_run(Env):
    return _run16(Env, 130, 1618)


@pytest.mark.parametrize("cuts", ["16,32,48,72", "16,32,48,76", "24,48,96,1048576"])
def test_first_hash_pair_guard(Env, monkeypatch, default_cuts_run, cuts):
    """The pair of hash rows a play stage loads with its opening starts at the
    cut before it: at the last row that fits the table (72 + 8 = 80), past it
    (76 + 8 > 80: not loaded ahead), and far past it (two cuts beyond the
    table, the largest the setting accepts).  Results equal the oracle's and
    the default cuts': states, ply counts and each board's next 32 stream
    words."""
    monkeypatch.setenv("HZ_P2_CUTS5", cuts)
    got = _run16(Env, 130, 1618)
    for ep, (a, b) in enumerate(zip(got, default_cuts_run)):
        for x, y in zip(a, b):
            assert (x == y).all(), ep
