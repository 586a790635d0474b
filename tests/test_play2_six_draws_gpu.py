"""hz_play's pipeline 2 (k_play2) with fifteen stages: the rule hashes are
computed by the seeding stages (each a fixed range of the 80 rows, stored
before the stage's tag, into a ring entry that travels with the stream slot)
and the wave they ran on is a sixth draw stage.  Nineteen calls, four more
than the pipeline's depth, so that five fully prepared episodes are replayed;
every hand-off stale once at the new depth; the draw cuts with four and with
five values at their extremes; the forced-replay path; pipelines alternated.
Every game, ply count and stream word bit-exact against the C oracle and
pipeline 1."""
import numpy as np
import pytest
import torch

import oracle
from hzamd.state import unpack_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DEPTH = 15          # kP2Stages (hz_env.hip) with six draw stages
CALLS = DEPTH + 4
WORDS = 700         # past a generation: every seeded row and the twisted rows reach a compared word


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
    """Every board: final state, ply count and (cursor and stream together)
    the next stream word, against the oracle's episode."""
    finals, plies, nxt = rule_games(env.n, base, ep)
    assert (states_of(env) == finals).all(), ep
    assert (steps.cpu().numpy() == plies).all(), ep
    mt, idx = streams_of(env)
    for b in range(env.n):
        assert oracle.mt_next32(oracle.mt_from_words(mt[b], idx[b])) == nxt[b], (ep, b)
    return mt, idx


@pytest.mark.parametrize("n", [1, 65, 130])
def test_whole_pipeline(Env, n):
    """A lone board, a full block plus one lane, two blocks plus two: nineteen
    calls, an hz_reset + hz_rollout, nineteen more, each against the oracle;
    for n = 65 a pipeline-1 env runs beside it and after each of the last
    three calls every board's next 700 words are the same in both."""
    base = 60221
    env = Env(n, seed_base=base, device=DEV)
    env.set_pipeline(2)
    twin = None
    if n == 65:
        twin = Env(n, seed_base=base, device=DEV)
        twin.set_pipeline(1)
    ep = 0

    def calls(count, compare_from):
        nonlocal ep
        for c in range(count):
            _, steps, _ = env.rollout(200, reset=True)
            mt, idx = check_episode(env, base, ep, steps)
            if twin is not None:
                twin.rollout(200, reset=True)
                if c >= compare_from:
                    mt1, i1 = streams_of(twin)
                    for b in range(n):
                        assert draw_words(mt, idx, b, WORDS) == draw_words(mt1, i1, b, WORDS), (ep, b)
            ep += 1

    calls(CALLS, CALLS - 3)
    env.reset()
    _, steps, _ = env.rollout(200)
    check_episode(env, base, ep, steps)
    if twin is not None:
        twin.reset()
        twin.rollout(200)
    ep += 1
    calls(CALLS, CALLS - 3)
    env.check_errors()
    env.close()
    if twin is not None:
        twin.check_errors()
        twin.close()


@pytest.mark.parametrize("k", list(range(1, DEPTH + 1)))
def test_every_phase_goes_stale_once(Env, k):
    """k calls, an hz_reset + hz_rollout (every hand-off, the hash rows among
    them, then holds an episode the stages no longer expect, the fifteen
    stages k calls into their filling), then sixteen more calls."""
    n, base = 65, 16022
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
    for _ in range(DEPTH + 1):
        _, steps, _ = env.rollout(200, reset=True)
        check_episode(env, base, ep, steps)
        ep += 1
    env.check_errors()
    env.close()


def _run19(Env, n, base):
    env = Env(n, seed_base=base, device=DEV)
    env.set_pipeline(2)
    out = []
    for ep in range(CALLS):
        _, steps, _ = env.rollout(200, reset=True)
        mt, idx = check_episode(env, base, ep, steps)
        words = np.array([draw_words(mt, idx, b, 32) for b in range(n)], dtype=np.uint64)
        out.append((states_of(env), steps.cpu().numpy().copy(), words))
    env.check_errors()
    env.close()
    return out


@pytest.fixture(scope="module")
def default_cuts_run(Env):
    return _run19(Env, 130, 29979)


@pytest.mark.parametrize("dcuts", [
    "7,14,21,23",      # four values: D6's first draw is the default's, raised to D5's: D5 empty
    "1,3,10,17,24",    # five values: D6 draws nothing
    "3,6,10,14,17",    # five values: D6 makes seven draws, the most a stage may
    "1,2,3,4,17",      # D6 seven again, but D5 thirteen: the gap rule rejects the set and the defaults apply
    "1,2,3,4,16",      # D6 would make eight: rejected too
])
def test_draw_cuts_at_their_extremes(Env, monkeypatch, default_cuts_run, dcuts):
    """HZ_P2_DCUTS, read when the env is created: nineteen calls against the
    oracle, and states, ply counts and each board's next 32 stream words equal
    the default cuts'."""
    monkeypatch.setenv("HZ_P2_DCUTS", dcuts)
    got = _run19(Env, 130, 29979)
    for ep, (a, b) in enumerate(zip(got, default_cuts_run)):
        for x, y in zip(a, b):
            assert (x == y).all(), ep


def test_forced_replay(Env, monkeypatch):
    """Scripts of twelve draws (every game goes on drawing from its slot) and
    HZ_P2_FELL_LIMIT=88, below what about half the games read: those boards
    are replayed from scratch by the last play stage.  Six draw stages;
    nineteen calls; states, plies and whole streams (624 words and the index)
    equal the oracle's on every board after the last five calls, and some but
    not all boards of the last call were replayed."""
    import hzamd._native as nat
    monkeypatch.setenv("HZ_P2_FELL_LIMIT", "88")
    n, base, plies_max = 130, 1729, 200
    env = Env(n, seed_base=base, device=DEV)
    env.set_pipeline(2)
    env.set_seed_ahead(True, 12)
    for ep in range(CALLS):
        _, steps, _ = env.rollout(plies_max, reset=True)
        if ep < CALLS - 5:
            continue
        torch.cuda.synchronize()

        class Raw:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "version": 2,
                                        "data": (int(nat.lib().hz_env_mt_pos_ptr(env.handle)), False)}
        tw = torch.as_tensor(Raw(), device=DEV).cpu().numpy() >> 16  # (before the export finishes the twist)
        st, (mt, idx), got_steps = states_of(env), streams_of(env), steps.cpu().numpy()
        used = np.zeros(n, np.int64)
        for b in range(n):
            seed = base + b + (ep << 32)
            m = oracle.mt_seed(seed)
            final, plies, stuck = oracle.play_rule_from(oracle.reset(m), m, seed, 0, plies_max)
            words, i = m.words()
            assert not stuck
            assert (st[b] == final).all() and got_steps[b] == plies, (ep, b)
            assert idx[b] == i and (mt[b] == words).all(), (ep, b)
            used[b] = i
        trip = used > 88
        # a board played from its slot keeps the slot's tw (kP2Twist = 160), a replayed one twisted on demand in LDS
        assert ((tw != 160) == trip).all(), ep
    assert trip.any() and not trip.all()
    env.check_errors()
    env.close()


def test_pipelines_alternated(Env):
    """200 boards: pipeline 2 and 1 alternated in runs (each one's hand-offs,
    scripts and hash rows go stale while the other runs and are loaded all
    the same by the next opening), then an auto-reset call that moves the
    episode counters board by board, then calls on pipeline 2 again."""
    n, base = 200, 8128
    env = Env(n, seed_base=base, device=DEV)
    ep = 0
    for pipe, calls in ((2, CALLS), (1, 2), (2, 3), (1, 1), (2, DEPTH + 1)):
        env.set_pipeline(pipe)
        for _ in range(calls):
            _, steps, _ = env.rollout(200, reset=True)
            check_episode(env, base, ep, steps)
            ep += 1
    games, _, _ = env.rollout(64, auto_reset=True, reset=True)  # episode ep, then maybe ep + 1
    resets = games.cpu().numpy() - env.done().cpu().numpy().astype(np.int64)
    nxt_ep = ep + 1 + resets
    for _ in range(2):
        _, steps, _ = env.rollout(200, reset=True)
        st, got = states_of(env), steps.cpu().numpy()
        for e in sorted(set(nxt_ep.tolist())):
            finals, plies, _ = rule_games(n, base, int(e))
            sel = nxt_ep == e
            assert (st[sel] == finals[sel]).all(), e
            assert (got[sel] == plies[sel]).all(), e
        nxt_ep = nxt_ep + 1
    env.check_errors()
    env.close()
