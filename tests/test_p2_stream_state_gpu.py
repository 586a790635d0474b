"""The stream a board is left with by hz_play's pipeline 2 (k_play2), word for
word.  A pipeline-2 stream slot holds only the rows the pipeline itself reads,
so a board's own stream is rebuilt from its episode seed and cursor when
another entry point needs it (k_mt_materialize2), and a game that would read
past the slot's rows is played again from scratch by the last play stage
(HZ_P2_FELL_LIMIT).  Here: all 624 words and the index against the C oracle
after chosen calls, the streams continued by per-ply steps, pipelines 1 and 2
alternated, and the replay path forced."""
import numpy as np
import pytest
import torch

import oracle
from hzamd.state import pack_ref, unpack_ref, words_to_array

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, BASE, PLIES = 100, 60221, 96  # one full block of 64 boards and a tail of 36
CALLS = 16                       # past the pipeline's depth of fourteen
CHECK = (1, 14, 16)              # calls after which the whole state is compared (and after the last)
K_P2_TWIST = 160                 # kP2Twist (hz_play2.hpp): the cursor's tw of a board played from a slot
SHORT_SCRIPT = 12                # scripted draws in the forced runs: every game then leaves its script
FELL_LIMIT = 88                  # slot rows in the forced run; games read ~87 words on average (tools/p2_fell_count.py)


@pytest.fixture(scope="module")
def Env():
    from hzamd.env import BatchedEnv
    return BatchedEnv


_games = {}


def oracle_game(seed):
    """(final state [78], plies, stream words [624], index) of the rule game
    seeded `seed`, computed once and shared."""
    if seed not in _games:
        m = oracle.mt_seed(seed)
        final, steps, stuck = oracle.play_rule_from(oracle.reset(m), m, seed, 0, PLIES)
        words, idx = m.words()
        assert not stuck
        for a in (final, words):
            a.setflags(write=False)
        _games[seed] = (final, steps, words, idx)
    return _games[seed]


def _device_view(ptr, n, typestr):
    class Raw:
        __cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(Raw(), device=DEV)


def seeds_of(env):
    import hzamd._native as nat
    torch.cuda.synchronize()
    return _device_view(nat.lib().hz_env_seed_ptr(env.handle), env.n, "<i8").cpu().numpy().astype(np.uint64)


def cursor_tw(env):
    import hzamd._native as nat
    torch.cuda.synchronize()
    pos = _device_view(nat.lib().hz_env_mt_pos_ptr(env.handle), env.n, "<i4").cpu().numpy()
    return pos >> 16


def exported(env):
    st, mt, idx = (t.cpu().numpy() for t in env.export_state(with_mt=True))
    return np.stack([unpack_ref(st[:, b]) for b in range(env.n)]), mt.view(np.uint32), idx


def check_against_oracle(env, ep, steps):
    seeds = seeds_of(env)
    assert (seeds == np.uint64(BASE) + np.arange(N, dtype=np.uint64) + (np.uint64(ep) << np.uint64(32))).all(), ep
    got_st, got_mt, got_idx = exported(env)
    got_steps = steps.cpu().numpy()
    for b in range(N):
        final, plies, words, idx = oracle_game(int(seeds[b]))
        assert (got_st[b] == final).all(), (ep, b)
        assert got_steps[b] == plies, (ep, b)
        assert got_idx[b] == idx, (ep, b)
        assert (got_mt[b] == words).all(), (ep, b, int(np.flatnonzero(got_mt[b] != words)[0]))
    return got_st, got_mt, got_idx


def play_calls(env, ep, calls, alternate, check=CHECK, probe=None):
    """`calls` hz_play calls from episode `ep`; the whole state compared after
    the calls in `check` and after the last (`probe`: called after the last
    call, before the export finishes the streams' twist).  Returns the
    episode reached and the last call's export."""
    out = None
    for c in range(1, calls + 1):
        if alternate:
            env.set_pipeline(1 if c % 2 else 2)
        games, steps, _ = env.rollout(PLIES, reset=True)
        if probe and c == calls:
            probe(env)
        if c in check or c == calls:
            out = check_against_oracle(env, ep, steps)
            assert int(games.sum()) == N
        ep += 1
    return ep, out


def continue_per_ply(env):
    """Fresh games put on the boards (states from unrelated streams; the
    boards keep their own streams), eight rule plies through hz_legal_mask,
    hz_rule_actions and hz_step, the oracle replaying the same actions on the
    streams its own games left: states and streams stay equal."""
    seeds = seeds_of(env)
    refs, streams = [], []
    for b in range(N):
        refs.append(oracle.reset(oracle.mt_seed(900000 + b)))
        _, _, words, idx = oracle_game(int(seeds[b]))
        streams.append(oracle.mt_from_words(words, idx))
    words = env.export_state().cpu().numpy().copy()
    for b in range(N):
        words[:, b] = words_to_array([pack_ref(refs[b])])[0]
    env.import_state(torch.from_numpy(words))
    for _ in range(8):  # two whole turns: two pile draws per board
        mask, count = env.legal_mask()
        action = env.rule_actions(mask, count)
        status = env.step(action)
        assert (status == 0).all()
        act = action.cpu().numpy()
        for b in range(N):
            r, refs[b] = oracle.step(refs[b], int(act[b]), streams[b])
            assert r == 0
    got_st, got_mt, got_idx = exported(env)
    for b in range(N):
        words_b, idx_b = streams[b].words()
        assert (got_st[b] == refs[b]).all(), b
        assert got_idx[b] == idx_b and (got_mt[b] == words_b).all(), b
    assert (got_idx != np.array([oracle_game(int(s))[3] for s in seeds])).all()  # every stream was drawn from


@pytest.mark.parametrize("alternate", [False, True], ids=["pipeline2", "alternated"])
def test_whole_stream_state_after_calls(Env, alternate):
    """Sixteen calls, hz_reset, sixteen more: after calls 1, 14, 16 and the
    last, every board's 624 stream words and index are the oracle's; then the
    streams continue exactly under per-ply steps."""
    env = Env(N, seed_base=BASE, device=DEV)
    env.set_pipeline(2)
    ep, _ = play_calls(env, 0, CALLS, alternate)
    env.reset()  # (starts episode `ep` on every board; the pipeline's hand-offs go stale)
    ep, _ = play_calls(env, ep + 1, CALLS, alternate)
    env.check_errors()
    continue_per_ply(env)
    env.close()


def test_forced_replay_equals_default(Env, monkeypatch):
    """Scripts of twelve draws (every game goes on drawing from its slot) and
    HZ_P2_FELL_LIMIT low enough that about half the games would read past it:
    those boards are replayed from scratch by the last play stage, and final
    states, ply counts, episode seeds and whole streams equal the oracle's and
    the default run's."""
    runs = {}
    for name, limit in (("default", None), ("forced", FELL_LIMIT)):
        if limit is None:
            monkeypatch.delenv("HZ_P2_FELL_LIMIT", raising=False)
        else:
            monkeypatch.setenv("HZ_P2_FELL_LIMIT", str(limit))  # (read when the env is created)
        env = Env(N, seed_base=BASE, device=DEV)
        env.set_pipeline(2)
        env.set_seed_ahead(True, SHORT_SCRIPT)
        tw = []
        ep, out = play_calls(env, 0, CALLS, False, probe=lambda e: tw.append(cursor_tw(e)))
        env.reset()
        ep, out2 = play_calls(env, ep + 1, CALLS, False)
        env.check_errors()
        runs[name] = (out, out2, tw[0], seeds_of(env))
        env.close()
    for a, b in zip(runs["default"][:2], runs["forced"][:2]):
        for x, y in zip(a, b):
            assert (x == y).all()
    assert (runs["default"][3] == runs["forced"][3]).all()
    # which boards of call 16 (episode 15: every stage prepared) read past the
    # limit, by the oracle's index; a board played from its slot keeps the
    # slot's tw, a replayed one has twisted on demand in LDS, well short of it
    seeds = np.uint64(BASE) + np.arange(N, dtype=np.uint64) + (np.uint64(CALLS - 1) << np.uint64(32))
    used = np.array([oracle_game(int(s))[3] for s in seeds])
    trip = used > FELL_LIMIT
    print(f"words used: max {used.max()}, boards past row {FELL_LIMIT}: {int(trip.sum())} of {N}")
    assert trip.any() and not trip.all() and used.max() + 32 < K_P2_TWIST
    assert (runs["default"][2] == K_P2_TWIST).all()
    assert ((runs["forced"][2] != K_P2_TWIST) == trip).all()
