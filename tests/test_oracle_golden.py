"""Pins the CPU oracle (oracle/hz_oracle.c) against fixtures captured from the
reference itself (tests/golden/make_golden.py).  CPU only."""
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def test_mt_stream_matches_cpython():
    f = load("mt_streams.npz")
    for i, seed in enumerate(f["seeds"]):
        m = oracle.mt_seed(int(seed))
        got = np.array([oracle.mt_next32(m) for _ in range(1000)], np.uint32)
        assert (got == f["words"][i]).all(), f"seed {seed}"


def test_sample_matches_cpython():
    f = load("mt_streams.npz")
    for i, seed in enumerate(f["seeds"]):
        m = oracle.mt_seed(int(seed))
        for j, n in enumerate(f["sample_n"]):
            assert list(oracle.sample(m, int(n), 3)) == list(f["sample"][i, j])
        assert oracle.mt_next32(m) == f["next_word"][i]
        m = oracle.mt_seed(int(seed))
        for n in range(1, 22):
            k = min(3, n)
            assert list(oracle.sample(m, n, k)) == list(f["small_sample"][i, n - 1, :k])


def test_env_traces_bit_exact():
    f = load("env_traces.npz")
    states, masks, acts, off = f["states"], f["masks"], f["actions"], f["offsets"]
    for g, seed in enumerate(f["seeds"]):
        m = oracle.mt_seed(int(seed))
        st = oracle.reset(m)
        for p in range(off[g], off[g + 1]):
            assert (st == states[p]).all(), (seed, p - off[g])
            mask = oracle.legal(st)
            assert (np.packbits(mask, bitorder="little") == masks[p]).all()
            k = oracle.rule(int(seed), p - off[g])
            L = int(mask.sum())
            a = np.flatnonzero(mask)[((k >> 32) * L) >> 32]
            assert a == acts[p]
            r, st = oracle.step(st, int(a), m)
            assert r == 0
        assert (st == f["finals"][g]).all()
        assert oracle.is_game_over(st)
        assert oracle.mt_next32(m) == f["next_word"][g]


def test_env_finals_batch_driver():
    f = load("env_finals.npz")
    seeds = f["seeds"]
    assert (np.diff(seeds) == 1).all()
    total, finals, plies, nxt = oracle.play_rule_games(len(seeds), int(seeds[0]), nthreads=4)
    assert (finals == f["finals"]).all()
    assert (plies == f["plies"]).all()
    assert (nxt == f["next_word"]).all()
    assert total == int(f["plies"].sum())


def test_encoder_matches_reference():
    f = load("encoder.npz")
    for st, b, g in zip(f["states"], f["boards"], f["globs"]):
        ob, og = oracle.encode(st)
        assert (ob.view(np.uint32) == b.view(np.uint32)).all()
        assert (og.view(np.uint32) == g.view(np.uint32)).all()


def test_scoring_known_answers():
    f = load("scoring.npz")
    for b, s in zip(f["boards"], f["scores"]):
        assert list(oracle.score_board(b)) == list(s)
    assert list(f["scores"][0]) == [4, 4, 5, 5, 5]


def test_illegal_moves_report_status():
    m = oracle.mt_seed(0)
    st = oracle.reset(m)
    assert oracle.step(st, 7, m)[0] == 1          # placement index during choose_pile
    assert oracle.step(st, 5 + 0, m)[0] == 1
    r, st1 = oracle.step(st, 0, m)
    assert r == 0
    assert oracle.step(st1, 0, m)[0] == 2         # pile index during placement
    hand = set(int(t) for t in st1[62:62 + st1[65]])
    missing = [t for t in range(6) if t not in hand][0]
    assert oracle.step(st1, 5 + missing * 23, m)[0] == 3
    done = st1.copy()
    done[73] = 4
    assert oracle.step(done, 0, m)[0] == 5


@pytest.mark.parametrize("k", range(80))
def test_mcts_matches_reference(k):
    f = load("mcts.npz")
    m = oracle.mt_seed(int(f["mt_seed"][k]))
    a, visits, nn, ne = oracle.mcts_search(
        f["state"][k], m, int(f["sims"][k]), float(f["cpuct"][k]), eps=float(f["eps"][k]),
        testing=bool(f["testing"][k]), tau0=int(f["tau0"][k]), ply=int(f["ply"][k]),
        u=float(f["u"][k]), noise=f["noise"][k])
    assert (visits == f["visits"][k]).all()
    assert a == f["action"][k]
    assert (nn, ne) == (f["n_nodes"][k], f["n_edges"][k])
    assert oracle.mt_next32(m) == f["next_word"][k]


def dense_row(f, k, variant=0):
    """Row k of mcts_dense.npz searched by the oracle under the dense stub:
    (action, visits, nodes, edges, next MT word)."""
    m = oracle.mt_seed(int(f["mt_seed"][k]))
    a, visits, nn, ne = oracle.mcts_search(
        f["state"][k], m, int(f["sims"][k]), float(f["cpuct"][k]), eps=float(f["eps"][k]),
        testing=bool(f["testing"][k]), tau0=int(f["tau0"][k]), ply=int(f["ply"][k]),
        u=float(f["u"][k]), noise=f["noise"][k], evaluator=1, variant=variant)
    return a, visits, nn, ne, oracle.mt_next32(m)


@pytest.mark.parametrize("k", range(48))
def test_mcts_dense_matches_reference(k):
    """The reference's search under the dense stub (mcts_dense.npz: priors with
    full 24-bit significands one ulp apart, zero priors, twenty binades,
    24-bit values, cpuct 1.1 / 0.3 / 3.7 / 2, eps 0.3 / 0.25 / 0), where the
    precision of each arithmetic step decides edges."""
    f = load("mcts_dense.npz")
    assert len(f["sims"]) == 48
    a, visits, nn, ne, nxt = dense_row(f, k)
    assert (visits == f["visits"][k]).all()
    assert a == f["action"][k]
    assert (nn, ne) == (f["n_nodes"][k], f["n_edges"][k])
    assert nxt == f["next_word"][k]


def test_mcts_dense_fixture_tells_precisions_apart():
    """Each wrong-precision variant of the oracle (hz_oracle.h OR_VARIANT_*),
    alone, gives other root visits than the reference on some row of
    mcts_dense.npz, so a kernel or oracle that took that precision would fail
    the fixture.  Rows changed, of 48 (NumPy 2.2.6 capture):
      bit 0, cpuct * P formed in double:              15
      bit 1, the root mix's (1 - eps) * P in double:  13  (of the 24 rows with
             testing false and eps > 0; on every other row it cannot act)
      bit 2, W accumulated in fp32:                    4
    The rows cycle sims over 16 / 64 / 200, cpuct over 1.1 / 0.3 / 3.7 / 2 and
    eps over 0.3 / 0.25 / 0, with testing and tau0 mixed: twelve settings,
    four rows each."""
    f = load("mcts_dense.npz")
    n = len(f["sims"])
    assert {int(s) for s in f["sims"]} == {16, 64, 200}
    assert {float(c) for c in f["cpuct"]} == {1.1, 0.3, 3.7, 2.0}
    assert {float(e) for e in f["eps"]} == {0.3, 0.25, 0.0}
    assert {int(t) for t in f["testing"]} == {0, 1} and {int(t) for t in f["tau0"]} == {0, 15}
    assert int(str(f["numpy_version"]).split(".")[0]) >= 2  # python_float * np.float32 -> float32
    changed = {1: [], 2: [], 4: []}
    for k in range(n):
        for bit in changed:
            if not (dense_row(f, k, variant=bit)[1] == f["visits"][k]).all():
                changed[bit].append(k)
    can_mix = [k for k in range(n) if not f["testing"][k] and f["eps"][k] > 0]
    assert set(changed[2]) <= set(can_mix)
    assert len(changed[1]) >= 1 and len(changed[2]) >= 1 and len(changed[4]) >= 1, changed
    print({bit: len(rows) for bit, rows in changed.items()}, "can_mix", len(can_mix))


def test_mcts_variant_zero_is_the_default():
    """evaluator / variant default to 0: a caller that names neither (the
    mcts.npz test above, bench.py) gets the stub and the reference's
    arithmetic, and naming them as 0 changes nothing."""
    f = load("mcts.npz")
    for k in (0, 5, 17):
        args = (f["state"][k], int(f["sims"][k]), float(f["cpuct"][k]))
        kw = dict(eps=float(f["eps"][k]), testing=bool(f["testing"][k]), noise=f["noise"][k])
        seed = int(f["mt_seed"][k])
        r0 = oracle.mcts_search(args[0], oracle.mt_seed(seed), *args[1:], **kw)
        r1 = oracle.mcts_search(args[0], oracle.mt_seed(seed), *args[1:], evaluator=0, variant=0, **kw)
        assert (r0[1] == r1[1]).all() and r0[2:] == r1[2:] and (r0[1] == f["visits"][k]).all()


def test_mcts_search_reads_no_further_than_the_nine_field_cfg():
    """or_mcts_search keeps the interface it had before or_mcts_cfg grew its
    trailing evaluator / variant fields: a caller whose struct ends at
    negate_value (here followed by set bits where the new fields would lie)
    gets the stub and the reference's arithmetic; or_mcts_search_ex reads the
    same bytes as evaluator and variant and so searches otherwise."""
    import ctypes

    class Cfg9(ctypes.Structure):
        _fields_ = oracle.MctsCfg._fields_[:9]

    class Padded(ctypes.Structure):
        _fields_ = [("cfg", Cfg9), ("after", ctypes.c_int32 * 2)]

    assert ctypes.sizeof(Cfg9) == oracle.MctsCfg.evaluator.offset
    f = load("mcts.npz")
    for k in (0, 5, 17):
        st = np.ascontiguousarray(f["state"][k], np.int16)
        nz = np.ascontiguousarray(f["noise"][k], np.float64)
        pad = Padded(Cfg9(int(f["sims"][k]), float(f["cpuct"][k]), float(f["eps"][k]), int(f["testing"][k]),
                          int(f["tau0"][k]), int(f["ply"][k]), float(f["u"][k]), 0, 0), (ctypes.c_int32 * 2)(1, 7))
        out = []
        for fn in (oracle.lib().or_mcts_search, oracle.lib().or_mcts_search_ex):
            m = oracle.mt_seed(int(f["mt_seed"][k]))
            visits = np.zeros(143, np.int32)
            nn, ne = ctypes.c_int32(0), ctypes.c_int32(0)
            a = fn(oracle._p(st), ctypes.byref(m), ctypes.cast(ctypes.byref(pad), ctypes.POINTER(oracle.MctsCfg)),
                   oracle._p(nz), oracle._p(visits), ctypes.byref(nn), ctypes.byref(ne))
            out.append((a, visits, nn.value, ne.value))
        a, visits, nn, ne = out[0]
        assert (visits == f["visits"][k]).all() and a == f["action"][k]
        assert (nn, ne) == (f["n_nodes"][k], f["n_edges"][k])
        assert not (out[1][1] == visits).all()  # the dense stub with every variant on


def test_greedy_games_match_reference():
    """evaluation.choose_move_greedy games (greedy.npz): every state, every
    chosen action, the final state and the next CPython word — the greedy
    agent's simulated apply_move calls consume `random` like real moves."""
    f = np.load(os.path.join(GOLDEN, "greedy.npz"))
    off = f["offsets"]
    for g in range(len(f["seeds"])):
        m = oracle.mt_seed(int(f["seeds"][g]))
        s = oracle.reset(m)
        for p in range(off[g], off[g + 1]):
            assert (s == f["states"][p]).all(), (g, p - off[g])
            a = oracle.greedy_move(s, m)
            assert a == f["actions"][p], (g, p - off[g])
            r, s = oracle.step(s, a, m)
            assert r == 0
        assert (s == f["finals"][g]).all() and oracle.is_game_over(s)
        assert oracle.mt_next32(m) == f["next_word"][g]


def test_play_rule_auto_matches_stepwise_loop():
    """or_play_rule_auto (the steady-state auto-reset oracle) equals the
    step-by-step loop over the oracle's primitives (reset, legal, rule, step),
    and its first game equals or_play_rule_games_ep's."""
    n, base, plies = 12, 4321, 170
    total, finals, games, ep = oracle.play_rule_auto(n, base, plies, ep0=2)
    assert total == n * plies
    _, first, first_plies, _ = oracle.play_rule_games(n, base, episode=2)
    for b in range(n):
        left, e, done = plies, 2, 0
        while True:
            seed = base + b + (e << 32)
            m = oracle.mt_seed(seed)
            s = oracle.reset(m)
            ply = 0
            while left > 0 and not oracle.is_game_over(s):
                mask = oracle.legal(s)
                L = int(mask.sum())
                a = np.flatnonzero(mask)[((oracle.rule(seed, ply) >> 32) * L) >> 32]
                s = oracle.step(s, int(a), m)[1]
                ply += 1
                left -= 1
            done += int(oracle.is_game_over(s))
            if e == 2 and oracle.is_game_over(s):
                assert ply == first_plies[b] and (s == first[b]).all()
            if left <= 0:
                break
            e += 1
        assert (finals[b] == s).all() and games[b] == done and ep[b] == e, b


def test_replay_actions_matches_reference_traces():
    """or_replay_actions (the api_caller leg's check: a caller's own moves
    replayed from the same seeds) reproduces the reference's recorded games
    from their action lists, with no-ops and rejected moves mixed in (a
    rejected move leaves the state as it was, like the reference's
    clone-then-commit)."""
    f = load("env_traces.npz")
    acts, off, seeds = f["actions"], f["offsets"], f["seeds"]
    n = len(seeds)
    lens = off[1:] - off[:-1]
    T = int(lens.max())
    clean = np.full((T, n), -1, np.int16)
    for g in range(n):
        clean[:lens[g], g] = acts[off[g]:off[g + 1]]
    total, finals, rej = oracle.replay_actions(seeds.astype(np.uint64), clean)
    assert total == int(lens.sum()) and (rej == 0).all()
    assert (finals == f["finals"]).all()
    # interleave no-op plies and an illegal action (142 never fits the
    # opening's pile phase, and a pile index past the piles never fits later)
    noisy = np.full((3 * T, n), -1, np.int16)
    noisy[1::3] = clean
    noisy[0, :] = 142
    total2, finals2, rej2 = oracle.replay_actions(seeds.astype(np.uint64), noisy)
    assert total2 == total and (rej2 == 1).all() and (finals2 == finals).all()


def test_play_rule_from_continues_rule_games():
    """or_play_rule_from from a reset state, and from a state part of the way
    through the game, ends where or_play_rule_games ends: final state, ply
    count and next stream word (no stuck board occurs in play from a reset)."""
    n, base = 24, 321
    _, finals, plies, nxt = oracle.play_rule_games(n, base, nthreads=2)
    for b in range(n):
        m = oracle.mt_seed(base + b)
        st = oracle.reset(m)
        mid, k, stuck = oracle.play_rule_from(st, m, base + b, 0, 3 + 2 * b)
        assert k == 3 + 2 * b and not stuck
        fin, k2, stuck = oracle.play_rule_from(mid, m, base + b, k, 1 << 20)
        assert not stuck and k + k2 == plies[b], b
        assert (fin == finals[b]).all() and oracle.is_game_over(fin), b
        assert oracle.mt_next32(m) == nxt[b], b
        again, k3, stuck = oracle.play_rule_from(fin, m, base + b, plies[b], 50)  # a finished game: nothing to do
        assert k3 == 0 and not stuck and (again == fin).all()


def test_stuck_board_is_left_alone():
    """A stuck board (no legal move, game not over; oracle.stuck_state) packs
    and unpacks like any state; or_play_rule_from stops on it at once, as
    or_play_rule_auto's loop does: no step, the stuck flag, state and stream
    untouched; or_mcts_search gives no move: -1, no visits, the root alone."""
    from conftest import PKG  # noqa: F401  (puts hzamd on the path)
    from hzamd.state import pack_ref, unpack_ref
    for seed in (7, 4242, 1 << 33):
        st, m = oracle.stuck_state(seed)
        words, idx = m.words()
        assert oracle.legal(st).sum() == 0 and not oracle.is_game_over(st)
        assert (unpack_ref(pack_ref(st)) == st).all()
        for plies in (1, 200):
            fin, steps, stuck = oracle.play_rule_from(st, m, seed, 1, plies)
            assert steps == 0 and stuck and (fin == st).all()
        a, visits, nn, ne = oracle.mcts_search(st, m, 24, 2.0, testing=True)
        assert a == -1 and visits.sum() == 0 and (nn, ne) == (1, 0)
        w2, i2 = m.words()
        assert (w2 == words).all() and i2 == idx



# ---------------------------------------------------------------- search limits
# hz_mcts_create's max_nodes / max_depth restated in the oracle (or_mcts_cfg's
# trailing fields, 0 = unlimited).  need = max(n_nodes, n_edges) of a fixture
# row: the smallest max_nodes its unbounded search fits (max_edges = max_nodes).
LIMIT_GROUP = (32, 2.0, 1, 0.25)   # the rows tests/test_mcts_limits_gpu.py searches
LIMIT_NODES = 500                  # ... with this max_nodes
LIMIT_NODES_EARLY = (250, 140)     # ... and these, where refusals change the stream and the visits
LIMIT_DEPTH = 2                    # ... and this max_depth (test_mcts_limits_fixture_conditions)


def limits_row(f, k, **kw):
    """Row k of mcts.npz searched by the oracle: (action, visits, nodes, edges,
    limit flag, deepest path, next MT word)."""
    m = oracle.mt_seed(int(f["mt_seed"][k]))
    r = oracle.mcts_search(
        f["state"][k], m, int(f["sims"][k]), float(f["cpuct"][k]), eps=float(f["eps"][k]),
        testing=bool(f["testing"][k]), tau0=int(f["tau0"][k]), ply=int(f["ply"][k]),
        u=float(f["u"][k]), noise=f["noise"][k], with_limits=True, **kw)
    return r + (oracle.mt_next32(m),)


def same_search(r, s):
    return r[0] == s[0] and (r[1] == s[1]).all() and r[2:] == s[2:]


def limit_rows(f):
    return [k for k in range(len(f["sims"])) if f["sims"][k] <= 64]


def group_rows(f, key):
    return [k for k in range(len(f["sims"]))
            if (int(f["sims"][k]), float(f["cpuct"][k]), int(f["testing"][k]), float(f["eps"][k])) == key]


def test_mcts_limits_that_fit_change_nothing():
    """max_nodes == need (and need + 1000) is the unbounded search, which is
    the fixture row: visits, action, counts, next MT word, flag 0."""
    f = load("mcts.npz")
    rows = limit_rows(f)
    assert len(rows) == 57
    for k in rows:
        need = max(int(f["n_nodes"][k]), int(f["n_edges"][k]))
        free = limits_row(f, k)
        assert (free[1] == f["visits"][k]).all() and free[0] == f["action"][k] and free[4] == 0
        assert free[2:4] == (f["n_nodes"][k], f["n_edges"][k]) and free[6] == f["next_word"][k]
        for cap in (need, need + 1000):
            assert same_search(limits_row(f, k, max_nodes=cap), free), (k, cap)


def test_mcts_one_entry_short_refuses_an_expansion():
    """max_nodes == need - 1: the flag is set, both counts stay within
    max_nodes, and the root's visits still sum to sims - 1 (a refused leaf is
    evaluated and backed up) -- unless the root's own expansion is what does
    not fit (the three rows with 2 or 3 legal moves): then every simulation
    tries it again, there are no edges and no visits.
    Those rows are place_tile_3 roots, so they pin the stream rule where the
    first refused leaf is known from outside: each refused attempt has replayed
    the children's turn-end draws and kept them.  The stream is the one
    or_step leaves after sims rounds over the legal moves (plus the no-visits
    fallback's random.choice), not the unbounded row's."""
    f = load("mcts.npz")
    root_refused = []
    for k in limit_rows(f):
        need = max(int(f["n_nodes"][k]), int(f["n_edges"][k]))
        if need < 3:
            continue
        sims = int(f["sims"][k])
        a, visits, nn, ne, flag, _, nxt = limits_row(f, k, max_nodes=need - 1)
        assert flag == 1 and nn <= need - 1 and ne <= need - 1, k
        legal = np.flatnonzero(oracle.legal(f["state"][k]))
        if 1 + len(legal) <= need - 1:
            assert visits.sum() == sims - 1, k
            continue
        root_refused.append(k)
        assert visits.sum() == 0 and (nn, ne) == (1, 0), k
        assert f["state"][k][73] == 3 and nxt != f["next_word"][k], k
        m = oracle.mt_seed(int(f["mt_seed"][k]))
        for _ in range(sims):
            for act in legal:
                assert oracle.step(f["state"][k], int(act), m)[0] == 0
        assert a == legal[oracle.lib().or_randbelow(m, len(legal))] and nxt == oracle.mt_next32(m), k
    assert len(root_refused) >= 1
    print("root refused:", root_refused)


def test_mcts_depth_limit():
    """max_depth >= the row's deepest path changes nothing; one less sets the
    flag; max_depth 1 keeps every walk at depth 1 (the flag tells whether one
    stood on an expanded child, as the unbounded search's first walk to depth 2
    does) with the visits still summing to sims - 1."""
    f = load("mcts.npz")
    for k in limit_rows(f):
        sims = int(f["sims"][k])
        free = limits_row(f, k)
        deep = free[5]
        assert 1 <= deep <= sims - 1
        for D in (deep, deep + 100):
            assert same_search(limits_row(f, k, max_depth=D), free), (k, D)
        if deep >= 2:
            cut = limits_row(f, k, max_depth=deep - 1)
            assert cut[4] == 1 and cut[5] == deep - 1 and cut[1].sum() == sims - 1, k
        one = limits_row(f, k, max_depth=1)
        assert one[5] == 1 and one[1].sum() == sims - 1, k
        assert one[4] == int(deep >= 2), k


def test_mcts_limits_fixture_conditions():
    """What tests/test_mcts_limits_gpu.py needs of mcts.npz.  The group
    (32 sims, cpuct 2, testing, eps 0.25) has 13 rows with needs 234, 508,
    500, 439, 627, 482, 277, 562, 987, 741, 215, 4, 292: under max_nodes 500
    eight fit (one, 492 nodes / 500 edges, exactly) and five do not (508 just
    over).  Their deepest paths are 3, 3, 4, 4, 2, 3, 4, 2, 3, 2, 3, 1, 3:
    max_depth 2 leaves four rows as they are and cuts nine (3 would leave ten
    and cut three; 2 is taken for the larger number of cut boards)."""
    f = load("mcts.npz")
    rows = group_rows(f, LIMIT_GROUP)
    need = [max(int(f["n_nodes"][k]), int(f["n_edges"][k])) for k in rows]
    assert need == [234, 508, 500, 439, 627, 482, 277, 562, 987, 741, 215, 4, 292]
    fit = [x <= LIMIT_NODES for x in need]
    assert sum(fit) == 8 and len(fit) - sum(fit) == 5 and LIMIT_NODES in need and LIMIT_NODES + 8 in need
    k = rows[need.index(LIMIT_NODES)]
    assert (f["n_nodes"][k], f["n_edges"][k]) == (492, 500)
    deep = [limits_row(f, k)[5] for k in rows]
    assert deep == [3, 3, 4, 4, 2, 3, 4, 2, 3, 2, 3, 1, 3]
    assert sum(d <= LIMIT_DEPTH for d in deep) >= 3 and sum(d > LIMIT_DEPTH for d in deep) >= 3
    # at 500 the refused rows lose only late expansions: flag and counts differ
    # from the unbounded search, visits, move and stream do not
    for k, ok in zip(rows, fit):
        r, free = limits_row(f, k, max_nodes=LIMIT_NODES), limits_row(f, k)
        assert (r[4] == 0) == ok and (r[2:4] == free[2:4]) == ok, k
        assert (r[1] == free[1]).all() and r[0] == free[0] and r[6] == free[6], k
    # ... so the GPU tests also run the group at 250 and 140, where refusals
    # come early: rows refused there whose next MT word is not the fixture's (a
    # refused place_tile_3 leaf's draws kept, and made again on re-selection)
    # and rows whose visits are not the fixture's, every one still backed up
    want = {250: (10, [4, 16], [12, 16]), 140: (12, [4, 16, 24, 28, 36, 40], [12, 16, 36])}
    assert tuple(want) == LIMIT_NODES_EARLY
    for cap, (refused, other_word, other_visits) in want.items():
        rs = {k: limits_row(f, k, max_nodes=cap) for k in rows}
        flagged = [k for k in rows if rs[k][4]]
        assert len(flagged) == refused and all((rs[k][4] == 0) == (x <= cap) for k, x in zip(rows, need))
        assert [k for k in flagged if rs[k][6] != f["next_word"][k]] == other_word
        assert [k for k in flagged if (rs[k][1] != f["visits"][k]).any()] == other_visits
        assert all(rs[k][1].sum() == 31 for k in rows)
    # ... and the three place_tile_3 roots whose own expansion does not fit
    # need - 1 (test_mcts_one_entry_short_refuses_an_expansion), one per handle
    shapes = [(int(f["n_nodes"][k]), int(f["n_edges"][k]), int(f["sims"][k]), int(f["state"][k][73]))
              for k in range(len(f["sims"])) if max(f["n_nodes"][k], f["n_edges"][k]) in (3, 4)]
    assert sorted(shapes) == [(3, 2, 8, 3), (4, 3, 32, 3), (4, 3, 64, 3), (4, 3, 200, 3)]
    # the 8-simulation row where only the edge pool binds
    k8 = [k for k in range(len(f["sims"])) if (f["n_nodes"][k], f["n_edges"][k], f["sims"][k]) == (267, 339, 8)]
    assert len(k8) == 1
