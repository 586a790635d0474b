"""Asynchronous self-play (SelfPlay.play_async; include/hz_abi.h: the turn of
asynchronous self-play): each board moves when its own search is spent, and
the records are play_steady's bit for bit.

40 boards (the layered gather for more than 32 boards), budgets 12 / 3 with
p = 0.5, default turns_until_tau0 (15: the sampled and the greedy choice both
occur), the stub and the dense stub.  K = 70 moves is past the length of most
games (64 plies or a few more), so boards end a game and start their next one
inside the run (asserted on `ended`).  The kernels of the turn are also pinned one by one
(masked begin, per-board-move draws, the choice), so a parity failure can be
located."""
import functools

import numpy as np
import pytest
import torch

import oracle
from hzamd.state import pack_ref, words_to_array
from selfplay_async_model import moves_done_after, sim_steps, step_bound, turn_steps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

N, BASE, SIMS, FAST, P, K, CPUCT = 40, 8800, 12, 3, 0.5, 70, 2.0
CFG = {"num_simulations": SIMS, "cpuct": CPUCT}
CAP = dict(CFG, playout_cap_p=P, playout_cap_fast=FAST)
REC_KEYS = ("states", "visits", "players", "game", "ended", "outcome", "plies")


def evaluator(name):
    from hzamd.mcts import dense_stub_evaluator, stub_evaluator
    return {"stub": stub_evaluator, "dense": dense_stub_evaluator}[name]


def make(cfg, ev, n=N, base=BASE, **kw):
    from hzamd.selfplay import SelfPlay
    return SelfPlay(n, ev, cfg, seed_base=base, device=DEV, **kw)


def next_words(env):
    _, mt, idx = env.export_state(with_mt=True)
    mt, idx = mt.cpu().numpy().view(np.uint32), idx.cpu().numpy()
    return [oracle.mt_next32(oracle.mt_from_words(mt[b], idx[b])) for b in range(env.n)]


@functools.lru_cache(maxsize=None)
def pair(name):
    """The capped run under both schedules, played once per evaluator."""
    a = make(CAP, evaluator(name))
    ra = a.play_async(K)
    s = make(CAP, evaluator(name))
    rs = s.play_steady(K)
    return a, ra, s, rs


@functools.lru_cache(maxsize=None)
def host_budgets(moves=K, n=N, base=BASE, sims=SIMS, fast=FAST, p=P):
    """The budgets of every board and move, from the coins: int64 numpy [n, moves]."""
    from hzamd.selfplay import NoiseSource, playout_budgets
    src = NoiseSource(base, DEV)
    cols = [playout_budgets(src.coin(k, n), p, sims, fast)[0].cpu().numpy() for k in range(moves)]
    return np.stack(cols, axis=1).astype(np.int64)


def assert_records_equal(ra, rs, keys=REC_KEYS):
    for key in keys:
        assert ra[key].dtype == rs[key].dtype and ra[key].shape == rs[key].shape, key
        assert torch.equal(ra[key], rs[key]), key


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("stub", "dense"))
def test_parity_with_the_barrier_schedule_caps_on(name):
    a, ra, s, rs = pair(name)
    assert ra["moves"] == rs["moves"] == K and set(rs) | {"moves_done", "sim_steps"} == set(ra)
    assert_records_equal(ra, rs, REC_KEYS + ("full",))
    assert (ra["moves_done"] == K).all() and ra["moves_done"].dtype == torch.int32
    # the env after the run: state words and every board's next stream word
    assert torch.equal(a.env.export_state(), s.env.export_state())
    assert next_words(a.env) == next_words(s.env)
    ca, cs = a.compact_steady(ra), s.compact_steady(rs)
    assert set(ca) == set(cs) and ca["states"].shape[0] > 0
    for key in cs:
        assert torch.equal(ca[key], cs[key]), key
    # a game ends and the next one starts inside the run: K is past a game's length (64 plies)
    ended = ra["ended"]
    over = ended[:K - 1].any(0)  # boards whose first game ends before their last move
    print(f"boards that end a game inside the run: {int(over.sum())} of {N}")
    assert over.any(), "a game ends, and the next one starts, inside the run"
    first = ended.int().argmax(0)  # the move that ended each board's first game; the next one is ply 1 of game 1
    nxt = (first + 1).clamp(max=K - 1)
    col = torch.arange(N, device=DEV)
    assert (ra["plies"][nxt, col] == 1)[over].all() and (ra["game"][nxt, col] == 1)[over].all()
    assert (ra["game"][K - 1] == ended[:K - 1].sum(0))[over].all() and (ra["game"][:, ~over] == 0).all()
    # not passing emptily: from the coins, on the host
    bud = host_budgets()
    full = (bud == SIMS)
    assert np.array_equal(full, ra["full"].cpu().numpy().T)
    assert full.any(1).all() and (~full).any(1).all(), "every board has a fast and a full move"
    steps = ra["sim_steps"]
    print(f"sim steps: async {steps}, barrier {K * SIMS}, model {sim_steps(bud)}, bound {step_bound(bud)}")
    assert steps < K * SIMS
    assert steps <= step_bound(bud)
    assert steps == sim_steps(bud)  # the layered sim step loses no slot
    # same searches, fewer steps
    assert int(a.mcts.eval_rows_total.item()) == int(s.mcts.eval_rows_total.item()) > 0


# 2 ---------------------------------------------------------------------------
def test_caps_off_is_the_barrier_schedule():
    moves = 5
    a = make(CFG, evaluator("stub"))
    ra = a.play_async(moves)
    s = make(CFG, evaluator("stub"))
    rs = s.play_steady(moves)
    assert "full" not in ra and set(rs) | {"moves_done", "sim_steps"} == set(ra)
    assert_records_equal(ra, rs)
    assert ra["sim_steps"] == moves * SIMS  # every board turns together
    assert (ra["visits"].sum(2) == SIMS - 1).all()
    assert torch.equal(a.env.export_state(), s.env.export_state())
    assert int(a.mcts.eval_rows_total.item()) == int(s.mcts.eval_rows_total.item())
    assert a.step_counter == s.step_counter == moves
    # ... and a second run continues the move counters where play_steady's would
    assert_records_equal(a.play_async(2, reset=False), s.play_steady(2, reset=False), ("states", "visits"))


# 3 ---------------------------------------------------------------------------
def test_a_real_network():
    from hzamd.mcts import BatchedPredictor
    from hzamd.net import TINY, HarmoniesNet
    torch.manual_seed(0)
    ev = BatchedPredictor(HarmoniesNet(TINY).to(DEV).eval())
    assert TINY["cnn_filters"] == 32 and ev.row_independent is True
    cfg = {"num_simulations": 8, "cpuct": 1.5, "playout_cap_p": P, "playout_cap_fast": 2}
    a = make(cfg, ev)
    ra = a.play_async(6)
    s = make(cfg, ev)
    rs = s.play_steady(6)
    assert_records_equal(ra, rs, REC_KEYS + ("full",))
    assert ra["full"].any() and not ra["full"].all()
    assert ra["sim_steps"] == sim_steps(host_budgets(6, sims=8, fast=2)) <= 6 * 8
    assert int(a.mcts.eval_rows_total.item()) == int(s.mcts.eval_rows_total.item())


# 4 ---------------------------------------------------------------------------
def sim(mcts, steps, noise=None):
    from hzamd.mcts import stub_evaluator
    for _ in range(steps):
        board, glob, rows, count = mcts.select_gather(CPUCT)
        k = int(count.item())
        pol, val = stub_evaluator(board[:k], glob[:k]) if k else (mcts._nil_pol, mcts._nil_val)
        mcts.expand_backup(pol, val, noise, 0.25, True, gathered=True)


def test_masked_begin():
    from hzamd.env import BatchedEnv
    from hzamd.mcts import BatchedMCTS
    n, stuck, stopped = 40, 9, 33
    env = BatchedEnv(n, seed_base=BASE, device=DEV)
    env.reset()
    st, mt, idx = env.export_state(with_mt=True)
    st[:, stuck] = torch.from_numpy(words_to_array([pack_ref(oracle.stuck_state(BASE + stuck)[0])])[0]).to(DEV)
    env.import_state(st, mt, idx)
    budget = torch.full((n,), 9, dtype=torch.int32, device=DEV)
    budget[::4] = 2   # spent after two of the three steps below
    bits = torch.ones(n, dtype=torch.uint8, device=DEV)
    a = BatchedMCTS(env, 16)
    a._set_gate(budget, bits)
    a.begin()
    sim(a, 3)
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    mask[[0, 4, 5, stuck, 31, 32, 39]] = 1   # spent boards, boards in mid-search, the stuck root, both ends
    mask[stopped] = 2
    out = [b for b in range(n) if mask[b] == 0]
    before = {"stats": a.stats().clone(), "result": a.result().clone(), "sims": a.sims_done().clone()}
    trees = {b: a.export_tree(b) for b in (1, 8, 38)}   # a board in mid-search, a spent one, the last unmasked one
    assert before["sims"][1] == 3 and before["sims"][8] == 2 and before["sims"][stuck] == 0
    # the masked boards get fresh budgets (the stuck root's too: the begin takes it back to 0)
    a.set_gate_some(mask, budget=torch.full((n,), 5, dtype=torch.int32, device=DEV))
    a.begin_some(mask)
    after = {"stats": a.stats().clone(), "result": a.result().clone(), "sims": a.sims_done().clone()}
    for key in before:
        assert torch.equal(after[key][out], before[key][out]), key
    for b, tree in trees.items():
        now = a.export_tree(b)
        assert set(now) == set(tree) and all(np.array_equal(now[k], tree[k]) for k in tree), b
    # inside the mask: a fresh begin of a second handle on the same env
    f = BatchedMCTS(env, 16)
    f._set_gate(torch.full((n,), 5, dtype=torch.int32, device=DEV), bits)
    f.begin()
    fresh = f.stats().clone()
    begun = [b for b in range(n) if mask[b] == 1]
    assert torch.equal(after["stats"][begun][:, [0, 1, 3]], fresh[begun][:, [0, 1, 3]])
    assert (after["stats"][begun, 0] == 1).all() and (after["stats"][begun, 1] == 0).all()
    assert torch.equal(after["stats"][begun, 2], before["stats"][begun, 2] + 1)   # a new generation
    assert (after["sims"][begun] == 0).all() and (after["result"][begun] == 0).all()
    for b in (4, stuck):
        ta, tf = a.export_tree(b), f.export_tree(b)
        assert np.array_equal(ta["state"], tf["state"]) and ta["state"].shape == (1, 6)   # node 0: the env's state
    # the stopped board: no tree
    assert after["stats"][stopped, 0] == 0 and after["stats"][stopped, 1] == 0 and after["sims"][stopped] == 0
    assert (after["result"][stopped] == 0).all()
    # what follows: the begun boards search as the fresh handle's do (each from its own copy of the env,
    # since expansions draw from the boards' streams), the stuck root and the stopped board are not walked,
    # the unmasked boards carry on with the budgets they had
    env2 = BatchedEnv(n, seed_base=BASE, device=DEV)
    env2.import_state(*env.export_state(with_mt=True))
    f2 = BatchedMCTS(env2, 16)
    f2._set_gate(torch.full((n,), 5, dtype=torch.int32, device=DEV), bits)
    f2.begin()
    sim(a, 6)
    sim(f2, 6)
    ra, rf, sa = a.result(), f2.result(), a.sims_done()
    assert torch.equal(ra[begun], rf[begun]) and torch.equal(a.stats()[begun][:, :2], f2.stats()[begun][:, :2])
    want = torch.full((n,), 5, dtype=torch.int32, device=DEV)
    want[stuck] = 0
    assert torch.equal(sa[begun], want[begun]) and sa[stopped] == 0 and a.stats()[stopped, 0] == 0
    assert torch.equal(sa[out], torch.minimum(budget, torch.tensor(9, device=DEV, dtype=torch.int32))[out])
    assert (ra[out].sum(1) == sa[out] - 1).all()
    for h in (a, f, f2):
        h.close()


# 5 ---------------------------------------------------------------------------
def test_per_board_move_draws():
    from hzamd.selfplay import NoiseSource
    n, alpha = 12, 0.4
    src = NoiseSource(BASE, DEV, seed=3)
    moves = torch.tensor([0, 1, 5, 2**33 + 7, 0, 1, 2**33 + 7, 2**62 + 1, 5, 5, 69, 1], dtype=torch.int64, device=DEV)
    counts = torch.tensor([1, 2, 69, 40, 64, 65, 7, 33, 0, 68, 12, 3], dtype=torch.int32, device=DEV)
    scalar = {int(m): (src.draw(int(m), counts, alpha), src.coin(int(m), n)) for m in set(moves.tolist())}
    patterns = [torch.zeros(n), torch.ones(n), torch.arange(n) % 2, (torch.arange(n) % 3 == 0).float(),
                torch.tensor([0, 0, 0, 1] + [0] * 8)]
    for pat in patterns:
        mask = pat.to(device=DEV, dtype=torch.uint8)
        noise = torch.full((n, 69), -7.0, dtype=torch.float64, device=DEV)
        u = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
        coin = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
        src.draw_at(moves, counts, alpha, mask, noise, u)
        src.coin_at(moves, mask, coin)
        for b in range(n):
            if mask[b]:
                (want_noise, want_u), want_coin = scalar[int(moves[b])]
                assert torch.equal(noise[b], want_noise[b]) and u[b] == want_u[b] and coin[b] == want_coin[b], b
            else:
                assert (noise[b] == -7.0).all() and u[b] == -7.0 and coin[b] == -7.0, b
    # the uint64 view of the counters draws the same bits
    noise2 = torch.zeros(n, 69, dtype=torch.float64, device=DEV)
    u2 = torch.zeros(n, dtype=torch.float64, device=DEV)
    src.draw_at(moves.view(torch.uint64), counts, alpha, torch.ones(n, dtype=torch.uint8, device=DEV), noise2, u2)
    for b in range(n):
        want_noise, want_u = scalar[int(moves[b])][0]
        assert torch.equal(noise2[b], want_noise[b]) and u2[b] == want_u[b], b
    with pytest.raises(ValueError):
        src.coin_at(moves.to(torch.int32), mask, coin)


# 6 ---------------------------------------------------------------------------
def both_choices(visits, explore, u):
    from hzamd.mcts import choose_actions, choose_actions_native
    want = choose_actions(visits, explore, u)
    got = choose_actions_native(visits, explore, u)
    assert got.dtype == torch.int16 and torch.equal(got.to(torch.int64), want)
    return want


def test_choose_kernel_on_hand_built_tables():
    below_one = 1.0 - 2.0 ** -53
    rows, us = [], []

    def add(v, *uu):
        for x in uu:
            rows.append(v)
            us.append(x)
    z = [0] * 143
    ties = list(z)
    for a in (7, 70, 142):
        ties[a] = 5
    add(ties, 0.0, 0.3, 0.5, 0.9, below_one, 1 / 3)   # u * 15 = 0, 4.5, 7.5, 13.5, just below 15, and 5 up to rounding
    single = list(z)
    single[141] = 9
    add(single, 0.0, 0.5, below_one)
    add(z, 0.0, 0.5, below_one)                      # no visits: -1
    wide = list(z)                                   # a 69-edge root, two actions apart: edges 64..68 are actions 128..136
    for e in range(69):
        wide[2 * e] = 1 + (e % 3)
    add(wide, 0.0, 0.5, 0.93, 0.97, 0.99, below_one)
    last = list(z)
    last[0], last[142] = 1, 1
    add(last, 0.0, 0.49999999999999994, 0.5, below_one)
    big = list(z)
    big[3], big[100] = 2**31 - 1, 2**31 - 1           # the total needs int64
    add(big, 0.0, 0.5, below_one)
    visits = torch.tensor(rows, dtype=torch.int32, device=DEV)
    u = torch.tensor(us, dtype=torch.float64, device=DEV)
    sampled = both_choices(visits, torch.ones(len(rows), dtype=torch.bool, device=DEV), u).tolist()
    greedy = both_choices(visits, torch.zeros(len(rows), dtype=torch.bool, device=DEV), u).tolist()
    assert sampled[:5] == [7, 7, 70, 142, 142] and greedy[:6] == [7] * 6   # the first of the tied actions
    assert sampled[6:9] == [141] * 3 and sampled[9:12] == [-1] * 3 and greedy[9:12] == [-1] * 3
    # the 69-edge root: 138 visits; u * 138 = 128.34, 133.86, 136.62 fall on edges 64, 67 and 68 (past lane 63)
    assert sampled[12] == 0 and sampled[14:17] == [128, 134, 136] and sampled[17] in (136, 0)
    assert greedy[12] == 4                                                 # the first edge with 3 visits
    assert sampled[18:22] == [0, 0, 142, 142]
    assert sampled[22:25] == [3, 100, 100] and greedy[22] == 3


def test_choose_kernel_on_the_runs_trees():
    """Every root of test 1's run, under the sampled and the greedy rule, and
    the explore rule the turn applies (the board's own ply below 15)."""
    _, ra, _, _ = pair("stub")
    visits = ra["visits"].reshape(K * N, 143)
    g = torch.Generator(device="cpu").manual_seed(5)
    u = torch.rand(K * N, dtype=torch.float64, generator=g).to(DEV)
    for explore in (torch.ones(K * N, dtype=torch.bool, device=DEV), torch.zeros(K * N, dtype=torch.bool, device=DEV),
                    (ra["plies"].reshape(-1) - 1) < 15):
        act = both_choices(visits, explore, u)
        assert (act >= 0).all()
    assert ((ra["plies"] - 1) < 15).any() and ((ra["plies"] - 1) >= 15).any()


# 7 ---------------------------------------------------------------------------
def test_sim_steps_cut():
    moves, cut = 10, 40
    whole = make(CAP, evaluator("stub")).play_async(moves)
    sp = make(CAP, evaluator("stub"))
    part = sp.play_async(moves, sim_steps=cut)
    bud = host_budgets(moves)
    assert whole["sim_steps"] == sim_steps(bud) > cut and part["sim_steps"] == cut
    done = part["moves_done"].cpu().numpy()
    assert np.array_equal(done, moves_done_after(bud, cut))
    assert done.min() < done.max() <= moves and done.min() >= 1, "the boards have made different numbers of moves"
    reached = torch.arange(moves, device=DEV).unsqueeze(1) < part["moves_done"].unsqueeze(0)   # [moves, n]
    for key in REC_KEYS + ("full",):
        w, p = whole[key], part[key]
        m = reached.unsqueeze(1) if key == "states" else reached
        m = m.unsqueeze(-1) if key == "visits" else m
        assert torch.equal(torch.where(m, w, torch.zeros_like(w)), p), key   # equal up to moves_done, zero past it
    comp = sp.compact_steady(part)   # no game ends in ten moves: no records, and the unreached slots are none either
    assert comp["states"].shape[0] == 0
    # a run without moves, and one without steps
    empty = make(CAP, evaluator("stub"), n=8).play_async(0)
    assert empty["sim_steps"] == 0 and empty["visits"].shape == (0, 8, 143) and (empty["moves_done"] == 0).all()
    none = make(CAP, evaluator("stub"), n=8).play_async(3, sim_steps=0)
    assert none["sim_steps"] == 0 and (none["moves_done"] == 0).all() and not none["visits"].any()


def test_turn_model_matches_the_run():
    """Move k of board b is recorded in the sim step the host model names: a
    run cut after each of a few step counts has made exactly the model's moves."""
    moves = 6
    bud = host_budgets(moves)
    t = turn_steps(bud)
    for cut in (int(t.min()), int(np.median(t)), int(t.max()) - 1):
        part = make(CAP, evaluator("stub")).play_async(moves, sim_steps=cut)
        assert np.array_equal(part["moves_done"].cpu().numpy(), moves_done_after(bud, cut)), cut


# 8 ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,kw", [({"tree_reuse": "add"}, {}), ({"root_policy": "gumbel"}, {}),
                                    ({"leaf_symmetry": "random"}, {}), ({"forced_playouts": 2.0}, {}),
                                    ({}, {"keep_root_value": True})])
def test_unsupported_keys(cfg, kw):
    sp = make(dict(CFG, **cfg), evaluator("stub"), n=8, **kw)
    with pytest.raises(ValueError, match="play_async does not take"):
        sp.play_async(2)
    with pytest.raises(ValueError):
        make(CFG, evaluator("stub"), n=8).play_async(-1)


def test_a_stuck_board_raises_at_the_end_of_the_run():
    stuck = 7
    sp = make(CAP, evaluator("stub"), n=16)
    sp.env.reset(seeds=BASE + torch.arange(16, device=DEV, dtype=torch.int64))
    st, mt, idx = sp.env.export_state(with_mt=True)
    st[:, stuck] = torch.from_numpy(words_to_array([pack_ref(oracle.stuck_state(BASE + stuck)[0])])[0]).to(DEV)
    sp.env.import_state(st, mt, idx)
    with pytest.raises(RuntimeError, match=r"step failed on boards \[7\]"):
        sp.play_async(3, reset=False)


def test_iteration_with_the_async_schedule():
    """SelfPlay.iteration(schedule="async"): play_async + compact_steady + the
    packed records into the buffer; the records are those of the games that
    ended inside the run."""
    from hzamd import distributed as hd
    sp = make(CAP, evaluator("stub"))
    buf = hd.ReplayBuffer(100000, DEV)
    packed, rec = sp.iteration(buf, schedule="async", moves_per_board=K)
    _, ra, _, _ = pair("stub")
    assert torch.equal(rec["visits"], ra["visits"]) and rec["sim_steps"] == ra["sim_steps"]
    comp = sp.compact_steady(rec)
    assert packed.shape[0] == comp["states"].shape[0] == len(buf) > 0
