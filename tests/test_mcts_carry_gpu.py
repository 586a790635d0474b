"""Tree reuse on the GPU (hz_mcts_advance, hz_mcts_begin_carried,
BatchedMCTS.advance / search(carry=True), SelfPlay's tree_reuse) against the
host model tests/mcts_carry_model.py, which tests/test_mcts_carry_cpu.py holds
to the C oracle's own search.  Every comparison is exact: integers as they
are, floats by their bits."""
import functools

import numpy as np
import pytest
import torch

import oracle
from hzamd.state import pack_ref, unpack_ref, words_to_array
from mcts_carry_model import (FIXTURE, CarryModel, carry_tree, choose, copy_mt, fixture_action, game_over, next_word,
                              positions, topup_budget)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPECIAL = (0, 63, 64, 129)  # a wave's first and last lane, the next wave's first, a partial wave's last
CHECK = SPECIAL + (5, 17, 26, 38, 47, 59, 70, 77, 88, 96, 107, 118)  # the boards the continued search is modelled on
TREE_KEYS = ("state", "e0", "ne", "action", "child", "n", "w", "p", "player")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.dtype == b.dtype and a.shape == b.shape and bool((bits(a) == bits(b)).all())
    return a.shape == b.shape and bool((a == b).all())


def same_tree(a, b):
    return all(same(a[k], b[k]) for k in TREE_KEYS)


@functools.lru_cache(maxsize=None)
def fixture_positions():
    F = FIXTURE
    return positions(F["base"], F["n"], F["spread"])


def make_env(pos):
    from hzamd.env import BatchedEnv
    env = BatchedEnv(len(pos), device=DEV)
    words = words_to_array([pack_ref(st) for st, _ in pos])
    mts = np.stack([m.words()[0] for _, m in pos])
    idx = np.array([m.words()[1] for _, m in pos], np.int32)
    env.import_state(torch.from_numpy(np.ascontiguousarray(words.T)), torch.from_numpy(mts.view(np.int32)),
                     torch.from_numpy(idx))
    return env


def models(pos, evaluator, max_nodes=None):
    return [CarryModel(st, copy_mt(m), evaluator, max_nodes=max_nodes) for st, m in pos]


def streams(env):
    _, mt, idx = env.export_state(with_mt=True)
    mt, idx = mt.cpu().numpy().view(np.uint32), idx.cpu().numpy()
    return [oracle.mt_next32(oracle.mt_from_words(mt[b], idx[b])) for b in range(env.n)]


class _Rows:
    """A stub evaluator on the device-row protocol (device ops only: capturable)."""
    device_rows = capturable = row_independent = True

    def __init__(self, fn):
        self.fn = fn

    def __call__(self, board, glob, rows=None, count=None):
        return self.fn(board, glob)


def evaluator_of(kind, device_rows=False):
    from hzamd.mcts import dense_stub_evaluator, stub_evaluator
    fn = dense_stub_evaluator if kind else stub_evaluator
    return _Rows(fn) if device_rows else fn


def fixture_moves(mcts):
    """fixture_action for every board, from the device's root edges."""
    root = {k: v.cpu().numpy() for k, v in mcts.root_edges(value=False).items()}
    return np.array([fixture_action(b, root["n"][b], root["child"][b] >= 0) for b in range(mcts.n)], np.int16)


def test_advance_matches_model():
    """The shared fixture: 130 boards searched for 32 simulations, each plays
    its fixture move, advance(): info and stats() match the rule applied by
    the model to the exported tree (dropped boards: zeros), and after
    search(carry=True, sims=0) the exported tree equals the model's carried
    tree on every board (a dropped board: the fresh root alone)."""
    from hzamd.mcts import BatchedMCTS
    F = FIXTURE
    n, sims = F["n"], F["sims"]
    env = make_env(fixture_positions())
    max_nodes = 2 * (1 + 69 * sims)
    mcts = BatchedMCTS(env, sims, max_nodes=max_nodes)
    ev = evaluator_of(F["evaluator"])
    mcts.search(ev, F["cpuct"])
    before = [mcts.export_tree(b) for b in range(n)]
    gen0 = mcts.stats()[:, 2].cpu().numpy().copy()
    act = fixture_moves(mcts)
    assert (act >= 0).all()
    status = env.step(torch.from_numpy(act).to(DEV))
    assert (status == 0).all()
    words = env.export_state().cpu().numpy().view(np.uint64)
    info = {k: v.cpu().numpy().copy() for k, v in mcts.advance(torch.from_numpy(act)).items()}
    counts = mcts.stats().cpu().numpy().copy()
    want = [carry_tree(before[b], int(act[b]), words[:, b], 69 * sims, max_nodes) for b in range(n)]
    carried = np.array([w[0] is not None for w in want])
    assert 20 <= carried.sum() <= 125 and carried[list(SPECIAL)].any() and not carried[list(SPECIAL)].all()
    for b in range(n):
        assert (info["nodes"][b], info["edges"][b], info["visits"][b]) == want[b][1], b
        assert tuple(counts[b, :2]) == want[b][1][:2], b
        assert counts[b, 2] == gen0[b] + carried[b] and (not carried[b] or counts[b, 3] == 0), b
    mcts.count_edges = mcts.count_path = True
    made, walked = int(mcts.edges_total.item()), int(mcts.path_total.item())
    visits = mcts.search(ev, F["cpuct"], carry=True, sims=0).cpu().numpy()
    # count_edges / count_path: only the edges a search creates and the levels it walks, and this one did neither
    assert int(mcts.edges_total.item()) == made and int(mcts.path_total.item()) == walked
    counts = mcts.stats().cpu().numpy().copy()
    for b in range(n):
        after = mcts.export_tree(b)
        if carried[b]:
            assert same_tree(after, want[b][0]), b
            assert visits[b].sum() == want[b][1][2], b
        else:
            assert tuple(counts[b, :2]) == (1, 0) and same(after["state"][0], words[:, b]) and visits[b].sum() == 0, b
    mcts.close()
    env.close()


PLIES, PLAY_SIMS = 12, 24


@functools.lru_cache(maxsize=None)
def modelled_play(evaluator, noisy):
    """The CHECK boards played by the model for PLIES plies, a carry after
    each: per ply and board (visits, root W bits, root P bits, counts, the
    move, the stream's next word after step)."""
    F = FIXTURE
    pos = [fixture_positions()[b] for b in CHECK]
    ms = models(pos, evaluator, max_nodes=3 * (1 + 69 * PLAY_SIMS))
    out = []
    for ply in range(PLIES):
        row = []
        for b, m in zip(CHECK, ms):
            if game_over(m.env):  # (no CHECK board's game ends within the plies; the device leaves such a board out)
                row.append(None)
                continue
            noise = play_noise(b, ply)
            m.begin(noise, F["eps"], noisy)
            m.search(PLAY_SIMS, F["cpuct"], noise, F["eps"], noisy)
            v = m.visits()
            t = m.export(words=False)
            r = slice(int(t["e0"][0]), int(t["e0"][0]) + max(int(t["ne"][0]), 0))
            w, p = np.zeros(143), np.zeros(143, np.float32)
            w[t["action"][r]], p[t["action"][r]] = t["w"][r], t["p"][r]
            a = choose(v, False, 0.0)
            m.play(a)
            info = m.advance(a, 69 * PLAY_SIMS)
            row.append((v, w, p, m_counts(t), a, next_word(m.mt), info))
        out.append(row)
    return out


def m_counts(t):
    return (len(t["e0"]), len(t["n"]))


def play_noise(board, ply):
    return np.random.default_rng(100000 * ply + board).dirichlet([0.4] * 69)


@pytest.mark.parametrize("form", ["small_batch", "fused_select_gather", "graph"])
@pytest.mark.parametrize("evaluator", [0, 1], ids=["stub", "dense"])
@pytest.mark.parametrize("noisy", [False, True], ids=["testing", "noisy"])
def test_continued_search_matches_model(form, evaluator, noisy):
    """Twelve plies with a carry after each under search(carry=True): after
    every move the visits, the root edges' W and P bits, the node and edge
    counts, advance's info and the env's next MT word equal the model's, on
    the CHECK boards (lanes 0, 63, 64 and 129 of a 130-board batch among them;
    the small-batch form runs the same sixteen boards as a batch of their own)."""
    from hzamd.mcts import BatchedMCTS, choose_actions
    F = FIXTURE
    want = modelled_play(evaluator, noisy)
    small = form == "small_batch"
    ids = list(CHECK) if small else list(range(F["n"]))
    env = make_env([fixture_positions()[b] for b in ids])
    n = env.n
    mcts = BatchedMCTS(env, PLAY_SIMS, max_nodes=3 * (1 + 69 * PLAY_SIMS))
    opts = {"graph": True} if form == "graph" else {}
    ev = evaluator_of(evaluator, device_rows=form == "graph")
    rows = [ids.index(b) for b in CHECK]
    greedy = torch.zeros(n, dtype=torch.bool)
    for ply in range(PLIES):
        noise = torch.from_numpy(np.stack([play_noise(b, ply) for b in ids]))
        active = ~env.done()
        visits = mcts.search(ev, F["cpuct"], active=active, noise=noise, eps=F["eps"], testing=not noisy, carry=True,
                             **opts)
        root = {k: v.cpu().numpy() for k, v in mcts.root_edges(value=False).items()}
        counts = mcts.stats().cpu().numpy().copy()
        act = choose_actions(visits.cpu(), greedy, torch.zeros(n, dtype=torch.float64)).to(torch.int16)
        status = env.step(act.to(DEV))
        info = {k: v.cpu().numpy().copy() for k, v in mcts.advance(act, active).items()}
        nxt = streams(env)
        v = visits.cpu().numpy()
        assert all(w is not None for w in want[ply])
        for j, (wv, ww, wp, wc, wa, wn, wi) in zip(rows, want[ply]):
            assert same(v[j], wv), (ply, j)
            assert same(root["w"][j], ww) and same(root["p"][j], wp), (ply, j)
            assert tuple(counts[j, :2]) == wc and counts[j, 3] == 0, (ply, j)
            assert int(act[j]) == wa and int(status[j]) == 0, (ply, j)
            assert (info["nodes"][j], info["edges"][j], info["visits"][j]) == wi, (ply, j)
            assert nxt[j] == wn, (ply, j)
    assert sum(w[6][2] > 0 for row in want for w in row) > PLIES * 4  # the plies did carry
    mcts.close()
    env.close()


def searched_and_advanced(max_nodes=None, headroom=None, evaluator=None, model_cap=None):
    """The fixture after its first search, move and advance: (env, mcts,
    models, moves, info)."""
    from hzamd.mcts import BatchedMCTS
    F = FIXTURE
    evaluator = F["evaluator"] if evaluator is None else evaluator
    pos = fixture_positions()
    env = make_env(pos)
    mcts = BatchedMCTS(env, F["sims"], max_nodes=2 * (1 + 69 * F["sims"]) if max_nodes is None else max_nodes)
    ms = models(pos, evaluator, max_nodes=model_cap)
    v0 = mcts.search(evaluator_of(evaluator), F["cpuct"]).cpu().numpy().copy()
    act = fixture_moves(mcts)
    env.step(torch.from_numpy(act).to(DEV))
    head = 69 * F["sims"] if headroom is None else headroom
    info = {k: v.cpu().numpy().copy() for k, v in mcts.advance(torch.from_numpy(act), headroom=headroom).items()}
    for b, m in enumerate(ms):
        m.begin()
        m.search(F["sims"], F["cpuct"])
        assert same(m.visits(), v0[b]), b
        m.play(int(act[b]))
        got = m.advance(int(act[b]), head)
        assert got == (info["nodes"][b], info["edges"][b], info["visits"][b]), b
    return env, mcts, ms, act, info


def test_carry_with_noise_mask_and_budget():
    """search(carry=True) with a per-board root_noise mask and budget=: masked
    boards are not mixed (the root priors' bits), sims_done() counts the new
    simulations only, and visits, counts and streams equal the model's."""
    F = FIXTURE
    env, mcts, ms, act, info = searched_and_advanced()
    n = env.n
    mask = np.arange(n) % 2 == 0
    budget = np.array([5, 11, F["sims"] + 7])[np.arange(n) % 3].astype(np.int32)
    noise = np.stack([play_noise(b, 1) for b in range(n)])
    visits = mcts.search(evaluator_of(F["evaluator"]), F["cpuct"], noise=torch.from_numpy(noise), eps=F["eps"],
                         testing=False, budget=torch.from_numpy(budget), root_noise=torch.from_numpy(mask),
                         carry=True).cpu().numpy()
    done = mcts.sims_done().cpu().numpy()
    root = {k: v.cpu().numpy() for k, v in mcts.root_edges(value=False).items()}
    counts = mcts.stats().cpu().numpy()
    nxt = streams(env)
    mixed = 0
    for b, m in enumerate(ms):
        k = min(int(budget[b]), F["sims"])
        assert done[b] == k, b
        before = list(m.E["p"]) if m.carried and m.tree else None
        kept = m.begin(noise[b], F["eps"], bool(mask[b]))
        if kept and before is not None and m.ne[0] > 0:
            changed = before[:len(m.E["p"])] != m.E["p"]
            assert changed == bool(mask[b]), b
            mixed += changed
        m.search(k, F["cpuct"], noise[b], F["eps"], bool(mask[b]))
        t = m.export(words=False)
        r = slice(int(t["e0"][0]), int(t["e0"][0]) + max(int(t["ne"][0]), 0))
        p = np.zeros(143, np.float32)
        p[t["action"][r]] = t["p"][r]
        assert same(visits[b], m.visits()) and same(root["p"][b], p), b
        assert tuple(counts[b, :2]) == m.counts() and counts[b, 3] == 0, b
        assert visits[b].sum() <= info["visits"][b] + k, b
        assert nxt[b] == next_word(m.mt), b
    assert mixed >= 10
    mcts.close()
    env.close()


def test_headroom_drops_what_does_not_fit():
    """max_nodes at the default of a fresh search and a headroom that leaves
    200 nodes: the boards whose kept tree is larger are dropped (advance's
    info equals the model's under the same rule), some are and some are not,
    and the next search, of as many simulations as the headroom covers, flags
    no board."""
    F = FIXTURE
    max_nodes = 1 + 69 * F["sims"]
    headroom = max_nodes - 200
    env, mcts, ms, act, info = searched_and_advanced(max_nodes=max_nodes, headroom=headroom, model_cap=max_nodes)
    fits = np.array([m.carried for m in ms])
    big = 0
    for b, m in enumerate(ms):
        if not m.carried:
            ref = CarryModel(fixture_positions()[b][0], copy_mt(fixture_positions()[b][1]), F["evaluator"])
            ref.begin()
            ref.search(F["sims"], F["cpuct"])
            ref.play(int(act[b]))
            big += ref.advance(int(act[b]), 0)[0] > 200
    assert big >= 3 and fits.sum() >= 10
    assert ((info["nodes"] > 0) == fits).all() and info["nodes"].max() <= 200 and info["edges"].max() <= 200
    sims = headroom // 69
    mcts.search(evaluator_of(F["evaluator"]), F["cpuct"], sims=sims, carry=True)
    counts = mcts.stats().cpu().numpy()
    assert (mcts.limit_flags().cpu().numpy() == 0).all()
    for b, m in enumerate(ms):
        m.begin()
        m.search(sims, F["cpuct"])
        assert tuple(counts[b, :2]) == m.counts() and m.flag == 0, b
    mcts.close()
    env.close()


def test_headroom_zero_in_a_tight_pool_flags_as_documented():
    """headroom=0 and max_nodes = 400: every kept tree that fits at all is
    carried, and the next search refuses the expansions that do not fit: the
    limit flag, visits and counts equal the model's under the same limit
    (hz_mcts_create, "Limits"), some boards are flagged, and the report stays
    inside the board's counts."""
    F = FIXTURE
    cap = 400
    env, mcts, ms, act, info = searched_and_advanced(max_nodes=cap, headroom=0, model_cap=cap)
    assert mcts.bounded
    visits = mcts.search(evaluator_of(F["evaluator"]), F["cpuct"], carry=True).cpu().numpy()
    counts = mcts.stats().cpu().numpy().copy()
    flags = mcts.limit_flags().cpu().numpy().copy()
    root = {k: v.cpu().numpy() for k, v in mcts.root_edges().items()}
    pv = {k: v.cpu().numpy() for k, v in mcts.principal_variation(16).items()}
    nxt = streams(env)
    for b, m in enumerate(ms):
        m.begin()
        m.search(F["sims"], F["cpuct"])
        assert same(visits[b], m.visits()) and tuple(counts[b, :2]) == m.counts() and flags[b] == m.flag, b
        assert nxt[b] == next_word(m.mt), b
        assert counts[b, 0] <= cap and counts[b, 1] <= cap, b
        kids = root["child"][b][root["child"][b] >= 0]
        assert (kids < counts[b, 0]).all() and same(root["n"][b], visits[b]), b
        assert 0 <= pv["len"][b] <= 16, b
        t = mcts.export_tree(b) if b in SPECIAL or flags[b] else None
        if t is not None:
            assert (t["child"] < counts[b, 0]).all() and (t["child"] >= 0).all(), b
            ex = t["ne"] > 0
            assert (t["e0"][ex] + t["ne"][ex] <= counts[b, 1]).all(), b
    assert 5 <= (flags != 0).sum() and (info["nodes"] > 0).sum() >= 20
    mcts.close()
    env.close()


def clone_env(env):
    from hzamd.env import BatchedEnv
    st, mt, idx = env.export_state(with_mt=True)
    twin = BatchedEnv(env.n, device=DEV)
    twin.import_state(st.clone(), mt.clone(), idx.clone())
    return twin


def search_record(mcts, env, **kw):
    F = FIXTURE
    v = mcts.search(evaluator_of(F["evaluator"]), F["cpuct"], **kw).cpu().numpy().copy()
    root = mcts.root_edges()
    return [v, mcts.stats()[:, :2].cpu().numpy().copy(), root["w"].cpu().numpy().copy(),
            root["p"].cpu().numpy().copy(), np.array(streams(env))]


def assert_same_records(a, b):
    for x, y in zip(a, b):
        assert same(x, y)


def test_carry_is_consumed():
    """A second search(carry=True) without an advance equals a fresh search;
    an import_state or a reset between advance and the search drops the carry;
    a plain search() after advance is the search of a handle that never
    advanced, bit for bit."""
    from hzamd.mcts import BatchedMCTS
    F = FIXTURE
    nodes = 2 * (1 + 69 * F["sims"])
    # (1) consumed by the first search(carry=True)
    env, mcts, ms, act, info = searched_and_advanced()
    first = search_record(mcts, env, carry=True)
    assert first[0].sum() > F["sims"] * env.n  # carried visits on top
    twin = clone_env(env)
    fresh = BatchedMCTS(twin, F["sims"], max_nodes=nodes)
    assert_same_records(search_record(mcts, env, carry=True), search_record(fresh, twin))
    # (2) a plain search after advance: the flags are cleared, nothing is kept
    env.step(torch.from_numpy(fixture_moves(mcts)).to(DEV))
    twin.step(torch.from_numpy(fixture_moves(fresh)).to(DEV))
    kept = mcts.advance(torch.from_numpy(fixture_moves(mcts)))["nodes"].cpu().numpy()
    assert (kept > 0).sum() >= 20
    assert_same_records(search_record(mcts, env), search_record(fresh, twin))
    assert_same_records(search_record(mcts, env, carry=True), search_record(fresh, twin))
    # (3) other states imported between advance and the search
    moves = torch.from_numpy(fixture_moves(mcts)).to(DEV)
    env.step(moves)
    assert (mcts.advance(moves)["nodes"] > 0).sum() >= 20
    st, mt, idx = env.export_state(with_mt=True)
    perm = torch.roll(torch.arange(env.n, device=DEV), 1)
    for e in (env, twin):
        e.import_state(st[:, perm].contiguous(), mt[perm].contiguous(), idx[perm].contiguous())
    assert_same_records(search_record(mcts, env, carry=True), search_record(fresh, twin))
    # (4) a reset
    moves = torch.from_numpy(fixture_moves(mcts)).to(DEV)
    env.step(moves)
    assert (mcts.advance(moves)["nodes"] > 0).sum() >= 20
    seeds = torch.arange(env.n, device=DEV, dtype=torch.int64) + 77
    env.reset(seeds=seeds)
    twin.reset(seeds=seeds)
    assert_same_records(search_record(mcts, env, carry=True), search_record(fresh, twin))
    for x in (mcts, fresh, env, twin):
        x.close()


SP_SIMS, SP_PLIES, SP_BASE = 24, 16, 52000


def self_play(n, base, **keys):
    from hzamd.mcts import dense_stub_evaluator
    from hzamd.selfplay import SelfPlay
    cfg = {"num_simulations": SP_SIMS, "cpuct": 1.25, "dirichlet_epsilon": 0.3, **keys}
    sp = SelfPlay(n, dense_stub_evaluator, cfg, seed_base=base, device=DEV, max_plies=SP_PLIES)
    sp.keep_noise = True
    rec = sp.play()
    out = {k: rec[k].cpu().numpy() for k in ("states", "visits", "valid") + (("carried",) if "carried" in rec else ())}
    log = [(a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()) for a, b, c in sp.noise_log]
    sp.mcts.close()
    sp.env.close()
    return out, log, sp


@pytest.mark.parametrize("mode", ["add", "topup"])
def test_self_play_tree_reuse_replayed_by_model(mode):
    """130 boards x 16 plies of self-play with tree_reuse: every move of every
    board is replayed by the model from the recorded carried visits, noise and
    budgets (visits, the carried visits, the move, the state); the records of
    a 65 + 65 split are those of the 130 boards."""
    n = 130
    keys = {"tree_reuse": mode, "tree_reuse_min_sims": 3}
    rec, log, sp = self_play(n, SP_BASE, **keys)
    assert rec["states"].shape[0] == SP_PLIES and rec["valid"].all()
    assert sp.mcts.max_nodes == 2 * (1 + 69 * SP_SIMS)
    cfg = sp.cfg
    total_carried = 0
    for b in range(n):
        mt = oracle.mt_seed(SP_BASE + b)
        m = CarryModel(oracle.reset(mt), mt, 1, max_nodes=sp.mcts.max_nodes)
        carried = 0
        for ply in range(SP_PLIES):
            noise, u, act = (x[b] for x in log[ply])
            assert same(unpack_ref(rec["states"][ply, :, b]), m.env), (b, ply)
            assert rec["carried"][ply, b] == carried, (b, ply)
            sims = SP_SIMS if mode == "add" else int(topup_budget(carried, SP_SIMS, 3))
            m.begin(noise, cfg["dirichlet_epsilon"], True)
            m.search(sims, cfg["cpuct"], noise, cfg["dirichlet_epsilon"], True)
            v = m.visits()
            assert same(rec["visits"][ply, b], v), (b, ply)
            a = choose(v, ply < cfg["turns_until_tau0"], u)
            assert a == act, (b, ply)
            m.play(a)
            carried = m.advance(a, 69 * SP_SIMS)[2]
            total_carried += carried > 0
    assert total_carried > n * SP_PLIES // 4
    halves = [self_play(65, SP_BASE + 65 * h, **keys)[0] for h in (0, 1)]
    for k, v in rec.items():
        assert same(v, np.concatenate([h[k] for h in halves], axis=-1 if k == "states" else 1)), k


def test_self_play_without_the_keys_is_unchanged():
    """With the tree_reuse keys absent a second SelfPlay, even one whose
    handle has been given an advance(), records what an untouched one records; tree_reuse with playout caps,
    or an unknown mode, raises."""
    from hzamd.mcts import dense_stub_evaluator
    from hzamd.selfplay import SelfPlay
    plain, _, _ = self_play(130, SP_BASE)
    assert "carried" not in plain
    cfg = {"num_simulations": SP_SIMS, "cpuct": 1.25, "dirichlet_epsilon": 0.3}
    sp = SelfPlay(130, dense_stub_evaluator, cfg, seed_base=SP_BASE, device=DEV, max_plies=SP_PLIES)
    # the handle has advanced (its carry flags and scratch exist); the keys stay absent
    sp.mcts.advance(torch.zeros(130, dtype=torch.int16), headroom=0)
    rec = sp.play()
    for k in ("states", "visits", "valid"):
        assert same(rec[k].cpu().numpy(), plain[k]), k
    for bad in ({"tree_reuse": "add", "playout_cap_p": 0.25, "playout_cap_fast": 8}, {"tree_reuse": "keep"}):
        with pytest.raises(ValueError):
            SelfPlay(4, dense_stub_evaluator, dict(cfg, **bad), seed_base=1, device=DEV)
    sp.mcts.close()
    sp.env.close()
