"""Forced playouts and policy target pruning on the GPU (hz_mcts_set_forced,
hz_mcts_pruned_visits, hz_mcts_forced_counts, BatchedMCTS.search(forced=),
SelfPlay's forced_playouts) against the host model tests/mcts_forced_model.py.
Everything is compared exactly: integers as they are, floats by their bits;
every operation of the two rules is one correctly rounded IEEE operation on
both sides.  tests/test_mcts_forced_cpu.py shows that the fixture holds the
cases these tests rely on (CASES there names the boards)."""
import numpy as np
import pytest
import torch

import oracle
from hzamd.state import pack_ref, unpack_ref, words_to_array
from mcts_carry_model import choose, copy_mt, next_word
from mcts_forced_model import FIXTURE, SMALL, ForcedModel, ForcedRule, fixture_noise, fixture_positions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TREE_KEYS = ("state", "e0", "ne", "action", "child", "n", "w", "p", "player")
TREES = (0, 1, 2, 5, 63, 64, 124, 128, 129)  # the boards whose whole tree is compared (every board of the small batch)
# k_select + the gather launch; the select inside the expansion; ... with the gather too; the captured simulation
FORMS = ("layered", "fused_select", "fused_select_gather", "graph")
K, K_LARGE = FIXTURE["k"], FIXTURE["k_large"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.dtype == b.dtype and a.shape == b.shape and bool((bits(a) == bits(b)).all())
    return a.shape == b.shape and bool((a == b).all())


_FIX = {}


def fixture(n=None):
    """(positions, noise f64 [n, 69]) of the first n fixture boards."""
    if not _FIX:
        pos = fixture_positions()
        _FIX["pos"] = pos
        _FIX["noise"] = fixture_noise(len(pos), [int(oracle.legal(st).sum()) for st, _ in pos])
    return list(_FIX["pos"][:n]), _FIX["noise"][:n]


def load_positions(env, pos):
    words = words_to_array([pack_ref(st) for st, _ in pos])
    mts = np.stack([m.words()[0] for _, m in pos])
    idx = np.array([m.words()[1] for _, m in pos], np.int32)
    env.import_state(torch.from_numpy(np.ascontiguousarray(words.T)), torch.from_numpy(mts.view(np.int32)),
                     torch.from_numpy(idx))


def make_env(pos):
    from hzamd.env import BatchedEnv
    env = BatchedEnv(len(pos), device=DEV)
    load_positions(env, pos)
    return env


def streams(env):
    _, mt, idx = env.export_state(with_mt=True)
    mt, idx = mt.cpu().numpy().view(np.uint32), idx.cpu().numpy()
    return [oracle.mt_next32(oracle.mt_from_words(mt[b], idx[b])) for b in range(env.n)]


class _DenseRows:
    """The dense stub on the device-row protocol (capturable; the captured simulation is kept between searches)."""
    device_rows = capturable = row_independent = True

    def __init__(self):
        self.graph_key = (self, 0)

    def __call__(self, board, glob, rows=None, count=None):
        from hzamd.mcts import dense_stub_evaluator
        return dense_stub_evaluator(board, glob)


ROWS = _DenseRows()


def make_mcts(env, form):
    from hzamd.mcts import BatchedMCTS
    mcts = BatchedMCTS(env, FIXTURE["sims"])
    mcts.fuse_select = form != "layered"
    mcts.fuse_gather = form in ("fused_select_gather", "graph")
    return mcts


def collect(mcts, env, visits, forced):
    F = FIXTURE
    out = {"visits": visits.cpu().numpy().copy(), "counts": mcts.stats().cpu().numpy().copy(), "next": streams(env),
           "trees": {b: mcts.export_tree(b) for b in (range(env.n) if env.n <= SMALL else TREES)}}
    if forced:
        out["pruned"] = mcts.pruned_visits(F["cpuct"]).cpu().numpy().copy()
        out["fcounts"] = mcts.forced_counts().cpu().numpy().copy()
    return out


def run_search(pos, noise, form, forced=True, k=K, evaluator=None, **opts):
    """One noisy search of the boards `pos`; everything the tests compare, on the host."""
    from hzamd.mcts import dense_stub_evaluator
    F = FIXTURE
    env = make_env(pos)
    mcts = make_mcts(env, form)
    if evaluator is None:
        evaluator = ROWS if form == "graph" or "max_rows" in opts else dense_stub_evaluator
    if forced is not None:
        opts.update(forced=forced, forced_k=k)
    visits = mcts.search(evaluator, F["cpuct"], noise=torch.from_numpy(noise), eps=F["eps"], testing=False,
                         graph=form == "graph", **opts)
    out = collect(mcts, env, visits, forced is not None)
    mcts.close()
    env.close()
    return out


_MODELS = {}


def modelled(name, k=K, active=None, budget=None, mask=None, cls=ForcedModel, evaluator=None, keys=None):
    """The model's search of every fixture board, kept by name.  mask: the
    boards that are noisy and forced (None: all); k None: no board is forced."""
    F = FIXTURE
    if name in _MODELS:
        return _MODELS[name]
    pos, noise = fixture()
    out = []
    for b, (st, m) in enumerate(pos):
        if active is not None and not active[b]:
            out.append(None)
            continue
        on = mask is None or bool(mask[b])
        kw = {} if keys is None else {"key": keys[b]}
        model = cls(st, copy_mt(m), F["evaluator"] if evaluator is None else evaluator, **kw)
        model.set_forced(k if on and k is not None else None)
        model.begin(carry=False)
        sims = F["sims"] if budget is None else min(int(budget[b]), F["sims"])
        model.search(sims, F["cpuct"], noise=noise[b], eps=F["eps"], noisy=on)
        out.append(model)
    _MODELS[name] = out
    return out


def assert_matches_model(dev, models):
    F = FIXTURE
    for b, model in enumerate(models):
        if model is None:  # left out of the search
            assert dev["visits"][b].sum() == 0 and tuple(dev["counts"][b, :2]) == (0, 0), b
            assert dev["pruned"][b].sum() == 0 and tuple(dev["fcounts"][b]) == (0, 0), b
            continue
        assert same(dev["visits"][b], model.visits()), b
        assert tuple(dev["counts"][b, :2]) == model.counts() and dev["counts"][b, 3] == 0, b
        assert dev["next"][b] == next_word(model.mt), b
        assert same(dev["pruned"][b], model.pruned(F["cpuct"])), b
        assert tuple(dev["fcounts"][b]) == (len(model.log), sum(bool(f) for f, _, _, _ in model.log)), b
    for b, tree in dev["trees"].items():
        if b < len(models) and models[b] is not None:
            want = models[b].export()
            assert all(same(tree[k], want[k]) for k in TREE_KEYS), b


def assert_same_search(a, b, boards=None):
    rows = list(range(len(a["next"]))) if boards is None else list(boards)
    assert same(a["visits"][rows], b["visits"][rows]) and same(a["counts"][rows][:, :2], b["counts"][rows][:, :2])
    assert all(a["next"][i] == b["next"][i] for i in rows)
    for t in a["trees"]:
        if boards is None or t in boards:
            assert all(same(a["trees"][t][k], b["trees"][t][k]) for k in TREE_KEYS), t


# --------------------------------------------------------------------- search
@pytest.mark.parametrize("form,n,k", [(f, FIXTURE["n"], K) for f in FORMS] +
                         [("layered", SMALL, K), ("graph", SMALL, K), ("fused_select_gather", FIXTURE["n"], K_LARGE),
                          ("layered", FIXTURE["n"], K_LARGE), ("layered", SMALL, K_LARGE)])
def test_search_matches_model(form, n, k):
    pos, noise = fixture(n)
    dev = run_search(pos, noise, form, k=k)
    models = modelled(f"k{k}", k=k)[:n]
    assert_matches_model(dev, models)
    plain = modelled("plain", k=None)[:n]
    # (the gate matters: most boards' visits differ from the search without it, and pruning took visits back)
    assert sum(not same(a.visits(), p.visits()) for a, p in zip(models, plain)) >= n // 2
    assert dev["pruned"].sum() < dev["visits"].sum() and dev["fcounts"][:, 1].sum() > 0


@pytest.mark.parametrize("form", FORMS)
def test_search_with_boards_left_out(form):
    pos, noise = fixture()
    active = np.arange(len(pos)) % 3 != 2
    dev = run_search(pos, noise, form, active=torch.from_numpy(active.astype(np.uint8)))
    assert_matches_model(dev, [m if active[b] else None for b, m in enumerate(modelled(f"k{K}"))])


@pytest.mark.parametrize("form", FORMS)
def test_search_with_budgets_and_one_mask_for_noise_and_forcing(form):
    """Per-board budgets, and a root_noise mask that is the forced mask too:
    a board whose bit is clear searches without noise and without forcing."""
    F = FIXTURE
    pos, noise = fixture()
    budget = (1 + (np.arange(len(pos)) * 7) % (F["sims"] + 4)).astype(np.int32)
    mask = np.arange(len(pos)) % 4 != 1
    tmask = torch.from_numpy(mask)
    dev = run_search(pos, noise, form, forced=tmask, budget=torch.from_numpy(budget), root_noise=tmask)
    assert_matches_model(dev, modelled("budget_mask", budget=budget, mask=mask))
    clear = np.flatnonzero(~mask)
    assert same(dev["pruned"][clear], dev["visits"][clear]) and not dev["fcounts"][clear].any()


@pytest.mark.parametrize("form", ("fused_select_gather", "graph"))
def test_search_under_max_rows(form):
    pos, noise = fixture()
    active = np.arange(len(pos)) % 5 != 3
    dev = run_search(pos, noise, form, active=torch.from_numpy(active.astype(np.uint8)), max_rows=int(active.sum()))
    assert_matches_model(dev, [m if active[b] else None for b, m in enumerate(modelled(f"k{K}"))])


@pytest.mark.parametrize("form,n", [(f, FIXTURE["n"]) for f in FORMS] + [("layered", SMALL), ("graph", SMALL)])
def test_boards_with_a_clear_bit_equal_the_plain_search(form, n):
    pos, noise = fixture(n)
    mask = np.arange(n) % 2 == 0
    gated = run_search(pos, noise, form, forced=torch.from_numpy(mask.astype(np.uint8)))
    plain = run_search(pos, noise, form, forced=None)
    clear = [int(b) for b in np.flatnonzero(~mask)]
    assert_same_search(gated, plain, clear)
    assert same(gated["pruned"][clear], plain["visits"][clear])
    models = modelled(f"k{K}")[:n]
    for b in np.flatnonzero(mask):
        assert same(gated["visits"][b], models[b].visits()) and same(gated["pruned"][b],
                                                                     models[b].pruned(FIXTURE["cpuct"])), b


# ------------------------------------------------------------ leaf symmetries
def leafsym_parts():
    from mcts_leafsym_model import CELL_STUB, KEYS, ORBIT_STUB, LeafSymModel, host_keys

    class ForcedLeafSymModel(ForcedRule, LeafSymModel):
        pass
    return CELL_STUB, ORBIT_STUB, KEYS, ForcedLeafSymModel, host_keys


def draw_keys(n):
    from hzamd.selfplay import NoiseSource
    from mcts_leafsym_model import KEYS
    return NoiseSource(KEYS["board_base"], DEV, seed=KEYS["seed"]).leaf_symmetry(KEYS["move"], n)


@pytest.mark.parametrize("form,n", [(f, FIXTURE["n"]) for f in FORMS] + [("layered", SMALL), ("graph", SMALL)])
def test_forced_with_leaf_symmetries(form, n):
    """Under the orbit stub (equivariant) the keys change nothing in a forced
    search; under the cell stub the search is the model's with both rules."""
    cell, orbit, KEYS, Model, host_keys = leafsym_parts()
    pos, noise = fixture(n)
    keyed = run_search(pos, noise, form, evaluator=orbit, leaf_symmetry=draw_keys(n))
    unkeyed = run_search(pos, noise, form, evaluator=orbit)
    assert_same_search(keyed, unkeyed)
    assert same(keyed["pruned"], unkeyed["pruned"]) and same(keyed["fcounts"], unkeyed["fcounts"])
    assert keyed["fcounts"][:, 1].sum() > 0
    dev = run_search(pos, noise, form, evaluator=cell, leaf_symmetry=draw_keys(n))
    models = modelled("cell_keyed", cls=Model, evaluator="cell", keys=host_keys(FIXTURE["n"], **KEYS))[:n]
    assert_matches_model(dev, models)
    assert sum(any(g != 0 for _, g, _ in m.evaluated) for m in models) >= n // 2


# ----------------------------------------------------------------------- gate
def test_gate_clears_and_captures_are_not_reused():
    """One handle, captured simulations kept between searches: forced (k), plain,
    forced again, forced with a mask at the same k, with another mask, forced
    on every board again, forced with another k, plain eagerly.  Every search
    is its model's, so no capture made under one gate, k or kind of mask (a
    capture holds by value whether there is one) is replayed under another,
    while a capture made with a mask serves another mask's contents; a plain
    search after a forced one is the search of a handle that never forced; and
    pruned_visits() refuses once the gate is off."""
    F = FIXTURE
    pos, noise = fixture()
    env = make_env(pos)
    mcts = make_mcts(env, "graph")
    tn = torch.from_numpy(noise)
    plain = modelled("plain", k=None)
    every = modelled(f"k{K}")
    even = np.arange(len(pos)) % 2 == 0

    def masked(mask):  # noise on every board, the rule on the mask's boards
        return [every[b] if mask[b] else plain[b] for b in range(len(pos))]

    def run(graph=True, **opts):
        load_positions(env, pos)
        visits = mcts.search(ROWS, F["cpuct"], noise=tn, eps=F["eps"], testing=False, graph=graph, **opts)
        return collect(mcts, env, visits, "forced" in opts)

    def is_plain(res):
        assert all(same(res["visits"][b], m.visits()) and tuple(res["counts"][b, :2]) == m.counts() and
                   res["next"][b] == next_word(m.mt) for b, m in enumerate(plain))
    assert_matches_model(run(forced=True, forced_k=K), every)
    kept = mcts._graph_cache
    assert kept is not None and kept[0][-1][4] == (K, False)
    is_plain(run())
    assert mcts._graph_cache is not kept and mcts._graph_cache[0][-1][4] is None
    with pytest.raises(ValueError):
        mcts.pruned_visits(F["cpuct"])
    with pytest.raises(ValueError):
        mcts.forced_counts()
    assert_matches_model(run(forced=True, forced_k=K), every)
    kept = mcts._graph_cache
    # the same k with a mask: another capture (the one above reads no mask) ...
    res = run(forced=torch.from_numpy(even), forced_k=K)
    assert_matches_model(res, masked(even))
    assert sum(not same(res["visits"][b], every[b].visits()) for b in np.flatnonzero(~even)) >= len(pos) // 4
    assert mcts._graph_cache is not kept and mcts._graph_cache[0][-1][4] == (K, True)
    kept = mcts._graph_cache
    # ... which serves another mask, whose contents it reads from the handle's buffer ...
    assert_matches_model(run(forced=torch.from_numpy((~even).astype(np.uint8)), forced_k=K), masked(~even))
    assert mcts._graph_cache is kept
    # ... and is not replayed once there is no mask again
    assert_matches_model(run(forced=True, forced_k=K), every)
    assert mcts._graph_cache is not kept and mcts._graph_cache[0][-1][4] == (K, False)
    kept = mcts._graph_cache
    assert_matches_model(run(forced=True, forced_k=K_LARGE), modelled(f"k{K_LARGE}", k=K_LARGE))
    assert mcts._graph_cache is not kept and mcts._graph_cache[0][-1][4] == (K_LARGE, False)
    is_plain(run(graph=False))
    is_plain(run())
    mcts.close()
    env.close()


def test_refusals():
    import hzamd._native as nat
    from hzamd.mcts import dense_stub_evaluator
    from hzamd.selfplay import NoiseSource
    pos, _ = fixture(SMALL)
    env = make_env(pos)
    mcts = make_mcts(env, "layered")
    g = NoiseSource(0, DEV).gumbel(0, env.n)
    ok = torch.ones(env.n, dtype=torch.uint8)
    for opts in ({"root": "gumbel", "gumbel": g, "forced": True}, {"carry": True, "forced": True},
                 {"forced": ok[:-1]}, {"forced": ok.to(torch.float32)}, {"forced": True, "forced_k": 0.0},
                 {"forced": True, "forced_k": -2.0}, {"forced": True, "forced_k": float("nan")}, {"forced_k": 2.0}):
        with pytest.raises(ValueError):
            mcts.search(dense_stub_evaluator, 1.25, **opts)
    with pytest.raises(ValueError):
        mcts.pruned_visits(1.25)
    # the ABI itself
    L, h = nat.lib(), mcts._h
    out = torch.zeros(env.n, 143, dtype=torch.int32, device=DEV)
    assert L.hz_mcts_set_forced(h, None, -1.0) == -1 and L.hz_mcts_set_forced(h, None, float("nan")) == -1
    assert L.hz_mcts_set_forced(None, None, 2.0) == -1
    assert L.hz_mcts_set_forced(h, None, 0.0) == 0
    assert L.hz_mcts_pruned_visits(h, 1.25, nat.ptr(out)) == -1  # the gate is off
    assert L.hz_mcts_forced_counts(h, nat.ptr(out)) == -1
    assert L.hz_mcts_set_forced(h, None, 2.0) == 0
    assert L.hz_mcts_pruned_visits(h, 1.25, None) == -1
    # with the Gumbel root on as well, nothing that selects or expands is enqueued
    table = mcts._set_gumbel(g, 8, None, None, None)
    assert table is not None
    mcts.begin()
    pol = torch.zeros(env.n, 143, device=DEV)
    val = torch.zeros(env.n, device=DEV)
    assert L.hz_mcts_select(h, None, 1.25) == -1
    assert L.hz_mcts_select_gather(h, None, 1.25, nat.ptr(mcts.board), nat.ptr(mcts.glob), nat.ptr(mcts.rows),
                                   nat.ptr(mcts.count)) == -1
    assert L.hz_mcts_expand_backup(h, env.handle, nat.ptr(pol), nat.ptr(val), None, 0.25, 1) == -1
    assert L.hz_mcts_expand_backup_select(h, env.handle, nat.ptr(pol), nat.ptr(val), None, 0.25, 1, None, 1.25) == -1
    mcts._set_gumbel(None, 8, None, None, None)
    # a carried tree: hz_mcts_begin_carried refuses while the gate is on, and serves once it is off
    assert L.hz_mcts_begin_carried(h, env.handle, None, None, 0.25, 1) == -1
    assert L.hz_mcts_set_forced(h, None, 0.0) == 0
    assert L.hz_mcts_begin_carried(h, env.handle, None, None, 0.25, 1) == 0
    torch.cuda.synchronize()
    mcts.close()
    env.close()


@pytest.mark.parametrize("form", ("layered", "fused_select_gather"))
def test_pruned_visits_without_a_tree_and_on_a_stuck_root(form):
    """Board 0 is left out by `active`, 63 is a stuck root (no legal move, game
    not over): zero rows for both; their neighbours are the model's."""
    F = FIXTURE
    pos, noise = fixture()
    left_out, stuck = 0, 63
    pos[stuck] = oracle.stuck_state(915 + stuck)
    assert not oracle.legal(pos[stuck][0]).any()
    active = np.ones(len(pos), np.uint8)
    active[left_out] = 0
    dev = run_search(pos, noise, form, active=torch.from_numpy(active))
    assert tuple(dev["counts"][left_out, :2]) == (0, 0) and tuple(dev["counts"][stuck, :2]) == (1, 0)
    for b in (left_out, stuck):
        assert not dev["visits"][b].any() and not dev["pruned"][b].any() and not dev["fcounts"][b].any(), b
    models = modelled(f"k{K}")
    for b in (1, 2, 62, 64, 129):
        assert same(dev["visits"][b], models[b].visits()) and same(dev["pruned"][b], models[b].pruned(F["cpuct"])), b
    assert (dev["pruned"] <= dev["visits"]).all()
    assert (dev["pruned"].argmax(1) == dev["visits"].argmax(1)).all()


# ------------------------------------------------------------------ self-play
SP = {"n": 16, "base": 3700, "plies": 4, "sims": 12, "fast": 4, "p": 0.5, "cpuct": 1.5, "eps": 0.25}


def sp_config(**more):
    return dict({"num_simulations": SP["sims"], "cpuct": SP["cpuct"], "testing": False, "playout_cap_p": SP["p"],
                 "playout_cap_fast": SP["fast"], "forced_playouts": K}, **more)


def test_self_play_records_pruned_visits_and_moves_from_raw_ones():
    """A few plies with playout caps on, replayed on the host: a full board's
    search is the model's forced, noisy search and its record the model's
    pruned visits; a fast board's is the plain search and its raw visits; every
    move is chosen from the raw visits."""
    from hzamd.selfplay import SelfPlay
    n, base, plies = SP["n"], SP["base"], SP["plies"]
    sp = SelfPlay(n, ROWS, sp_config(), seed_base=base, device=DEV)
    sp.keep_noise = True
    sp.env.reset()
    states, recorded, raw, full = [], [], [], []
    for ply in range(plies):  # (the visits are the handle's own tensors, rewritten by the next search)
        st, v, _ = sp.move(ply)
        states.append(st.cpu().numpy().copy())
        recorded.append(v.cpu().numpy().copy())
        raw.append(sp.last_visits.cpu().numpy().copy())
        full.append(sp.last_full.cpu().numpy().copy())
    sp.check_steps()
    log = [[t.cpu().numpy() for t in entry] for entry in sp.noise_log]
    final = sp.env.export_state().cpu().numpy()
    full = np.stack(full)
    assert full.any() and not full.all()
    pruned_away = 0
    for b in range(n):
        m = oracle.mt_seed(base + b)
        s = oracle.reset(m)
        for ply in range(plies):
            assert (unpack_ref(states[ply][:, b]) == s).all(), (b, ply)
            noise, u, act = log[ply]
            f = bool(full[ply, b])
            model = ForcedModel(s, m, 1, k=K if f else None)
            model.begin(carry=False)
            model.search(SP["sims"] if f else SP["fast"], SP["cpuct"], noise=noise[b], eps=SP["eps"], noisy=f)
            assert same(raw[ply][b], model.visits()), (b, ply)
            assert same(recorded[ply][b], model.pruned(SP["cpuct"])), (b, ply)
            if not f:
                assert same(recorded[ply][b], raw[ply][b]), (b, ply)
            pruned_away += int(raw[ply][b].sum() - recorded[ply][b].sum())
            a = choose(model.visits(), True, u[b])
            assert a == act[b], (b, ply)
            s = model.play(a)
        assert (unpack_ref(final[:, b]) == s).all(), b
    assert pruned_away > 0


def test_self_play_options():
    """prune_targets False keeps the raw visits in the records; testing turns
    the gate off; without the key the handle never sees the gate."""
    from hzamd.selfplay import SelfPlay
    n, base = SP["n"], SP["base"]

    def first_move(cfg):
        sp = SelfPlay(n, ROWS, cfg, seed_base=base, device=DEV)
        sp.env.reset()
        _, v, _ = sp.move(0)
        sp.check_steps()
        return sp, v.cpu().numpy().copy(), sp.last_visits.cpu().numpy().copy()
    _, pruned, raw = first_move(sp_config())
    sp, kept, raw2 = first_move(sp_config(prune_targets=False))
    assert same(raw, raw2) and same(kept, raw) and not same(pruned, raw) and (pruned <= raw).all()
    assert sp.mcts._gate[4] == (K, True)  # (under playout caps the mask is the full boards)
    sp, v, rawt = first_move(sp_config(testing=True))
    assert sp.mcts._gate[4] is None and same(v, rawt)
    cfg = sp_config()
    del cfg["forced_playouts"]
    sp, v, rawp = first_move(cfg)
    assert sp.mcts._gate[4] is None and same(v, rawp) and not same(rawp, raw)


def test_one_batch_equals_two_halves():
    """16 boards at one base against 8 and 8 with split bases: the same records."""
    from hzamd.selfplay import SelfPlay
    n, base, plies = SP["n"], SP["base"], SP["plies"]

    def play(k, b0):
        sp = SelfPlay(k, ROWS, sp_config(), seed_base=b0, device=DEV, max_plies=plies)
        sp.env.reset(seeds=b0 + torch.arange(k, device=DEV, dtype=torch.int64))
        rec = sp.play(reset=False)
        return {key: rec[key].clone() for key in ("states", "visits", "valid", "full", "final")}
    whole = play(n, base)
    assert whole["full"].any() and not whole["full"].all()
    for h in range(2):
        part = play(n // 2, base + h * (n // 2))
        sl = slice(h * (n // 2), (h + 1) * (n // 2))
        for key in ("visits", "valid", "full"):
            assert torch.equal(part[key], whole[key][:, sl]), key
        assert torch.equal(part["states"], whole["states"][:, :, sl])
        assert torch.equal(part["final"], whole["final"][:, sl])
