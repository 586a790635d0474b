"""Leaf symmetries on the GPU (hz_leaf_sym_keys, hz_mcts_set_leaf_symmetry,
hz_mcts_leaf_symmetry, BatchedMCTS.search(leaf_symmetry=), SelfPlay's
leaf_symmetry) against the host model tests/mcts_leafsym_model.py.

Both parity stubs are blind to a board symmetry, so the searches here run the
model's cell stub (it tells a position from its images: the same integer
formula on the host and the device) or its orbit stub (equivariant by
construction).  Everything is compared exactly: integers as they are, floats
by their bits.  tests/test_mcts_leafsym_cpu.py shows that the fixture holds the
cases these tests rely on."""
import numpy as np
import pytest
import torch

import oracle
from hzamd.state import pack_ref, unpack_ref, words_to_array
from hzamd.symmetry import transform_states
from mcts_carry_model import choose, copy_mt, next_word, positions
from mcts_leafsym_model import (CELL_STUB, FIXTURE, KEYS, ORBIT_STUB, SMALL, LeafSymModel, host_keys, leaf_sym)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TREE_KEYS = ("state", "e0", "ne", "action", "child", "n", "w", "p", "player")
TREES = (0, 5, 31, 63, 64, 100, 129)  # the boards whose whole tree is compared (every board of the small batch)
# tests/test_mcts_gumbel_gpu.py's three forms, and the layered form with k_gather + the encoder launches
FORMS = ("layered", "fused_select_gather", "graph", "layered_encoders")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.dtype == b.dtype and a.shape == b.shape and bool((bits(a) == bits(b)).all())
    return a.shape == b.shape and bool((a == b).all())


_POS = []


def fixture_positions(n=None):
    if not _POS:
        F = FIXTURE
        _POS.extend(positions(F["base"], F["n"], F["spread"]))
    return list(_POS[:n])


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


def draw_keys(n, seed=None, board_base=None, move=None):
    from hzamd.selfplay import NoiseSource
    K = KEYS
    src = NoiseSource(K["board_base"] if board_base is None else board_base, DEV,
                      seed=K["seed"] if seed is None else seed)
    return src.leaf_symmetry(K["move"] if move is None else move, n)


def as_u64(keys):
    return keys.cpu().numpy().view(np.uint64)


def make_mcts(env, form, sims=None):
    import hzamd._native as nat
    from hzamd.mcts import BatchedMCTS
    mcts = BatchedMCTS(env, FIXTURE["sims"] if sims is None else sims)
    mcts.fuse_select = mcts.fuse_gather = form == "fused_select_gather" or form == "graph"
    if form == "layered_encoders":
        assert nat.lib().hz_mcts_set_gather_encode(mcts._h, 0) == 0
    return mcts


def run_search(pos, form, evaluator, keyed=True, **opts):
    """One search of the boards `pos`; everything the tests compare, on the host."""
    env = make_env(pos)
    mcts = make_mcts(env, form)
    keys = draw_keys(env.n) if keyed else None
    visits = mcts.search(evaluator, FIXTURE["cpuct"], graph=form == "graph", leaf_symmetry=keys, **opts)
    out = {"visits": visits.cpu().numpy().copy(), "counts": mcts.stats().cpu().numpy().copy(), "next": streams(env),
           "trees": {b: mcts.export_tree(b) for b in (range(env.n) if env.n <= SMALL else TREES)}}
    mcts.close()
    env.close()
    return out


_MODELS = {}


def modelled(pos, name, keyed=True, active=None, budget=None, noise=None):
    """The model's search of every board with the cell stub, kept by name."""
    F = FIXTURE
    if name in _MODELS:
        return _MODELS[name]
    keys = host_keys(len(pos), **KEYS)
    out = []
    for b, (st, m) in enumerate(pos):
        if active is not None and not active[b]:
            out.append(None)
            continue
        model = LeafSymModel(st, copy_mt(m), "cell", key=keys[b] if keyed else None)
        model.begin(carry=False)
        sims = F["sims"] if budget is None else min(int(budget[b]), F["sims"])
        model.search(sims, F["cpuct"], noise=None if noise is None else noise[b], eps=F["eps"],
                     noisy=noise is not None)
        out.append(model)
    _MODELS[name] = out
    return out


def assert_matches_model(dev, models):
    for b, model in enumerate(models):
        if model is None:  # left out of the search
            assert dev["visits"][b].sum() == 0 and tuple(dev["counts"][b, :2]) == (0, 0), b
            continue
        assert same(dev["visits"][b], model.visits()), b
        assert tuple(dev["counts"][b, :2]) == model.counts() and dev["counts"][b, 3] == 0, b
        assert dev["next"][b] == next_word(model.mt), b
    for b, tree in dev["trees"].items():
        if b < len(models) and models[b] is not None:
            want = models[b].export()
            assert all(same(tree[k], want[k]) for k in TREE_KEYS), b


def assert_same_search(a, b):
    assert same(a["visits"], b["visits"]) and same(a["counts"], b["counts"]) and a["next"] == b["next"]
    for t in a["trees"]:
        assert all(same(a["trees"][t][k], b["trees"][t][k]) for k in TREE_KEYS), t


# ----------------------------------------------------------------------- keys
def test_keys_do_not_depend_on_the_batch():
    n, K = FIXTURE["n"], KEYS
    whole = as_u64(draw_keys(n))
    assert whole.shape == (n,) and whole.dtype == np.uint64
    assert [int(x) for x in whole] == host_keys(n, **K)  # the generator is the one the host form restates
    halves = [as_u64(draw_keys(64)), as_u64(draw_keys(n - 64, board_base=K["board_base"] + 64))]
    assert same(whole, np.concatenate(halves))
    assert len(set(whole.tolist())) == n
    assert not same(whole, as_u64(draw_keys(n, move=K["move"] + 1)))
    assert not same(whole, as_u64(draw_keys(n, seed=K["seed"] + 1)))


def test_other_draws_keep_their_bits():
    """hz_root_noise's noise and u, hz_playout_coin's coin and hz_root_gumbel's
    Gumbels are the same bytes after key draws under the same key as before."""
    from hzamd.selfplay import NoiseSource
    n = FIXTURE["n"]
    src = NoiseSource(KEYS["board_base"], DEV, seed=KEYS["seed"])
    counts = torch.from_numpy((np.arange(n) % 69 + 1).astype(np.int32))

    def others():
        noise, u = src.draw(KEYS["move"], counts, 0.4)
        return [t.cpu().numpy().copy() for t in (noise, u, src.coin(KEYS["move"], n), src.gumbel(KEYS["move"], n))]
    before = others()
    src.leaf_symmetry(KEYS["move"], n)
    for a, b in zip(before, others()):
        assert same(a, b)


# -------------------------------------------------------------------- encoder
class _DevArray:
    """A device array the library owns, for torch.as_tensor."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def leaf_ids(mcts):
    """The boards' current leaves (hz_mcts_leaf_ptrs): (leaf, leaf_gidx) on the host."""
    import ctypes

    import hzamd._native as nat
    leaf, gidx = ctypes.c_void_p(), ctypes.c_void_p()
    assert nat.lib().hz_mcts_leaf_ptrs(mcts._h, ctypes.byref(leaf), ctypes.byref(gidx)) == 0
    torch.cuda.synchronize()
    return tuple(torch.as_tensor(_DevArray(p.value, mcts.n, "<i4"), device=DEV).cpu().numpy().copy()
                 for p in (leaf, gidx))


ENCODERS = ("gather_fused", "gather_layered", "per_board", "select_gather", "expand_select_gather")


@pytest.mark.parametrize("n", [FIXTURE["n"], SMALL])
@pytest.mark.parametrize("path", ENCODERS)
def test_every_encoder_writes_the_leafs_image(path, n):
    """After a few simulations, the rows the next simulation would evaluate:
    row j is hz_encode_states of transform_states(leaf state, g), bit for bit,
    with the leaf from hz_mcts_leaf_ptrs, its state from export_tree and g from
    leaf_symmetries() and, independently, from the rule restated in Python."""
    import hzamd._native as nat
    from hzamd.selfplay import encode_states
    F = FIXTURE
    pos = fixture_positions(n)
    env = make_env(pos)
    mcts = make_mcts(env, "layered", sims=12)
    assert nat.lib().hz_mcts_set_gather_encode(mcts._h, 0 if path == "gather_layered" else 1) == 0
    keys = draw_keys(n)
    mcts._sync()
    assert mcts._set_leaf_symmetry(keys)
    active = torch.from_numpy((np.arange(n) % 7 != 3).astype(np.uint8)).to(DEV)
    mcts.begin(active)
    done = 6
    for s in range(done):
        board, glob, rows, count = mcts.select_gather(F["cpuct"], active)
        policy, value = CELL_STUB(board, glob, rows, count)
        if s + 1 < done or path != "expand_select_gather":
            mcts.expand_backup(policy, value, gathered=True)
    mcts.board.fill_(float("nan"))
    mcts.glob.fill_(float("nan"))
    if path == "expand_select_gather":  # the last expansion carries the next simulation's select, gather and encode
        mcts.count_b.zero_()
        mcts.expand_backup_select_gather(policy, value, F["cpuct"], active, None, F["eps"], True, mcts.count_b,
                                         mcts.count, False)
        count = mcts.count_b
    elif path == "select_gather":
        _, _, _, count = mcts.select_gather(F["cpuct"], active)
    else:
        mcts.select(F["cpuct"], active)
        if path == "per_board":
            mcts.encode_leaves()
        else:
            _, _, _, count = mcts.gather_leaves()
    torch.cuda.synchronize()
    leaf, gidx = leaf_ids(mcts)
    reported = mcts.leaf_symmetries().cpu().numpy().copy()
    hk = as_u64(keys)
    need = np.flatnonzero(gidx >= 0)
    assert len(need) > n // 2 and (gidx[need] == need * mcts.max_nodes + leaf[need]).all()
    want_g = np.array([leaf_sym(hk[b], leaf[b]) if gidx[b] >= 0 else 0 for b in range(n)], np.uint8)
    assert same(reported, want_g)
    assert len(set(want_g[need].tolist())) == 4 or n == SMALL
    if path == "per_board":
        row_board = np.arange(n)
    else:
        k = int(count.item())
        row_board = mcts.rows[:k].cpu().numpy()
        assert sorted(row_board.tolist()) == need.tolist()
        if path != "expand_select_gather":
            assert row_board.tolist() == need.tolist()  # board order
    states = np.zeros((len(row_board), 6), np.uint64)
    for j, b in enumerate(row_board):
        if gidx[b] >= 0:
            states[j] = mcts.export_tree(int(b))["state"][leaf[b]]
    st = torch.from_numpy(states.view(np.int64)).to(DEV)
    g = torch.from_numpy(want_g[row_board].astype(np.int64)).to(DEV)
    want_board, want_glob = encode_states(transform_states(st, g))
    plain_board, _ = encode_states(st)
    live = torch.from_numpy(gidx[row_board] >= 0).to(DEV)
    want_board[~live] = 0  # a board without a leaf to evaluate: a zero record (per-board form)
    want_glob[~live] = 0
    k = len(row_board)
    assert torch.equal(mcts.board[:k].view(torch.int32), want_board.view(torch.int32))
    assert torch.equal(mcts.glob[:k].view(torch.int32), want_glob.view(torch.int32))
    # (the comparison has teeth: the images differ from the leaves as stored)
    assert not torch.equal(want_board.view(torch.int32), plain_board.view(torch.int32) * live.view(-1, 1, 1, 1))
    if path == "expand_select_gather":
        mcts.count_b.zero_()
    mcts.close()
    env.close()


# --------------------------------------------------------------------- search
@pytest.mark.parametrize("n", [FIXTURE["n"], SMALL])
@pytest.mark.parametrize("form", FORMS)
def test_search_matches_model(form, n):
    pos = fixture_positions(n)
    dev = run_search(pos, form, CELL_STUB)
    models = modelled(fixture_positions(), "keyed")[:n]
    assert_matches_model(dev, models)
    plain = modelled(fixture_positions(), "plain", keyed=False)[:n]
    assert sum(not same(a.visits(), b.visits()) for a, b in zip(models, plain)) >= n // 2  # the keys matter


@pytest.mark.parametrize("form", FORMS)
def test_search_with_boards_left_out(form):
    pos = fixture_positions()
    active = np.arange(len(pos)) % 3 != 2
    dev = run_search(pos, form, CELL_STUB, active=torch.from_numpy(active.astype(np.uint8)))
    models = [m if active[b] else None for b, m in enumerate(modelled(pos, "keyed"))]
    assert_matches_model(dev, models)


@pytest.mark.parametrize("form", FORMS)
def test_search_with_budgets(form):
    F = FIXTURE
    pos = fixture_positions()
    budget = (1 + (np.arange(len(pos)) * 7) % (F["sims"] + 4)).astype(np.int32)
    dev = run_search(pos, form, CELL_STUB, budget=torch.from_numpy(budget))
    assert_matches_model(dev, modelled(pos, "budget", budget=budget))


@pytest.mark.parametrize("form", FORMS)
def test_search_with_root_noise(form):
    from hzamd.selfplay import NoiseSource
    F = FIXTURE
    pos = fixture_positions()
    counts = torch.tensor([int(oracle.legal(st).sum()) for st, _ in pos], dtype=torch.int32)
    noise, _ = NoiseSource(KEYS["board_base"], DEV, seed=KEYS["seed"]).draw(KEYS["move"], counts, 0.4)
    dev = run_search(pos, form, CELL_STUB, noise=noise, eps=F["eps"], testing=False)
    assert_matches_model(dev, modelled(pos, "noise", noise=noise.cpu().numpy()))


@pytest.mark.parametrize("n", [FIXTURE["n"], SMALL])
@pytest.mark.parametrize("form", FORMS)
def test_equivariant_evaluator_hides_the_keys(form, n):
    pos = fixture_positions(n)
    assert_same_search(run_search(pos, form, ORBIT_STUB), run_search(pos, form, ORBIT_STUB, keyed=False))


# ----------------------------------------------------------------------- gate
class _DenseRows:
    """The dense stub on the device-row protocol (capturable; the captured simulation is kept between searches)."""
    device_rows = capturable = row_independent = True

    def __init__(self):
        self.graph_key = (self, 0)

    def __call__(self, board, glob, rows=None, count=None):
        from hzamd.mcts import dense_stub_evaluator
        return dense_stub_evaluator(board, glob)


def test_plain_search_after_a_keyed_one_is_the_oracles():
    """A search without leaf_symmetry= on a handle that has searched with it,
    eagerly and through a kept capture: oracle.mcts_search's visits, counts and
    stream; the capture kept under the gate is not replayed once it is off; and
    the report reads 0."""
    F = FIXTURE
    pos = fixture_positions()
    env = make_env(pos)
    mcts = make_mcts(env, "graph")
    ev = _DenseRows()
    keys = draw_keys(env.n)
    want = []
    for st, m in pos:
        m2 = copy_mt(m)
        _, ov, nn, ne = oracle.mcts_search(st, m2, F["sims"], F["cpuct"], testing=True, tau0=0, evaluator=1)
        want.append((ov, (nn, ne), next_word(m2)))

    def run(**opts):
        load_positions(env, pos)
        visits = mcts.search(ev, F["cpuct"], **opts).cpu().numpy().copy()
        return visits, mcts.stats().cpu().numpy().copy(), streams(env)

    def is_oracle(res):
        visits, counts, nxt = res
        return [same(visits[b], w[0]) and tuple(counts[b, :2]) == w[1] and nxt[b] == w[2]
                for b, w in enumerate(want)]
    keyed = run(graph=True, leaf_symmetry=keys)
    kept = mcts._graph_cache
    assert kept is not None and kept[0][-1][3] is True
    assert sum(is_oracle(keyed)) < env.n // 2  # the priors were read through g: another search
    for opts in ({"graph": True}, {}, {"graph": True}):
        assert all(is_oracle(run(**opts)))
        assert not mcts.leaf_symmetries().any()
    assert mcts._graph_cache is not kept and mcts._graph_cache[0][-1][3] is False
    again = run(graph=True, leaf_symmetry=keys)  # and back: a fresh capture under the gate
    # (stats()' third column is the handle's search generation: it counts the searches)
    assert same(keyed[0], again[0]) and same(keyed[1][:, :2], again[1][:, :2]) and keyed[2] == again[2]
    mcts.close()
    env.close()


def test_forbidden_combinations_raise():
    from hzamd.selfplay import NoiseSource, SelfPlay
    pos = fixture_positions(SMALL)
    env = make_env(pos)
    mcts = make_mcts(env, "layered")
    keys = draw_keys(env.n)
    g = NoiseSource(0, DEV).gumbel(0, env.n)
    with pytest.raises(ValueError):
        mcts.search(CELL_STUB, 1.25, root="gumbel", gumbel=g, leaf_symmetry=keys)
    with pytest.raises(ValueError):
        mcts.search(CELL_STUB, 1.25, carry=True, leaf_symmetry=keys)
    with pytest.raises(ValueError):
        mcts.search(CELL_STUB, 1.25, leaf_symmetry=keys[:-1])
    with pytest.raises(ValueError):
        mcts.search(CELL_STUB, 1.25, leaf_symmetry=keys.to(torch.float64))
    for cfg in ({"tree_reuse": "add"}, {"root_policy": "gumbel"}, {"leaf_symmetry": "mirror"}):
        with pytest.raises(ValueError):
            SelfPlay(env.n, CELL_STUB, dict({"num_simulations": 4, "leaf_symmetry": "random"}, **cfg), env=env,
                     device=DEV)
    mcts.close()
    env.close()


# ------------------------------------------------------------------ self-play
def test_self_play_without_the_key_is_what_it_was(monkeypatch):
    """Without the config key no key is drawn and the records are, byte for
    byte, those of the move loop as it was before the key existed (restated
    here: the draws, a search() without leaf_symmetry=, the choice, the step)."""
    from hzamd.mcts import choose_actions
    from hzamd.selfplay import NoiseSource, SelfPlay
    n, base, plies = 40, 3100, 4
    cfg = {"num_simulations": 8, "cpuct": 1.5, "testing": False}

    def refuse(self, step, n):
        raise AssertionError("a key was drawn")
    monkeypatch.setattr(NoiseSource, "leaf_symmetry", refuse)
    sp = SelfPlay(n, CELL_STUB, cfg, seed_base=base, device=DEV)
    sp.env.reset()
    got = []
    for ply in range(plies):  # (the visits are the handle's own tensor, rewritten by the next search)
        st, v, _ = sp.move(ply)
        got.append((st.cpu().numpy().copy(), v.cpu().numpy().copy()))
    sp.check_steps()
    final = sp.env.export_state().cpu().numpy().copy()

    old = SelfPlay(n, CELL_STUB, cfg, seed_base=base, device=DEV)
    env = old.env
    env.reset()
    for ply in range(plies):
        active = ~env.done()
        st = env.export_state()
        _, count = env.legal_mask()
        noise, u = old.noise.draw(ply, count, old.cfg["dirichlet_alpha"])
        v = old.mcts.search(CELL_STUB, old.cfg["cpuct"], active=active, noise=noise,
                            eps=old.cfg["dirichlet_epsilon"], testing=False, max_rows=n)
        explore = torch.full((n,), ply < old.cfg["turns_until_tau0"], dtype=torch.bool, device=DEV)
        act = choose_actions(v, explore, u)
        assert same(got[ply][0], st.cpu().numpy()) and same(got[ply][1], v.cpu().numpy()), ply
        status = env.step(torch.where(active, act, torch.full_like(act, -1)).to(torch.int16))
        assert not (status != 0)[active].any()
    assert same(final, env.export_state().cpu().numpy())


def test_self_play_with_the_key_plays_the_models_moves():
    from hzamd.selfplay import SelfPlay
    n, base, plies, sims, cpuct, eps = 12, 3300, 3, 10, 1.5, 0.25
    cfg = {"num_simulations": sims, "cpuct": cpuct, "testing": False, "leaf_symmetry": "random"}
    sp = SelfPlay(n, CELL_STUB, cfg, seed_base=base, device=DEV)
    sp.keep_noise = True
    sp.env.reset()
    states, visits = [], []
    for ply in range(plies):  # (the visits are the handle's own tensor, rewritten by the next search)
        st, v, _ = sp.move(ply)
        states.append(st.cpu().numpy().copy())
        visits.append(v.cpu().numpy().copy())
    sp.check_steps()
    log = [[t.cpu().numpy() for t in entry] for entry in sp.noise_log]
    final = sp.env.export_state().cpu().numpy()
    changed = 0
    for b in range(n):
        m = oracle.mt_seed(base + b)
        s = oracle.reset(m)
        for ply in range(plies):
            assert (unpack_ref(states[ply][:, b]) == s).all(), (b, ply)
            noise, u, act = log[ply]
            key = host_keys(1, 0, base + b, ply)[0]
            model = LeafSymModel(s, m, "cell", key=key)
            model.begin(carry=False)
            model.search(sims, cpuct, noise=noise[b], eps=eps, noisy=True)
            assert same(visits[ply][b], model.visits()), (b, ply)
            a = choose(model.visits(), True, u[b])
            assert a == act[b], (b, ply)
            changed += any(g != 0 for _, g, _ in model.evaluated)
            s = model.play(a)
        assert (unpack_ref(final[:, b]) == s).all(), b
    assert changed > 0
