"""The Gumbel root on the GPU (hz_root_gumbel, hz_mcts_set_gumbel,
hz_mcts_root_gumbel_scores, hz_mcts_gumbel_result, BatchedMCTS.search(root=
"gumbel"), SelfPlay's root_policy) against the host model
tests/mcts_gumbel_model.py fed the scores G + log P the device exported.
Searches are compared exactly (integers as they are, floats by their bits);
the improved policy to 1e-6 and v_mix to 1e-12, as fp64 results of a few
dozen operations on values below 100 in size."""
import os

import numpy as np
import pytest
import torch

import oracle
from conftest import GOLDEN
from hzamd.state import pack_ref, unpack_ref, words_to_array
from mcts_carry_model import FIXTURE, copy_mt, game_over, next_word, positions
from mcts_gumbel_model import GUMBEL_KEY, GumbelModel, host_gumbel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TREES = (0, 5, 63, 64, 129)  # the boards whose whole tree is compared
TREE_KEYS = ("state", "e0", "ne", "action", "child", "n", "w", "p", "player")
# (S, max_considered, c_scale)
SETTINGS = {"s33_m16": (33, 16, 1.0), "s17_m16": (17, 16, 1.0), "s9_m4": (9, 4, 1.0), "s5_m1": (5, 1, 1.0),
            "s34_m16_scale0.1": (34, 16, 0.1)}
FORMS = ("layered", "fused_select_gather", "graph")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.dtype == b.dtype and a.shape == b.shape and bool((bits(a) == bits(b)).all())
    return a.shape == b.shape and bool((a == b).all())


_POS = []


def fixture_positions():
    if not _POS:
        F = FIXTURE
        _POS.extend(positions(F["base"], F["n"], F["spread"]))
    return list(_POS)


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


class _Rows:
    """The dense stub on the device-row protocol (device ops only: capturable)."""
    device_rows = capturable = row_independent = True

    def __init__(self):
        self.graph_key = (self, 0)  # search(graph=True) keeps the captured simulation between searches

    def __call__(self, board, glob, rows=None, count=None):
        from hzamd.mcts import dense_stub_evaluator
        return dense_stub_evaluator(board, glob)


ROWS = _Rows()


def draw(n, seed=None, board_base=None, move=None):
    from hzamd.selfplay import NoiseSource
    K = GUMBEL_KEY
    src = NoiseSource(K["board_base"] if board_base is None else board_base, DEV,
                      seed=K["seed"] if seed is None else seed)
    return src.gumbel(K["move"] if move is None else move, n)


def gumbel_search(pos, setting, form, active=None):
    """One search(root="gumbel") of the boards `pos`; everything the tests compare, on the host."""
    from hzamd.mcts import BatchedMCTS, dense_stub_evaluator
    sims, mc, c_scale = SETTINGS[setting]
    env = make_env(pos)
    mcts = BatchedMCTS(env, sims)
    mcts.fuse_select = mcts.fuse_gather = form != "layered"
    ev = ROWS if form == "graph" else dense_stub_evaluator
    g = draw(env.n)
    act = None if active is None else torch.from_numpy(active)
    visits = mcts.search(ev, FIXTURE["cpuct"], active=act, graph=form == "graph", root="gumbel", gumbel=g,
                         max_considered=mc, c_scale=c_scale)
    out = {"visits": visits.cpu().numpy().copy(), "g": g.cpu().numpy(),
           "scores": mcts.root_gumbel_scores().cpu().numpy().copy(),
           "root": {k: v.cpu().numpy().copy() for k, v in mcts.root_edges(value=False).items()},
           "counts": mcts.stats().cpu().numpy().copy(), "next": streams(env),
           "result": {k: v.cpu().numpy().copy() for k, v in mcts.gumbel_result().items()},
           "trees": {b: mcts.export_tree(b) for b in TREES if b < env.n}}
    return out, mcts, env


_MODELS = {}


def modelled(pos, setting, scores, active=None, key=None):
    """The model's search of every board, fed the device's scores; kept per
    (key, setting) and reused while the scores are the same bits."""
    sims, mc, c_scale = SETTINGS[setting]
    kept = _MODELS.get((key, setting))
    if key is not None and kept is not None and same(kept[0], scores):
        return kept[1]
    out = []
    for b, (st, m) in enumerate(pos):
        if active is not None and not active[b]:
            out.append(None)
            continue
        model = GumbelModel(st, copy_mt(m), FIXTURE["evaluator"], sims=sims, max_considered=mc, c_scale=c_scale,
                            score0=scores[b])
        model.begin()
        model.search(sims, FIXTURE["cpuct"])
        out.append(model)
    if key is not None:
        _MODELS[(key, setting)] = (scores.copy(), out)
    return out


def by_action(model, key, dtype):
    out = np.zeros(143, dtype)
    for e in model.root_edges():
        out[model.E["action"][e]] = model.E[key][e]
    return out


def assert_matches_model(dev, models, setting):
    sims = SETTINGS[setting][0]
    res = dev["result"]
    for b, model in enumerate(models):
        if model is None:  # left out of the search
            assert dev["visits"][b].sum() == 0 and tuple(dev["counts"][b, :2]) == (0, 0), b
            assert res["action"][b] == -1 and not res["pi"][b].any() and res["value"][b] == 0.0, b
            continue
        assert same(dev["visits"][b], model.visits()), b
        assert same(dev["root"]["n"][b], model.visits()), b
        assert same(dev["root"]["w"][b], by_action(model, "w", np.float64)), b
        assert tuple(dev["counts"][b, :2]) == model.counts() and dev["counts"][b, 3] == 0, b
        assert dev["next"][b] == next_word(model.mt), b
        if model.ne[0] > 0:
            assert dev["visits"][b].sum() == sims - 1, b
        a, pi, v_mix = model.result()
        assert res["action"][b] == a, b
        assert np.abs(res["pi"][b].astype(np.float64) - pi).max() <= 1e-6, b
        assert abs(float(res["value"][b]) - float(v_mix)) <= 1e-12, b
        if a >= 0:
            assert abs(float(res["pi"][b].astype(np.float64).sum()) - 1.0) <= 1e-6, b
            assert not res["pi"][b][dev["root"]["child"][b] < 0].any(), b
        else:
            assert not res["pi"][b].any(), b
    for b, tree in dev["trees"].items():
        if models[b] is not None:
            want = models[b].export()
            assert all(same(tree[k], want[k]) for k in TREE_KEYS), b


# ---------------------------------------------------------------------- draws
def test_draws_are_finite_and_do_not_depend_on_the_batch():
    n = FIXTURE["n"]
    K = GUMBEL_KEY
    whole = draw(n).cpu().numpy()
    assert whole.shape == (n, 69) and np.isfinite(whole).all()
    halves = [draw(64).cpu().numpy(), draw(n - 64, board_base=K["board_base"] + 64).cpu().numpy()]
    assert same(whole, np.concatenate(halves))
    assert not same(whole, draw(n, move=K["move"] + 1).cpu().numpy())
    assert not same(whole, draw(n, seed=K["seed"] + 1).cpu().numpy())
    # the generator is the one the host form restates (np.log against the device's log: a few ulps at most)
    assert np.abs(whole - host_gumbel(n, **K)).max() <= 1e-12


def test_draws_have_the_gumbel_moments():
    """4,096 x 69 draws: the mean within 5 standard errors of Euler's gamma
    (sigma = pi / sqrt 6 = 1.283: one standard error is 1.283 / sqrt(282,624) =
    0.0024), the variance within 5 of pi^2 / 6 (var(s^2) = (mu4 - sigma^4) / N,
    and a Gumbel's kurtosis mu4 / sigma^4 is 27 / 5, so one standard error is
    sigma^2 sqrt(4.4 / N) = 0.0065)."""
    g = draw(4096, seed=11, board_base=0, move=0).cpu().numpy().ravel()
    assert g.size == 282624 and np.isfinite(g).all()
    sd = np.pi / np.sqrt(6.0)
    assert abs(g.mean() - 0.5772156649) <= 5 * sd / np.sqrt(g.size)
    assert abs(g.var() - sd ** 2) <= 5 * sd ** 2 * np.sqrt(4.4 / g.size)


def test_noise_and_coin_keep_their_bits():
    """hz_root_noise's noise and u and hz_playout_coin's coin are the same
    bytes after Gumbel draws under the same key as before any."""
    from hzamd.selfplay import NoiseSource
    n = FIXTURE["n"]
    src = NoiseSource(GUMBEL_KEY["board_base"], DEV, seed=GUMBEL_KEY["seed"])
    counts = torch.from_numpy((np.arange(n) % 69 + 1).astype(np.int32))

    def others():
        noise, u = src.draw(GUMBEL_KEY["move"], counts, 0.4)
        return noise.cpu().numpy().copy(), u.cpu().numpy().copy(), src.coin(GUMBEL_KEY["move"], n).cpu().numpy().copy()
    before = others()
    src.gumbel(GUMBEL_KEY["move"], n)
    for a, b in zip(before, others()):
        assert same(a, b)


# --------------------------------------------------------------------- scores
def test_exported_scores_are_g_plus_log_p():
    pos = fixture_positions()
    dev, mcts, env = gumbel_search(pos, "s33_m16", "fused_select_gather")
    zeros = 0
    for b, (st, _) in enumerate(pos):
        has = dev["root"]["child"][b] >= 0
        actions = np.flatnonzero(has)
        legal = np.flatnonzero(oracle.legal(st))
        rank = np.searchsorted(legal, actions)
        assert (legal[rank] == actions).all(), b
        p = dev["root"]["p"][b][actions].astype(np.float64)
        with np.errstate(divide="ignore"):
            want = dev["g"][b][rank] + np.log(p)
        got = dev["scores"][b]
        ok = p > 0
        assert np.abs(got[:len(actions)][ok] - want[ok]).max() <= 1e-12, b
        assert (got[:len(actions)][~ok] == -np.inf).all(), b
        assert (got[len(actions):] == 0.0).all(), b
        zeros += int((~ok).sum())
    assert zeros > 0  # the dense stub's zero priors: a score of -inf was exported
    mcts.close()
    env.close()


# --------------------------------------------------------------------- search
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_search_matches_model(setting, form):
    pos = fixture_positions()
    dev, mcts, env = gumbel_search(pos, setting, form)
    models = modelled(pos, setting, dev["scores"], key="fixture")
    assert_matches_model(dev, models, setting)
    wide = [b for b, m in enumerate(models) if m.ne[0] == 69]
    if setting == "s33_m16":  # a lane's second edge was chosen: the fixture holds it (test_mcts_gumbel_cpu.py)
        assert any(dev["visits"][b][np.flatnonzero(dev["root"]["child"][b] >= 0)[64:]].any() for b in wide)
    mcts.close()
    env.close()


@pytest.mark.parametrize("form", FORMS)
def test_search_with_boards_left_out(form):
    pos = fixture_positions()
    active = (np.arange(len(pos)) % 3 != 2)
    dev, mcts, env = gumbel_search(pos, "s17_m16", form, active=active.astype(np.uint8))
    models = modelled(pos, "s17_m16", dev["scores"], active=active, key="left_out")
    assert_matches_model(dev, models, "s17_m16")
    mcts.close()
    env.close()


@pytest.mark.parametrize("form", FORMS)
def test_search_with_a_stuck_and_a_terminal_root(form):
    pos = fixture_positions()
    stuck, terminal = 63, 64
    pos[stuck] = oracle.stuck_state(915 + stuck)
    final = np.load(os.path.join(GOLDEN, "env_traces.npz"))["finals"][3]
    pos[terminal] = (np.array(final, np.int16), oracle.mt_seed(1))
    assert game_over(pos[terminal][0]) and not oracle.legal(pos[stuck][0]).any()
    dev, mcts, env = gumbel_search(pos, "s17_m16", form)
    models = modelled(pos, "s17_m16", dev["scores"], key="stuck_terminal")
    assert_matches_model(dev, models, "s17_m16")
    for b in (stuck, terminal):
        assert tuple(dev["counts"][b, :2]) == (1, 0) and dev["result"]["action"][b] == -1, b
    mcts.close()
    env.close()


# ----------------------------------------------------------------------- gate
def test_plain_search_after_gumbel_is_the_oracles():
    """A plain search() on a handle that has searched with the Gumbel root
    (eagerly and through a captured simulation) equals oracle.mcts_search:
    visits, node and edge counts, the stream's next word."""
    from hzamd.mcts import dense_stub_evaluator
    F = FIXTURE
    pos = fixture_positions()
    dev, mcts, env = gumbel_search(pos, "s33_m16", "graph")
    with pytest.raises(ValueError):
        mcts.search(dense_stub_evaluator, F["cpuct"], max_considered=4)  # the Gumbel settings without root=
    # (the graph form's evaluator is the one the Gumbel search captured with: the gate belongs to the cache key)
    for opts, ev in (({}, dense_stub_evaluator), ({"graph": True}, ROWS)):
        load_positions(env, pos)
        visits = mcts.search(ev, F["cpuct"], **opts).cpu().numpy()
        counts, nxt = mcts.stats().cpu().numpy(), streams(env)
        with pytest.raises(ValueError):
            mcts.gumbel_result()
        for b, (st, m) in enumerate(pos):
            m2 = copy_mt(m)
            _, ov, nn, ne = oracle.mcts_search(st, m2, 33, F["cpuct"], testing=True, tau0=0, evaluator=F["evaluator"])
            assert same(visits[b], ov) and tuple(counts[b, :2]) == (nn, ne), b
            assert nxt[b] == next_word(m2), b
    mcts.close()
    env.close()


def test_kept_capture_survives_a_larger_table_on_the_same_handle():
    """One handle: search(graph=True, S 17) captures and keeps a simulation;
    an eager search with S 33 then sets a table twice as large; the next
    search(graph=True, S 17) has the first one's cache key and replays the
    kept capture.  The handle's table keeps its address (hz_mcts_set_gumbel),
    so the replays read the live table: all three searches equal the model."""
    from hzamd.mcts import BatchedMCTS, dense_stub_evaluator
    pos = fixture_positions()
    env = make_env(pos)
    mcts = BatchedMCTS(env, 33)
    g = draw(env.n)

    def run(setting, **opts):
        load_positions(env, pos)
        sims, mc, c_scale = SETTINGS[setting]
        ev = ROWS if opts.get("graph") else dense_stub_evaluator
        visits = mcts.search(ev, FIXTURE["cpuct"], sims=sims, root="gumbel", gumbel=g, max_considered=mc,
                             c_scale=c_scale, **opts).cpu().numpy().copy()
        dev = {"visits": visits, "scores": mcts.root_gumbel_scores().cpu().numpy().copy(),
               "root": {k: v.cpu().numpy().copy() for k, v in mcts.root_edges(value=False).items()},
               "counts": mcts.stats().cpu().numpy().copy(), "next": streams(env),
               "result": {k: v.cpu().numpy().copy() for k, v in mcts.gumbel_result().items()},
               "trees": {b: mcts.export_tree(b) for b in TREES}}
        assert_matches_model(dev, modelled(pos, setting, dev["scores"], key="fixture"), setting)
        return dev
    first = run("s17_m16", graph=True)
    kept = mcts._graph_cache
    assert kept is not None and len(kept[1]) >= 1
    captured = dict(kept[1])
    run("s33_m16")
    assert mcts._graph_cache is kept  # the eager search leaves the kept capture alone
    again = run("s17_m16", graph=True)
    assert mcts._graph_cache is kept and all(kept[1].get(k) is v for k, v in captured.items())  # replayed, not re-captured
    assert same(first["visits"], again["visits"]) and same(first["root"]["w"], again["root"]["w"])
    mcts.close()
    env.close()


def test_forbidden_combinations_raise():
    from hzamd.mcts import BatchedMCTS, dense_stub_evaluator
    from hzamd.selfplay import SelfPlay
    pos = fixture_positions()[:8]
    env = make_env(pos)
    mcts = BatchedMCTS(env, 9)
    g = draw(8)
    noise = torch.zeros(8, 69, dtype=torch.float64)
    bad = ({"noise": noise}, {"root_noise": torch.ones(8, dtype=torch.uint8)},
           {"budget": torch.full((8,), 4, dtype=torch.int32)}, {"tail": (4, 2)}, {"carry": True})
    for kw in bad:
        with pytest.raises(ValueError):
            mcts.search(dense_stub_evaluator, 1.25, root="gumbel", gumbel=g, **kw)
    for kw in ({"root": "gumbel"}, {"root": "halving", "gumbel": g}, {"root": "gumbel", "gumbel": g[:4]},
               {"root": "gumbel", "gumbel": g, "max_considered": 0},
               {"root": "gumbel", "gumbel": g, "max_considered": 70},
               {"root": "gumbel", "gumbel": g, "c_scale": -1.0}):
        with pytest.raises(ValueError):
            mcts.search(dense_stub_evaluator, 1.25, **kw)
    with pytest.raises(ValueError):
        mcts.gumbel_result()
    cfg = {"num_simulations": 9, "cpuct": 1.25, "root_policy": "gumbel"}
    for extra in ({"playout_cap_p": 0.25, "playout_cap_fast": 4}, {"tree_reuse": "add"}):
        with pytest.raises(ValueError):
            SelfPlay(4, dense_stub_evaluator, dict(cfg, **extra), seed_base=1, device=DEV)
    with pytest.raises(ValueError):
        SelfPlay(4, dense_stub_evaluator, dict(cfg, root_policy="halving"), seed_base=1, device=DEV)
    mcts.close()
    env.close()


# ------------------------------------------------------------------ self-play
SP_N, SP_SIMS, SP_MOVES, SP_BASE = 16, 17, 12, 61000


def test_self_play_moves_are_the_models():
    """16 boards, S 17, twelve moves of self-play with root_policy "gumbel":
    every move of every board is replayed by the model from the move's
    exported scores (the action, v_mix under keep_root_value, the state before
    the next move), the visit slots hold rint(pi' * 65535), and pi_of the
    packed records is within 143 / 65535 of pi'."""
    import hzamd.distributed as hd
    from hzamd.mcts import dense_stub_evaluator
    from hzamd.selfplay import SelfPlay
    cfg = {"num_simulations": SP_SIMS, "cpuct": 1.25, "root_policy": "gumbel"}
    sp = SelfPlay(SP_N, dense_stub_evaluator, cfg, seed_base=SP_BASE, device=DEV, max_plies=SP_MOVES,
                  keep_root_value=True)
    sp.keep_noise = True
    sp.env.reset()
    mts = [oracle.mt_seed(SP_BASE + b) for b in range(SP_N)]
    states = [oracle.reset(m) for m in mts]
    for ply in range(SP_MOVES):
        st, v, active = sp.move(ply)
        assert bool(active.all())
        words = st.cpu().numpy()
        scores = sp.mcts.root_gumbel_scores().cpu().numpy()
        res = {k: x.cpu().numpy() for k, x in sp.last_gumbel.items()}
        g, u, act = sp.noise_log[-1]
        # no Dirichlet noise, no move-choice uniform: the move's Gumbels under (seed 0, seed_base + b, move)
        assert u is None and np.abs(g.cpu().numpy() - host_gumbel(SP_N, 0, SP_BASE, ply)).max() <= 1e-12
        # the move's records, packed and unpacked: pi_of rebuilds pi' (each slot is off by at most half a
        # count of 65535 and their sum by at most 143 halves)
        z = torch.zeros(SP_N, device=DEV)
        packed = hd.pack_records(st.t().contiguous(), v, z, z)
        assert packed.shape == (SP_N, 42) and packed.dtype == torch.int64  # 336 bytes
        rebuilt = hd.pi_of(hd.unpack_records(packed)[1]).cpu().numpy().astype(np.float64)
        assert np.abs(rebuilt - res["pi"].astype(np.float64)).max() <= 143.0 / 65535.0, ply
        for b in range(SP_N):
            assert same(unpack_ref(words[:, b]), states[b]), (ply, b)
            model = GumbelModel(states[b], mts[b], 1, sims=SP_SIMS, score0=scores[b])
            model.begin()
            model.search(SP_SIMS, 1.25)
            a, pi, v_mix = model.result()
            assert a >= 0 and int(act[b]) == a and res["action"][b] == a, (ply, b)
            assert abs(float(sp.last_root_value[b]) - float(v_mix)) <= 1e-12, (ply, b)
            assert same(v[b].cpu().numpy(), np.rint(res["pi"][b].astype(np.float64) * 65535.0).astype(np.int32)), (ply, b)
            states[b] = model.play(a)
    sp.check_steps()
    sp.mcts.close()
    sp.env.close()


def test_self_play_reports_a_stuck_board_as_puct_does():
    """An active board whose root has no edges (stuck: no legal move, game not
    over; play from a reset never reaches one) gets action -1 from the Gumbel
    search, as it gets -1 from zero visits under PUCT.  env.step takes -1 as
    no move and reports it: under either root policy the board's state stays,
    its record row is zero, and check_steps() raises for that board alone."""
    from hzamd.mcts import dense_stub_evaluator
    from hzamd.selfplay import SelfPlay
    pos = fixture_positions()[:4]
    pos[1] = oracle.stuck_state(915)
    for extra in ({"root_policy": "gumbel"}, {}):
        sp = SelfPlay(4, dense_stub_evaluator, dict({"num_simulations": 9, "cpuct": 1.25}, **extra), seed_base=3,
                      device=DEV)
        sp.keep_noise = True
        load_positions(sp.env, pos)
        st, v, active = sp.move(0)
        with pytest.raises(RuntimeError, match=r"boards \[1\]"):
            sp.check_steps()
        after = sp.env.export_state().cpu().numpy()
        act = sp.noise_log[-1][2].cpu().numpy()
        assert bool(active.all()) and act[1] == -1 and (act[[0, 2, 3]] >= 0).all(), extra
        assert same(after[:, 1], st.cpu().numpy()[:, 1]) and not v[1].any() and v[0].any(), extra
        if extra:
            assert sp.last_gumbel["action"][1] == -1 and not sp.last_gumbel["pi"][1].any()
        sp.mcts.close()
        sp.env.close()


def sp_records(n, cfg, warm=False):
    from hzamd.mcts import dense_stub_evaluator
    from hzamd.selfplay import SelfPlay
    sp = SelfPlay(n, dense_stub_evaluator, cfg, seed_base=SP_BASE, device=DEV, max_plies=SP_MOVES,
                  keep_root_value=True)
    seeds = torch.arange(n, device=DEV, dtype=torch.int64) + SP_BASE
    sp.env.reset(seeds=seeds)
    if warm:  # the handle has searched with the Gumbel root before (the search draws from the boards' streams)
        sp.mcts.search(dense_stub_evaluator, 1.25, root="gumbel", gumbel=draw(n))
        sp.env.reset(seeds=seeds)
    rec = sp.play(reset=False)
    comp = sp.compact(rec)
    out = {k: rec[k].cpu().numpy().copy() for k in ("states", "visits", "valid", "root_value")}
    out["comp"] = {k: v.cpu().numpy().copy() for k, v in comp.items()}
    pi = None
    if sp.gumbel is not None:
        pi = sp.last_gumbel["pi"].cpu().numpy().copy()
    sp.mcts.close()
    sp.env.close()
    return out, pi


def test_self_play_records_rebuild_the_improved_policy():
    """play() with root_policy "gumbel": the records keep their 336-byte
    format, and pi_of the packed records is within 143 / 65535 of the improved
    policy (each slot is off by at most half a count of 65535, the sum of the
    slots by at most 143 halves); the last move's pi' from the handle is the
    last record's."""
    import hzamd.distributed as hd
    cfg = {"num_simulations": SP_SIMS, "cpuct": 1.25, "root_policy": "gumbel", "gumbel_max_considered": 8}
    rec, last_pi = sp_records(SP_N, cfg)
    comp = rec["comp"]
    assert rec["visits"].shape == (SP_MOVES, SP_N, 143) and rec["valid"].all()
    packed = hd.pack_records(*(torch.from_numpy(comp[k]) for k in ("states", "visits", "z", "player")))
    assert packed.shape == (SP_MOVES * SP_N, 42) and packed.dtype == torch.int64  # 336 bytes
    _, visits, _, _ = hd.unpack_records(packed)[:4]
    pi = hd.pi_of(visits).numpy().astype(np.float64)
    want = comp["visits"].astype(np.float64) / 65535.0  # pi' to within half a count per slot
    assert np.abs(pi - want).max() <= 143.0 / 65535.0
    assert np.abs(pi[-SP_N:] - last_pi.astype(np.float64)).max() <= 143.0 / 65535.0
    assert np.abs(comp["pi"].astype(np.float64).sum(1) - 1.0).max() <= 1e-6
    assert np.abs(rec["root_value"]).max() <= 1.0 and rec["root_value"].any()


def test_self_play_without_the_key_is_unchanged():
    """With root_policy absent a SelfPlay whose handle has searched with the
    Gumbel root records, byte for byte, what an untouched one records, and so
    does root_policy "puct".  All three runs are this build's: the test shows
    that the gate clears and that "puct" is the absent key, not that the
    records are an earlier build's; that rests on the self-play tests and
    goldens from before this feature, which it leaves as they were."""
    cfg = {"num_simulations": SP_SIMS, "cpuct": 1.25, "dirichlet_epsilon": 0.3}
    plain, _ = sp_records(SP_N, cfg)
    warm, _ = sp_records(SP_N, cfg, warm=True)
    for k in ("states", "visits", "valid", "root_value"):
        assert same(plain[k], warm[k]), k
    also, _ = sp_records(SP_N, dict(cfg, root_policy="puct"))
    for k in ("states", "visits", "valid", "root_value"):
        assert same(plain[k], also[k]), k
