"""The search report on the GPU (hz_mcts_root_edges, hz_mcts_pv,
hz_mcts_export_tree and what hzamd builds on them): the root edges' stored
W, Q = W / N and mixed P, the root value and the principal variation against
the reference's own trees (tests/golden/mcts_report.npz), against the
exported tree walked on the host, and through self-play and the drop-in.
Every comparison is exact: integers as they are, floats by their bits."""
import os
import random
from collections import defaultdict

import numpy as np
import pytest
import torch

import oracle
from conftest import GOLDEN
from hzamd.state import pack_ref, words_to_array
from test_mcts_gpu import DENSE_FORMS, _DenseRows, make_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPECIAL = (0, 63, 64, 129)  # a wave's first and last lane, the next wave's first, a partial wave's last


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.dtype == b.dtype and a.shape == b.shape and bool((bits(a) == bits(b)).all())
    return a.shape == b.shape and bool((a == b).all())


def cpu(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def dense_groups(f):
    groups = defaultdict(list)
    for k in range(len(f["sims"])):
        groups[(int(f["sims"][k]), float(f["cpuct"][k]), int(f["testing"][k]), float(f["eps"][k]))].append(k)
    return groups


@pytest.mark.parametrize("form", ["small_batch", "fused_select_gather", "graph"])
def test_report_matches_reference_fixtures(form):
    """The 48 reference searches of mcts_dense.npz through three forms of
    search(): the root edges' N, the stored fp64 W, Q = W / N, the stored fp32
    P (the root's (1 - eps) * P + eps * noise where the search mixes), the
    root value and every principal-variation array equal what the reference's
    own Node / Edge objects hold (mcts_report.npz)."""
    from hzamd.mcts import BatchedMCTS, dense_stub_evaluator
    copies, opts = DENSE_FORMS[form]
    opts = dict(opts)
    f, r = load("mcts_dense.npz"), load("mcts_report.npz")
    groups = dense_groups(f)
    assert len(groups) == 12
    ev = _DenseRows() if opts.get("graph") else dense_stub_evaluator
    checked = 0
    for (sims, cpuct, testing, eps), rows in groups.items():
        ks = rows * copies
        assert (len(ks) > 32) == (copies > 1)
        env = make_env(f["state"][ks], f["mt_seed"][ks])
        mcts = BatchedMCTS(env, sims)
        noise = torch.from_numpy(np.ascontiguousarray(f["noise"][ks][:, :69]))
        visits = mcts.search(ev, cpuct, noise=noise, eps=eps, testing=bool(testing), **opts).cpu().numpy()
        root, pv = cpu(mcts.root_edges()), cpu(mcts.principal_variation(16))
        for j, k in enumerate(ks):
            assert same(root["n"][j], f["visits"][k]) and same(root["n"][j], visits[j]), k
            for key in ("w", "q", "p"):
                assert same(root[key][j], r[key][k]), (k, key)
            assert same(root["value"][j], r["value"][k]), k
            assert ((root["child"][j] >= 0) >= (f["visits"][k] > 0)).all(), k
            for key in ("action", "visits", "q", "player"):
                assert same(pv[key][j], r["pv_" + key][k]), (k, key)
            assert pv["len"][j] == r["pv_len"][k], k
            checked += 1
        mcts.close()
        env.close()
    assert checked == 48 * copies


def drive(mcts, evaluator, sims, cpuct, noise, eps, testing, active=None, after=None):
    """A search through the per-simulation calls; after(s) runs after simulation s."""
    mcts.begin(active(0) if callable(active) else active)
    for s in range(sims):
        act = active(s) if callable(active) else active
        board, glob, _, count = mcts.select_gather(cpuct, act)
        k = int(count.item())
        policy, value = evaluator(board[:k], glob[:k]) if k else (mcts._nil_pol, mcts._nil_val)
        mcts.expand_backup(policy, value, noise, eps, testing, gathered=True)
        if after:
            after(s)


def test_report_calls_leave_search_unchanged():
    """Sixteen simulations on the 48 fixture positions, driven call by call,
    once plain and once with root_edges, principal_variation and export_tree
    called after every simulation: the same visits, tree sizes, root W and
    chance streams (the report reads, and never writes, tree, env or streams)."""
    from hzamd.mcts import BatchedMCTS, dense_stub_evaluator
    f = load("mcts_dense.npz")
    ks = list(range(48))
    noise = torch.from_numpy(np.ascontiguousarray(f["noise"][ks][:, :69]))
    out = []
    for report in (False, True):
        env = make_env(f["state"][ks], f["mt_seed"][ks])
        mcts = BatchedMCTS(env, 16)
        seen = []

        def after(s):
            root, pv = mcts.root_edges(), mcts.principal_variation(1 + s % 16)
            tree = mcts.export_tree((5 * s) % 48)
            seen.append((int(root["n"].sum()), int(pv["len"].sum()), len(tree["n"])))
        drive(mcts, dense_stub_evaluator, 16, 1.1, noise, 0.3, False, after=after if report else None)
        st, mt, idx = env.export_state(with_mt=True)
        out.append((mcts.result().cpu().numpy().copy(), mcts.stats().cpu().numpy().copy(),
                    mcts.root_edges()["w"].cpu().numpy(), st.cpu().numpy(), mt.cpu().numpy(), idx.cpu().numpy()))
        if report:  # the calls did see the growing trees
            assert [s[0] for s in seen] == [48 * s for s in range(16)] and seen[-1][1] >= 48 and seen[-1][2] > 0
        mcts.close()
        env.close()
    for a, b in zip(*out):
        assert same(a, b)
    assert out[0][0].sum() == 48 * 15 and (out[0][1][:, 3] == 0).all()


def test_report_edge_cases_in_one_ragged_batch():
    """130 boards; board 0 is left out by `active`, 63 is a stuck root, 64 a
    terminal root and 129 is searched for one simulation only (the others for
    eight).  The first three report no edge at all (0, 0.0, 0.0, 0.0, child
    -1, value 0.0, an empty line); the one-simulation root has its edges, with
    their priors and children and every N = 0, value 0.0 and an empty line;
    every other board's N equals hz_mcts_result and sums to seven.  hz_mcts_pv
    refuses max_len < 1 and > max_depth."""
    import hzamd._native as nat
    from hzamd.env import BatchedEnv, unpack_mask
    from hzamd.mcts import BatchedMCTS, stub_evaluator
    n, base, sims, cpuct = 130, 915, 8, 1.25
    left_out, stuck, terminal, one_sim = SPECIAL
    env = BatchedEnv(n, seed_base=base, device=DEV)
    env.reset()
    plies = torch.arange(n, device=DEV) % 41
    for p in range(41):
        mask, count = env.legal_mask()
        act = env.rule_actions(mask, count)
        env.step(torch.where(plies > p, act, torch.full_like(act, -1)))
    words = env.export_state().cpu().numpy().copy()
    words[:, stuck] = words_to_array([pack_ref(oracle.stuck_state(base + stuck)[0])])[0]
    words[:, terminal] = words_to_array([pack_ref(load("env_traces.npz")["finals"][3])])[0]
    env.import_state(torch.from_numpy(words))
    done = env.done().cpu().numpy()
    assert done[terminal] and done.sum() == 1
    legal = unpack_mask(env.legal_mask()[0]).cpu().numpy()
    assert not legal[stuck].any() and legal[one_sim].any()
    pol = stub_evaluator(*env.encode())[0].cpu().numpy()
    a_all = torch.ones(n, dtype=torch.uint8, device=DEV)
    a_all[left_out] = 0
    a_rest = a_all.clone()
    a_rest[one_sim] = 0
    mcts = BatchedMCTS(env, sims, max_depth=24)
    drive(mcts, stub_evaluator, sims, cpuct, None, 0.25, True, active=lambda s: a_all if s == 0 else a_rest)
    visits, counts = mcts.result().cpu().numpy().copy(), mcts.stats().cpu().numpy().copy()
    root, pv = cpu(mcts.root_edges()), cpu(mcts.principal_variation(24))
    assert same(root["n"], visits)
    assert [tuple(counts[b, :2]) for b in (left_out, stuck, terminal)] == [(0, 0), (1, 0), (1, 0)]
    for b in (left_out, stuck, terminal, one_sim):
        assert (root["n"][b] == 0).all() and (bits(root["w"][b]) == 0).all() and (bits(root["q"][b]) == 0).all(), b
        assert bits(root["value"][b]) == 0 and pv["len"][b] == 0, b
        assert (pv["action"][b] == -1).all() and (pv["visits"][b] == 0).all(), b
        assert (bits(pv["q"][b]) == 0).all() and (pv["player"][b] == 0).all(), b
    for b in (left_out, stuck, terminal):
        assert (bits(root["p"][b]) == 0).all() and (root["child"][b] == -1).all(), b
    # the one-simulation search: the root expanded, nothing backed up through an edge yet
    assert counts[one_sim, 1] == legal[one_sim].sum() and counts[one_sim, 0] > 1
    assert ((root["child"][one_sim] >= 0) == legal[one_sim]).all()
    assert same(root["p"][one_sim], np.where(legal[one_sim], pol[one_sim], np.float32(0)))
    kids = root["child"][one_sim][legal[one_sim]]
    assert kids.min() >= 1 and kids.max() < counts[one_sim, 0]
    for b in range(n):
        if b in SPECIAL:
            continue
        assert root["n"][b].sum() == sims - 1 and ((root["child"][b] >= 0) == legal[b]).all(), b
        assert 1 <= pv["len"][b] <= sims - 1 and pv["action"][b, 0] == np.argmax(visits[b]), b
        L = pv["len"][b]
        assert (pv["action"][b, L:] == -1).all() and (pv["visits"][b, L:] == 0).all(), b
    # refusals: nothing enqueued, the buffers keep their contents
    L = nat.lib()
    r = mcts.principal_variation(1)
    args = [nat.ptr(r[k]) for k in ("action", "visits", "q", "player", "len")]
    assert L.hz_mcts_pv(mcts._h, 0, *args) == -1 and L.hz_mcts_pv(mcts._h, 25, *args) == -1
    assert L.hz_mcts_pv(mcts._h, 24, None, *args[1:]) == -1
    assert L.hz_mcts_export_tree(mcts._h, n, *([None] * 9)) == -1
    assert L.hz_mcts_export_tree(mcts._h, -1, *([None] * 9)) == -1
    with pytest.raises(ValueError):
        mcts.principal_variation(0)
    with pytest.raises(ValueError):
        mcts.principal_variation(25)
    assert same(cpu(mcts.principal_variation(1))["action"][:, 0], pv["action"][:, 0])
    mcts.close()
    env.close()


def host_pv(t, max_len):
    """hz_mcts_pv's rule walked over an exported tree."""
    line, node = [], 0
    while len(line) < max_len and node < len(t["ne"]) and t["ne"][node] > 0:
        e0, ne = int(t["e0"][node]), int(t["ne"][node])
        i = int(np.argmax(t["n"][e0:e0 + ne]))  # the first among equals
        e = e0 + i
        if t["n"][e] == 0:
            break
        line.append((t["action"][e], t["n"][e], t["w"][e] / np.float64(t["n"][e]), t["player"][e]))
        node = int(t["child"][e])
    return line


def test_report_matches_exported_trees():
    """256 boards at plies 3 to 45 (hz_rollout), 64 simulations with the stub
    evaluator: a host walk of every board's export_tree reproduces
    principal_variation at max_len 1, 16 and max_depth and the root's slice
    reproduces root_edges; the trimmed sizes are hz_mcts_stats'."""
    from hzamd.env import BatchedEnv
    from hzamd.mcts import BatchedMCTS, stub_evaluator
    n, sims, depth = 256, 64, 64
    parts = []
    for i, plies in enumerate((3, 17, 31, 45)):
        part = BatchedEnv(64, seed_base=7700 + 64 * i, device=DEV)
        part.reset()
        part.rollout(max_plies=plies)
        parts.append([t.clone() for t in part.export_state(with_mt=True)])
        part.close()
    env = BatchedEnv(n, seed_base=7700, device=DEV)
    env.import_state(torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts]),
                     torch.cat([p[2] for p in parts]))
    active = ~env.done()
    assert int(active.sum()) > 200
    mcts = BatchedMCTS(env, sims, max_depth=depth)
    mcts.search(stub_evaluator, 1.5, active=active)
    counts = mcts.stats().cpu().numpy().copy()
    root = cpu(mcts.root_edges())
    pvs = {m: cpu(mcts.principal_variation(m)) for m in (1, 16, depth)}
    players = ((env.export_state()[5] >> 41) & 1).cpu().numpy()
    longest = 0
    for b in range(n):
        t = mcts.export_tree(b)
        assert (len(t["ne"]), len(t["n"])) == tuple(counts[b, :2]) and len(t["state"]) == counts[b, 0], b
        # the root's slice against root_edges
        want = {"n": np.zeros(143, np.int32), "w": np.zeros(143), "q": np.zeros(143),
                "p": np.zeros(143, np.float32), "child": np.full(143, -1, np.int32)}
        sw, sn = np.float64(0), 0
        if counts[b, 0]:
            for e in range(int(t["e0"][0]), int(t["e0"][0]) + max(0, int(t["ne"][0]))):
                a, k = t["action"][e], t["n"][e]
                want["n"][a], want["w"][a], want["p"][a], want["child"][a] = k, t["w"][e], t["p"][e], t["child"][e]
                want["q"][a] = t["w"][e] / np.float64(k) if k else 0.0
                sw, sn = sw + t["w"][e], sn + int(k)
                assert t["player"][e] == players[b], b
        for key, v in want.items():
            assert same(root[key][b], v), (b, key)
        assert same(root["value"][b], np.float64(sw / sn if sn else 0.0)), b
        assert sn == (sims - 1 if counts[b, 1] else 0), b
        # the line
        for m, pv in pvs.items():
            line = host_pv(t, m)
            assert pv["len"][b] == len(line), (b, m)
            for d, (a, k, q, pl) in enumerate(line):
                assert (pv["action"][b, d], pv["visits"][b, d], pv["player"][b, d]) == (a, k, pl), (b, m, d)
                assert same(pv["q"][b, d], q), (b, m, d)
            L = len(line)
            assert (pv["action"][b, L:] == -1).all() and (pv["visits"][b, L:] == 0).all(), (b, m)
            assert (bits(pv["q"][b, L:]) == 0).all() and (pv["player"][b, L:] == 0).all(), (b, m)
        longest = max(longest, int(pvs[depth]["len"][b]))
    assert 1 < longest < depth and (pvs[1]["len"] <= 1).all()
    mcts.close()
    env.close()


def test_selfplay_keeps_root_value():
    """64 boards, 8 simulations, 6 plies: keep_root_value changes nothing that
    was recorded before; root_value[t] is root_edges()["value"] of move t's
    search, as a hand-driven run of the same moves reads it; compact()'s q is
    that value in f32 from the recorded player's side (the recorded player is
    the mover of every root edge, whose W the value sums)."""
    from hzamd.mcts import stub_evaluator
    from hzamd.selfplay import SelfPlay
    cfg = {"num_simulations": 8}
    recs = {}
    for keep in (False, True):
        sp = SelfPlay(64, stub_evaluator, cfg, seed_base=31, device=DEV, max_plies=6, keep_root_value=keep)
        recs[keep] = rec = sp.play()
        if keep:
            comp = sp.compact(rec)
            # the continuous form records it too, one row per move (no game ends in three moves)
            steady = sp.play_steady(3)
            assert steady["root_value"].dtype == torch.float64 and tuple(steady["root_value"].shape) == (3, 64)
            assert torch.equal(steady["root_value"][2], sp.last_root_value)
            cs = sp.compact_steady(steady)
            assert cs["q"].dtype == torch.float32 and cs["q"].shape == cs["z"].shape
        else:
            assert "root_value" not in rec and "q" not in sp.compact(rec)
            assert sp.last_root_value is None
        sp.mcts.close()
        sp.env.close()
    off, on = recs[False], recs[True]
    assert sorted(set(on) - set(off)) == ["root_value"] and on["plies"] == off["plies"] == 6
    for key in ("states", "visits", "valid", "final", "players"):
        assert torch.equal(on[key], off[key]), key
    rv = on["root_value"]
    assert rv.dtype == torch.float64 and tuple(rv.shape) == (6, 64) and bool(on["valid"].all())
    sp = SelfPlay(64, stub_evaluator, cfg, seed_base=31, device=DEV, max_plies=6)
    sp.env.reset()
    for t in range(6):
        sp.move(t)
        root, pv = sp.mcts.root_edges(), sp.mcts.principal_variation(1)
        assert same(root["value"].cpu().numpy(), rv[t].cpu().numpy()), t
        assert torch.equal(root["n"], on["visits"][t]), t
        # the side: the root edges' mover is the recorded player
        assert bool((pv["len"] == 1).all()) and torch.equal(pv["player"][:, 0].to(torch.int8), on["players"][t]), t
        assert bool((root["n"].sum(1) == 7).all()), t
    sp.check_steps()
    sp.mcts.close()
    sp.env.close()
    assert comp["q"].dtype == torch.float32 and comp["q"].shape == comp["z"].shape
    assert same(comp["q"].cpu().numpy(), rv[on["valid"]].to(torch.float32).cpu().numpy())
    assert float(rv.abs().max()) > 0 and bool((rv < 0).any()) and bool((rv > 0).any())


class _DenseManager:
    def predict(self, board, glob):
        from hzamd.mcts import dense_stub_evaluator
        p, v = dense_stub_evaluator(board.unsqueeze(0), glob.unsqueeze(0))
        return p[0].numpy(), float(v[0])


@pytest.mark.parametrize("k", [0, 6])
def test_dropin_last_search_returns_reference_root_edges(k):
    """A fixture row (k = 0: noise mixed into the root, 6: testing) through
    the drop-in's get_best_action_and_pi: the move, pi and Python stream are
    the fixture's as before, and last_search().get_root_edges() holds the
    reference's N, W, Q and P for every legal move, in ascending action order."""
    import harmonies_engine as he
    import MCTS
    import process_game_state as pgs
    from hzamd.state import apply_ref_to_object
    f, r = load("mcts_dense.npz"), load("mcts_report.npz")
    sims = int(f["sims"][k])
    assert sims == 16 and bool(f["testing"][k]) == (k == 6)
    obj = apply_ref_to_object(f["state"][k], he.HarmoniesGameState.__new__(he.HarmoniesGameState))
    cfg = {"num_simulations": sims, "cpuct": float(f["cpuct"][k]), "dirichlet_alpha": 0.4,
           "dirichlet_epsilon": float(f["eps"][k]), "turns_until_tau0": int(f["tau0"][k]),
           "action_size": 143, "testing": bool(f["testing"][k])}
    noise, u = f["noise"][k], float(f["u"][k])

    def fake_dirichlet(alpha):
        return noise[:len(alpha)].copy()

    def fake_choice(n, p):
        T = sims - 1
        c = np.rint(np.asarray(p) * T).astype(np.int64)
        return int(np.argmax(u * T < np.cumsum(c)))

    saved = (np.random.dirichlet, np.random.choice)
    np.random.dirichlet, np.random.choice = fake_dirichlet, fake_choice
    try:
        random.seed(int(f["mt_seed"][k]))
        mv, pi = MCTS.get_best_action_and_pi(obj, _DenseManager(), cfg, int(f["ply"][k]))
        nxt = random.getrandbits(32)
    finally:
        np.random.dirichlet, np.random.choice = saved
    assert np.array_equal(pi, f["pi"][k]) and pgs.get_action_index(mv) == f["action"][k] and nxt == f["next_word"][k]
    tree = MCTS.last_search()
    assert isinstance(tree, MCTS.MCTS) and tree.root.state is obj and tree.mcts_config is cfg
    edges = tree.get_root_edges()
    assert edges is tree.root.edges
    acts = [pgs.get_action_index(m) for m in edges]
    legal = [pgs.get_action_index(m) for m in obj.get_legal_moves()]
    assert acts == legal == sorted(acts) and len(acts) > 1
    for m, e in edges.items():
        a, s = pgs.get_action_index(m), e.stats
        assert e.action == m and e.out_node is None and e.current_player == obj.current_player
        assert type(s["N"]) is int and type(s["W"]) is float and type(s["Q"]) is float and type(s["P"]) is np.float32
        assert s["N"] == f["visits"][k][a], a
        assert same(np.float64(s["W"]), r["w"][k][a]) and same(np.float64(s["Q"]), r["q"][k][a]), a
        assert same(s["P"], r["p"][k][a]), a
    assert sum(e.stats["N"] for e in edges.values()) == sims - 1
