"""The search report without a GPU: tests/golden/mcts_report.npz (the
reference's root-edge W, Q, P, root value and principal variation for the 48
searches of mcts_dense.npz) is consistent with mcts_dense.npz and with
itself, bit for bit; the three report entry points are exported, bound and
refuse a NULL handle; the drop-in's record builder turns root-edge arrays
into the reference's Edge records."""
import os

import numpy as np

from conftest import GOLDEN

NEW = ("hz_mcts_root_edges", "hz_mcts_pv", "hz_mcts_export_tree")


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def test_report_fixture_consistent_with_dense_fixture():
    d, r = load("mcts_dense.npz"), load("mcts_report.npz")
    n = d["visits"].astype(np.int64)
    w, q, p = r["w"], r["q"], r["p"]
    assert w.shape == q.shape == p.shape == n.shape == (48, 143)
    assert (w.dtype, q.dtype, p.dtype, r["value"].dtype) == (np.float64, np.float64, np.float32, np.float64)
    assert str(r["numpy_version"]) == str(d["numpy_version"])
    # q == w / n where visited (one fp64 division), +0.0 elsewhere; unvisited edges hold W = +0.0
    vis = n > 0
    assert (bits(q[vis]) == bits(w[vis] / n[vis])).all()
    assert (bits(q[~vis]) == 0).all() and (bits(w[~vis]) == 0).all()
    assert int((~vis & (p != 0)).sum()) > 300  # plenty of root edges with a prior and no visit
    # value: sum W / sum N over the root's edges in ascending action (= edge) order
    for k in range(48):
        sw = 0.0
        for a in range(143):  # actions without an edge add +0.0: the sum's bits do not change
            sw += float(w[k, a])
        want = sw / int(n[k].sum()) if n[k].sum() else 0.0
        assert bits(np.float64(want)) == bits(r["value"][k]), k
    # the principal variation starts with the first most-visited root edge
    ln = r["pv_len"]
    assert ln.min() >= 0 and ln.max() <= 16 and len(set(ln.tolist())) > 4
    rows = np.flatnonzero(ln > 0)
    assert len(rows) > 40 and (n[ln == 0] == 0).all()
    first = np.argmax(n, axis=1)[rows]  # (argmax: the first among equals)
    assert (r["pv_action"][rows, 0] == first).all()
    assert (r["pv_visits"][rows, 0] == n[rows, first]).all()
    assert (bits(r["pv_q"][rows, 0]) == bits(q[rows, first])).all()
    assert (r["pv_player"][rows, 0] == d["state"][rows, 72]).all()  # the root's mover
    for k in range(48):
        L = ln[k]
        assert (r["pv_visits"][k, :L] > 0).all() and (r["pv_action"][k, :L] >= 0).all()
        assert (r["pv_action"][k, L:] == -1).all() and (r["pv_visits"][k, L:] == 0).all()
        assert (bits(r["pv_q"][k, L:]) == 0).all() and (r["pv_player"][k, L:] == 0).all()
    # the tie rule is exercised: some root has two edges tied for the most visits
    tied = [k for k in range(48) if ln[k] > 0 and (n[k] == n[k].max()).sum() > 1]
    assert tied, "no principal-variation level with a tie"


def test_report_symbols_exported_bound_and_refuse_null():
    import hzamd._native as nat
    from test_abi_cpu import declared_symbols
    assert set(NEW) <= set(declared_symbols())
    assert set(NEW) <= set(nat.exported_symbols())
    L = nat.lib()
    assert L.hz_env_size(None) == -1
    assert L.hz_mcts_root_edges(None, None, None, None, None, None, None) == -1
    assert L.hz_mcts_pv(None, 16, None, None, None, None, None) == -1
    assert L.hz_mcts_export_tree(None, 0, *([None] * 9)) == -1


def test_dropin_root_edge_records_equal_fixture():
    import MCTS
    import process_game_state as pgs
    d, r = load("mcts_dense.npz"), load("mcts_report.npz")

    class Root:
        current_player = 1

    for k in range(48):
        n, w, q, p = d["visits"][k], r["w"][k], r["q"][k], r["p"][k]
        # an edge exists for every legal move: the fixture's visited or prior-carrying actions at least
        has = (n > 0) | (p != 0)
        child = np.where(has, 7, -1).astype(np.int32)
        edges = MCTS.root_edge_records(Root, n, w, q, p, child)
        acts = [pgs.get_action_index(mv) for mv in edges]
        assert acts == np.flatnonzero(has).tolist()  # keyed by move, ascending action order
        for mv, e in edges.items():
            a = pgs.get_action_index(mv)
            s = e.stats
            assert e.action == mv and e.out_node is None and e.current_player == 1
            assert list(s) == ["N", "W", "Q", "P"]
            assert type(s["N"]) is int and type(s["W"]) is float and type(s["Q"]) is float
            assert type(s["P"]) is np.float32
            assert s["N"] == n[a] and bits(np.float64(s["W"])) == bits(w[a]) and bits(np.float64(s["Q"])) == bits(q[a])
            assert bits(s["P"]) == bits(p[a])
