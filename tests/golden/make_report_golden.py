"""Golden capture of the search report (TEST INFRASTRUCTURE, CPU only).

Like make_golden.py, whose helpers it imports, this runs only where the
reference checkout is mounted; the tests read the .npz it writes.

  mcts_report.npz    for each of the 48 rows of the committed mcts_dense.npz,
                     the reference's own get_best_action_and_pi rebuilt from
                     the row's fields (state, mt_seed, sims, cpuct, eps,
                     testing, tau0, ply, u, the stored noise vector returned
                     by the patched np.random.dirichlet, the dense stub
                     manager, canonical move order), and from the tree it
                     leaves: the root edges' W and Q (f64 [48,143]) and P
                     (f32) by action id, value = sum W / sum N over the root's
                     edges in edge order (f64 [48]), and the principal
                     variation at max_len 16 walked over the reference's Node
                     and Edge objects (at every node the first edge with the
                     most visits; stop at a node without edges, an edge with
                     N == 0, or 16 moves): pv_action int16, pv_visits int32,
                     pv_q f64 (the edge's Q), pv_player uint8 (the edge's
                     current_player) [48,16] with -1 / 0 / 0.0 / 0 past
                     pv_len int32 [48].  `numpy_version` as in mcts_dense.npz.

Before anything is written, every row's visits, action, next_word, n_nodes
and n_edges must equal the committed row.  At least one principal-variation
level must have two edges tied for the most visits (the tie rule is then
exercised); the 48 rows give several, so no further rows were added.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_report_golden.py
"""
import io
import os
import random
import zipfile

import numpy as np

import make_golden as mg

PV_LEN = 16


def search_row(he, pgs, mcts_mod, f, k, sorted_coords, manager, last):
    """Row k of mcts_dense.npz through the reference; returns (tree, move, next MT word)."""
    sims, noise, u = int(f["sims"][k]), f["noise"][k], float(f["u"][k])
    cfg = {"num_simulations": sims, "cpuct": float(f["cpuct"][k]), "dirichlet_alpha": float(f["alpha"][k]),
           "dirichlet_epsilon": float(f["eps"][k]), "fpu_value": 0.25, "turns_until_tau0": int(f["tau0"][k]),
           "action_size": 143, "testing": bool(f["testing"][k])}

    def fake_dirichlet(alpha):
        return noise[:len(alpha)].copy()

    def fake_choice(nact, p):
        T = sims - 1
        c = np.rint(np.asarray(p, np.float64) * T).astype(np.int64)
        assert c.sum() == T
        return int(np.argmax(u * T < np.cumsum(c)))

    saved = (np.random.dirichlet, np.random.choice)
    np.random.dirichlet, np.random.choice = fake_dirichlet, fake_choice
    try:
        g = mg.state_from_ref(he, f["state"][k], sorted_coords)
        random.seed(int(f["mt_seed"][k]))
        mv, _ = mcts_mod.get_best_action_and_pi(g, manager, cfg, int(f["ply"][k]))
        nxt = random.getrandbits(32)
    finally:
        np.random.dirichlet, np.random.choice = saved
    return last["tree"], mv, nxt


def principal_variation(root, max_len):
    """(edges of the line, levels with a tie for the most visits)."""
    line, ties, node = [], 0, root
    while len(line) < max_len and node.edges:
        edges = list(node.edges.values())
        best = edges[0]
        for e in edges[1:]:
            if e.stats["N"] > best.stats["N"]:  # strict: the first among equals stays
                best = e
        if best.stats["N"] == 0:
            break
        ties += sum(e.stats["N"] == best.stats["N"] for e in edges) > 1
        line.append(best)
        node = best.out_node
    return line, ties


def save_npz(path, **arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give
    the same bytes on every run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    he, pgs, mcts_mod = mg.import_reference()
    import constants as C
    sorted_coords = list(C.sorted_coords)
    f = np.load(os.path.join(mg.OUT, "mcts_dense.npz"))
    n = len(f["sims"])
    assert n == 48

    orig_legal = he.HarmoniesGameState.get_legal_moves
    he.HarmoniesGameState.get_legal_moves = lambda self: sorted(orig_legal(self), key=pgs.get_action_index)
    last = {}
    orig_init = mcts_mod.MCTS.__init__

    def init(self, root, cfg):
        orig_init(self, root, cfg)
        last["tree"] = self
    mcts_mod.MCTS.__init__ = init

    w = np.zeros((n, 143), np.float64)
    q = np.zeros((n, 143), np.float64)
    p = np.zeros((n, 143), np.float32)
    value = np.zeros(n, np.float64)
    pv_action = np.full((n, PV_LEN), -1, np.int16)
    pv_visits = np.zeros((n, PV_LEN), np.int32)
    pv_q = np.zeros((n, PV_LEN), np.float64)
    pv_player = np.zeros((n, PV_LEN), np.uint8)
    pv_len = np.zeros(n, np.int32)
    tie_levels = zero_n = 0
    try:
        manager = mg.DenseStubManager()
        for k in range(n):
            tree, mv, nxt = search_row(he, pgs, mcts_mod, f, k, sorted_coords, manager, last)
            visits = np.zeros(143, np.int32)
            sw, sn = 0.0, 0
            for a, e in tree.root.edges.items():
                i = pgs.get_action_index(a)
                st = e.stats
                assert isinstance(st["P"], np.float32) and isinstance(st["W"], (int, float))
                assert st["Q"] == (st["W"] / st["N"] if st["N"] else 0)
                visits[i], w[k, i], q[k, i], p[k, i] = st["N"], st["W"], st["Q"], st["P"]
                sw += float(st["W"])
                zero_n += st["N"] == 0
                sn += st["N"]
            order = [pgs.get_action_index(a) for a in tree.root.edges]
            assert order == sorted(order)
            assert (visits == f["visits"][k]).all(), k
            assert pgs.get_action_index(mv) == f["action"][k], k
            assert nxt == f["next_word"][k], k
            assert len(tree.tree) == f["n_nodes"][k], k
            assert sum(len(nd.edges) for nd in tree.tree.values()) == f["n_edges"][k], k
            value[k] = sw / sn if sn else 0.0
            line, ties = principal_variation(tree.root, PV_LEN)
            tie_levels += ties
            pv_len[k] = len(line)
            for d, e in enumerate(line):
                pv_action[k, d] = pgs.get_action_index(e.action)
                pv_visits[k, d] = e.stats["N"]
                pv_q[k, d] = e.stats["Q"]
                pv_player[k, d] = e.current_player
    finally:
        he.HarmoniesGameState.get_legal_moves = orig_legal
        mcts_mod.MCTS.__init__ = orig_init
    assert tie_levels > 0, "no principal-variation level has a tie: add rows from env_traces.npz"
    out = os.path.join(mg.OUT, "mcts_report.npz")
    save_npz(out, w=w, q=q, p=p, value=value, pv_action=pv_action, pv_visits=pv_visits, pv_q=pv_q,
             pv_player=pv_player, pv_len=pv_len, numpy_version=np.array(np.__version__))
    print("mcts_report.npz", os.path.getsize(out), "tie levels", tie_levels, "pv_len", pv_len.min(), pv_len.max(),
          "root edges with N = 0:", zero_n)


if __name__ == "__main__":
    main()
