"""Host model of tree reuse (hz_mcts_advance / hz_mcts_begin_carried and the
search that continues on a carried tree).  A helper, not a test.

It restates, in NumPy over the C oracle's rules (oracle.step / legal /
canonical / stub_eval / dense_stub_eval), the whole rule include/hz_abi.h
states: the carry conditions, the kept sub-DAG's numbering (the played child
becomes node 0, the others follow in ascending old id; edge blocks keep their
pool order), the root mix of a carried root, and the PUCT search with the
arithmetic the README states (cpuct * P an fp32 product, W and Q in fp64, the
first strict '>' wins, children in ascending action order, transposition by
canonical key, self-loops skipped, turn-end draws from the board's stream in
child order).  From an empty tree it is oracle.mcts_search
(tests/test_mcts_carry_cpu.py), which licenses it as the yardstick of
tests/test_mcts_carry_gpu.py.

Trees are held in BatchedMCTS.export_tree's form: per node state, e0, ne
(-1 terminal, 0 unexpanded), per edge action, child, n, w (fp64), p (fp32),
player.  carry_tree works on any such dict (a node's state is a row: six u64
words from the device, or the 78 int16 of the host form)."""
import ctypes

import numpy as np

import oracle
from hzamd.state import pack_ref

EDGE_KEYS = ("action", "child", "n", "w", "p", "player")
EDGE_DTYPES = {"action": np.int16, "child": np.int32, "n": np.int32, "w": np.float64, "p": np.float32,
               "player": np.uint8}


def game_over(st):
    return bool(st[74]) and int(st[75]) != -2


def copy_mt(m):
    return oracle.mt_from_words(*m.words())


def next_word(m):
    """The stream's next 32-bit word (the stream itself is left alone)."""
    return oracle.mt_next32(copy_mt(m))


def topup_budget(carried, num_simulations, min_sims):
    """The "topup" rule of self-play: clamp(num_simulations - carried visits,
    min_sims, num_simulations), in int64."""
    carried = np.asarray(carried, np.int64)
    return np.clip(int(num_simulations) - carried, int(min_sims), int(num_simulations))


def mix(p, eps, noise_i):
    """The root mix of one prior (MCTS.py:323 as the expansion computes it)."""
    a32 = np.float32(np.float32(1.0 - eps) * np.float32(p))
    return np.float32(np.float64(a32) + np.float64(eps) * np.float64(noise_i))


def carry_tree(tree, action, env_state, headroom, max_nodes, active=True):
    """The carry rule.  tree: export_tree's dict (None or no nodes: no tree);
    env_state: the board's state after the step, in the form of tree["state"]
    rows.  Returns (new tree or None when dropped, (nodes, edges, visits),
    diagnostics: the old ids kept, in new-id order)."""
    drop = (None, (0, 0, 0), None)
    if not active or tree is None or len(tree["e0"]) == 0 or action < 0:
        return drop
    e0, ne, child = tree["e0"], tree["ne"], tree["child"]
    root = range(int(e0[0]), int(e0[0]) + max(int(ne[0]), 0))
    hit = [e for e in root if int(tree["action"][e]) == int(action)]
    if not hit:
        return drop
    c = int(child[hit[0]])
    if int(ne[c]) < 0 or not np.array_equal(np.asarray(tree["state"][c]), np.asarray(env_state)):
        return drop
    seen, stack = {c}, [c]
    while stack:
        v = stack.pop()
        for e in range(int(e0[v]), int(e0[v]) + max(int(ne[v]), 0)):
            k = int(child[e])
            if k not in seen:
                seen.add(k)
                stack.append(k)
    nodes = [c] + sorted(seen - {c})
    blocks = sorted((int(e0[v]), int(ne[v])) for v in nodes if int(ne[v]) > 0)
    edges = [e for b0, cnt in blocks for e in range(b0, b0 + cnt)]
    if len(nodes) + headroom > max_nodes or len(edges) + headroom > max_nodes:
        return drop
    new_id = {v: i for i, v in enumerate(nodes)}
    new_edge = {e: i for i, e in enumerate(edges)}
    out = {"state": np.stack([np.asarray(tree["state"][v]) for v in nodes]),
           "ne": np.array([ne[v] for v in nodes], np.int32),
           "e0": np.array([new_edge[int(e0[v])] if int(ne[v]) > 0 else 0 for v in nodes], np.int32)}
    for k in EDGE_KEYS:
        out[k] = np.asarray(tree[k])[edges].astype(EDGE_DTYPES[k]) if edges else np.zeros(0, EDGE_DTYPES[k])
    out["child"] = np.array([new_id[int(child[e])] for e in edges], np.int32)
    r0, rn = int(out["e0"][0]), max(int(out["ne"][0]), 0)
    return out, (len(nodes), len(edges), int(out["n"][r0:r0 + rn].sum())), nodes


class CarryModel:
    """One board: its env state and stream, and its search tree."""

    def __init__(self, ref_state, mt, evaluator=0, exact_keys=False, max_nodes=None):
        self.env = np.array(ref_state, np.int16)
        self.mt = mt
        self.eval = oracle.dense_stub_eval if evaluator else oracle.stub_eval
        self.pyhash = not exact_keys
        self.max_nodes = max_nodes  # None: unbounded
        self.flag = 0
        self.carried = False
        self.tree = None
        self.keys, self.index = [], {}
        self.first_edge = None  # the first edge the last search() selected at the root

    # -- tree storage: export form, edges in Python lists while searching -----
    def _load(self, tree, keys):
        self.state = [np.asarray(s) for s in tree["state"]]
        self.e0, self.ne = [int(x) for x in tree["e0"]], [int(x) for x in tree["ne"]]
        self.E = {k: np.asarray(tree[k]).astype(EDGE_DTYPES[k]).tolist() for k in EDGE_KEYS}
        self.keys = list(keys)
        self.index = {k: i for i, k in enumerate(self.keys)}
        self.tree = True

    def fresh(self):
        key = oracle.canonical(self.env, self.pyhash)
        self._load({"state": [self.env.copy()], "e0": [0], "ne": [0], **{k: [] for k in EDGE_KEYS}}, [key])
        self.flag = 0

    def export(self, words=True):
        """The tree in export_tree's form (words: states as six u64 words)."""
        if not self.tree:
            return None
        st = (np.array([pack_ref(s) for s in self.state], np.uint64) if words
              else np.stack(self.state).astype(np.int16))
        out = {"state": st, "e0": np.array(self.e0, np.int32), "ne": np.array(self.ne, np.int32)}
        out.update({k: np.array(self.E[k], EDGE_DTYPES[k]) for k in EDGE_KEYS})
        return out

    def counts(self):
        return (len(self.e0), len(self.E["n"])) if self.tree else (0, 0)

    def root_edges(self):
        return range(self.e0[0], self.e0[0] + max(self.ne[0], 0)) if self.tree else range(0)

    def visits(self):
        v = np.zeros(143, np.int32)
        for e in self.root_edges():
            v[self.E["action"][e]] = self.E["n"][e]
        return v

    # -- between searches -------------------------------------------------------
    def play(self, action):
        """hz_step on the board (the real move: a turn end draws from the
        stream where the search left it)."""
        status, self.env = oracle.step(self.env, int(action), self.mt)
        assert status == 0, status
        return self.env

    def advance(self, action, headroom, active=True):
        """hz_mcts_advance after play(action).  Returns info (nodes, edges, visits)."""
        tree = self.export(words=False) if self.tree else None
        cap = self.max_nodes if self.max_nodes is not None else 1 << 62
        new, info, kept = carry_tree(tree, int(action), self.env, headroom, cap, active)
        self.carried = new is not None
        if new is None:
            self.tree = None
        else:
            self._load(new, [self.keys[v] for v in kept])
            self.flag = 0
        return info

    def begin(self, noise=None, eps=0.25, noisy=False, carry=True):
        """hz_mcts_begin_carried (carry=False: hz_mcts_begin).  Returns True
        when the search starts from a carried tree."""
        keep = carry and self.carried and self.tree and np.array_equal(self.state[0], self.env)
        self.carried = False
        if not keep:
            self.fresh()
            return False
        self.flag = 0
        if noisy and noise is not None and self.ne[0] > 0:
            legal = np.flatnonzero(oracle.legal(self.env))
            rank = {int(a): i for i, a in enumerate(legal)}
            for e in self.root_edges():
                self.E["p"][e] = float(mix(self.E["p"][e], eps, noise[rank[int(self.E["action"][e])]]))
        return True

    # -- the simulations --------------------------------------------------------
    def _select(self, node, cpuct):
        e0, ne = self.e0[node], self.ne[node]
        n = np.array(self.E["n"][e0:e0 + ne], np.int32)
        w = np.array(self.E["w"][e0:e0 + ne], np.float64)
        p = np.array(self.E["p"][e0:e0 + ne], np.float32)
        ns = int(n.sum())
        sqrt_ns = np.sqrt(np.float64(ns if ns > 1 else 1))
        cp = np.float32(cpuct) * p  # fp32 product
        u = cp.astype(np.float64) * sqrt_ns / (1 + n).astype(np.float64)
        q = np.divide(w, n.astype(np.float64), out=np.zeros_like(w), where=n > 0)
        return e0 + int(np.argmax(q + u))  # the first of the largest: the first strict '>'

    def search(self, sims, cpuct, noise=None, eps=0.25, noisy=False, max_depth=None):
        """`sims` simulations on the tree begin() left (MCTS.py:291-352)."""
        E = self.E
        self.first_edge = None
        for _ in range(int(sims)):
            node, path = 0, []
            while self.ne[node] > 0:
                if max_depth is not None and len(path) >= max_depth:
                    self.flag = 1
                    break
                sel = self._select(node, cpuct)
                if node == 0 and self.first_edge is None:
                    self.first_edge = sel - self.e0[0]
                path.append(sel)
                node = int(E["child"][sel])
            st = self.state[node]
            player = int(st[72])
            if game_over(st):
                outcome = 1 if st[75] == 0 else -1 if st[75] == 1 else 0
                value = float(outcome if player == 0 else -outcome) if outcome else 0.0
            else:
                pol, value = self.eval(st)
                legal = np.flatnonzero(oracle.legal(st))
                if node == 0 and noisy and noise is not None:
                    for i, a in enumerate(legal):
                        pol[a] = mix(pol[a], eps, noise[i])
                if len(legal) and self.ne[node] == 0:
                    self._expand(node, st, legal, pol, player)
            for e in path:
                E["n"][e] += 1
                E["w"][e] = E["w"][e] + float(value) * (1.0 if E["player"][e] == player else -1.0)

    def _expand(self, node, st, legal, pol, player):
        E = self.E
        base_n, base_e = len(self.e0), len(E["n"])
        new_nodes, new_edges = [], []
        local = {}
        # oracle.step and oracle.canonical for every child, on one block of
        # rows (the library called directly: a wrapper call per child costs more than the rules)
        L, mt = oracle.lib(), ctypes.byref(self.mt)
        rows = np.repeat(np.ascontiguousarray(st, np.int16)[None], len(legal), 0)
        kbuf = np.zeros((len(legal), 128), np.uint8)
        r0, k0, pyhash = rows.ctypes.data, kbuf.ctypes.data, int(self.pyhash)
        for i, a in enumerate(legal):
            status = L.or_step(r0 + 156 * i, int(a), mt)
            assert status == 0, status
            L.or_canonical(r0 + 156 * i, k0 + 128 * i, pyhash)
        for i, a in enumerate(legal):
            ch, key = rows[i], kbuf[i].tobytes()
            c = self.index.get(key, local.get(key))
            if c == node:
                continue  # a self-loop child (MCTS.py:189-194)
            if c is None:
                c = local[key] = base_n + len(new_nodes)
                new_nodes.append((ch, key))
            new_edges.append((int(a), c))
        if self.max_nodes is not None and (base_n + len(new_nodes) > self.max_nodes or
                                           base_e + len(new_edges) > self.max_nodes):
            self.flag = 1  # refused whole; the children's draws are kept
            return
        for ch, key in new_nodes:
            self.index[key] = len(self.e0)
            self.keys.append(key)
            self.state.append(ch)
            self.e0.append(0)
            self.ne.append(-1 if game_over(ch) else 0)
        k = len(new_edges)  # (plain Python numbers: the same IEEE doubles, every fp32 prior exact in one)
        E["action"].extend(a for a, _ in new_edges)
        E["child"].extend(c for _, c in new_edges)
        E["n"].extend([0] * k)
        E["w"].extend([0.0] * k)
        E["p"].extend(pol[[a for a, _ in new_edges]].tolist())
        E["player"].extend([player] * k)
        self.e0[node], self.ne[node] = base_e, len(new_edges)


def choose(visits, explore, u):
    """hzamd.mcts.choose_actions for one board."""
    v = np.asarray(visits, np.int64)
    total = int(v.sum())
    if total == 0:
        return -1
    if explore:
        return int(np.argmax(np.float64(u) * np.float64(total) < np.cumsum(v).astype(np.float64)))
    return int(np.argmax(v))


# The boards the carry tests share (tests/test_mcts_carry_cpu.py shows, with
# this model, that they hold every case the device tests rely on)
FIXTURE = {"base": 4100, "n": 130, "spread": 41, "sims": 32, "cpuct": 1.25, "evaluator": 1, "eps": 0.3}


def fixture_action(b, n_by_action, has_edge):
    """The move board b plays in the shared fixture, from its root's visits
    by action and the actions that have a root edge: by b % 4 the most
    visited edge (0, 3), one sampled in proportion to the visits (1), or the
    first of the least visited edges (2: usually an unexpanded child)."""
    v = np.where(has_edge, np.asarray(n_by_action, np.int64), 0)
    if not np.any(has_edge):
        return -1
    if b % 4 == 1 and v.sum() > 0:
        return choose(v, True, (b * 0.6180339887) % 1.0)
    if b % 4 == 2:
        return int(np.argmin(np.where(has_edge, v, 1 << 40)))
    return int(np.argmax(np.where(has_edge, v, -1)))


def positions(base, n, spread=41):
    """n boards at assorted points of rule-driven games: board b is reset
    after random.seed(base + b) and advanced b % spread rule plies (a board
    whose game would have ended is left one ply short of it).  Returns the
    boards' (ref state, stream) pairs."""
    out = []
    for b in range(n):
        plies = b % spread
        while True:
            m = oracle.mt_seed(base + b)
            st, _, _ = oracle.play_rule_from(oracle.reset(m), m, base + b, 0, plies)
            if not game_over(st) and oracle.legal(st).any():
                break
            plies -= 1
        out.append((st, m))
    return out
