"""Host model of the Gumbel root (hz_mcts_set_gumbel: sequential halving at the
root, improved-policy targets).  A helper, not a test.

A CarryModel (tests/mcts_carry_model.py) whose choice at node 0 is the rule
include/hz_abi.h states, restated here in NumPy float64, one IEEE operation at
a time; below the root it is the PUCT model unchanged.  The model takes each
root edge's G + log P as an input (`score0`, by root edge index): the device
tests feed it the values the device exported (hz_mcts_root_gumbel_scores), so
the one transcendental is the device's; the CPU tests let it take np.log.
The table, the butterfly sums and the host form of hz_root_gumbel's generator
are restated here too, independently of hzamd."""
import functools
import math

import numpy as np

import oracle
from mcts_carry_model import CarryModel

M64 = (1 << 64) - 1


# The draws the fixture tests share: hz_root_gumbel's key for the 130 boards of
# mcts_carry_model.FIXTURE (tests/test_mcts_gumbel_cpu.py shows that a root with
# 69 edges then visits an edge past lane 63)
GUMBEL_KEY = {"seed": 7, "board_base": 4100, "move": 3}


@functools.lru_cache(maxsize=None)
def considered_visits(m, n_root):
    """Row m of the considered-visit table for n_root root visits."""
    if m <= 1:
        return list(range(n_root))
    log2m = math.ceil(math.log2(m))
    seq, visits, k = [], np.zeros(m, np.int64), m
    while len(seq) < n_root:
        for _ in range(max(1, int(n_root / (log2m * k)))):
            seq.extend(int(x) for x in visits[:k])
            visits[:k] += 1
        k = max(2, k // 2)
    return seq[:n_root]


def butterfly(terms):
    """The sum of up to 128 float64 terms as the wave takes it: lane l starts
    with term l plus term l + 64, then v[l] += v[l ^ off], off = 1 .. 32."""
    a = np.zeros(128, np.float64)
    a[:len(terms)] = terms
    v = a[:64] + a[64:]
    lanes = np.arange(64)
    for off in (1, 2, 4, 8, 16, 32):
        v = v + v[lanes ^ off]
    assert (v == v[0]).all()
    return np.float64(v[0])


def sigma(n, w, p, v_root, c_visit, c_scale):
    """(sigma per edge, v_mix, max N) from the root's N (int), W (f64), P (f32)."""
    n = np.asarray(n, np.int64)
    w = np.asarray(w, np.float64)
    p64 = np.asarray(p, np.float32).astype(np.float64)
    t = int(n.sum())
    vis = n > 0
    q = np.divide(w, n.astype(np.float64), out=np.zeros_like(w), where=vis)
    sp = butterfly(np.where(vis, p64, 0.0))
    spq = butterfly(np.where(vis, p64 * q, 0.0))
    wq = spq / sp if sp > 0.0 else np.float64(0.0)
    v_mix = (np.float64(v_root) + np.float64(t) * wq) / np.float64(t + 1)
    cq = np.where(vis, q, v_mix)
    mn, mx = cq.min(), cq.max()
    den = max(mx - mn, np.float64(1e-8))
    max_n = int(n.max())
    scale = (np.float64(c_visit) + np.float64(max_n)) * np.float64(c_scale)
    return scale * ((cq - mn) / den), v_mix, max_n


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def host_gumbel(n, seed, board_base, move):
    """hz_root_gumbel on the host: f64 [n, 69] (np.log: within an ulp or two of the device's)."""
    out = np.zeros((n, 69), np.float64)
    for b in range(n):
        key = mix64(mix64(mix64(seed ^ 0x6A09E667F3BCC908) ^ ((board_base + b) & M64)) ^ move)
        for c in range(69):
            z = mix64((mix64(key ^ ((0xA0761D6478BD642F * (c + 1)) & M64)) + 0x9E3779B97F4A7C15) & M64)
            out[b, c] = (float(z >> 12) + 0.5) * 2.0 ** -52
    return -np.log(-np.log(out))


class GumbelModel(CarryModel):
    """One board under search(root="gumbel").  gumbel: G by legal rank (the
    scores are then G + np.log(P), taken where node 0 is expanded), or score0:
    G + log P by root edge index, as the device exported it."""

    def __init__(self, ref_state, mt, evaluator=0, sims=32, max_considered=16, c_visit=50.0, c_scale=1.0,
                 gumbel=None, score0=None, **kw):
        super().__init__(ref_state, mt, evaluator, **kw)
        self.n_root = max(1, int(sims) - 1)
        self.mc, self.c_visit, self.c_scale = int(max_considered), float(c_visit), float(c_scale)
        self.gumbel = None if gumbel is None else np.asarray(gumbel, np.float64)
        self.score0 = None if score0 is None else np.asarray(score0, np.float64)
        self.v_root = np.float64(0.0)
        self.root_order = []  # the root edges (indices) in the order the simulations chose them
        base = self.eval

        def ev(st):
            pol, value = base(st)
            self._value = value
            return pol, value
        self.eval = ev

    def _expand(self, node, st, legal, pol, player):
        super()._expand(node, st, legal, pol, player)
        if node != 0:
            return
        self.v_root = np.float64(np.float32(self._value))
        if self.gumbel is not None and self.ne[0] > 0:
            rank = {int(a): i for i, a in enumerate(legal)}
            e = self.root_edges()
            p64 = np.array([self.E["p"][k] for k in e], np.float32).astype(np.float64)
            g = np.array([self.gumbel[rank[int(self.E["action"][k])]] for k in e], np.float64)
            with np.errstate(divide="ignore"):
                self.score0 = g + np.log(p64)

    def _root(self):
        e0, ne = self.e0[0], self.ne[0]
        n = np.array(self.E["n"][e0:e0 + ne], np.int64)
        w = np.array(self.E["w"][e0:e0 + ne], np.float64)
        p = np.array(self.E["p"][e0:e0 + ne], np.float32)
        return n, w, p

    def _scores(self):
        n, w, p = self._root()
        sg, v_mix, max_n = sigma(n, w, p, self.v_root, self.c_visit, self.c_scale)
        return n, p, sg, np.maximum(np.float64(-1e9), self.score0[:len(n)] + sg), v_mix, max_n

    def _select(self, node, cpuct):
        if node != 0:
            return super()._select(node, cpuct)
        n, _, _, score, _, _ = self._scores()
        t = int(n.sum())
        cv = considered_visits(min(self.mc, len(n)), self.n_root)[min(t, self.n_root - 1)]
        cand = n == cv
        if not cand.any():
            cand[:] = True
        i = int(np.argmax(np.where(cand, score, -np.inf)))  # the first of the largest
        self.root_order.append(i)
        return self.e0[0] + i

    def result(self):
        """(action, pi' f64 [143], v_mix) after the search; (-1, zeros, 0.0) for a root without edges."""
        pi = np.zeros(143, np.float64)
        if not self.tree or self.ne[0] <= 0:
            return -1, pi, np.float64(0.0)
        n, p, sg, score, v_mix, max_n = self._scores()
        i = int(np.argmax(np.where(n == max_n, score, -np.inf)))
        with np.errstate(divide="ignore"):
            logits = np.log(p.astype(np.float64)) + sg
        if logits.max() == -np.inf:
            logits = sg
        x = np.exp(logits - logits.max())
        actions = [int(self.E["action"][k]) for k in self.root_edges()]
        pi[actions] = x / x.sum()
        return actions[i], pi, v_mix
