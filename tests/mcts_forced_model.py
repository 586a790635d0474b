"""Host model of forced playouts at the root and policy target pruning
(hz_mcts_set_forced, hz_mcts_pruned_visits, BatchedMCTS.search(forced=)).  A
helper, not a test.

ForcedModel is tests/mcts_carry_model.py's CarryModel whose root select first
asks the forced rule of include/hz_abi.h ("forced playouts"), restated here in
NumPy float64 one operation at a time: edge e is forced iff N_e > 0 and
float64(N_e N_e) < (k float64(P_e)) float64(t), and the first forced edge in
ascending index wins; otherwise the choice is CarryModel's PUCT.  pruned()
restates the pruning.  With k None (the board's bit clear) it is CarryModel
(tests/test_mcts_forced_cpu.py).  ForcedRule is the rule alone, to be mixed
into another model of the family (the leaf-symmetry one).

The fixture below is what tests/test_mcts_forced_cpu.py proved to hold every
case the device tests rely on; its boards are named there."""
import numpy as np

from mcts_carry_model import CarryModel, positions

# The boards the forced tests share: mcts_carry_model.positions(base, n), the
# dense stub (evaluator 1), noisy roots.  32 simulations with k = 2 and with
# k = 8 as the larger k each give every case (tests/test_mcts_forced_cpu.py
# names the boards), so neither had to be raised.
FIXTURE = {"base": 4100, "n": 130, "spread": 41, "sims": 32, "cpuct": 1.25, "evaluator": 1, "eps": 0.3,
           "k": 2.0, "k_large": 8.0}
SMALL = 20  # the boards of the one-workgroup path (n <= 32)
MAX_CHILDREN = 69


def fixture_positions():
    F = FIXTURE
    return positions(F["base"], F["n"], F["spread"])


def fixture_noise(n_boards, counts):
    """The fixture's root noise: float64 [n, 69], row b a distribution over
    board b's counts[b] legal moves, spiky like a Dirichlet(0.4) draw: u^4 of
    a hashed u in (0, 1], normalised (products, one running sum and one
    division per entry: the same bits wherever it runs)."""
    out = np.zeros((n_boards, MAX_CHILDREN), np.float64)
    for b in range(n_boards):
        k = int(counts[b])
        raw, total = [], np.float64(0.0)
        for i in range(k):
            h = ((b * MAX_CHILDREN + i + 1) * 2654435761) % (1 << 32)
            u = np.float64((h >> 8) + 1) / np.float64(1 << 24)
            r = (u * u) * (u * u)
            raw.append(r)
            total = total + r
        for i in range(k):
            out[b, i] = raw[i] / total
    return out


def forced_edges(k, n, p, t):
    """The forced rule over a root's edges (lists / arrays of N and fp32 P, t =
    sum N): the indices of the forced edges, ascending."""
    out = []
    for i in range(len(n)):
        if int(n[i]) > 0:
            lhs = np.float64(int(n[i]) * int(n[i]))           # an exact integer product
            kp = np.float64(k) * np.float64(np.float32(p[i]))  # two fp64 products, in this order
            if lhs < kp * np.float64(t):
                out.append(i)
    return out


class ForcedRule:
    """The two rules over a CarryModel-like tree.  forced_k None: the board's
    bit is clear.  log: per root selection under the gate (forced edge indices,
    the chosen edge index, PUCT's edge index, the root's edge count)."""
    forced_k = None

    def set_forced(self, k):
        self.forced_k = None if k is None else float(k)
        self.log = []
        return self

    def _select(self, node, cpuct):
        puct = super()._select(node, cpuct)
        if node != 0 or self.forced_k is None or not 1 <= self.ne[0] <= MAX_CHILDREN:
            return puct
        e0, ne = self.e0[0], self.ne[0]
        n, p = self.E["n"][e0:e0 + ne], self.E["p"][e0:e0 + ne]
        t = int(sum(int(x) for x in n))
        forced = forced_edges(self.forced_k, n, p, t)
        pick = e0 + forced[0] if forced else puct
        self.log.append((forced, pick - e0, puct - e0, ne))
        return pick

    def pruned(self, cpuct, detail=None):
        """hz_mcts_pruned_visits' row of this board: int32 [143].  detail (a
        list, optional) gets (edge index, N, nf, r, N') per edge that could
        give visits back, and ("best", index) first."""
        v = self.visits()
        if self.forced_k is None or not self.tree or self.ne[0] <= 0:
            return v
        e0, ne = self.e0[0], self.ne[0]
        n = [int(x) for x in self.E["n"][e0:e0 + ne]]
        w = [np.float64(x) for x in self.E["w"][e0:e0 + ne]]
        p = [np.float32(x) for x in self.E["p"][e0:e0 + ne]]
        t = sum(n)
        if t <= 0:
            return v
        s = np.sqrt(np.float64(t if t > 1 else 1))
        k = np.float64(self.forced_k)

        def u(i, x):
            cp = np.float32(cpuct) * p[i]                      # the fp32 product
            return (np.float64(cp) * s) / np.float64(1 + x)

        def q(i):
            return w[i] / np.float64(n[i]) if n[i] else np.float64(0.0)
        best = int(np.argmax(np.array(n, np.int64)))           # the first of the largest
        bound = q(best) + u(best, n[best])
        if detail is not None:
            detail.append(("best", best))
        for i in range(ne):
            if i == best or n[i] <= 0:
                continue
            root = np.floor(np.sqrt((k * np.float64(p[i])) * np.float64(t)))
            nf = n[i] if root >= n[i] else (int(root) if root > 0 else 0)   # min(nf, N_e)
            qi, r = q(i), 0
            for j in range(1, nf + 1):
                if not qi + u(i, n[i] - j) < bound:
                    break
                r = j
            left = n[i] - r
            if r > 0 and left <= 1:
                left = 0
            if detail is not None:
                detail.append((i, n[i], int(root) if np.isfinite(root) else -1, r, left))
            v[self.E["action"][e0 + i]] = left
        return v


class ForcedModel(ForcedRule, CarryModel):
    """One board under search(forced=): CarryModel with the forced root."""

    def __init__(self, ref_state, mt, evaluator=0, k=None, **kw):
        super().__init__(ref_state, mt, evaluator, **kw)
        self.set_forced(k)
