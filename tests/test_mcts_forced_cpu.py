"""The conditions tests/test_mcts_forced_gpu.py rests on, shown on the CPU with
the host model tests/mcts_forced_model.py over the C oracle: with no board's
bit set the model is CarryModel bit for bit; the two rules on trees worked out
by hand; on the shared fixture (mcts_carry_model.positions(4100, 130), dense
stub, cpuct 1.25, eps 0.3, noisy roots, 32 simulations) both k = 2 and k = 8
give every case the device tests rely on, on the boards named in CASES; the
pruning's invariants; and the self-play config keys are validated."""
import types

import numpy as np
import pytest

import oracle
from mcts_carry_model import CarryModel, copy_mt, next_word
from mcts_forced_model import FIXTURE, ForcedModel, ForcedRule, fixture_noise, fixture_positions, forced_edges

TREE_KEYS = ("state", "e0", "ne", "action", "child", "n", "w", "p", "player")
# k -> case -> a board of the fixture that shows it
CASES = {
    2.0: {"forced_differs_from_puct": 0, "forced_at_edge_64_up_of_69": 124, "two_forced_at_once": 1,
          "reduced_to_2_or_more": 0, "zeroed": 2, "stopped_by_the_bound": 0, "best_is_not_edge_0": 0,
          "tie_in_the_largest_n": 5},
    8.0: {"forced_differs_from_puct": 0, "forced_at_edge_64_up_of_69": 128, "two_forced_at_once": 0,
          "reduced_to_2_or_more": 0, "zeroed": 3, "stopped_by_the_bound": 0, "best_is_not_edge_0": 0,
          "tie_in_the_largest_n": 9},
}
_CACHE = {}


def fixture():
    if "pos" not in _CACHE:
        pos = fixture_positions()
        counts = [int(oracle.legal(st).sum()) for st, _ in pos]
        _CACHE["pos"], _CACHE["noise"] = pos, fixture_noise(len(pos), counts)
    return _CACHE["pos"], _CACHE["noise"]


def searched(k):
    """The model's noisy search of every fixture board under k (None: plain CarryModel)."""
    F = FIXTURE
    if k not in _CACHE:
        pos, noise = fixture()
        out = []
        for b, (st, m) in enumerate(pos):
            model = (CarryModel(st, copy_mt(m), F["evaluator"]) if k is None
                     else ForcedModel(st, copy_mt(m), F["evaluator"], k=k))
            model.begin(carry=False)
            model.search(F["sims"], F["cpuct"], noise=noise[b], eps=F["eps"], noisy=True)
            out.append(model)
        _CACHE[k] = out
    return _CACHE[k]


def same_tree(a, b):
    a, b = a.export(), b.export()
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
               for k in TREE_KEYS)


def test_model_with_no_bit_set_is_carry_model():
    F = FIXTURE
    pos, noise = fixture()
    plain = searched(None)
    for b in range(0, F["n"], 7):
        st, m = pos[b]
        model = ForcedModel(st, copy_mt(m), F["evaluator"], k=None)
        model.begin(carry=False)
        model.search(F["sims"], F["cpuct"], noise=noise[b], eps=F["eps"], noisy=True)
        assert same_tree(model, plain[b]) and next_word(model.mt) == next_word(plain[b].mt), b
        assert model.log == [] and (model.pruned(F["cpuct"]) == plain[b].visits()).all(), b


def test_fixture_noise_rows_cover_the_legal_moves():
    """Positive weights, each a share of the row (at most 1), on the board's
    legal moves and zero past them.  (How close a row's sum is to 1 is not
    asserted: the searches take the rows as they are, bit for bit.)"""
    pos, noise = fixture()
    for b, (st, _) in enumerate(pos):
        k = int(oracle.legal(st).sum())
        assert (noise[b, :k] > 0).all() and (noise[b, :k] <= 1).all() and (noise[b, k:] == 0).all(), b


class _Tree(ForcedRule):
    """A one-node tree with given root edges, for the rules alone."""

    def __init__(self, n, w, p, k):
        self.tree, self.e0, self.ne = True, [0], [len(n)]
        self.E = {"n": list(n), "w": list(w), "p": [float(np.float32(x)) for x in p],
                  "action": list(range(10, 10 + len(n)))}
        self.set_forced(k)

    def visits(self):
        v = np.zeros(143, np.int32)
        v[10:10 + len(self.E["n"])] = self.E["n"]
        return v


def test_rules_on_trees_worked_out_by_hand():
    # forced: N^2 < k P t.  t = 5, k = 2: edge 0: 1 < 5; edge 1 unvisited; edge 2: 16 < 2 is false
    assert forced_edges(2.0, [1, 0, 4], [0.5, 0.3, 0.2], 5) == [0]
    # edge 1: 4 < 2 * 0.25 * 9 = 4.5 and edge 2: 1 < 2.25: both, ascending; at N^2 == k P t an edge is not forced
    assert forced_edges(2.0, [6, 2, 1], [0.5, 0.25, 0.125], 9) == [1, 2]
    assert forced_edges(2.0, [3, 0], [0.5, 0.5], 9) == []
    # pruning, cpuct 1, k 2, t = 14, s = sqrt(14) = 3.74166: the best edge 0 has q 0.5 and U = 0.5 s / 11, bound
    # 0.67008.  Edge 1 (N 3, q 0.1, nf = floor(sqrt(7)) = 2): 0.1 + 0.25 s / 3 = 0.4118 and 0.1 + 0.25 s / 2 =
    # 0.5677 are both below it: 3 - 2 = 1 -> 0.  Edge 2 (N 1, q -0.5, nf = floor(sqrt(3.5)) = 1): -0.5 + 0.125 s
    # is below: 0.  Edge 3 is unvisited.
    t = _Tree([10, 3, 1, 0], [5.0, 0.3, -0.5, 0.0], [0.5, 0.25, 0.125, 0.125], 2.0)
    assert t.pruned(1.0)[10:14].tolist() == [10, 0, 0, 0]
    # edge 1 (N 4, q 0.6, nf = floor(sqrt(14)) = 3): 0.6 + 0.5 s / 4 = 1.0677 is not below the bound: kept whole
    t = _Tree([10, 4], [5.0, 2.4], [0.5, 0.5], 2.0)
    assert t.pruned(1.0)[10:12].tolist() == [10, 4]
    # a tie in the largest N: the first is the best and keeps its count, the second is reduced like any other:
    # t = 8, s = sqrt(8), bound = 0.5 + 0.5 s / 5 = 0.78284; edge 1 (q 0, nf = floor(sqrt(8)) = 2): 0.5 s / 4 =
    # 0.35355 and 0.5 s / 3 = 0.4714 are below: 4 - 2 = 2 stays 2
    t = _Tree([4, 4], [2.0, 0.0], [0.5, 0.5], 2.0)
    assert t.pruned(1.0)[10:12].tolist() == [4, 2]
    # the bit clear, or no visit at all: the raw row
    assert _Tree([10, 3], [5.0, 0.3], [0.5, 0.25], None).pruned(1.0)[10:12].tolist() == [10, 3]
    assert _Tree([0, 0], [0.0, 0.0], [0.5, 0.25], 2.0).pruned(1.0)[10:12].tolist() == [0, 0]


def shown(model, cpuct):
    """The cases one searched board shows."""
    out = set()
    for forced, pick, puct, ne in model.log:
        if forced:
            assert pick == forced[0] and forced == sorted(forced)
            if pick != puct:
                out.add("forced_differs_from_puct")
            if pick >= 64 and ne == 69:
                out.add("forced_at_edge_64_up_of_69")
            if len(forced) >= 2:
                out.add("two_forced_at_once")
        else:
            assert pick == puct
    detail = []
    model.pruned(cpuct, detail)
    e0, ne = model.e0[0], model.ne[0]
    n = [int(x) for x in model.E["n"][e0:e0 + ne]]
    if detail:
        if detail[0][1] != 0:
            out.add("best_is_not_edge_0")
        if n.count(max(n)) > 1:
            out.add("tie_in_the_largest_n")
            assert detail[0][1] == n.index(max(n))
        for _, ni, nf, r, left in detail[1:]:
            if r > 0 and left >= 2:
                out.add("reduced_to_2_or_more")
            if r > 0 and left == 0:
                out.add("zeroed")
            if r < min(nf, ni):
                out.add("stopped_by_the_bound")
    return out


@pytest.mark.parametrize("k", [FIXTURE["k"], FIXTURE["k_large"]])
def test_fixture_holds_every_case(k):
    F = FIXTURE
    models = searched(k)
    for case, b in CASES[k].items():
        assert case in shown(models[b], F["cpuct"]), (case, b)
    plain = searched(None)
    changed = sum(not (a.visits() == p.visits()).all() for a, p in zip(models, plain))
    assert changed >= F["n"] // 2, changed  # the gate matters on most boards
    picks = sum(bool(f) for m in models for f, _, _, _ in m.log)
    print(f"k {k}: boards whose visits changed {changed} of {F['n']}; root selections the rule decided {picks} of "
          f"{sum(len(m.log) for m in models)}")


@pytest.mark.parametrize("k", [FIXTURE["k"], FIXTURE["k_large"]])
def test_pruning_invariants(k):
    F = FIXTURE
    for b, model in enumerate(searched(k)):
        raw, pruned = model.visits(), model.pruned(F["cpuct"])
        assert (pruned <= raw).all() and (pruned >= 0).all(), b
        assert int(np.argmax(pruned)) == int(np.argmax(raw)) and pruned.max() == raw.max(), b  # the best edge stays
        assert (raw.sum() == 0) == (pruned.sum() == 0), b
        assert not ((pruned == 1) & (raw > 1)).any(), b  # a reduced edge never rests at one visit


def test_self_play_config_is_validated():
    """The keys' values and the forbidden combinations (each refused before
    any device object is made: the env here is a stand-in)."""
    from hzamd.selfplay import SelfPlay
    env = types.SimpleNamespace(n=4)

    def make(**cfg):
        return SelfPlay(4, None, cfg, device="cpu", env=env)
    for bad in (0, -1.0, float("nan"), True, "2"):
        with pytest.raises(ValueError, match="forced_playouts"):
            make(forced_playouts=bad)
    with pytest.raises(ValueError, match="forced_playouts"):
        make(forced_playouts=2.0, tree_reuse="add")
    with pytest.raises(ValueError, match="forced_playouts"):
        make(forced_playouts=2.0, root_policy="gumbel")
    with pytest.raises(ValueError, match="prune_targets"):
        make(forced_playouts=2.0, prune_targets=1)
    with pytest.raises(ValueError, match="prune_targets"):
        make(prune_targets=True)
