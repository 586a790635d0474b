"""The host model of tree reuse (tests/mcts_carry_model.py) against the C
oracle, and the shared fixture's coverage.  No GPU.

From an empty tree the model is oracle.mcts_search: that is its licence as the
yardstick of tests/test_mcts_carry_gpu.py.  The fixture test then shows, with
the model, that the boards the device tests use hold every case of the carry
rule worth pinning."""
import numpy as np
import pytest

import oracle
from mcts_carry_model import (FIXTURE, CarryModel, carry_tree, choose, copy_mt, fixture_action, next_word, positions,
                              topup_budget)

SIMS = 48


@pytest.mark.parametrize("evaluator", [0, 1], ids=["stub", "dense"])
@pytest.mark.parametrize("noisy", [False, True], ids=["testing", "noisy"])
@pytest.mark.parametrize("cpuct", [1.1, 3.7])
def test_model_from_empty_tree_is_the_oracle(evaluator, noisy, cpuct):
    """8 seeds x 48 simulations: visits, node and edge counts, the chosen move
    and the stream's next word equal oracle.mcts_search's."""
    rng = np.random.default_rng(17)
    for seed, (st, m) in enumerate(positions(9000 + 100 * evaluator, 8 * 5, spread=61)[::5]):
        L = int(oracle.legal(st).sum())
        noise = np.zeros(143)
        noise[:L] = rng.dirichlet([0.4] * L)
        m2 = copy_mt(m)
        a, ov, nn, ne = oracle.mcts_search(st, m2, SIMS, cpuct, eps=0.3, testing=not noisy, tau0=0, noise=noise,
                                           evaluator=evaluator)
        model = CarryModel(st, m, evaluator)
        assert not model.begin(noise[:69], 0.3, noisy)
        model.search(SIMS, cpuct, noise[:69], 0.3, noisy)
        assert (model.visits() == ov).all(), seed
        assert model.counts() == (nn, ne), seed
        assert choose(model.visits(), False, 0.0) == a, seed
        assert next_word(model.mt) == next_word(m2), seed
        assert model.flag == 0


def fixture_boards():
    """The shared fixture played through one search and one move by the model:
    per board (model, old tree, action, info, kept old ids, the child's state
    before the step)."""
    F = FIXTURE
    out = []
    for b, (st, m) in enumerate(positions(F["base"], F["n"], F["spread"])):
        model = CarryModel(st, m, F["evaluator"])
        model.begin()
        model.search(F["sims"], F["cpuct"])
        old = model.export(words=False)
        v = model.visits()
        has = np.zeros(143, bool)
        has[[int(old["action"][e]) for e in model.root_edges()]] = True
        a = fixture_action(b, v, has)
        model.play(a)
        _, info, kept = carry_tree(old, a, model.env, 69 * F["sims"], 1 << 30)
        assert model.advance(a, 69 * F["sims"]) == info
        out.append((model, old, a, info, kept, st))
    return out


def test_carry_fixture_conditions():
    """The fixture's boards hold: a kept node with two kept parent edges; a
    kept node whose other parent is dropped; a carried root without edges; a
    turn-end move dropped because the states differ; a deterministic ply
    carried with more than half of the root's visits; a noisy carried root
    whose mix changes the first selected edge.  The special lanes 0, 63, 64
    and 129 are boards of it."""
    F = FIXTURE
    boards = fixture_boards()
    assert len(boards) == 130
    two_parents = other_dropped = bare_root = turn_end_drop = majority = mix_moves = 0
    carried = 0
    rng = np.random.default_rng(5)
    for b, (model, old, a, info, kept, st0) in enumerate(boards):
        root = range(int(old["e0"][0]), int(old["e0"][0]) + int(old["ne"][0]))
        edge = [e for e in root if old["action"][e] == a][0]
        c = int(old["child"][edge])
        if kept is None:
            if st0[73] == 3 and old["ne"][c] >= 0 and not np.array_equal(old["state"][c], model.env):
                turn_end_drop += 1
            continue
        carried += 1
        new = model.export(words=False)
        indeg = np.bincount(new["child"], minlength=len(new["e0"]))
        two_parents += bool((indeg >= 2).any())
        keptset = set(kept)
        owner = {}
        for v in range(len(old["e0"])):
            for e in range(int(old["e0"][v]), int(old["e0"][v]) + max(int(old["ne"][v]), 0)):
                owner[e] = v
        other_dropped += any(int(old["child"][e]) in keptset and v not in keptset and int(old["child"][e]) != c
                             for e, v in owner.items())
        bare_root += new["ne"][0] == 0
        if st0[73] != 3 and 2 * info[2] > int(old["n"][list(root)].sum()):
            majority += 1
        if new["ne"][0] > 0:
            L = int(oracle.legal(model.env).sum())
            noise = rng.dirichlet([0.4] * L)
            plain = model._select(0, F["cpuct"])
            p0 = list(model.E["p"])
            model.carried = True
            assert model.begin(noise, F["eps"], True)
            mix_moves += model._select(0, F["cpuct"]) != plain
            model.E["p"] = p0
    print("carried", carried, "two_parents", two_parents, "other_dropped", other_dropped, "bare_root", bare_root,
          "turn_end_drop", turn_end_drop, "majority", majority, "mix_moves", mix_moves)
    assert min(two_parents, other_dropped, bare_root, turn_end_drop, majority, mix_moves) >= 1
    assert 20 <= carried <= 125


def test_topup_budget_clamp():
    """hzamd.selfplay.topup_budgets: budget = clamp(num_simulations - carried
    visits, min_sims, num_simulations) as int32, on hand-made carried visits:
    none carried, the interior, carried at and above num_simulations (a tree
    kept under "add" can hold more), min_sims 0, and min_sims above
    num_simulations (the upper bound wins).  The model's helper, which the
    self-play replay on the device uses, gives the same numbers."""
    import torch
    from hzamd.selfplay import topup_budgets
    cases = [([0, 1, 150, 199, 200, 201, 5000], 200, 1, [200, 199, 50, 1, 1, 1, 1]),
             ([0, 190, 400], 200, 16, [200, 16, 16]),
             ([3, 300], 200, 0, [197, 0]),
             ([0, 10, 24, 90], 24, 3, [24, 14, 3, 3]),
             ([0, 100, 300], 200, 500, [200, 200, 200])]
    for carried, sims, floor, want in cases:
        got = topup_budgets(torch.tensor(carried, dtype=torch.int32), sims, floor)
        assert got.dtype == torch.int32 and got.shape == (len(carried),)
        assert got.tolist() == want, (carried, sims, floor)
        assert topup_budget(carried, sims, floor).tolist() == want, (carried, sims, floor)
    # int32 carried visits near the type's end do not wrap
    assert topup_budgets(torch.tensor([2**31 - 1], dtype=torch.int32), 200, 1).tolist() == [1]
