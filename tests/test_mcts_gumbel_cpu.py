"""The Gumbel root's host side: the considered-visit table hzamd builds, the
host model of the rule (tests/mcts_gumbel_model.py) on small cases, and the
conditions the shared fixture must hold for tests/test_mcts_gumbel_gpu.py to
pin what it means to pin.  No GPU."""
import functools

import numpy as np
import pytest

import oracle
from mcts_carry_model import FIXTURE, CarryModel, copy_mt, positions
from mcts_gumbel_model import GUMBEL_KEY, GumbelModel, butterfly, considered_visits, host_gumbel

SIMS, CONSIDERED = 33, 16  # the device tests' main setting


def test_table_rows_are_the_pinned_sequences():
    from hzamd.mcts import considered_visit_table
    assert considered_visit_table(4, 8)[4].tolist() == [0, 0, 0, 0, 1, 1, 2, 2]
    assert considered_visit_table(16, 32)[16].tolist() == [0] * 16 + [1] * 8 + [2] * 4 + [3] * 4
    want = [0] * 5 + [1] * 5 + [v for k in range(2, 13) for v in (k, k)]
    assert len(want) == 32 and considered_visit_table(5, 32)[5].tolist() == want


@pytest.mark.parametrize("shape", [(16, 32), (16, 16), (4, 8), (1, 4), (69, 199), (7, 1)])
def test_table_equals_the_models_rows(shape):
    """Every row of hzamd's table is the model's own restatement of the
    sequence; rows 0 and 1 count up; the dtype and shape are the ABI's."""
    from hzamd.mcts import considered_visit_table
    mc, n_root = shape
    t = considered_visit_table(mc, n_root)
    assert t.dtype == np.int16 and t.shape == (mc + 1, n_root)
    for m in range(mc + 1):
        assert t[m].tolist() == list(considered_visits(m, n_root)), m
    assert t[0].tolist() == t[1].tolist() == list(range(n_root))
    with pytest.raises(ValueError):
        considered_visit_table(0, 8)
    with pytest.raises(ValueError):
        considered_visit_table(4, 0)


def test_butterfly_is_a_sum_in_a_fixed_order():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(69) * 10.0 ** rng.integers(-8, 8, 69)
    s = butterfly(x)
    assert abs(s - np.sum(x.astype(np.longdouble))) <= 1e-9 * np.abs(x).sum()
    assert butterfly([]) == 0.0 and butterfly([1.5]) == 1.5


@functools.lru_cache(maxsize=None)
def fixture():
    F = FIXTURE
    return positions(F["base"], F["n"], F["spread"])


def searched(b, sims=SIMS, gumbel=None, **kw):
    F = FIXTURE
    st, m = fixture()[b]
    g = host_gumbel_fixture()[b] if gumbel is None else gumbel
    model = GumbelModel(st, copy_mt(m), F["evaluator"], sims=sims, gumbel=g, **kw)
    model.begin()
    model.search(sims, F["cpuct"])
    return model


@functools.lru_cache(maxsize=None)
def host_gumbel_fixture():
    return host_gumbel(FIXTURE["n"], **GUMBEL_KEY)


def test_one_considered_action_gets_every_visit():
    for b in (0, 40, 129):
        model = searched(b, sims=9, max_considered=1)
        v = model.visits()
        assert v.sum() == 8 and v.max() == 8 and len(set(model.root_order)) == 1, b


def test_zero_gumbel_and_zero_scale_visit_the_largest_priors_first():
    """G = 0 and c_scale = 0: the scores are log P alone, so the first m =
    min(max_considered, edges) root visits go to the m largest priors in
    descending order, the lowest index first among equal priors."""
    for b in (3, 17, 40, 64, 100, 129):
        model = searched(b, gumbel=np.zeros(69), c_scale=0.0)
        p = np.array([model.E["p"][e] for e in model.root_edges()], np.float32)
        m = min(CONSIDERED, len(p))
        want = sorted(range(len(p)), key=lambda i: (-float(p[i]), i))[:m]
        assert model.root_order[:m] == want, b


def test_gumbel_fixture_conditions():
    """On positions(4100, 130, 41) under the dense stub, cpuct 1.25, S 33 and
    m 16, with the Gumbels the device test draws (GUMBEL_KEY, here from the
    host form of the generator): every board ends with sum N = S - 1; a root
    with 69 edges visits an edge at index >= 64; at least 40 roots have fewer
    legal moves than m; the visits differ from the PUCT model's on at least
    120 boards."""
    F = FIXTURE
    g = host_gumbel_fixture()
    assert np.isfinite(g).all()
    wide_hit = narrow = differ = wide = 0
    for b, (st, m) in enumerate(fixture()):
        model = searched(b)
        v = model.visits()
        assert v.sum() == SIMS - 1, b
        ne = model.ne[0]
        assert 0 < ne <= int(oracle.legal(st).sum()), b  # (a self-loop child has no edge)
        narrow += int(oracle.legal(st).sum()) < CONSIDERED
        if ne == 69:
            wide += 1
            n = np.array([model.E["n"][e] for e in model.root_edges()])
            wide_hit += bool((n[64:] > 0).any())
        plain = CarryModel(st, copy_mt(m), F["evaluator"])
        plain.begin()
        plain.search(SIMS, F["cpuct"])
        differ += not (plain.visits() == v).all()
        # the move and the improved policy exist and agree with the visits' support
        a, pi, v_mix = model.result()
        assert v[a] == v.max() and abs(pi.sum() - 1.0) < 1e-12 and abs(v_mix) <= 1.0, b
    assert wide >= 1 and wide_hit >= 1, (wide, wide_hit)
    assert narrow >= 40, narrow
    assert differ >= 120, differ
