"""The conditions tests/test_mcts_leafsym_gpu.py rests on, shown on the CPU
with the host model tests/mcts_leafsym_model.py over the C oracle: without a
key the model is oracle.mcts_search; on the shared fixture the cell stub makes
a search with keys differ from one without, every symmetry occurs among the
evaluated leaves and the stub tells a leaf from its image; under the orbit
stub (equivariant) the keys change nothing; and the self-play config key is
validated.  The rule has no host entry point in the ABI, so its device form is
compared with the Python restatement on the GPU
(test_mcts_leafsym_gpu.py::test_every_encoder_writes_the_leafs_image)."""
import types

import numpy as np
import pytest

import oracle
from mcts_carry_model import copy_mt, next_word, positions
from mcts_leafsym_model import FIXTURE, KEYS, LeafSymModel, cell_key, host_keys, image, leaf_sym

TREE_KEYS = ("state", "e0", "ne", "action", "child", "n", "w", "p", "player")
_CACHE = {}


def fixture_positions():
    if "pos" not in _CACHE:
        F = FIXTURE
        _CACHE["pos"] = positions(F["base"], F["n"], F["spread"])
    return _CACHE["pos"]


def searched(evaluator, keyed, boards):
    """The model's search of the fixture's boards `boards`, kept per setting."""
    F = FIXTURE
    pos = fixture_positions()
    keys = host_keys(F["n"], **KEYS)
    out = _CACHE.setdefault((evaluator, keyed), {})
    for b in boards:
        if b not in out:
            st, m = pos[b]
            model = LeafSymModel(st, copy_mt(m), evaluator, key=keys[b] if keyed else None)
            model.begin(carry=False)
            model.search(F["sims"], F["cpuct"])
            out[b] = model
    return [out[b] for b in boards]


def same_tree(a, b):
    a, b = a.export(), b.export()
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
               for k in TREE_KEYS)


@pytest.mark.parametrize("evaluator", [0, 1])
def test_model_without_a_key_is_the_oracle(evaluator):
    F = FIXTURE
    pos = fixture_positions()
    boards = list(range(0, F["n"], 9))
    for b, model in zip(boards, searched(evaluator, False, boards)):
        st, m = pos[b]
        m2 = copy_mt(m)
        _, visits, nn, ne = oracle.mcts_search(st, m2, F["sims"], F["cpuct"], testing=True, tau0=0, evaluator=evaluator)
        assert (model.visits() == visits).all() and model.counts() == (nn, ne), b
        assert next_word(model.mt) == next_word(m2), b
        assert all(g == 0 for _, g, _ in model.evaluated), b


def test_rule_restatement():
    """mix64 and the rule on values worked out by hand from the constants: key
    0, node 0 mixes the salt alone; the top two bits are the result."""
    from mcts_leafsym_model import LEAF_SALT, M64, mix64
    z = LEAF_SALT
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    assert mix64(LEAF_SALT) == z and leaf_sym(0, 0) == z >> 62
    # a key's four symmetries come about equally often over the node ids: 4,096 draws, each count within
    # 5 standard deviations (sqrt(4096 * 3 / 16) = 27.7) of 1,024
    counts = np.bincount([leaf_sym(0x1234567, node) for node in range(4096)], minlength=4)
    assert counts.sum() == 4096 and (np.abs(counts - 1024) <= 139).all(), counts
    assert len(set(host_keys(64, **KEYS))) == 64


def test_fixture_tells_a_search_with_keys_from_one_without():
    F = FIXTURE
    boards = list(range(F["n"]))
    keyed, plain = searched("cell", True, boards), searched("cell", False, boards)
    changed = sum(not (a.visits() == b.visits()).all() for a, b in zip(keyed, plain))
    assert changed >= 0.75 * F["n"], changed
    per_g = np.zeros(4, np.int64)
    seen = differ = 0
    for model in keyed:
        for node, g, st in model.evaluated:
            per_g[g] += 1
            if node != 0 and g != 0:
                seen += 1
                differ += cell_key(image(st, g)) != cell_key(st)
    assert (per_g > 0).all(), per_g
    assert seen > 0 and differ >= 0.9 * seen, (differ, seen)
    print(f"boards with changed visits {changed} of {F['n']}; leaves per g {per_g.tolist()}; "
          f"non-root leaves with g != 0 whose key moves {differ} of {seen}")


def test_orbit_stub_makes_the_keys_invisible():
    boards = list(range(0, FIXTURE["n"], 3))
    keyed, plain = searched("orbit", True, boards), searched("orbit", False, boards)
    assert any(g != 0 for model in keyed for _, g, _ in model.evaluated)
    for b, a, p in zip(boards, keyed, plain):
        assert same_tree(a, p) and next_word(a.mt) == next_word(p.mt), b


def test_self_play_config_is_validated():
    """The key's values and the forbidden combinations (each refused before
    any device object is made: the env here is a stand-in)."""
    from hzamd.selfplay import SelfPlay
    env = types.SimpleNamespace(n=4)

    def make(**cfg):
        return SelfPlay(4, None, cfg, device="cpu", env=env)
    for bad in ("mirror", True, 1):
        with pytest.raises(ValueError, match="leaf_symmetry"):
            make(leaf_symmetry=bad)
    with pytest.raises(ValueError, match="leaf_symmetry"):
        make(leaf_symmetry="random", tree_reuse="add")
    with pytest.raises(ValueError, match="leaf_symmetry"):
        make(leaf_symmetry="random", root_policy="gumbel")
