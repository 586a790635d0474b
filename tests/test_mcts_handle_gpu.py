"""The search handle's first-use buffer groups on the GPU (hz_mcts_create's
base group, the carry group of the first hz_mcts_advance, the Gumbel group of
the first hz_mcts_set_gumbel): what a handle computes does not depend on which
groups it has asked for, in which order, or on the handles before it.

Three boards of tests/golden/mcts.npz (rows of its 8-simulation, cpuct 1.0,
testing group), 6 simulations, the stub evaluator.  Every search starts from
the fixture's states and streams, imported anew, so searches of different
handles are comparable; every comparison is exact (visits are integers, the
improved policy is compared by its bits).  The fixture file holds visits for
8 simulations and up, none for 6: the plain 6-simulation search is held to
the C oracle (which tests/test_oracle_golden.py holds to the fixture), and the
same handle's 8-simulation search to the fixture's own visits."""
import functools
import os

import numpy as np
import pytest
import torch

import oracle
from conftest import GOLDEN
from hzamd.state import pack_ref, words_to_array

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIMS, CPUCT = 6, 1.0


@functools.lru_cache(maxsize=None)
def boards():
    """(fixture rows, state words [6, 3], MT words [3, 624], MT indices [3], Gumbels [3, 69])"""
    f = np.load(os.path.join(GOLDEN, "mcts.npz"))
    ks = [k for k in range(len(f["sims"])) if (f["sims"][k], f["cpuct"][k], f["testing"][k]) == (8, 1.0, 1)]
    ks = [ks[0], ks[len(ks) // 2], ks[-1]]
    words = np.ascontiguousarray(words_to_array([pack_ref(f["state"][k]) for k in ks]).T)
    mts, idx = np.zeros((3, 624), np.uint32), np.zeros(3, np.int32)
    for i, k in enumerate(ks):
        mts[i], idx[i] = oracle.mt_seed(int(f["mt_seed"][k])).words()
    u = (np.arange(3 * 69, dtype=np.float64).reshape(3, 69) * 0.6180339887 % 1.0) * 0.98 + 0.01
    return f, ks, words, mts, idx, -np.log(-np.log(u))


class Handle:
    def __init__(self):
        from hzamd.env import BatchedEnv
        from hzamd.mcts import BatchedMCTS
        self.env = BatchedEnv(3, device=DEV)
        self.mcts = BatchedMCTS(self.env, SIMS, max_nodes=1 + 69 * 8)  # (room for the fixture's 8 simulations)

    def start(self):
        _, _, words, mts, idx, _ = boards()
        self.env.import_state(torch.from_numpy(words), torch.from_numpy(mts.view(np.int32)), torch.from_numpy(idx))

    def plain(self, sims=SIMS):
        from hzamd.mcts import stub_evaluator
        self.start()
        return self.mcts.search(stub_evaluator, CPUCT, sims=sims).cpu().numpy().copy()

    def carried(self):
        """search, play each board's most visited move, advance (the carry
        group's first use on a handle that had none), search the kept trees"""
        from hzamd.mcts import stub_evaluator
        first = self.plain()
        action = torch.from_numpy(first.argmax(axis=1).astype(np.int16))
        self.env.step(action)
        info = {k: v.cpu().numpy().copy() for k, v in self.mcts.advance(action).items()}
        second = self.mcts.search(stub_evaluator, CPUCT, sims=SIMS, carry=True).cpu().numpy().copy()
        return {"first": first, "second": second, **info}

    def gumbel(self):
        """one search under the Gumbel root (the Gumbel group's first use on a handle that had none)"""
        from hzamd.mcts import stub_evaluator
        self.start()
        g = torch.from_numpy(boards()[5])
        visits = self.mcts.search(stub_evaluator, CPUCT, sims=SIMS, root="gumbel", gumbel=g).cpu().numpy().copy()
        res = self.mcts.gumbel_result()
        return {"visits": visits, "action": res["action"].cpu().numpy().copy(),
                "pi": res["pi"].cpu().numpy().view(np.uint32).copy()}

    def close(self):
        self.mcts.close()
        self.env.close()


def same(a, b):
    return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in a)


@functools.lru_cache(maxsize=None)
def alone():
    """what a handle that used one group only computes: (carried, gumbel), each from its own handle"""
    a, g = Handle(), Handle()
    out = a.carried(), g.gumbel()
    a.close()
    g.close()
    # the scenario exercises what it is meant to: a tree was carried, and the Gumbel root searched
    assert out[0]["nodes"].max() > 1 and out[0]["visits"].max() > 0
    assert out[1]["visits"].sum() == 3 * (SIMS - 1) and (out[1]["action"] >= 0).all()
    return out


def test_neither_group_matches_the_oracle_and_the_fixture():
    f, ks, _, _, _, _ = boards()
    h = Handle()
    got6, got8 = h.plain(), h.plain(sims=8)
    h.close()
    for i, k in enumerate(ks):
        _, want, _, _ = oracle.mcts_search(f["state"][k], oracle.mt_seed(int(f["mt_seed"][k])), SIMS, CPUCT, testing=True)
        assert (got6[i] == want).all(), (k, got6[i][got6[i] > 0], want[want > 0])
        assert (got8[i] == f["visits"][k]).all(), (k, got8[i][got8[i] > 0])
    assert same({"v": got6}, {"v": alone()[0]["first"]})  # the other handles' first searches are this one


@pytest.mark.parametrize("order", ["advance_then_gumbel", "gumbel_then_advance"])
def test_both_groups_in_either_order_equal_one_group_alone(order):
    want_carried, want_gumbel = alone()
    h = Handle()
    if order == "advance_then_gumbel":
        carried, gumbel = h.carried(), h.gumbel()
    else:
        gumbel, carried = h.gumbel(), h.carried()
    h.close()
    assert same(carried, want_carried), (carried, want_carried)
    assert same(gumbel, want_gumbel), (gumbel, want_gumbel)


def test_close_twice_and_del_do_nothing():
    h = Handle()
    h.carried()
    h.gumbel()
    h.mcts.close()
    assert h.mcts._h is None
    h.mcts.close()
    h.mcts.__del__()
    assert h.mcts._h is None
    h.env.close()
    # the process' next handle is sound
    again = Handle()
    assert same(again.gumbel(), alone()[1])
    again.close()


def test_three_handles_in_a_row_compute_the_same():
    runs = []
    for _ in range(3):
        h = Handle()
        runs.append((h.carried(), h.gumbel()))
        h.close()
    for carried, gumbel in runs[1:]:
        assert same(carried, runs[0][0]) and same(gumbel, runs[0][1])
    assert same(runs[0][0], alone()[0]) and same(runs[0][1], alone()[1])
