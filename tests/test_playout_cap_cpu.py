"""CPU-side checks of playout-cap randomization: the budget rule
(hzamd.selfplay.playout_budgets) on hand-made coins, the config keys, and the
presence of the budget entry points in include/hz_abi.h and the binding's
symbol table.  No GPU calls."""
import os
import re

import torch

from conftest import ROOT

NEW_SYMBOLS = ("hz_mcts_set_row_cap", "hz_mcts_set_budget", "hz_mcts_sims_done", "hz_mcts_set_root_noise_mask")


def test_playout_budgets_rule():
    from hzamd.selfplay import playout_budgets
    # coins live in (0, 1]: just below p, p itself, just above, the two ends
    p = 0.25
    below, above = float(torch.nextafter(torch.tensor(p, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64))), \
        float(torch.nextafter(torch.tensor(p, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64)))
    coin = torch.tensor([2.0 ** -53, below, p, above, 0.5, 1.0], dtype=torch.float64)
    budget, full = playout_budgets(coin, p, 200, 40)
    assert full.dtype == torch.bool and budget.dtype == torch.int32
    assert full.tolist() == [True, True, False, False, False, False]  # equality with p is not full
    assert budget.tolist() == [200, 200, 40, 40, 40, 40]


def test_playout_budgets_ends():
    from hzamd.selfplay import playout_budgets
    coin = torch.tensor([2.0 ** -53, 0.3, 1.0], dtype=torch.float64)
    budget, full = playout_budgets(coin, 1.0, 16, 4)   # p = 1: every board, the coin 1.0 included
    assert full.tolist() == [True, True, True] and budget.tolist() == [16, 16, 16]
    budget, full = playout_budgets(coin, 0.0, 16, 4)   # p = 0: none
    assert full.tolist() == [False, False, False] and budget.tolist() == [4, 4, 4]
    budget, full = playout_budgets(coin, 0.3, 16, 0)   # a fast budget of 0 is allowed
    assert full.tolist() == [True, False, False] and budget.tolist() == [16, 0, 0]


def test_new_symbols_in_header_and_table():
    import hzamd._native as nat
    src = open(os.path.join(ROOT, "include", "hz_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*hz_mcts\s*\*" % s, code), s
        assert s in nat.exported_symbols(), s
    # the exactness rule stands next to them
    assert "bit for bit the search of min(k, S) simulations" in src
    L = nat.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s
    # host-only argument checks (no GPU call is made for a NULL handle)
    assert L.hz_mcts_set_row_cap(None, 4) == -1
    assert L.hz_mcts_set_budget(None, None) == -1
    assert L.hz_mcts_sims_done(None, None) == -1
    assert L.hz_mcts_set_root_noise_mask(None, None) == -1
