"""CPU-side checks of asynchronous self-play (SelfPlay.play_async): the new
entry points in include/hz_abi.h, the binding's table and libhz.so, the
`schedule` / `moves_per_board` validation of SelfPlay.iteration and Trainer,
and the host model of the turn order (tests/selfplay_async_model.py) that the
GPU test's step-count checks use.  No GPU calls."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HANDLE_SYMBOLS = ("hz_mcts_begin_some", "hz_mcts_set_gate_some", "hz_turn_choose")
FREE_SYMBOLS = ("hz_root_noise_at", "hz_playout_coin_at", "hz_choose_actions", "hz_turn_after")


def test_new_symbols_in_header_table_and_library():
    import hzamd._native as nat
    src = open(os.path.join(ROOT, "include", "hz_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for s in HANDLE_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*hz_mcts\s*\*" % s, code), s
    for s in FREE_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
    L = nat.lib()
    for s in HANDLE_SYMBOLS + FREE_SYMBOLS:
        assert s in nat.exported_symbols() and hasattr(L, s), s
    # the rule that sets the masked begin apart from hz_mcts_begin stands next to it
    assert "mask[b] == 0 NOTHING is written" in src
    # host-only argument checks (nothing is launched)
    assert L.hz_mcts_begin_some(None, None, None) == -1
    assert L.hz_mcts_set_gate_some(None, None, None, None) == -1
    assert L.hz_root_noise_at(None, 4, 0, 0, None, None, 0.4, None, None, None) == -1
    assert L.hz_playout_coin_at(-1, 0, 0, None, None, None, None) == -1
    assert L.hz_choose_actions(None, 4, None, None, None, None) == -1
    assert L.hz_turn_choose(*([None] * 6), 1, 15, 0, *([None] * 6)) == -1
    assert L.hz_turn_after(*([None] * 6), 1, 0, *([None] * 9)) == -1


def test_turn_unit_is_listed():
    units = open(os.path.join(ROOT, "harmonies-alphazero_amd", "csrc", "units.mk")).read()
    assert re.search(r"HZ_UNITS\s*:=.*\bhz_turn\b", units)


def test_check_schedule():
    from hzamd.selfplay import check_schedule
    assert check_schedule(None, None) is None
    assert check_schedule("async", 12) == 12
    for schedule, moves in (("steady", None), ("async", None), ("async", 0), ("async", -3), ("async", 2.5),
                            ("async", True), (None, 8), ("ASYNC", 8)):
        with pytest.raises(ValueError):
            check_schedule(schedule, moves)


def test_iteration_validates_before_it_plays():
    """SelfPlay.iteration checks the keys before it touches the boards (an
    object without any stands in for the SelfPlay)."""
    from hzamd.selfplay import SelfPlay
    for kw in ({"schedule": "barrier"}, {"schedule": "async"}, {"moves_per_board": 4},
               {"schedule": "async", "moves_per_board": 0}):
        with pytest.raises(ValueError):
            SelfPlay.iteration(object(), **kw)


def test_trainer_validates_the_schedule_keys():
    """Trainer reads the keys in its constructor, before it needs a model."""
    from hzamd.trainer import Trainer
    for keys in ({"schedule": "async"}, {"schedule": "later", "moves_per_board": 4}, {"moves_per_board": 4},
                 {"schedule": "async", "moves_per_board": "8"}):
        with pytest.raises(ValueError, match="schedule|moves_per_board"):
            Trainer(None, {}, dict({"replay_buffer_size": 10}, **keys), {})


def test_turn_model():
    from selfplay_async_model import moves_done_after, sim_steps, step_bound, turn_steps
    b = np.array([[3, 3, 3], [12, 3, 12], [0, 12, 3], [12, 12, 12]])
    t = turn_steps(b)
    assert t.tolist() == [[3, 6, 9], [12, 15, 27], [1, 13, 16], [12, 24, 36]]
    assert sim_steps(b) == 36 and step_bound(b) == 39
    assert sim_steps(b) <= step_bound(b)
    assert moves_done_after(b, 0).tolist() == [0, 0, 0, 0]
    assert moves_done_after(b, 12).tolist() == [3, 1, 1, 1]
    assert moves_done_after(b, 13).tolist() == [3, 1, 2, 1]
    assert moves_done_after(b, 36).tolist() == [3, 3, 3, 3]
    # equal budgets: the degenerate schedule, every board turns together
    same = np.full((5, 4), 7)
    assert (turn_steps(same) == np.arange(1, 5) * 7).all() and sim_steps(same) == 28
    assert sim_steps(np.zeros((3, 0), int)) == 0
    with pytest.raises(ValueError):
        turn_steps(np.array([[1, -1]]))
