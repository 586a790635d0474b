"""The torch stub evaluator (hzamd.mcts.stub_evaluator) equals the golden
stub (tests/golden/make_golden.py) and the oracle's C restatement. CPU only."""
import os

import numpy as np
import torch

import oracle
from conftest import GOLDEN


def test_stub_evaluator_matches_oracle_stub():
    from hzamd.mcts import stub_evaluator
    f = np.load(os.path.join(GOLDEN, "env_traces.npz"))
    states = f["states"][::11]
    boards, globs = zip(*[oracle.encode(s) for s in states])
    pol, val = stub_evaluator(torch.from_numpy(np.stack(boards)), torch.from_numpy(np.stack(globs)))
    for i, s in enumerate(states):
        op, ov = oracle.stub_eval(s)
        assert (pol[i].numpy() == op).all()
        assert float(val[i]) == ov


def test_choose_actions_rules():
    from hzamd.mcts import choose_actions, pi_from_visits
    v = torch.tensor([[0, 3, 5, 5, 0], [2, 0, 2, 1, 0], [0, 0, 0, 0, 0]], dtype=torch.int32)
    g = choose_actions(v, torch.zeros(3, dtype=torch.bool), torch.zeros(3))
    assert g.tolist() == [2, 0, -1]          # first maximum
    e = choose_actions(v, torch.ones(3, dtype=torch.bool), torch.tensor([0.0, 0.5, 0.3], dtype=torch.float64))
    assert e.tolist() == [1, 2, -1]          # 0*13 < 3 -> 1; 0.5*5 = 2.5 < cum 4 -> 2
    p = pi_from_visits(v)
    assert torch.allclose(p[0], torch.tensor([0, 3, 5, 5, 0]) / 13.0)


def test_dense_stub_three_restatements_agree_bit_for_bit():
    """The dense stub in NumPy (tests/golden/make_golden.py, what the reference
    searched under for mcts_dense.npz), C (oracle.dense_stub_eval) and torch
    (hzamd.mcts.dense_stub_evaluator, on the CPU) on every state of
    env_traces.npz: the same bits, and the properties the fixture relies on:
    every non-zero prior mant * 2^-(24+s) with mant in [2^23, 2^24) and s in
    0..19, actions 3g, 3g+1, 3g+2 one fp32 ulp apart or all zero, zeros
    present, every binade used, values integers times 2^-23 in [-1, 1)."""
    import importlib.util
    from hzamd.mcts import dense_stub_evaluator
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    states = np.load(os.path.join(GOLDEN, "env_traces.npz"))["states"]
    enc = [oracle.encode(s) for s in states]
    pol, val = dense_stub_evaluator(torch.from_numpy(np.stack([b for b, _ in enc])),
                                    torch.from_numpy(np.stack([g for _, g in enc])))
    assert pol.dtype == torch.float32 and val.dtype == torch.float32
    pol, val = pol.numpy(), val.numpy()
    binades, zeros = set(), 0
    for i, s in enumerate(states):
        cp, cv = oracle.dense_stub_eval(s)
        npol, nval = mg.dense_stub_predict_np(*enc[i])
        assert npol.dtype == np.float32 and isinstance(nval, float)
        assert (cp.view(np.uint32) == npol.view(np.uint32)).all(), i
        assert (cp.view(np.uint32) == pol[i].view(np.uint32)).all(), i
        assert cv == nval == float(val[i]), i
        assert -1.0 <= cv < 1.0 and cv * 2.0 ** 23 == int(cv * 2.0 ** 23)
        bits = cp.view(np.uint32).astype(np.int64)
        z = cp == 0
        zeros += int(z.sum())
        e = (bits[~z] >> 23) - 127            # non-zero priors lie in [2^-(s+1), 2^-s): exponent -(s+1)
        assert ((e >= -20) & (e <= -1)).all()
        binades.update(int(x) for x in e)
        for g in range(48):
            t = bits[3 * g:3 * g + 3]
            assert (t == 0).all() or (t[0] % 4 == 0 and (np.diff(t) == 1).all()), (i, g)
    assert binades == set(range(-20, 0)) and 0 < zeros < 0.1 * pol.size
