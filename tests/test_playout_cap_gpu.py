"""Playout-cap randomization in SelfPlay (config keys playout_cap_p and
playout_cap_fast): each move a coin per board decides between the full search
(num_simulations, root noise) and the fast one (playout_cap_fast simulations,
no noise); the records gain `full`, and only the full moves become training
records.  64 boards, the stub evaluator, 16 / 4 simulations, p = 0.25, 12
moves, replayed board by board by the C oracle."""
import functools

import numpy as np
import pytest
import torch

import oracle
from hzamd.state import unpack_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

N, BASE, SIMS, FAST, P, MOVES, CPUCT, TAU0 = 64, 5100, 16, 4, 0.25, 12, 2.0, 15
CFG = {"num_simulations": SIMS, "cpuct": CPUCT, "testing": False, "turns_until_tau0": TAU0}
CAP = dict(CFG, playout_cap_p=P, playout_cap_fast=FAST)


def start(sp):
    """Every board's game from its own seed, whatever the env played before."""
    sp.env.reset(seeds=int(sp.env.seed_base) + torch.arange(sp.n, device=DEV, dtype=torch.int64))
    sp.step_counter = 0


def play(cfg, n=N, base=BASE, keep_noise=False):
    from hzamd.mcts import stub_evaluator
    from hzamd.selfplay import SelfPlay
    sp = SelfPlay(n, stub_evaluator, cfg, seed_base=base, device=DEV, max_plies=MOVES)
    sp.keep_noise = keep_noise
    start(sp)
    return sp, sp.play(reset=False)


@functools.lru_cache(maxsize=None)
def capped():
    """The 64-board run with the cap on, played once."""
    return play(CAP, keep_noise=True)


def test_full_is_the_coin_below_p():
    from hzamd.selfplay import NoiseSource
    sp, rec = capped()
    assert rec["plies"] == MOVES and rec["full"].shape == (MOVES, N) and rec["full"].dtype == torch.bool
    assert rec["valid"].all()
    src = NoiseSource(BASE, DEV)
    for t in range(MOVES):
        assert torch.equal(rec["full"][t], src.coin(t, N) < P), t
    share = rec["full"].float().mean().item()
    assert 0.15 < share < 0.35   # 768 coins at p = 0.25: 0.25 +- 6 sigma (0.0156 each)


def test_every_move_matches_oracle_with_its_budget():
    """Each board's 12 moves replayed by the oracle: a full move is the
    oracle's 16-simulation search with the move's noise row, a fast one its
    4-simulation search without noise; the move is chosen from the visits as
    always (tau = 1 sampling with the move's uniform)."""
    from hzamd.mcts import choose_actions
    sp, rec = capped()
    states, visits, full = (rec[k].cpu().numpy() for k in ("states", "visits", "full"))
    log = [tuple(t.cpu().numpy() for t in x) for x in sp.noise_log]
    assert len(log) == MOVES and full.any() and not full.all()
    for b in range(N):
        m = oracle.mt_seed(BASE + b)
        s = oracle.reset(m)
        for t in range(MOVES):
            assert (unpack_ref(states[t, :, b]) == s).all(), (b, t)
            noise, u, act = log[t]
            f = bool(full[t, b])
            a, ov, _, _ = oracle.mcts_search(s, m, SIMS if f else FAST, CPUCT, eps=0.25, testing=not f, tau0=TAU0,
                                             ply=t, u=float(u[b]), noise=noise[b])
            assert (visits[t, b] == ov).all(), (b, t, f)
            assert ov.sum() == (SIMS if f else FAST) - 1
            want = a if f else int(choose_actions(torch.from_numpy(ov)[None], torch.tensor([True]),
                                                  torch.tensor([u[b]], dtype=torch.float64))[0])
            assert act[b] == want, (b, t, f)
            r, s = oracle.step(s, int(act[b]), m)
            assert r == 0
        assert (unpack_ref(rec["final"].cpu().numpy()[:, b]) == s).all(), b


def test_one_batch_equals_two_halves():
    """64 boards at base 5100 against 32 at 5100 and 32 at 5132: coins, noise
    and budgets are keyed by the global board id."""
    _, whole = capped()
    for k in range(2):
        _, part = play(CAP, n=32, base=BASE + 32 * k)
        sl = slice(32 * k, 32 * k + 32)
        assert part["plies"] == MOVES
        for key in ("valid", "visits", "full"):
            assert torch.equal(part[key], whole[key][:, sl]), key
        assert torch.equal(part["states"], whole["states"][:, :, sl])
        assert torch.equal(part["final"], whole["final"][:, sl])


def test_compact_keeps_exactly_the_full_moves():
    sp, rec = capped()
    comp = sp.compact(rec)   # full_only by default with the cap on
    nfull = int(rec["full"].sum())
    assert 0 < nfull < MOVES * N and comp["states"].shape[0] == nfull
    assert (comp["visits"].sum(1) == SIMS - 1).all()
    want = rec["states"].permute(0, 2, 1)[rec["full"]]
    assert torch.equal(comp["states"], want)
    every = sp.compact(rec, full_only=False)
    assert every["states"].shape[0] == MOVES * N
    assert sorted(set(every["visits"].sum(1).tolist())) == [FAST - 1, SIMS - 1]


def test_keys_absent_changes_nothing():
    """Without the keys there is no budget, no mask, no `full`: a SelfPlay
    whose search handle has run capped moves, with the cap then taken away,
    records what one that never saw a budget records."""
    fresh, rec0 = play(CFG)
    assert fresh.playout_cap is None and "full" not in rec0
    assert set(rec0) == {"states", "players", "visits", "valid", "final", "plies"}
    assert (rec0["visits"].sum(2) == SIMS - 1).all() and (fresh.mcts.sims_done() == 0).all()
    sp, rec1 = play(CAP)
    assert not torch.equal(rec1["visits"], rec0["visits"])
    sp.playout_cap = None
    start(sp)
    rec2 = sp.play(reset=False)
    assert set(rec2) == set(rec0)
    for key in ("states", "players", "visits", "valid", "final"):
        assert torch.equal(rec2[key], rec0[key]), key
    comp = sp.compact(rec2)
    assert comp["states"].shape[0] == MOVES * N


def test_tail_bound_from_selfplay_changes_no_bit():
    """With a device-row network evaluator SelfPlay passes search() the tail
    (fast, full boards of the move), known two moves ahead from the coins: the
    records are those of the same run without the tail, and no search raises."""
    from hzamd.mcts import BatchedPredictor
    from hzamd.net import TINY, HarmoniesNet
    from hzamd.selfplay import SelfPlay
    torch.manual_seed(0)
    ev = BatchedPredictor(HarmoniesNet(TINY).to(DEV).eval())
    cfg = {"num_simulations": 8, "cpuct": 1.5, "playout_cap_p": P, "playout_cap_fast": 2}
    recs, tails = [], []
    for use_tail in (True, False):
        sp = SelfPlay(N, ev, cfg, seed_base=BASE, device=DEV)
        search = sp.mcts.search
        seen = []

        def spy(*a, _search=search, _seen=seen, _keep=use_tail, **kw):
            if not _keep:
                kw["tail"] = None
            _seen.append(kw.get("tail"))
            return _search(*a, **kw)
        sp.mcts.search = spy
        recs.append(sp.play_steady(8))
        tails.append(seen)
    assert tails[0][:2] == [None, None] and all(t is not None for t in tails[0][2:]) and not any(tails[1])
    full = recs[0]["full"]
    for t, tl in enumerate(tails[0]):
        if tl is not None:
            assert tl == (2, int(full[t].sum()))
    for key in ("states", "visits", "full", "game", "ended"):
        assert torch.equal(recs[0][key], recs[1][key]), key
