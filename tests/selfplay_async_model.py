"""Host model of the turn order of SelfPlay.play_async (the layered sim step:
select, evaluate, expand + backup, then the turn).

A board's k-th search begins in the turn of the sim step in which its move
k - 1 was played (before the first sim step for k = 0), is walked once per sim
step for budget[b, k] steps, and the board turns in the sim step of its last
simulation.  A search of budget 0 (a fast budget of 0, or a stuck root) is not
walked and turns in the first sim step after it began.  So move k of board b
is played in sim step

    turn[b, k] = sum over j <= k of max(budget[b, j], 1)        (1-based)

and the run takes max over b of turn[b, K - 1] sim steps."""
import numpy as np


def turn_steps(budgets):
    """budgets int [n, K] -> the 1-based sim step in which each move is played, int64 [n, K]."""
    b = np.asarray(budgets, np.int64)
    if b.ndim != 2 or (b < 0).any():
        raise ValueError("budgets: a non-negative [n, K] array")
    return np.cumsum(np.maximum(b, 1), axis=1)


def sim_steps(budgets):
    """The sim steps of a whole run (0 for a run without moves)."""
    t = turn_steps(budgets)
    return int(t[:, -1].max()) if t.size else 0


def moves_done_after(budgets, steps):
    """The moves each board has made after `steps` sim steps, int64 [n]."""
    return (turn_steps(budgets) <= int(steps)).sum(axis=1)


def step_bound(budgets):
    """The bound a run must meet in either form of the sim step (a turned board
    may sit out one evaluation slot in the fused form): max_b sum_k (budget + 1)."""
    b = np.asarray(budgets, np.int64)
    return int((b + 1).sum(axis=1).max()) if b.size else 0
