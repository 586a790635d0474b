"""Measurements for asynchronous self-play (SelfPlay.play_async; DESIGN.md §10
item 11; results under profiles/r24/).

    python tools/async_selfplay_ab.py --out DIR --parent-tree PARENT [--boards 4096] [--moves 32]
                                      [--only claim|same|turn]

PARENT is a checkout of the parent commit with its libhz.so built.  The driver
runs every leg as a fresh child process under a time limit of its own, legs
alternating between the two trees, and stops at the first leg that does not
exit with status 0; each leg prints one JSON line, collected in
DIR/async_legs.jsonl.  Playout caps on in every self-play leg: fast 40, full
200, p 0.25, the default network, one GPU.

  claim  three legs per side, the same board-moves each: play_async(moves) of
         this tree against play_steady(moves) of PARENT.  Board-moves/s, full
         records/s, leaf evaluations per board-move, sim steps, mean live rows
         per sim step.  The async leg then runs play_async cut after a fixed
         number of sim steps that no board can finish in: the steady-state rate
         without the ragged end of a finite run.
  same   play_steady(moves) of this tree (against PARENT's legs of `claim`) and
         bench.py --gpus 1 --steps 20 --warmup 5 in both trees, three
         alternating legs per side: nothing else moved.
  turn   one leg: events after expand + backup, after the masked begin and
         before the next select over a stretch of sim steps: microseconds per
         sim step in the turn sequence next to the step's total.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMS, FAST, P = 200, 40, 0.25
CUT_STEPS, CUT_MOVES = 1500, 48   # 48 moves take a board at least 48 * 40 sim steps: none stops before the cut


def selfplay(tree, boards):
    sys.path[:0] = [tree, os.path.join(tree, "harmonies-alphazero_amd")]
    import torch
    from hzamd.mcts import BatchedPredictor
    from hzamd.net import HarmoniesNet
    from hzamd.selfplay import SelfPlay
    torch.manual_seed(0)
    ev = BatchedPredictor(HarmoniesNet().cuda().eval())
    cfg = {"num_simulations": SIMS, "playout_cap_p": P, "playout_cap_fast": FAST}
    return torch, SelfPlay(boards, ev, cfg, seed_base=5, device="cuda")


def timed(torch, sp, run):
    torch.cuda.synchronize()
    rows0 = int(sp.mcts.eval_rows_total.item())
    t0 = time.perf_counter()
    rec = run()
    torch.cuda.synchronize()
    return rec, time.perf_counter() - t0, int(sp.mcts.eval_rows_total.item()) - rows0


def figures(rec, seconds, rows, board_moves, steps, full):
    return {"seconds": seconds, "board_moves": board_moves, "board_moves_per_s": board_moves / seconds,
            "full_records_per_s": full / seconds, "leaf_evals_per_board_move": rows / board_moves,
            "sim_steps": steps, "live_rows_per_step": rows / max(1, steps), "us_per_sim_step": seconds / steps * 1e6}


def leg_steady(args):
    torch, sp = selfplay(args.tree, args.boards)
    sp.play_steady(3)   # warm-up (the tail bound is known from the third move on)
    rec, el, rows = timed(torch, sp, lambda: sp.play_steady(args.moves))
    return figures(rec, el, rows, args.boards * args.moves, args.moves * SIMS, int(rec["full"].sum()))


def leg_async(args):
    torch, sp = selfplay(args.tree, args.boards)
    sp.play_async(3)    # warm-up (as many moves as the barrier leg's: the timed runs draw under the same move keys)
    rec, el, rows = timed(torch, sp, lambda: sp.play_async(args.moves))
    out = figures(rec, el, rows, args.boards * args.moves, rec["sim_steps"], int(rec["full"].sum()))
    # the steady state: a run cut before any board can stop
    rec, el, rows = timed(torch, sp, lambda: sp.play_async(CUT_MOVES, sim_steps=CUT_STEPS))
    done = rec["moves_done"].to(torch.int64)
    assert int(done.max()) < CUT_MOVES
    reached = torch.arange(CUT_MOVES, device=done.device).unsqueeze(1) < done.unsqueeze(0)
    cut = figures(rec, el, rows, int(done.sum()), rec["sim_steps"], int((rec["full"] & reached).sum()))
    out["cut"] = cut
    return out


def leg_turn(args):
    torch, sp = selfplay(args.tree, args.boards)
    sp.play_async(2)    # warm-up
    marks = {"select": [], "expanded": [], "begun": []}

    def mark(name):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks[name].append(ev)
    m = sp.mcts
    select_gather, expand_backup, begin_some = m.select_gather, m.expand_backup, m.begin_some

    def sel(*a, **kw):
        mark("select")
        return select_gather(*a, **kw)

    def exp(*a, **kw):
        expand_backup(*a, **kw)
        mark("expanded")

    def beg(*a, **kw):
        begin_some(*a, **kw)
        mark("begun")
    m.select_gather, m.expand_backup, m.begin_some = sel, exp, beg
    sp.play_async(CUT_MOVES, sim_steps=args.turn_steps)
    torch.cuda.synchronize()
    begun = marks["begun"][1:]   # (the first masked begin comes before the first sim step)
    n = min(len(marks["select"]), len(marks["expanded"]), len(begun))
    lo = n // 4                  # past the start, where every board turns in the same few steps
    turn = [marks["expanded"][i].elapsed_time(begun[i]) for i in range(lo, n)]
    step = [marks["select"][i].elapsed_time(marks["select"][i + 1]) for i in range(lo, n - 1)]
    turn_us, step_us = sum(turn) / len(turn) * 1e3, sum(step) / len(step) * 1e3
    return {"steps_timed": len(step), "turn_us_per_sim_step": turn_us, "sim_step_us": step_us,
            "turn_share": turn_us / step_us}


def leg_bench(args):
    cmd = [sys.executable, os.path.join(args.tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=args.tree, check=True)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return {"bench": json.loads(line)}


LEGS = {"async": leg_async, "steady": leg_steady, "turn": leg_turn, "bench": leg_bench}


def child(args):
    out = LEGS[args.leg](args)
    out.update({"leg": args.leg, "name": args.name, "tree": "parent" if args.is_parent else "this", "boards": args.boards,
                "moves": args.moves})
    print("LEG " + json.dumps(out), flush=True)


def driver(args):
    if not args.out or not args.parent_tree:
        sys.exit("the driver needs --out DIR and --parent-tree PARENT")
    os.makedirs(args.out, exist_ok=True)
    parent = os.path.abspath(args.parent_tree)
    legs = []
    for i in range(3):
        if args.only in (None, "claim"):
            legs += [("async", HERE, 300), ("steady", parent, 300)]
        if args.only in (None, "same"):
            legs += [("steady", HERE, 300), ("bench", HERE, 300), ("bench", parent, 300)]
    if args.only in (None, "turn"):
        legs.append(("turn", HERE, 300))
    with open(os.path.join(args.out, "async_legs.jsonl"), "a") as log:
        for k, (leg, tree, limit) in enumerate(legs):
            env = dict(os.environ)
            env.pop("HZ_LIB", None)
            name = f"{k:02d}_{leg}_{'parent' if tree == parent else 'this'}"
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg,
                   "--name", name, "--tree", tree, "--boards", str(args.boards), "--moves", str(args.moves),
                   "--turn-steps", str(args.turn_steps)] + (["--is-parent"] if tree == parent else [])
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            lines = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
            if r.returncode != 0 or not lines:
                log.write(json.dumps({"name": name, "status": r.returncode, "stderr": r.stderr[-2000:]}) + "\n")
                print(f"{name}: status {r.returncode}; stopping\n{r.stderr[-2000:]}")
                sys.exit(1)   # nothing more is started on the GPU
            log.write(lines[-1] + "\n")
            log.flush()
            print(name, lines[-1], flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="directory for async_legs.jsonl (the driver needs it)")
    ap.add_argument("--parent-tree", help="a checkout of the parent commit, built (the driver needs it)")
    ap.add_argument("--boards", type=int, default=4096)
    ap.add_argument("--moves", type=int, default=32)
    ap.add_argument("--turn-steps", type=int, default=400)
    ap.add_argument("--only", choices=["claim", "same", "turn"])
    ap.add_argument("--leg", choices=sorted(LEGS))
    ap.add_argument("--name")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--is-parent", action="store_true")
    a = ap.parse_args()
    child(a) if a.leg else driver(a)
