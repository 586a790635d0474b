"""Measurements for the per-board budgets and playout caps (DESIGN.md §10
item 5; results under profiles/r16/).

    python tools/playout_cap_ab.py --out DIR [--boards 4096] [--parent-lib OLD.so] [--only gate|cap]

The driver runs every leg as a fresh child process (this file with --leg)
under a time limit of its own and stops at the first leg that does not exit
with status 0; each leg prints one JSON line, collected in DIR/legs.jsonl.

  gate   (needs --parent-lib: libhz.so of the parent commit) three alternating
         legs per side, budgets off: ms per move and tree ms per move (move time
         minus the event-timed leaf evaluations) over 3 moves from the game
         start, then one complete game on every board (games/s).
  cap    the same boards, 200 / 40 / p 0.25, 80 continuous moves
         (SelfPlay.play_steady): cap off, cap on, cap on without the tail
         bound.  Board-moves/s, leaf evaluations per board-move, full
         records/s, and the time of a sim step before and after simulation 40
         (events at the evaluator's calls over 3 probe moves).

Every max_rows and tail a search gets here is the one SelfPlay.move passes.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "harmonies-alphazero_amd")]

SIMS, FAST, P = 200, 40, 0.25


class Timed:
    """The evaluator with an event before and after every call while `on`:
    the gaps between calls are the sim steps, the pairs the leaf evaluations."""
    device_rows = True

    def __init__(self, ev):
        import torch
        self.ev, self.torch = ev, torch
        self.capturable, self.row_independent = ev.capturable, ev.row_independent
        self.on, self.starts, self.ends = False, [], []

    def __call__(self, board, glob, rows=None, count=None):
        if not self.on:
            return self.ev(board, glob, rows, count)
        a, b = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        a.record()
        out = self.ev(board, glob, rows, count)
        b.record()
        self.starts.append(a)
        self.ends.append(b)
        return out

    def take(self):
        self.torch.cuda.synchronize()
        s, e = self.starts, self.ends
        self.starts, self.ends = [], []
        return s, e


def selfplay(boards, cfg):
    import torch
    from hzamd.mcts import BatchedPredictor
    from hzamd.net import HarmoniesNet
    from hzamd.selfplay import SelfPlay
    torch.manual_seed(0)
    ev = Timed(BatchedPredictor(HarmoniesNet().cuda().eval()))
    return SelfPlay(boards, ev, dict({"num_simulations": SIMS}, **cfg), seed_base=5, device="cuda"), ev


def leg_gate(args):
    import torch
    sp, ev = selfplay(args.boards, {})
    sp.env.reset()
    sp.move(0)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(3):
        sp.move(1 + k)
    torch.cuda.synchronize()
    ms_move = (time.perf_counter() - t0) / 3 * 1e3
    ev.on = True
    t0 = time.perf_counter()
    for k in range(3):
        sp.move(4 + k)
    torch.cuda.synchronize()
    ms_inst = (time.perf_counter() - t0) / 3 * 1e3
    s, e = ev.take()
    nn_ms = sum(a.elapsed_time(b) for a, b in zip(s, e)) / 3
    ev.on = False
    sp.check_steps()
    t0 = time.perf_counter()
    rec = sp.play()
    torch.cuda.synchronize()
    game_s = time.perf_counter() - t0
    return {"ms_per_move": ms_move, "tree_ms_per_move": ms_inst - nn_ms, "nn_ms_per_move": nn_ms,
            "game_s": game_s, "games_per_s": args.boards / game_s, "plies": rec["plies"]}


def leg_cap(args):
    import torch
    on = args.leg != "cap_off"
    sp, ev = selfplay(args.boards, {"playout_cap_p": P, "playout_cap_fast": FAST} if on else {})
    use_tail = args.leg != "cap_on_notail"
    if not use_tail:   # the same searches without the tail bound SelfPlay.move passes
        search = sp.mcts.search
        sp.mcts.search = lambda *a, **kw: search(*a, **dict(kw, tail=None))
    sp.play_steady(3)   # warm-up (the tail bound is known from the third move on)
    torch.cuda.synchronize()
    rows0 = int(sp.mcts.eval_rows_total.item())
    t0 = time.perf_counter()
    rec = sp.play_steady(args.moves, reset=False)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    rows = int(sp.mcts.eval_rows_total.item()) - rows0
    bm = args.boards * args.moves
    full = int(rec["full"].sum()) if "full" in rec else bm
    out = {"moves": args.moves, "seconds": el, "board_moves_per_s": bm / el, "leaf_evals_per_board_move": rows / bm,
           "full_records_per_s": full / el, "full_share": full / bm, "tail": bool(on and use_tail)}
    # sim-step times: the gaps between the evaluator's calls over 3 probe moves
    ev.on = True
    sp.play_steady(3, reset=False)
    s, _ = ev.take()
    assert len(s) == 3 * SIMS
    early, late = [], []
    for mv in range(3):
        st = s[mv * SIMS:(mv + 1) * SIMS]
        gaps = [st[i].elapsed_time(st[i + 1]) for i in range(SIMS - 1)]
        early += gaps[5:FAST - 5]
        late += gaps[FAST + 5:SIMS - 5]
    out["sim_step_us_before_40"] = sum(early) / len(early) * 1e3
    out["sim_step_us_after_40"] = sum(late) / len(late) * 1e3
    return out


def child(args):
    out = leg_gate(args) if args.leg.startswith("gate") else leg_cap(args)
    out.update({"leg": args.leg, "boards": args.boards, "lib": os.environ.get("HZ_LIB") or "in-tree"})
    print("LEG " + json.dumps(out), flush=True)


def driver(args):
    if not args.out:
        sys.exit("the driver needs --out DIR")
    os.makedirs(args.out, exist_ok=True)
    legs = []
    if args.only in (None, "gate"):
        if not args.parent_lib:
            sys.exit("the gate legs need --parent-lib")
        for i in range(3):
            legs += [("gate_new_%d" % i, None, 240), ("gate_old_%d" % i, os.path.abspath(args.parent_lib), 240)]
    if args.only in (None, "cap"):
        legs += [("cap_off", None, 300), ("cap_on", None, 240), ("cap_on_notail", None, 240)]
    with open(os.path.join(args.out, "legs.jsonl"), "a") as log:
        for name, lib, limit in legs:
            env = dict(os.environ)
            env.pop("HZ_LIB", None)
            if lib:
                env["HZ_LIB"] = lib
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", name,
                   "--boards", str(args.boards), "--moves", str(args.moves)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            lines = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
            if r.returncode != 0 or not lines:
                log.write(json.dumps({"leg": name, "status": r.returncode, "stderr": r.stderr[-2000:]}) + "\n")
                print(f"{name}: status {r.returncode}; stopping\n{r.stderr[-2000:]}")
                sys.exit(1)   # nothing more is started on the GPU
            log.write(lines[-1] + "\n")
            log.flush()
            print(name, lines[-1], flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="directory for legs.jsonl (the driver needs it)")
    ap.add_argument("--boards", type=int, default=4096)
    ap.add_argument("--moves", type=int, default=80)
    ap.add_argument("--parent-lib")
    ap.add_argument("--only", choices=["gate", "cap"])
    ap.add_argument("--leg")
    a = ap.parse_args()
    child(a) if a.leg else driver(a)
