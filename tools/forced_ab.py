"""Measurements for forced playouts and policy target pruning (DESIGN.md §10
item 10; results under profiles/r23/).

    python tools/forced_ab.py --out DIR [--boards 4096] [--parent-lib OLD.so] [--only off|forced]

The driver runs every leg as a fresh child process (this file with --leg)
under a time limit of its own and stops at the first leg that does not exit
with status 0; each leg prints one JSON line, collected in
DIR/forced_legs.jsonl.  Default network, one GPU, 200 simulations.

  off     (needs --parent-lib: libhz.so of the parent commit) three alternating
          legs per side, the gate off: ms per move and tree ms per move (move
          time minus the event-timed leaf evaluations) over 3 moves from the
          game start, then one complete game on every board (games/s).  With
          the gate off the search launches instantiations that hold none of the
          new code, so the two sides' ranges should overlap.
  forced  the same boards, continuous moves (SelfPlay.play_steady): the gate off
          against `forced_playouts: 2`.  Board-moves/s, leaf evaluations per
          board-move and tree ms per move (event-timed over 3 probe moves);
          with the gate on also, over 3 further moves outside the timed ones,
          the share of root selections the forced rule decided
          (BatchedMCTS.forced_counts), the share of root visits pruning took
          back and the share of visited root edges it zeroed.

Whether records made this way train a stronger network is a strength question
this tool does not answer.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "harmonies-alphazero_amd"), os.path.join(ROOT, "tools")]

K = 2.0  # KataGo's value; not tuned here


def leg_off(args):
    from playout_cap_ab import leg_gate
    return leg_gate(args)  # the same probe: 3 + 3 moves from the start, then one complete game


def leg_forced(args):
    import torch
    from playout_cap_ab import SIMS, selfplay  # the same boards, network and seed as that tool's legs
    on = args.leg == "forced_on"
    sp, ev = selfplay(args.boards, {"forced_playouts": K} if on else {})
    sp.play_steady(3)  # warm-up
    torch.cuda.synchronize()
    rows0 = int(sp.mcts.eval_rows_total.item())
    t0 = time.perf_counter()
    sp.play_steady(args.moves, reset=False)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    rows = int(sp.mcts.eval_rows_total.item()) - rows0
    bm = args.boards * args.moves
    # tree ms per move: 3 probe moves, the move time minus the event-timed leaf evaluations
    ev.on = True
    t0 = time.perf_counter()
    sp.play_steady(3, reset=False)
    torch.cuda.synchronize()
    ms_inst = (time.perf_counter() - t0) / 3 * 1e3
    s, e = ev.take()
    nn_ms = sum(a.elapsed_time(b) for a, b in zip(s, e)) / 3
    ev.on = False
    out = {"sims": SIMS, "forced_playouts": K if on else None, "moves": args.moves, "seconds": el,
           "board_moves_per_s": bm / el, "leaf_evals_per_board_move": rows / bm, "ms_per_move": el / args.moves * 1e3,
           "tree_ms_per_move": ms_inst - nn_ms, "nn_ms_per_move": nn_ms}
    if on:
        # what the two rules did, over 3 further moves: after each move (play_steady's progress hook; the gate and
        # the tree are the move's until the next search) the raw and the pruned visits and the search's counters
        tot = torch.zeros(6, dtype=torch.int64, device=sp.device)

        def counted(move):
            raw, fc = sp.last_visits, sp.mcts.forced_counts()
            pruned = sp.mcts.pruned_visits(sp.cfg["cpuct"])
            tot.add_(torch.stack([fc[:, 0].sum(), fc[:, 1].sum(), raw.sum(), pruned.sum(), (raw > 0).sum(),
                                  ((raw > 0) & (pruned == 0)).sum()]).to(torch.int64))
        sp.play_steady(3, reset=False, progress=counted)
        sel, forced, raw, kept, edges, zeroed = (int(x) for x in tot.tolist())
        out.update({"stat_moves": 3, "root_selections": sel, "root_selections_forced": forced,
                    "forced_share_of_root_selections": forced / max(sel, 1), "root_visits": raw,
                    "root_visits_pruned": raw - kept, "pruned_share_of_root_visits": (raw - kept) / max(raw, 1),
                    "visited_root_edges": edges, "root_edges_zeroed": zeroed,
                    "zeroed_share_of_visited_root_edges": zeroed / max(edges, 1)})
    return out


def child(args):
    out = leg_off(args) if args.leg.startswith("off") else leg_forced(args)
    out.update({"leg": args.leg, "boards": args.boards,
                "lib": "parent commit (HZ_LIB)" if os.environ.get("HZ_LIB") else "in-tree"})
    print("LEG " + json.dumps(out), flush=True)


def driver(args):
    if not args.out:
        sys.exit("the driver needs --out DIR")
    os.makedirs(args.out, exist_ok=True)
    legs = []
    if args.only in (None, "off"):
        if not args.parent_lib:
            sys.exit("the off legs need --parent-lib")
        for i in range(3):
            legs += [("off_new_%d" % i, None, 240), ("off_old_%d" % i, os.path.abspath(args.parent_lib), 240)]
    if args.only in (None, "forced"):
        legs += [("forced_off", None, 240), ("forced_on", None, 240)]
    with open(os.path.join(args.out, "forced_legs.jsonl"), "a") as log:
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
                sys.exit(1)  # nothing more is started on the GPU
            log.write(lines[-1] + "\n")
            log.flush()
            print(name, lines[-1], flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="directory for forced_legs.jsonl (the driver needs it)")
    ap.add_argument("--boards", type=int, default=4096)
    ap.add_argument("--moves", type=int, default=30)
    ap.add_argument("--parent-lib")
    ap.add_argument("--only", choices=["off", "forced"])
    ap.add_argument("--leg")
    a = ap.parse_args()
    child(a) if a.leg else driver(a)
