"""Measurements for tree reuse (results under
profiles/r17/).

    python tools/tree_reuse_ab.py --out DIR [--boards 4096] [--parent-lib OLD.so] [--only off|reuse]

The driver runs every leg as a fresh child process (this file with --leg)
under a time limit of its own and stops at the first leg that does not exit
with status 0; each leg prints one JSON line, collected in
DIR/tree_reuse_legs.jsonl.  Default network, 200 simulations.

  off    (needs --parent-lib: libhz.so of the parent commit) three alternating
         legs per side, tree reuse off: ms per move and tree ms per move (move
         time minus the event-timed leaf evaluations) over 3 moves from the
         game start, then one complete game on every board (games/s).  No
         search kernel changed, so the two sides' ranges should overlap.
  reuse  the same boards, continuous moves (SelfPlay.play_steady): reuse off,
         "add" and "topup".  Board-moves/s, leaf evaluations per board-move,
         the share of board-moves whose tree was carried by the phase of the
         move played, the mean carried visits, and the event-timed cost of
         advance() per move.

Whether "topup" records train as well as fresh 200-simulation ones is a
strength question this tool does not answer.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "harmonies-alphazero_amd"), os.path.join(ROOT, "tools")]

PHASES = ["choose_pile", "place_tile_1", "place_tile_2", "place_tile_3"]


def leg_off(args):
    from playout_cap_ab import leg_gate
    return leg_gate(args)  # the same probe: 3 + 3 moves from the start, then one complete game


def leg_reuse(args):
    import torch
    from playout_cap_ab import selfplay  # the same boards, network and seed as that tool's legs
    mode = {"reuse_off": None, "reuse_add": "add", "reuse_topup": "topup"}[args.leg]
    sp, ev = selfplay(args.boards, {"tree_reuse": mode} if mode else {})
    events = []
    if mode:  # advance() between two events, every move
        advance = sp.mcts.advance

        def timed(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = advance(*a, **kw)
            e1.record()
            events.append((e0, e1))
            return out
        sp.mcts.advance = timed
    sp.play_steady(3)  # warm-up
    torch.cuda.synchronize()
    del events[:]
    rows0 = int(sp.mcts.eval_rows_total.item())
    t0 = time.perf_counter()
    rec = sp.play_steady(args.moves, reset=False)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    rows = int(sp.mcts.eval_rows_total.item()) - rows0
    bm = args.boards * args.moves
    out = {"mode": mode or "off", "moves": args.moves, "seconds": el, "board_moves_per_s": bm / el,
           "leaf_evals_per_board_move": rows / bm, "max_nodes": sp.mcts.max_nodes}
    if mode:
        us = [a.elapsed_time(b) * 1e3 for a, b in events]
        out["advance_us_per_move"] = sum(us) / len(us)
        out["advance_us_max"] = max(us)
        carried = rec["carried"][1:]  # what the move before left for this one
        # the turn phase of the recorded state: bits 42-44 of its sixth word (hzamd/state.py pack_ref:
        # misc |= v[73] << 42; PHASES order)
        phase = (rec["states"][:-1, 5] >> 42) & 7
        out["carried_share"] = float((carried > 0).float().mean())
        out["mean_carried_visits"] = float(carried.float().mean())
        out["mean_carried_visits_where_carried"] = float(carried[carried > 0].float().mean())
        out["carried_share_by_phase"] = {
            PHASES[p]: float((carried[phase == p] > 0).float().mean()) for p in range(4) if bool((phase == p).any())}
        out["flagged_boards"] = int(sp.mcts.limit_hits_total.item())
    return out


def child(args):
    out = leg_off(args) if args.leg.startswith("off") else leg_reuse(args)
    out.update({"leg": args.leg, "boards": args.boards, "lib": os.environ.get("HZ_LIB") or "in-tree"})
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
    if args.only in (None, "reuse"):
        legs += [("reuse_off", None, 300), ("reuse_add", None, 300), ("reuse_topup", None, 300)]
    with open(os.path.join(args.out, "tree_reuse_legs.jsonl"), "a") as log:
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
    ap.add_argument("--out", help="directory for tree_reuse_legs.jsonl (the driver needs it)")
    ap.add_argument("--boards", type=int, default=4096)
    ap.add_argument("--moves", type=int, default=40)
    ap.add_argument("--parent-lib")
    ap.add_argument("--only", choices=["off", "reuse"])
    ap.add_argument("--leg")
    a = ap.parse_args()
    child(a) if a.leg else driver(a)
