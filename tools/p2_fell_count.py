"""How far into its stream a rule game reads, on the CPU oracle: for boards
0..n-1 (seed_base 0, as bench.py's) and episodes 0..E-1 the stream index at
the game's end, i.e. the words of the generation after seeding that the game
consumed.  A pipeline-2 slot holds rows below kAheadTwist = 224 of that
generation; a play stage that has left its script and would read past them
makes the last play stage replay the board's game from scratch
(HZ_P2_FELL_LIMIT).  Prints one JSON line: the count of board-episodes at or
past each row of interest, and the largest index seen.
Usage: python tools/p2_fell_count.py [n=4096] [episodes=256] [procs=8]"""
import json, os, sys
from multiprocessing import Pool
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import oracle

ROWS = (96, 112, 128, 145, 160, 192, 224)


def episode(args):
    n, ep = args
    idx = np.zeros(n, np.int32)
    for b in range(n):
        seed = b + (ep << 32)
        m = oracle.mt_seed(seed)
        st = oracle.reset(m)
        oracle.play_rule_from(st, m, seed, 0, 200)
        idx[b] = m.idx
    return idx


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    E = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    procs = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    oracle.lib()
    with Pool(procs) as pool:
        idx = np.stack(pool.map(episode, [(n, ep) for ep in range(E)]))
    print(json.dumps({"boards": n, "episodes": E, "seed_base": 0, "board_episodes": int(idx.size),
                      "words_max": int(idx.max()), "words_mean": float(idx.mean()),
                      "reaching_row": {str(r): int((idx >= r).sum()) for r in ROWS}}))
