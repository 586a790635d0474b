"""canon_key_child == canon_key over whole games (libhz.so's hz_key_check).

Plays 4096 boards from reset to the end with the build's action rule and,
at every ply, checks the child key of every legal action of every board in
both key forms.  Prints one JSON line: pairs checked, mismatches.
    python tools/key_check.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "harmonies-alphazero_amd"))
from hzamd import _native as nat  # noqa: E402
from hzamd.env import BatchedEnv  # noqa: E402


def main():
    lib = nat.lib()
    n = int(os.environ.get("HZ_KC_BOARDS", "4096"))
    env = BatchedEnv(n, seed_base=12345)
    env.reset()
    out = torch.zeros(3, dtype=torch.int64, device="cuda")
    plies = 0
    while not bool(env.done().all()):
        st = env.export_state().contiguous()
        nat.check(lib.hz_key_check(nat.ptr(st), n, nat.ptr(out), nat.stream_ptr(st.device)), "hz_key_check")
        env.rule_ply()
        plies += 1
    torch.cuda.synchronize()
    r = {"boards": n, "plies": plies, "pairs": int(out[0]), "mismatch": int(out[1]), "step_fail": int(out[2])}
    print(json.dumps(r))
    if r["mismatch"] or r["step_fail"] or not r["pairs"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
