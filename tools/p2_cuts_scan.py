"""k_play2's draw cuts (HZ_P2_DCUTS) scanned on one build: us per hz_play
launch by HIP events, 200 back-to-back launches x 5, twice per setting, at
4096 boards.  The build is HZ_LIB's (compile-time cuts such as -DHZ_P2_BEND,
-DHZ_P2_AEND: one process per build).  Prints one JSON line:
{"lib": ..., "cuts": {"a,b,c,d": [[min, median], [min, median]], ...}}.
Usage (GPU box): HZ_LIB=... python tools/p2_cuts_scan.py "6,11,15,19" "5,10,15,19" ..."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "harmonies-alphazero_amd"))
import numpy as np
import torch
from hzamd.env import BatchedEnv

n = int(os.environ.get("HZ_P2_BOARDS", "4096"))
settings = sys.argv[1:] or ["6,11,15,19"]
g = torch.zeros(n, dtype=torch.int32, device="cuda")
st = torch.zeros(n, dtype=torch.int32, device="cuda")


def measure(env):
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            env.rollout(200, games_done=g, steps_done=st, reset=True)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / 200)
    return [round(float(np.min(ts)), 3), round(float(np.median(ts)), 3)]


out = {}
for rep in range(2):
    for s in settings:
        os.environ["HZ_P2_DCUTS"] = s  # (read when the env is created)
        env = BatchedEnv(n, device="cuda")
        env.set_pipeline(2)
        for _ in range(40):
            env.rollout(200, games_done=g, steps_done=st, reset=True)
        torch.cuda.synchronize()
        out.setdefault(s, []).append(measure(env))
        env.check_errors()
        env.close()
print(json.dumps({"lib": os.path.basename(os.environ.get("HZ_LIB", "libhz.so")), "boards": n, "cuts": out}))
