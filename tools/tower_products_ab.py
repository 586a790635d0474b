"""A/B of the tower modes x6 / x3 / x1 (6, 3 or 1 bf16 piece products per fp32
product: FoldedNet(tower=...)) on the whole leaf-eval forward
(FoldedNet.predict), in ONE process with the modes interleaved round by
round: events around 20 forwards per round, a warm-up for every (mode,
batch), batches 1, 32, 256, 896, 4096.  A second process of the same call
(HZ_X6_W4=0 HZ_X6_BLOCK=0 HZ_TOWER_LOOP=0 set at its start) times x6 layered
through the generic k_conv3x3_x6 forms, the kernels x3 and x1 run, with x3
beside it as the yardstick between the two processes.
At 4096 rows each mode's logits, probabilities and value are compared with
the unfolded float64 network (max and RMS deviation), beside PyTorch's fp32
CPU forward's deviation on the same rows.
Writes profiles/r08/tower_products_ab.json (and prints it).
Usage (GPU box): python tools/tower_products_ab.py [rounds] [outdir]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "harmonies-alphazero_amd")]

import torch  # noqa: E402

from hzamd.infer import FoldedNet  # noqa: E402
from hzamd.net import HarmoniesNet  # noqa: E402

CHILD = "--generic-child" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
rounds = int(args[0]) if args else 10
outdir = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "r08")
BATCHES = (1, 32, 256, 896, 4096)
FWD = 20
MODES = ("x6", "x3") if CHILD else ("x6", "x3", "x1")


def randomise_bn(net, g):  # tests/test_infer_cpu.py:_randomise_bn
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            with torch.no_grad():
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)


g = torch.Generator().manual_seed(11)
torch.manual_seed(1)
net = HarmoniesNet().eval()
randomise_bn(net, g)
n = max(BATCHES)
board = (torch.rand(n, 38, 5, 7, generator=g) > 0.8).float()
glob = torch.rand(n, 42, generator=g)

accuracy = None
if not CHILD:
    with torch.no_grad():
        l64, v64 = net.double()(board.double(), glob.double())
        net.float()
        l32, v32 = net(board, glob)
    p64 = torch.softmax(l64, 1)

    def dev(lo, pr, v):
        out = {}
        for name, got, want in (("logits", lo, l64), ("probs", pr, p64), ("value", v.reshape(-1), v64.reshape(-1))):
            d = got.double().cpu() - want
            out[name] = {"max": d.abs().max().item(), "rms": d.pow(2).mean().sqrt().item()}
        out["argmax_agrees"] = (lo.cpu().argmax(1) == l64.argmax(1)).float().mean().item()
        return out
    accuracy = {"torch_fp32_cpu": dev(l32, torch.softmax(l32, 1), v32)}

net = net.cuda()
board, glob = board.cuda(), glob.cuda()
fnets = {m: FoldedNet(net, tower=m) for m in MODES}
if not CHILD:
    for m, f in fnets.items():
        lo, v = f(board, glob)
        accuracy[m] = dev(lo, f.predict(board, glob)[0], v)

times = {}
for B in BATCHES:
    b, gl = board[:B].contiguous(), glob[:B].contiguous()
    ts = {m: [] for m in MODES}
    for m in MODES:  # warm-up of every (mode, batch)
        for _ in range(FWD):
            fnets[m].predict(b, gl)
    torch.cuda.synchronize()
    for r in range(rounds):
        order = MODES[r % len(MODES):] + MODES[:r % len(MODES)]
        for m in order:
            f = fnets[m]
            f.predict(b, gl)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(FWD):
                f.predict(b, gl)
            e1.record()
            torch.cuda.synchronize()
            ts[m].append(e0.elapsed_time(e1) / FWD)
    times[B] = {m: {"ms_median": sorted(v)[len(v) // 2], "ms_min": min(v), "ms_max": max(v),
                    "ms_all": [round(x, 4) for x in v]} for m, v in ts.items()}

result = {"rounds": rounds, "forwards_per_round": FWD, "device": torch.cuda.get_device_name(0),
          "env": {k: os.environ.get(k) for k in ("HZ_X6_W4", "HZ_X6_BLOCK", "HZ_TOWER_LOOP", "HZ_TOWER")},
          "ms_per_forward": times}
if CHILD:
    print("CHILD_JSON " + json.dumps(result))
    sys.exit(0)
result["accuracy_4096_rows_vs_float64"] = accuracy
env = dict(os.environ, HZ_X6_W4="0", HZ_X6_BLOCK="0", HZ_TOWER_LOOP="0")
del fnets
torch.cuda.synchronize()
torch.cuda.empty_cache()
r = subprocess.run([sys.executable, os.path.abspath(__file__), str(rounds), "--generic-child"], env=env,
                   capture_output=True, text=True, timeout=600)
child = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD_JSON ")]
if r.returncode != 0 or not child:
    sys.stderr.write(r.stdout + r.stderr)
    raise SystemExit(f"the generic-forms process failed ({r.returncode})")
result["x6_generic_forms_process"] = json.loads(child[0][len("CHILD_JSON "):])
os.makedirs(outdir, exist_ok=True)
with open(os.path.join(outdir, "tower_products_ab.json"), "w") as fh:
    json.dump(result, fh, indent=1)
print(json.dumps({"ms_median": {str(B): {m: round(v["ms_median"], 4) for m, v in t.items()} for B, t in times.items()},
                  "ms_median_generic_process": {str(B): {m: round(v["ms_median"], 4) for m, v in t.items()}
                                                for B, t in result["x6_generic_forms_process"]["ms_per_forward"].items()},
                  "accuracy": accuracy}, indent=1))
