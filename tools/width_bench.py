"""FoldedNet.predict at other filter counts: the width-generic HIP path
(csrc/hz_net_wide.hip) against the MIOpen / PyTorch fallback, and its one-
against its eight-state workgroup form.

Nets: 32x1 (hidden 64: hzamd.net.TINY), 64x8 and 256x8.  Each measurement is
microseconds per predict from HIP events around n back-to-back calls after a
warm-up (n sized to a window of ~0.1 s), in a process of its own per tree.
With --parent DIR (the package directory of a build of the parent commit:
its hzamd/ and libhz.so) the processes alternate between this tree and that
one, --reps times each; the table gives each entry's median and its
(min, max) over the repetitions.

    python tools/width_bench.py [--parent DIR] [--reps 3] [--out FILE]

Modes: "hip" = the default dispatch, "spg1" / "spg8" = the conv form forced,
"fallback" = native_conv=False (MIOpen convs, hz_bias_act, PyTorch heads);
a tree without the width-generic path (the parent) has "default" only, which
is that fallback.  "sha" is a digest of predict's output for 32 rows: equal
digests mean equal bits."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = {"32x1": dict(cnn_filters=32, num_res_blocks=1, value_head_hidden_dim=64),
        "64x8": dict(cnn_filters=64, num_res_blocks=8),
        "256x8": dict(cnn_filters=256, num_res_blocks=8)}
ROWS = (1, 32, 256, 1024, 4096)
FORM_ROWS = (1, 32, 64, 128, 256, 512, 1024, 4096)  # the two forms' curves, for the threshold


def worker(pkg):
    sys.path[:0] = [ROOT, pkg]
    import torch
    from hzamd.infer import FoldedNet
    from hzamd.net import HarmoniesNet
    if not torch.cuda.is_available():
        raise SystemExit("width_bench needs a GPU")

    def timed(fnet, board, glob):
        for _ in range(5):
            fnet.predict(board, glob)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 5
        while True:
            e0.record()
            for _ in range(n):
                fnet.predict(board, glob)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 100.0 or n >= 2000:
                return round(ms * 1e3 / n, 1)
            n = min(2000, max(n * 2, int(n * 110.0 / max(ms, 1e-3))))

    out = {}
    for name, cfg in NETS.items():
        torch.manual_seed(0)
        net = HarmoniesNet(cfg).eval().cuda()
        hip = FoldedNet(net)
        wide = getattr(hip, "wide", None) is not None
        modes = {"hip": (hip, 0), "spg1": (hip, 1), "spg8": (hip, 8),
                 "fallback": (FoldedNet(net, native_conv=False), 0)} if wide else {"default": (hip, 0)}
        g = torch.Generator().manual_seed(1)
        board = (torch.rand(max(FORM_ROWS), 38, 5, 7, generator=g) > 0.8).float().cuda()
        glob = torch.rand(max(FORM_ROWS), 42, generator=g).cuda()
        res = {}
        for mode, (fnet, spg) in modes.items():
            fnet.wide_spg = spg
            row = {}
            for batch in (FORM_ROWS if mode in ("spg1", "spg8") else ROWS):
                row[batch] = timed(fnet, board[:batch].contiguous(), glob[:batch].contiguous())
            p, v = fnet.predict(board[:32].contiguous(), glob[:32].contiguous())
            row["sha"] = hashlib.sha1(p.cpu().numpy().tobytes() + v.cpu().numpy().tobytes()).hexdigest()[:12]
            res[mode] = row
            fnet.wide_spg = 0
        out[name] = res
    print("WIDTH_BENCH " + json.dumps(out))


def summarise(runs):
    """[{net: {mode: {rows: us}}}] -> {net: {mode: {rows: [median, min, max]}}} (sha: the set seen)."""
    out = {}
    for net in runs[0]:
        out[net] = {}
        for mode in runs[0][net]:
            cell = {}
            for k in runs[0][net][mode]:
                vals = [r[net][mode][k] for r in runs]
                cell[k] = sorted(set(vals)) if k == "sha" else [statistics.median(vals), min(vals), max(vals)]
            out[net][mode] = cell
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", metavar="PKG")
    ap.add_argument("--parent", metavar="DIR")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    trees = {"this": os.path.join(ROOT, "harmonies-alphazero_amd")}
    if a.parent:
        trees["parent"] = os.path.abspath(a.parent)
    runs = {k: [] for k in trees}
    for rep in range(a.reps):
        for k, pkg in trees.items():  # alternating processes
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", pkg], capture_output=True,
                               text=True, timeout=900)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("WIDTH_BENCH ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
                raise SystemExit(f"worker for {k} failed ({r.returncode})")
            runs[k].append(json.loads(line[0][len("WIDTH_BENCH "):]))
            print(f"rep {rep} {k}: done", flush=True)
    res = {"us_per_predict": {k: summarise(v) for k, v in runs.items()}, "reps": a.reps,
           "entries": "[median, min, max] over the repetitions"}
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
