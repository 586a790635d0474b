"""Measurements for the fused, augmenting train batch (DESIGN.md §10 item 8;
results under profiles/r19/train_batch_legs.jsonl).

    python tools/train_batch_ab.py --out DIR [--records 50000] [--rounds 3] [--only batch|phase]

The driver runs every leg as a fresh child process (this file with --leg)
under a time limit of its own and stops at the first leg that does not exit
with status 0; each leg prints one JSON line, collected in
DIR/train_batch_legs.jsonl.  The legs alternate (a b c d a b c d ...), so the
spread between the rounds of one leg is the noise the differences are read
against.  One GPU; the buffer is `records` packed records made from a seed
(rule-played positions, random sparse visit counts).

  batch   ms per batch at batch sizes 64, 256 and 1,024, event-pair timed
          over `--batches` batches after a warm-up, five windows per size:
            a  RecordSource.batch: index_select, unpack, hz_encode_states,
               pi_of (the per-batch path before hz_train_batch)
            b  train_batch, identity (sym NULL)
            c  train_batch, one random symmetry per item (the draw included)
            d  TensorSource.batch over the featurized buffer, with the
               one-off featurize time and the tensors' bytes beside it
  phase   one training_phase at the reference configuration (default
          network, Adam, batch 64, 2 epochs over the buffer) as
          Trainer.execute_training_phase builds it: symmetry absent
          (featurize + TensorSource), "random", "all" (four times the items).
          Wall seconds around a device synchronize, source construction
          included, after a warm-up phase over 4,096 records.

Whether augmented training learns faster is a strength question this tool
does not answer.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "harmonies-alphazero_amd")]

BATCH_SIZES = (64, 256, 1024)
WINDOWS = 5


def make_records(n, seed=20):
    """n packed records on cuda:0: positions of rule-played games (every ply
    of n / 50 boards over 50 plies), visit counts on a random third of the
    slots, z cycling through -1, 0, 1, the mover as the player byte."""
    import torch
    from hzamd import distributed as hd
    from hzamd.env import BatchedEnv
    plies = 50
    boards = (n + plies - 1) // plies
    env = BatchedEnv(boards, seed_base=seed, device="cuda:0")
    env.reset()
    states = []
    for _ in range(plies):
        states.append(env.export_state().t().contiguous())
        env.rule_ply()
    env.close()
    st = torch.cat(states)[:n]
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    visits = torch.randint(1, 400, (n, 143), generator=gen, device="cuda:0", dtype=torch.int32)
    visits[torch.rand(n, 143, generator=gen, device="cuda:0") < 0.67] = 0
    z = (torch.arange(n, device="cuda:0") % 3 - 1).to(torch.float32)
    player = (st[:, 5] >> 41) & 1
    return hd.pack_records(st, visits, z, player)


def time_batches(fn, perm, bs, batches):
    """ms per batch of fn(idx) over `batches` consecutive batches of one
    permutation, one event pair per window; WINDOWS windows after a warm-up."""
    import torch
    idxs = [perm[s:s + bs] for s in range(0, bs * batches, bs)]
    for i in idxs[:20]:
        fn(i)
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in idxs:
            fn(i)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / len(idxs))
    return out


def leg_batch(args):
    import torch
    from hzamd.train import RecordSource, featurize, train_batch
    rec = make_records(args.records)
    n = rec.shape[0]
    kind = args.leg.split("_")[1]
    extra = {}
    if kind == "a":
        src = RecordSource(rec)
        fn = src.batch
    elif kind == "b":
        def fn(i):
            return train_batch(rec, i)
    elif kind == "c":
        gen = torch.Generator(device="cuda:0").manual_seed(3)

        def fn(i):
            g = torch.randint(0, 4, (i.shape[0],), device="cuda:0", generator=gen, dtype=torch.uint8)
            return train_batch(rec, i, g)
    else:
        featurize(rec[:4096])  # warm-up
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        src = featurize(rec)
        torch.cuda.synchronize()
        extra = {"featurize_ms": (time.perf_counter() - t0) * 1e3,
                 "featurized_bytes": sum(t.numel() * t.element_size() for t in src.t),
                 "allocated_after_featurize_bytes": torch.cuda.memory_allocated() - m0,
                 "record_bytes": rec.numel() * 8}
        fn = src.batch
    res = {}
    for bs in BATCH_SIZES:
        batches = min(args.batches, n // bs)
        perm = torch.randperm(n, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(bs))
        ms = time_batches(fn, perm, bs, batches)
        res[str(bs)] = {"batches_per_window": batches, "ms_per_batch": ms, "min": min(ms), "median": sorted(ms)[len(ms) // 2]}
    return dict(extra, sizes=res)


def leg_phase(args):
    import torch
    from hzamd.manager import ModelManager
    from hzamd.net import DEFAULT
    from hzamd.train import SymRecordSource, featurize, training_phase
    torch.manual_seed(0)
    torch.backends.cudnn.benchmark = True
    mode = args.leg.split("_")[1]
    train_cfg = {"device": "cuda:0", "optimizer_type": "Adam", "learning_rate": 0.001, "weight_decay": 0.0001,
                 "value_loss_weight": 1.0, "policy_loss_weight": 1.0, "batch_size": 64, "momentum": 0.9,
                 "use_scheduler": True, "scheduler_type": "StepLR", "scheduler_step_size": 30,
                 "scheduler_gamma": 0.5, "force_lr_reset_on_load": False, "new_forced_lr": 0.000125}
    mgr = ModelManager(dict(DEFAULT, board_size=(5, 7)), train_cfg)
    rec = make_records(args.records)

    def phase(r, epochs):
        src = featurize(r) if mode == "none" else SymRecordSource(r, mode)
        return training_phase(mgr, src, epochs, 64)
    phase(rec[:4096], 1)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = phase(rec, 2)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return {"symmetry": mode, "seconds": el, "batches": res["batches"], "ms_per_batch": el / res["batches"] * 1e3,
            "loss": res["loss"]}


def child(args):
    out = leg_batch(args) if args.leg.startswith("batch") else leg_phase(args)
    out.update({"leg": args.leg, "records": args.records})
    print("LEG " + json.dumps(out), flush=True)


def driver(args):
    if not args.out:
        sys.exit("the driver needs --out DIR")
    os.makedirs(args.out, exist_ok=True)
    legs = []
    if args.only in (None, "batch"):
        for i in range(args.rounds):
            legs += [("batch_%s_%d" % (k, i), 150) for k in "abcd"]
    if args.only in (None, "phase"):
        for i in range(max(1, args.rounds - 1)):
            legs += [("phase_%s_%d" % (k, i), 300) for k in ("none", "random", "all")]
    with open(os.path.join(args.out, "train_batch_legs.jsonl"), "a") as log:
        for name, limit in legs:
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", name,
                   "--records", str(args.records), "--batches", str(args.batches)]
            r = subprocess.run(cmd, capture_output=True, text=True)
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
    ap.add_argument("--out", help="directory for train_batch_legs.jsonl (the driver needs it)")
    ap.add_argument("--records", type=int, default=50000)
    ap.add_argument("--batches", type=int, default=400, help="batches per timed window (capped by the buffer)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["batch", "phase"])
    ap.add_argument("--leg")
    a = ap.parse_args()
    child(a) if a.leg else driver(a)
