#!/usr/bin/env python3
"""What the training-run driver costs (wtpse_hip/trainer.py; numbers in profiles/trainer_driver.md).

    python tools/bench_trainer.py                 ms/step of TrainStep(graph="plan") with and without a LossLog, alternating
    python tools/bench_trainer.py --freeze-bn     ms/step of TrainStep(graph="plan") on batch statistics and on frozen ones (freeze_bn=True), alternating
    python tools/bench_trainer.py --end-to-end    images/s of TrainRun.train_epoch() fed from a synthetic PNG tree, beside the bare step
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_trainer.py --adam-only [--tree PARENT_CHECKOUT]
                                                  Adam launches alone, for the per-call time of the kernel in a trace of its own

Time is taken with device events around the replayed steps; nothing synchronises inside a timed block.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--steps", type=int, default=200, help="replayed steps per timed block")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3, help="timed blocks per variant, alternating")
ap.add_argument("--end-to-end", action="store_true")
ap.add_argument("--epochs", type=int, default=3)
ap.add_argument("--iters", type=int, default=40, help="iterations per epoch of the end-to-end run")
ap.add_argument("--adam-only", action="store_true")
ap.add_argument("--freeze-bn", action="store_true", help="the step on frozen BatchNorm statistics beside the train-mode step")
ap.add_argument("--tree", default=None, help="import the package from this checkout (e.g. an export of the parent commit)")
args = ap.parse_args()

ROOT = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

import torch  # noqa: E402

import bench  # noqa: E402
from wtpse_hip import ops  # noqa: E402
from wtpse_hip.step import TrainStep  # noqa: E402
from wtpse_hip.synth import default_hparams, make_batch  # noqa: E402

DEV = torch.device("cuda:0")
HP = default_hparams(True)


def timed(fn, steps):
    """ms per call of fn over `steps` calls, between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def spread(v):
    return {"runs": [round(x, 4) for x in v], "median": round(sorted(v)[len(v) // 2], 4), "spread": round(max(v) - min(v), 4)}


def step_with_and_without_log():
    from wtpse_hip.trainer import LossLog
    B = args.batch
    batch = make_batch(B, args.size, args.size, DEV, seed=1)
    variants = {}
    for name in ("plain", "logged"):
        nets = bench.build_nets(HP, B // 3, DEV)
        log = LossLog(DEV, TrainStep.log_names(HP)) if name == "logged" else None
        ts = TrainStep(*nets, HP, graph="plan", log=log)
        for _ in range(args.warmup):
            ts.step(*batch)
        torch.cuda.synchronize()
        variants[name] = ts
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, ts in variants.items():
            ms[name].append(timed(lambda: ts.step(*batch), args.steps))
    sums, flag = variants["logged"].log.read()
    out = {"what": "TrainStep(graph='plan') ms/step, B=%d %dx%d, %d steps per block" % (B, args.size, args.size, args.steps),
           "plain": spread(ms["plain"]), "logged": spread(ms["logged"]), "nan_flag": flag[0],
           "images_per_s": {k: round(1e3 * B / sorted(v)[len(v) // 2], 2) for k, v in ms.items()}}
    print(json.dumps(out))


def step_frozen_and_train():
    B = args.batch
    batch = make_batch(B, args.size, args.size, DEV, seed=1)
    variants = {}
    for name in ("train", "frozen"):
        nets = bench.build_nets(HP, B // 3, DEV)
        ts = TrainStep(*nets, HP, graph="plan", freeze_bn=name == "frozen")
        for _ in range(args.warmup):
            ts.step(*batch)
        torch.cuda.synchronize()
        variants[name] = ts
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, ts in variants.items():
            ms[name].append(timed(lambda: ts.step(*batch), args.steps))
    out = {"what": "TrainStep(graph='plan') ms/step, B=%d %dx%d, %d steps per block" % (B, args.size, args.size, args.steps),
           "train": spread(ms["train"]), "frozen": spread(ms["frozen"]),
           "images_per_s": {k: round(1e3 * B / sorted(v)[len(v) // 2], 2) for k, v in ms.items()}}
    print(json.dumps(out))


def end_to_end():
    from oracle.fundus_tree import make_tree
    from wtpse_hip.fundus_data import FundusTree
    from wtpse_hip.trainer import FundusBatches, TrainRun
    B = args.batch
    with tempfile.TemporaryDirectory() as root:          # the samples are decoded into memory once (fundus_dataloader.py:180-199)
        make_tree(root, seed=5)
        sets = [FundusTree(root, "train", (i,)) for i in (1, 2, 3)]
        for ds in sets:
            for imgs, masks, _ in ds.pools.values():
                for im in imgs + masks:
                    im.load()
    feed = FundusBatches(sets, B, DEV, args.size)
    n = feed.per_domain * 3                            # images per step (30 for batch 32: Trainer.py:1011)
    nets = bench.build_nets(HP, feed.per_domain, DEV)
    run = TrainRun(*nets, HP, feed, iter_per_epoch=args.iters, max_epoch=args.epochs + 1, graph="plan", seed=1)
    run.train_epoch()                                  # records the step
    fed = []
    for _ in range(args.epochs):
        t0 = time.perf_counter()
        run.train_epoch()                              # ends with the one read of the loss log: the epoch is complete
        fed.append(n * args.iters / (time.perf_counter() - t0))
    # the bare step on one of those batches, same networks and recording, same images per step
    batch = feed(run.py_rng, run.np_rng)
    torch.cuda.synchronize()
    bare = [1e3 * n / timed(lambda: run.train_step.step(*batch), args.iters) for _ in range(args.epochs)]
    # the input side alone
    t0 = time.perf_counter()
    for _ in range(args.iters):
        feed(run.py_rng, run.np_rng)
    torch.cuda.synchronize()
    feed_ms = 1e3 * (time.perf_counter() - t0) / args.iters
    out = {"what": "TrainRun.train_epoch() from a synthetic PNG tree, %d images per step, %d iterations per epoch" % (n, args.iters),
           "fed_images_per_s": spread(fed), "bare_step_images_per_s": spread(bare), "input_side_ms_per_batch": round(feed_ms, 3)}
    print(json.dumps(out))


def adam_only():
    n = sum(p.numel() for p in bench.build_nets(HP, 2, DEV)[0].parameters())
    p, g = torch.randn(n, device=DEV), torch.randn(n, device=DEV) * 0.01
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    t_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    lr_dev = torch.full((1,), 5e-4, device=DEV)
    hold = torch.zeros(1, dtype=torch.int32, device=DEV)
    dev_entry = "wtpse_adam_dev" in ops.lib().protos
    for _ in range(args.steps):
        if dev_entry:
            ops.adam_step_dev(p, g, m, v, lr_dev, 0.9, 0.99, 1e-8, 1, t_dev, hold)
        else:
            ops.adam_step(p, g, m, v, 5e-4, 0.9, 0.99, 1e-8, 1, t_dev)
    torch.cuda.synchronize()
    print(json.dumps({"what": "%d Adam launches over %d parameters" % (args.steps, n),
                      "entry": "wtpse_adam_dev" if dev_entry else "wtpse_adam", "bytes_per_launch": 28 * n}))


if __name__ == "__main__":
    if args.adam_only:
        adam_only()
    elif args.freeze_bn:
        step_frozen_and_train()
    elif args.end_to_end:
        end_to_end()
    else:
        step_with_and_without_log()
