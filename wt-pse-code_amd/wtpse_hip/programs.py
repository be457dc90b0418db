"""What the run programs' command lines share: the switches of a labelled test split, the GPU check, the networks from a checkpoint,
the split's batches — with each program's own name in `prog=` and in the exit texts.  (test_run.py is imported where it is used:
it imports this module for its own command line.)"""
import os

import torch


def add_split_arguments(ap):
    """The four switches every program over a labelled test split takes."""
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--datasetTest", type=int, required=True, help="the target domain: Domain<N>/test is read")
    ap.add_argument("--checkpoint", required=True, help="checkpoint_<epoch>.pth.tar as validate.Validator saves it")
    ap.add_argument("--out", required=True)


def require_gpu(program):
    if not torch.cuda.is_available():
        raise SystemExit("wtpse_hip.%s needs the GPU: the networks have no CPU path" % program)


def load_networks(checkpoint):
    """-> (the four networks on device 0 with the checkpoint loaded, the device)."""
    from .test_run import build_networks, load_checkpoint
    device = "cuda:0"
    torch.cuda.set_device(0)
    nets = build_networks(device)
    load_checkpoint(checkpoint, *nets)
    return nets, device


def open_test_split(program, args):
    """A test-split program's start: the GPU check, the networks from args.checkpoint, the split of args.data_dir / args.datasetTest
    -> (nets, FundusTestBatches of args.batch_size); ends the program when there is no GPU or no test image."""
    from .fundus_data import FundusTree
    from .test_run import FundusTestBatches
    require_gpu(program)
    nets, device = load_networks(args.checkpoint)
    tree = FundusTree(args.data_dir, phase="test", splitid=(args.datasetTest,), state="prediction")
    if len(tree) < 1:
        raise SystemExit("no test images under %s" % os.path.join(args.data_dir, "Domain%d" % args.datasetTest, "test"))
    return nets, FundusTestBatches(tree, args.batch_size, device)


def test_run_parser(prog, doc):
    """The switches of `python -m wtpse_hip.test_run` (wtpse_hip.morphometry_run adds its own to them)."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m wtpse_hip." + prog, description=doc.split("\n\n")[0])
    add_split_arguments(ap)
    ap.add_argument("--batch-size", type=int, default=9)
    ap.add_argument("--overlay", choices=("device", "host"), default="device")
    ap.add_argument("--metrics", choices=("device", "host"), default="device")
    return ap
