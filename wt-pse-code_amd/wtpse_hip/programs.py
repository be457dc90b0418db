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
    add_clahe_argument(ap)


CLAHE_HELP = ("CLAHE preprocessing in front of the networks (contrast-limited adaptive histogram equalisation on the device; the "
              "project's own integer definition, not byte-equal to OpenCV; effect on held-out Dice / HD95 unmeasured): 'checkpoint' "
              "(default) applies what the checkpoint records under \"clahe\", or nothing if it records nothing (the stage is off by default); "
              "'off'; or "
              "CLIP[:TY,TX[:FLOOR[:MODE]]], e.g. 2.0:8,8:0:luma")


def add_clahe_argument(ap):
    """--clahe on a program's parser (segment, locate, adapt, test_run, calibration_run, morphometry_run)."""
    ap.add_argument("--clahe", default="checkpoint", help=CLAHE_HELP.replace("%", "%%"))


def resolve_clahe(ap, text, record):
    """The --clahe switch against the checkpoint's "clahe" entry (a `Clahe.record()` or None) -> the Clahe to apply, or None.  One
    line is printed when the switch overrides what the checkpoint records; a malformed switch ends the program through ap.error."""
    from .input_pipeline import Clahe, parse_clahe
    try:
        want = parse_clahe(text)
        recorded = None if record is None else Clahe.from_record(record)
    except ValueError as e:
        ap.error(str(e))
    if want == "checkpoint":
        return recorded
    if want != recorded:
        print("--clahe %s overrides the checkpoint's record (%s)" % (text, "none" if recorded is None else repr(recorded)))
    return want


def require_gpu(program):
    if not torch.cuda.is_available():
        raise SystemExit("wtpse_hip.%s needs the GPU: the networks have no CPU path" % program)


def load_networks(checkpoint, want_clahe=False):
    """-> (the four networks on device 0 with the checkpoint loaded, the device); with want_clahe also the checkpoint's "clahe" entry
    (a `Clahe.record()`, or None when it has none)."""
    from .test_run import build_networks, load_checkpoint
    device = "cuda:0"
    torch.cuda.set_device(0)
    nets = build_networks(device)
    ckpt = load_checkpoint(checkpoint, *nets)
    return (nets, device, ckpt.get("clahe")) if want_clahe else (nets, device)


def open_test_split(program, args, ap=None):
    """A test-split program's start: the GPU check, the networks from args.checkpoint, the split of args.data_dir / args.datasetTest
    -> (nets, FundusTestBatches of args.batch_size — labelled_split.ClaheTestBatches when args.clahe and the checkpoint's "clahe" entry
    name a preprocessing: `resolve_clahe`);
    ends the program when there is no GPU or no test image."""
    from .fundus_data import FundusTree
    from .test_run import FundusTestBatches
    require_gpu(program)
    nets, device, record = load_networks(args.checkpoint, want_clahe=True)
    if ap is None:
        import argparse
        ap = argparse.ArgumentParser(prog="python -m wtpse_hip." + program)
    clahe = resolve_clahe(ap, getattr(args, "clahe", "checkpoint"), record)
    tree = FundusTree(args.data_dir, phase="test", splitid=(args.datasetTest,), state="prediction")
    if len(tree) < 1:
        raise SystemExit("no test images under %s" % os.path.join(args.data_dir, "Domain%d" % args.datasetTest, "test"))
    if clahe is None:
        return nets, FundusTestBatches(tree, args.batch_size, device)
    from .labelled_split import ClaheTestBatches
    return nets, ClaheTestBatches(tree, args.batch_size, device, clahe=clahe)


def test_run_parser(prog, doc):
    """The switches of `python -m wtpse_hip.test_run` (wtpse_hip.morphometry_run adds its own to them)."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m wtpse_hip." + prog, description=doc.split("\n\n")[0])
    add_split_arguments(ap)
    ap.add_argument("--batch-size", type=int, default=9)
    ap.add_argument("--overlay", choices=("device", "host"), default="device")
    ap.add_argument("--metrics", choices=("device", "host"), default="device")
    return ap
