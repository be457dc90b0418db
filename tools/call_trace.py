#!/usr/bin/env python3
"""Trace of every C-ABI call of two eager training steps and one eval predict (B = 6, 64 x 64, fixed seed), for comparing the
host launch layer of two trees:

    python tools/call_trace.py OUT_PREFIX [--root OTHER_TREE]

OUT_PREFIX.trace: one line per _Lib.call — the entry name, every non-pointer argument by value, "P" / "0" for a non-null / null
pointer, the stream as "s<index of first appearance>".  Two trees issue the same launches iff these files are identical.
OUT_PREFIX.ptrs: the same lines with pointers as first-appearance indices (information only: allocation order may differ).
OUT_PREFIX.sha: SHA-256 of every network's flat_params() after the two steps, and of the prediction.
The WTPSE_* switches are read at import: run each configuration in a fresh process."""
import argparse
import ctypes
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
a = ap.parse_args()
ROOT = os.path.abspath(a.root)
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

import torch  # noqa: E402
import algorithms  # noqa: E402
import shape_networks  # noqa: E402
from wtpse_hip import lib as wlib  # noqa: E402
from wtpse_hip.step import TrainStep  # noqa: E402
from wtpse_hip.synth import make_batch, default_hparams  # noqa: E402

dev = torch.device("cuda:0")
torch.cuda.set_device(0)
L = wlib.lib()
trace, ptrs = open(a.out + ".trace", "w"), open(a.out + ".ptrs", "w")
streams, seen = {}, {}
orig_call = wlib._Lib.call


def traced_call(self, name, *args):
    types = self.protos[name]
    has_stream = name in self._plan_fn            # the recordable entry points: their last argument is the stream
    t, p = [name], [name]
    for k, (ty, v) in enumerate(zip(types, args)):
        if ty is not ctypes.c_void_p:
            t.append(repr(v)); p.append(repr(v))
        elif has_stream and k == len(types) - 1:
            s = "s%d" % streams.setdefault(v, len(streams))
            t.append(s); p.append(s)
        else:
            t.append("P" if v else "0")
            p.append("p%d" % seen.setdefault(v, len(seen)) if v else "0")
    assert len(args) == len(types), name
    trace.write(" ".join(t) + "\n"); ptrs.write(" ".join(p) + "\n")
    return orig_call(self, name, *args)


wlib._Lib.call = traced_call


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


hp = default_hparams(True)
B, H = 6, 64
torch.manual_seed(1)
mk = lambda ts: algorithms.WT_PSE(3, 1, hp, dev, ts, per_domain_batch=B // 3, source_domain_num=3).to(dev)
mks = lambda: shape_networks.ShapeVariationalDist_x(hp, dev, n_classes=1, number_source_domain=3, batch_size=B // 3).to(dev)
model_od, model_oc = mk(False), mk(True)
shape_od, shape_oc = mks(), mks()
ts = TrainStep(model_od, shape_od, model_oc, shape_oc, hp, dp=None, graph=False)
image, od, oc = make_batch(B, H, H, dev, seed=1)
for _ in range(2):
    ts.step(image, od, oc)
torch.cuda.synchronize()
with open(a.out + ".sha", "w") as f:
    for name, n in (("model_od", model_od), ("shape_od", shape_od), ("model_oc", model_oc), ("shape_oc", shape_oc)):
        f.write("%s %s\n" % (name, sha(n.flat_params())))
    trace.write("# predict\n"); ptrs.write("# predict\n")
    model_od.eval()
    shape_od.eval()
    with torch.no_grad():
        pred = model_od.predict(shape_od, image)[0]
    torch.cuda.synchronize()
    f.write("predict %s\n" % sha(pred))
trace.close(); ptrs.close()
print("call_trace: %d streams, %d pointers -> %s.{trace,ptrs,sha}" % (len(streams), len(seen), a.out))
