#!/usr/bin/env python3
"""BUILD CONTAINER / any CPU box with the reference checked out (TEST INFRASTRUCTURE): the reference's OWN WT_PSE.predict under a
substituted latent -> tests/golden/uncertainty.npz, the fixture of tests/test_uncertainty_cpu.py and tests/test_uncertainty_gpu.py.

    python tools/make_golden_uncertainty.py          # seconds

The reference predicts with z = mu (algorithms.py:1334-1338) and never evaluates the student's logvar head there.  For every sample k
the student's `sample_forward` is temporarily replaced by one that returns mu + exp(logvar / 2) * eps_k — mu and logvar from the
student's own unet_extractor / mu_prior / logvar_prior, mu scrubbed as sample_forward scrubs it — and the reference's own
predict(...) is called: the stored logits are literally the reference's prediction under that latent.

Three cases at B = 2, 32 x 32, K = 4, scale = 1, eval mode, weights from oracle.filler, inputs and eps from oracle.inputs:
    0  two_step = False, cat_shape = False        1  two_step = True (a second image as the shape network's input)
    2  cat_shape = True
Stored per case (numbers only — no weights, no code): the flags and seeds, eps [B,K,H,W] fp32, the fp32 logits [B,K,H,W] and the same
from an fp64 evaluation.  At most 0.1 % of a case's stored logits may lie within 1e-3 of ln 3 (the 0.75 vote threshold); another
input seed is taken otherwise, so that a vote test has something to count.
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from oracle.filler import fill_state_dict  # noqa: E402
from oracle.inputs import make_inputs, make_noise  # noqa: E402

B, H, K = 2, 32, 4
SEED_W, SEED_IN, SEED_EPS = 1234, 3100, 3200
CASES = [(False, False), (True, False), (False, True)]          # (two_step, cat_shape)
LN3, NEAR, SHARE = math.log(3.0), 1e-3, 1e-3


def sampled_logits(alg, shp, hp, two_step, dtype, seed_in, eps):
    torch.set_default_dtype(dtype)
    try:
        main_net = alg.WT_PSE(n_channels=3, n_classes=1, hparams=hp, device="cpu", two_step=two_step, per_domain_batch=1,
                              source_domain_num=3)
        shape = shp.ShapeVariationalDist_x(hp, "cpu", n_classes=1, number_source_domain=3, batch_size=1)
        fill_state_dict(main_net, SEED_W + 50)
        fill_state_dict(shape, SEED_W + 53)
        main_net.to(dtype).eval()
        shape.to(dtype).eval()
        img = make_inputs(seed_in, B, H, H)[0].to(dtype)
        data = torch.stack((img, make_inputs(seed_in + 500, B, H, H)[0].to(dtype)), 0) if two_step else img
        out = []
        for k in range(K):
            def sample_forward(inputs, training, k=k):
                fmap = shape.unet_extractor(inputs)
                mu, logvar = shape.mu_prior(fmap), shape.logvar_prior(fmap)
                if torch.isnan(mu).any():
                    mu = torch.nan_to_num(mu)
                return mu + torch.exp(logvar / 2) * eps[:, k:k + 1].to(dtype)
            shape.sample_forward = sample_forward
            try:
                with torch.no_grad():
                    out.append(main_net.predict(shape, data)[0])
            finally:
                del shape.sample_forward
        return torch.cat(out, 1)
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", min(os.cpu_count() or 8, 16))))
    hreg, alg, shp = ref_import.load()
    out = {"meta": np.array([B, H, K, SEED_W + 50, SEED_W + 53], np.int64)}
    cases = []
    for ci, (two_step, cat_shape) in enumerate(CASES):
        hp = dict(hreg.default_hparams("WT_PSE", "fundus"), cat_shape=cat_shape)
        eps = make_noise(SEED_EPS + ci, (B, K, H, H))
        for attempt in range(20):
            seed_in = SEED_IN + ci + 10 * attempt
            l32 = sampled_logits(alg, shp, hp, two_step, torch.float32, seed_in, eps).numpy()
            l64 = sampled_logits(alg, shp, hp, two_step, torch.float64, seed_in, eps).numpy()
            share = float((np.abs(l64 - LN3) < NEAR).mean())
            print("case %d seed %d: logits in [%.3f, %.3f], share above ln 3 %.3f, within %g of it %.4f, fp32 from fp64 %.2e"
                  % (ci, seed_in, l64.min(), l64.max(), (l64 > LN3).mean(), NEAR, share, np.abs(l32 - l64).max()))
            if share <= SHARE:
                break
        assert share <= SHARE, "no input seed keeps the logits away from ln 3"
        assert l32.dtype == np.float32 and l64.dtype == np.float64 and l32.shape == (B, K, H, H)
        cases.append((int(two_step), int(cat_shape), seed_in, SEED_EPS + ci))
        out["c%d_eps" % ci] = eps.numpy()
        out["c%d_logits" % ci] = l32
        out["c%d_logits64" % ci] = l64
    out["cases"] = np.array(cases, np.int64)
    dst = os.path.join(ROOT, "tests", "golden", "uncertainty.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    if not ref_import.available():
        sys.exit("reference not present at %s — this fixture can only be generated where it is" % ref_import.REFERENCE_ROOT)
    main()
