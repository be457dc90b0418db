#!/usr/bin/env python3
"""BUILD CONTAINER / any CPU box with the reference checked out (TEST INFRASTRUCTURE): the reference's OWN modules in .eval() through
update() and backward() -> tests/golden/frozen_bn.npz, the fixture of tests/test_frozen_bn_gpu.py and tests/test_frozen_bn_cpu.py.

    python tools/make_golden_frozen.py          # about a minute on 8 cores

The reference's update() samples as in training whatever the module mode is (algorithms.py:1238, shape_networks.py:524-526), so
.eval() changes BatchNorm alone: every BatchNorm normalises with its running statistics, no buffer moves, and the bias of a
convolution in front of a BatchNorm — whose gradient batch statistics cancel exactly — receives one.

Two cases, B = 6 with 2 rows per domain at 64x64 and at 256x256; per case two calls on seeded inputs / weights / noise (oracle/inputs.py,
oracle/filler.py, ref_import.replay_noise), as oracle/make_golden.py and oracle/make_golden_grads.py make them:
    A  WT_PSE.update + BCE(sigmoid(out), od) + ins + dom          B  ShapeVariationalDist_x.update: kd + ins_total + dom
Stored per case (numbers and parameter names only — no reference code, no weights):
    the seeds; the fp32 logits of call A (whole at 64x64; every fourth row and column at 256x256, which keeps the file small) and
    its checksum; the fp32 loss scalars of both calls;
    per parameter tensor the oracle/sketch.py fingerprint of the fp64 gradient (kept as float32: 6e-8 relative, four orders below the
    5e-4 floor of the band it is used in) and the squared distances of three fp32 evaluations from it — the inputs as given and
    perturbed by 1e-6 and 3e-6, the yardstick of tests/golden/grads_b32.npz;
    a checksum of every buffer after both calls (= before them: the test also compares against the filler's values).
"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import, sketch  # noqa: E402
from oracle.filler import fill_state_dict  # noqa: E402
from oracle.inputs import make_inputs, make_noise  # noqa: E402
from oracle.wtpse_cpu import checksum  # noqa: E402

CASES = [(6, 2, 64), (6, 2, 256)]
SEED_W = 1234
SEED_IN, SEED_A, SEED_T, SEED_S = 2600, 2700, 2800, 2900
SKETCH_SEED = 9000


def perturbed(image, probes):           # = tests/test_parity_gpu.perturbed
    gen = torch.Generator().manual_seed(77)
    for i in range(probes):
        yield image * (1 + (1e-6, 3e-6, 1e-5)[i % 3] * torch.randn(image.shape, generator=gen)).to(image.dtype)


def main():
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", min(os.cpu_count() or 8, 16))))
    hreg, alg, shp = ref_import.load()
    hp = hreg.default_hparams("WT_PSE", "fundus")
    out = {"cases": np.array([(B, pb, H, SEED_IN + ci, SEED_A + ci, SEED_T + ci, SEED_S + ci) for ci, (B, pb, H) in enumerate(CASES)],
                             dtype=np.float64),
           "meta": np.array([sketch.K, sketch.SMALL, SEED_W, SKETCH_SEED])}

    def evaluate(ci, dtype, image):
        """Both calls on fresh eval-mode reference modules in `dtype` -> (values, {call: {name: fp64 gradient}}, buffers)."""
        B, pb, H = CASES[ci]
        torch.set_default_dtype(dtype)           # (the reference creates its identity matrices and masks in the default dtype)
        try:
            main_net = alg.WT_PSE(n_channels=3, n_classes=1, hparams=hp, device="cpu", two_step=False, per_domain_batch=pb,
                                  source_domain_num=3)
            shape = shp.ShapeVariationalDist_x(hp, "cpu", n_classes=1, number_source_domain=3, batch_size=pb)
            fill_state_dict(main_net, SEED_W)
            fill_state_dict(shape, SEED_W + 3)
            main_net.to(dtype).eval()
            shape.to(dtype).eval()
            _, od, _ = make_inputs(SEED_IN + ci, B, H, H)
            image, od = image.to(dtype), od.to(dtype)
            noise = [make_noise(s + ci, (B, 1, H, H)).to(dtype) for s in (SEED_A, SEED_T, SEED_S)]
            with ref_import.replay_noise(noise[:1]):
                logits, _, _, ins, dom = main_net.update(image, od, two_stage_inputs=image, sp_mask=od, two_step=True)
            seg = F.binary_cross_entropy(torch.sigmoid(logits), od)
            (seg + ins + dom).backward()
            vals = {"logits": logits.detach(), "A_loss": torch.stack([seg.detach(), ins.detach(), dom.detach()])}
            grads = {"A": {n: p.grad.double().clone() for n, p in main_net.named_parameters() if p.grad is not None}}
            shape.zero_grad(); main_net.zero_grad()
            with ref_import.replay_noise(noise[1:]):
                kd, ins_t, ins_ij, ins_ii, dom_s = shape.update(main_net, image, od, two_stage_inputs=image, two_step=True)
            (kd + ins_t + dom_s).backward()
            vals["B_loss"] = torch.stack([v.detach() for v in (kd, ins_t, ins_ij, ins_ii, dom_s)])
            grads["B"] = {n: p.grad.double().clone() for n, p in shape.named_parameters() if p.grad is not None}
            bufs = {"A": {n: b.detach().clone() for n, b in main_net.named_buffers()},
                    "B": {n: b.detach().clone() for n, b in shape.named_buffers()}}
            assert not main_net.training and not shape.training
            # every parameter receives a gradient, but for the student's logvar head: its sample has no grad_fn (shape_networks.py:507-509)
            assert len(grads["A"]) == len(list(main_net.parameters()))
            assert sorted(n for n, p in shape.named_parameters() if p.grad is None) == \
                sorted(n for n, _ in shape.named_parameters() if n.startswith("logvar_prior."))
            return vals, grads, bufs
        finally:
            torch.set_default_dtype(torch.float32)

    for ci, (B, pb, H) in enumerate(CASES):
        img, _, _ = make_inputs(SEED_IN + ci, B, H, H)
        t0 = time.time()
        _, g64, _ = evaluate(ci, torch.float64, img)
        print("case %d fp64 %.0f s" % (ci, time.time() - t0), flush=True)
        names = {call: sorted(g64[call]) for call in "AB"}
        dist = {call: np.zeros((len(names[call]), 3)) for call in "AB"}
        for j, q in enumerate([img] + list(perturbed(img, 2))):
            t0 = time.time()
            vals, g32, bufs = evaluate(ci, torch.float32, q)
            for call in "AB":
                for i, k in enumerate(names[call]):
                    dist[call][i, j] = float((g32[call][k] - g64[call][k]).pow(2).sum())
            if j == 0:
                lg = vals["logits"].float()
                out["c%d_logits" % ci] = (lg if H <= 64 else lg[:, :, ::4, ::4]).numpy()
                out["c%d_logits_cs" % ci] = checksum(lg)
                out["c%d_A_loss" % ci] = vals["A_loss"].float().numpy()
                out["c%d_B_loss" % ci] = vals["B_loss"].float().numpy()
                for call in "AB":
                    bn = sorted(bufs[call])
                    out["c%d_%s_buf_names" % (ci, call)] = np.array(bn)
                    out["c%d_%s_buf_cs" % (ci, call)] = np.stack([checksum(bufs[call][n].float())[:2] for n in bn])     # (sum, sum |.|)
                    # no buffer moved: the values are still the filler's
                    ref = shp.ShapeVariationalDist_x(hp, "cpu", n_classes=1, number_source_domain=3, batch_size=pb) if call == "B" else \
                        alg.WT_PSE(n_channels=3, n_classes=1, hparams=hp, device="cpu", two_step=False, per_domain_batch=pb, source_domain_num=3)
                    fill_state_dict(ref, SEED_W + (3 if call == "B" else 0))
                    for n, b in ref.named_buffers():
                        assert torch.equal(b, bufs[call][n]), n
            print("case %d fp32 draw %d %.0f s" % (ci, j, time.time() - t0), flush=True)
        for call in "AB":
            out["c%d_%s_names" % (ci, call)] = np.array(names[call])
            out["c%d_%s_yard2" % (ci, call)] = dist[call]
            n2, small, proj = [], [], []
            for i, k in enumerate(names[call]):
                fp = sketch.fingerprint(g64[call][k], SKETCH_SEED + i)
                n2.append([fp["n"], fp["norm2"]])
                (small if fp["n"] <= sketch.SMALL else proj).append(fp["data"].astype(np.float32))
            out["c%d_%s_n2" % (ci, call)] = np.array(n2)
            out["c%d_%s_fp_small" % (ci, call)] = np.concatenate(small)       # tensors of at most sketch.SMALL elements, whole, in name order
            out["c%d_%s_fp_proj" % (ci, call)] = np.stack(proj)                # the others: sketch.K projections each, in name order
            tot = (dist[call].sum(0).max() / np.array(n2)[:, 1].sum()) ** 0.5
            worst = max((dist[call][i].max() / (n2[i][1] + 1e-60)) ** 0.5 for i in range(len(n2)))
            print("case %d call %s: %d tensors, fp32 from fp64: all gradients %.2e, worst tensor %.2e" % (ci, call, len(n2), tot, worst))
    dst = os.path.join(ROOT, "tests", "golden", "frozen_bn.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    if not ref_import.available():
        sys.exit("reference not present at %s — this fixture can only be generated where it is" % ref_import.REFERENCE_ROOT)
    main()
