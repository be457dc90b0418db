"""All five input stages at once on the device: the pipeline's output is the chain of `ops` calls in the run order, the entry points
it launches are those the one-file pipeline launched (the literal lists below were recorded from it, not from the code under test),
and a feed with every stage on resumes bit for bit."""
import random

import numpy as np
import pytest
import torch

from test_quality_gpu import _inputs, normalised, to_u8
from wtpse_hip import ops
from wtpse_hip.input_pipeline import (AmplitudeMix, AppearanceNets, Augment, Clahe, DeviceInputPipeline, ImageQuality, JpegCompression,
                                      appearance_neutral, draw, draw_appearance, draw_augment, draw_jpeg, draw_mix, draw_quality,
                                      jpeg_neutral, quality_neutral, quality_positions)

pytestmark = pytest.mark.gpu

S, N = 32, 4


def pipeline_args():
    """-> (images, masks, draws, aug_draws) of the N samples: sizes differ, every augmentation enabled."""
    imgs, masks = _inputs(S, N)
    draws = [draw(random.Random(i), S) for i in range(N)]
    aug_draws = [draw_augment(random.Random(20 + i), np.random.RandomState(20 + i), S, Augment()) for i in range(N)]
    return imgs, masks, draws, aug_draws


def stage_values(neutral=False):
    """The five stage keywords: forced, non-neutral draws (every coin fires), or the tables that leave every sample alone."""
    clahe = Clahe(tiles=(2, 2))
    if neutral:
        return {"mix_draws": (np.full(N, -1, np.int32), np.zeros(N), 3), "appearance_draws": appearance_neutral(N, S, 8) + (8,),
                "quality_draws": quality_neutral(N), "jpeg_draws": jpeg_neutral(N), "clahe": clahe}
    rng = np.random.RandomState(4)
    mix = AmplitudeMix(p=1)
    return {"mix_draws": draw_mix(rng, 2, N // 2, mix) + (mix.band(S),),
            "appearance_draws": draw_appearance(rng, N, S, AppearanceNets(p=1, spacing=8)) + (8,),
            "quality_draws": draw_quality(rng, N, ImageQuality(p_focus=1, p_contrast=1, p_brightness=1, p_noise=1)),
            "jpeg_draws": draw_jpeg(rng, N, JpegCompression(p=1, quality=(5, 60), p_420=0.5)),
            "clahe": clahe}


def recorded_calls(monkeypatch, **kw):
    """The names handed to `lib().call` during one call of a fresh pipeline."""
    args = pipeline_args()
    pipe = DeviceInputPipeline(S, "cuda", noise_seed=9)
    L, names = ops.lib(), []
    real = L.call
    with monkeypatch.context() as m:
        m.setattr(L, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
        pipe(*args, **kw)
    torch.cuda.synchronize()
    return names


def test_all_stages_equal_the_chain_in_run_order():
    args = pipeline_args()
    kw = stage_values()
    pipe = DeviceInputPipeline(S, "cuda", noise_seed=9)
    got = pipe(*args, **kw)
    before = DeviceInputPipeline(S, "cuda", noise_seed=9)(*args)
    x = torch.from_numpy(to_u8(before[0])).cuda()
    x = ops.amplitude_mix(x, *kw["mix_draws"])
    x = ops.appearance_nets(x, *kw["appearance_draws"])
    x, pos = ops.image_quality(x, kw["quality_draws"], 9, 0, want_pos=True)
    x = ops.jpeg_roundtrip(x, *kw["jpeg_draws"])
    x = ops.clahe(x, kw["clahe"])
    assert np.array_equal(got[0].cpu().numpy(), normalised(x.cpu().numpy()))
    assert not torch.equal(got[0], before[0])
    assert torch.equal(got[1], before[1]) and torch.equal(got[2], before[2])            # the masks are those of the augment-only run
    assert pipe.quality_pos == pos == quality_positions(kw["quality_draws"], S, 0)[1] == N * S * S


# recorded from the one-file pipeline (the commit before the stages were given one protocol), same inputs, same machine
CROP_AND_AUGMENT = ["wtpse_resample_u8"] * 14 + ["wtpse_aug_geometry", "wtpse_uniform_f64", "wtpse_aug_blur", "wtpse_aug_blur",
                                                   "wtpse_aug_warp", "wtpse_aug_photometric"]
ALL_ON = ["wtpse_amplitude_mix", "wtpse_appearance_nets", "wtpse_appearance_finish", "wtpse_quality_sums", "wtpse_quality_apply",
          "wtpse_jpeg_roundtrip", "wtpse_clahe_hist", "wtpse_clahe_lut", "wtpse_clahe_apply"]
NEUTRAL = ["wtpse_clahe_hist", "wtpse_clahe_lut", "wtpse_clahe_apply"]


def test_entry_point_sequence(monkeypatch):
    """Which entry points one call launches, in order: every stage on; every stage on and neutral (only CLAHE, which is never
    idle, launches); no stage keyword — not one launch added."""
    assert recorded_calls(monkeypatch, **stage_values()) == CROP_AND_AUGMENT + ALL_ON + ["wtpse_input_finish"]
    assert recorded_calls(monkeypatch, **stage_values(neutral=True)) == CROP_AND_AUGMENT + NEUTRAL + ["wtpse_input_finish"]
    assert recorded_calls(monkeypatch) == CROP_AND_AUGMENT + ["wtpse_input_finish"]


def test_feed_resumes_with_every_stage_on(tmp_path):
    from oracle.fundus_tree import make_tree
    from wtpse_hip.fundus_data import FundusTree
    from wtpse_hip.trainer import FundusBatches
    root = str(tmp_path / "tree")
    make_tree(root, seed=5)
    sets = [FundusTree(root, "train", (i,), size=64) for i in (1, 2, 3)]

    def feed():
        f = FundusBatches(sets, 6, "cuda", size=64, augment=Augment(), style=AmplitudeMix(p=1), quality=ImageQuality(p_noise=1),
                          clahe=Clahe(tiles=(4, 4)), appearance=AppearanceNets(p=1, spacing=16), jpeg=JpegCompression(p=1))
        f.set_seed(7)
        return f

    a, py_a, np_a = feed(), random.Random(3), np.random.RandomState(3)
    a(py_a, np_a)
    a(py_a, np_a)
    saved = (a.state(), py_a.getstate(), np_a.get_state())
    assert set(saved[0]) == {"order", "noise_pos", "quality_pos"} and saved[0]["quality_pos"] > 0
    third = a(py_a, np_a)
    b, py_b, np_b = feed(), random.Random(0), np.random.RandomState(0)
    b.load_state(saved[0])
    py_b.setstate(saved[1])
    np_b.set_state(saved[2])
    again = b(py_b, np_b)
    assert all(torch.equal(x, y) for x, y in zip(again, third))
    assert b.state() == a.state()
