"""The input stages' protocol (`input_pipeline.stages`) and the property it exists for: a stage's random stream does not move when
another stage is added or switched on behind it.  Nothing here needs a GPU: the feed runs against a recording pipeline.
tests/golden/input_stage_draws.npz (tools/make_golden_stage_draws.py) was recorded before the stages were given one protocol."""
import importlib.util
import inspect
import os
import random

import numpy as np
import pytest

from wtpse_hip import input_pipeline as P
from wtpse_hip.input_pipeline import stages
from wtpse_hip.input_pipeline.stages import DRAW_ORDER, RUN_ORDER
from wtpse_hip.trainer import FundusBatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_stage_draws", os.path.join(ROOT, "tools", "make_golden_stage_draws.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

FEED_KW = ["style", "quality", "clahe", "appearance", "jpeg"]                              # in draw order
PIPE_KW = ["mix_draws", "quality_draws", "clahe", "appearance_draws", "jpeg_draws"]

# every name anything in the repository imported from the one-file module, and every public name it had
NAMES = """APPEARANCE_BIAS_MAX APPEARANCE_BLEND APPEARANCE_B_OFF APPEARANCE_CHANNELS APPEARANCE_CL APPEARANCE_COLS APPEARANCE_LAYERS
APPEARANCE_MAX_SIZE APPEARANCE_NET_COLS APPEARANCE_R_MAX APPEARANCE_SELECTED APPEARANCE_SPACING APPEARANCE_W_MAX APPEARANCE_W_OFF
AmplitudeMix AppearanceNets Augment CLAHE_MAX_SIDE CLAHE_MAX_TILES CLAHE_MODES Clahe DeviceInputPipeline ImageQuality JPEG_IDCT_WINDOW
JPEG_MAX_SIZE JpegCompression MIX_SIZES PRECISION_BITS QUALITY_A QUALITY_BETA QUALITY_C QUALITY_COLS QUALITY_K QUALITY_MAX_SIZE
QUALITY_RADIUS amplitude_mix_host appearance_axis_table appearance_field_host appearance_gain appearance_grid appearance_host
appearance_is_neutral appearance_layer_host appearance_net_of appearance_net_row appearance_neutral augment_host
check_appearance_params check_jpeg_params check_quality_params clahe_axis_table clahe_bounds clahe_device_tables clahe_host clahe_lut
clahe_luts_host clahe_record clahe_redistribute device_uniform draw draw_appearance draw_augment draw_jpeg draw_mix draw_quality
elastic_displacement gamma_table gaussian_weights jpeg_host jpeg_is_neutral jpeg_neutral jpeg_reciprocals jpeg_tables nearest_table
parse_clahe quality_host quality_is_neutral quality_neutral quality_noise_host quality_positions quality_taps resample_table
twiddle_table _dev_i32 _check_mix_size _check_jpeg_size _check_appearance_size""".split()


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return tool.make_sets(str(tmp_path_factory.mktemp("stages") / "tree"))


def run_feed(sets, on, augment=True, batches=1):
    """The feed with the stages `on` (feed keywords), generators seeded 11 -> (the recorded calls, py_rng, np_rng)."""
    configs = {k: v for k, v in tool.stage_configs().items() if k in on}
    pipe = tool.RecordingPipe()
    feed = FundusBatches(sets, 6, "cpu", size=64, augment=P.Augment() if augment else None, pipe=pipe, **configs)
    py_rng, np_rng = random.Random(11), np.random.RandomState(11)
    for _ in range(batches):
        feed(py_rng, np_rng)
    return pipe.calls, py_rng, np_rng


def same(a, b):
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


def same_aug(a, b):
    fa, fb = tool.flatten_aug(a), tool.flatten_aug(b)
    return all(np.array_equal(fa[k], fb[k]) for k in fa)


def same_state(x, y):
    return same(list(x.get_state()), list(y.get_state()))


# ---------------------------------------------------------------------------------------------------------------- the tuples
def test_tuples_and_signatures():
    assert len(RUN_ORDER) == 5 and len(set(map(id, RUN_ORDER))) == 5 and set(map(id, RUN_ORDER)) == set(map(id, DRAW_ORDER))
    assert [s.feed_kw for s in RUN_ORDER] == ["style", "appearance", "quality", "jpeg", "clahe"]
    assert [s.feed_kw for s in DRAW_ORDER] == FEED_KW and [s.pipe_kw for s in DRAW_ORDER] == PIPE_KW
    assert [s.config for s in DRAW_ORDER] == [P.AmplitudeMix, P.ImageQuality, P.Clahe, P.AppearanceNets, P.JpegCompression]
    feed = list(inspect.signature(FundusBatches.__init__).parameters)
    assert feed == ["self", "datasets", "batch_size", "device", "size", "augment", "pipe", "style", "quality", "clahe", "appearance", "jpeg"]
    assert sorted(feed[7:]) == sorted(FEED_KW)
    call = inspect.signature(P.DeviceInputPipeline.__call__).parameters
    assert list(call) == ["self", "images", "disc_masks", "draws", "aug_draws", "noise", "mix_draws", "quality_draws", "clahe",
                          "appearance_draws", "jpeg_draws"]
    assert sorted(list(call)[6:]) == sorted(PIPE_KW) and all(call[k].default is None for k in list(call)[4:])


def test_every_name_resolves():
    missing = [n for n in NAMES if not hasattr(P, n)]
    assert not missing, missing
    assert P.stages is stages and P.RUN_ORDER is RUN_ORDER and P.DRAW_ORDER is DRAW_ORDER


# ---------------------------------------------------------------------------------------------------------------- the feed
def test_keywords(sets):
    for augment in (False, True):
        calls, _, _ = run_feed(sets, FEED_KW, augment)
        _, args, kw = calls[0]
        assert list(kw) == PIPE_KW and len(args) == int(augment)
        calls, _, _ = run_feed(sets, (), augment)
        assert calls[0][2] == {} and len(calls[0][1]) == int(augment)


def test_draw_order(sets):
    """The stages draw mix, quality, appearance, JPEG behind everything else of the batch: a twin generator advanced by the feed with
    no stage on, then by the four draw functions by hand, makes the recorded values and ends in the same state."""
    calls, py_a, np_a = run_feed(sets, FEED_KW)
    plain, py_b, np_b = run_feed(sets, ())
    assert py_a.getstate() == py_b.getstate() and same(calls[0][0], plain[0][0]) and same_aug(calls[0][1][0], plain[0][1][0])
    c = tool.stage_configs()
    kw = calls[0][2]
    assert same(kw["mix_draws"], P.draw_mix(np_b, 3, 2, c["style"]) + (c["style"].band(64),))
    assert same(kw["quality_draws"], P.draw_quality(np_b, 6, c["quality"]))
    assert same(kw["appearance_draws"], P.draw_appearance(np_b, 6, 64, c["appearance"]) + (16,))
    assert same(kw["jpeg_draws"], P.draw_jpeg(np_b, 6, c["jpeg"]))
    assert kw["clahe"] is not None and kw["clahe"] == c["clahe"]
    assert same_state(np_a, np_b)


def test_stream_stability(sets):
    """Switching on a stage later in DRAW_ORDER leaves every earlier stage's value as it was — for each stage alone and for each
    prefix of DRAW_ORDER.  (One batch from one generator state: whatever draws more leaves the generator further on for the next.)"""
    def values(on):
        return run_feed(sets, on)[0]

    for i, first in enumerate(FEED_KW):
        for earlier in ([first], FEED_KW[:i + 1]):
            base = values(earlier)
            for later in FEED_KW[i + 1:]:
                more = values(earlier + [later])
                for (_, _, kw), (_, _, kw2) in zip(base, more):
                    assert list(kw2)[:len(kw)] == list(kw) and len(kw2) == len(kw) + 1
                    assert all(same(kw[k], kw2[k]) for k in kw), (earlier, later)


def test_golden(sets, golden_dir, tmp_path):
    """What the all-stages feed hands the pipeline over two batches, array for array, against the record made before the refactor."""
    want = np.load(os.path.join(golden_dir, "input_stage_draws.npz"))
    got = tool.record(str(tmp_path / "tree"))
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_check_size_and_check_refuse():
    c = tool.stage_configs()
    by = {s.feed_kw: s for s in RUN_ORDER}
    for kw, bad in (("style", 40), ("jpeg", 40), ("quality", 0), ("appearance", 0)):
        by[kw].check_size(64, c[kw])
        with pytest.raises(ValueError):
            by[kw].check_size(bad, c[kw])
    by["clahe"].check_size(4, c["clahe"])
    with pytest.raises(ValueError):
        by["clahe"].check_size(3, c["clahe"])                       # tiles (4, 4)
    # one bad table per stage: `check` raises what the stage's own check function raises
    N, S = 2, 32
    q = P.quality_neutral(N)
    q[0, 0] = 600
    a, f = P.appearance_neutral(N, S, 8)
    a[1, 1] = 257
    m, t = P.jpeg_neutral(N)
    m[0], t[0, 0, 0] = 1, 256
    cases = [("style", ([5, -1], [0.5, 0.5], 4), lambda: P.check_mix_params([5, -1], [0.5, 0.5], 4, N, S)),
             ("quality", q, lambda: P.check_quality_params(q, N)),
             ("appearance", (a, f, 8), lambda: P.check_appearance_params(a, f, N, S, 8)),
             ("jpeg", (m, t), lambda: P.check_jpeg_params(m, t, N)),
             ("clahe", "luma", lambda: P.check_clahe("luma", S, S))]
    for kw, bad, direct in cases:
        with pytest.raises(ValueError) as direct_error:
            direct()
        with pytest.raises(ValueError) as e:
            by[kw].check(bad, N, S)
        assert str(e.value) == str(direct_error.value), kw
    # and good ones pass, idle or not
    good = {"style": ([1, -1], [0.5, 0.0], 4), "quality": P.quality_neutral(N), "appearance": P.appearance_neutral(N, S, 8) + (8,),
            "jpeg": P.jpeg_neutral(N), "clahe": P.Clahe(tiles=(2, 2))}
    for kw, value in good.items():
        checked = by[kw].check(value, N, S)
        assert by[kw].idle(checked) == (kw in ("quality", "appearance", "jpeg")), kw
    assert by["style"].idle(by["style"].check(([-1, -1], [0.0, 0.0], 4), N, S))
    with pytest.raises(ValueError):
        FundusBatches([object(), object()], 2, "cpu", size=64, style=P.ImageQuality(), pipe=object())
    with pytest.raises(ValueError):
        FundusBatches([object()], 1, "cpu", size=64, quality=P.AmplitudeMix(), pipe=object())
