"""The device's CLAHE preprocessing (csrc/clahe.hip) against `clahe_host`, the integer specification: every comparison is
np.array_equal, and the input buffer is checked to be unwritten.

Code paths by size.  The histogram pass gives a workgroup at most 4096 pixels of a tile (CL_CHUNK): a tile of up to 4096 pixels is
one workgroup's, a larger one is split over workgroups that meet in integer atomics — 64 x 64 with tiles (1, 1) is exactly 4096
(one workgroup), 64 x 65 is 4160 (two), and the 600 x 700 / 512 x 512 cases have tiles of 105 000 / 262 144 pixels (26 / 64
workgroups each).  The apply pass gives a workgroup at most 2048 groups of 4 pixels (CL_APPLY_GROUPS) of the rows that blend the same
two tile rows (a band: with tiles (1, 1) the whole picture): 128 x 64 with tiles (1, 1) is exactly 2048 groups (one workgroup), 129 x
64 is 2064 (two).  It moves 12 bytes at a time with dword accesses where the address is 4-byte aligned and the 12 bytes lie inside
the row, and with byte accesses elsewhere: rows of 159 bytes (W = 53) take both, and a width that is no multiple of 4 has a short
last group.  Nothing else depends on a size."""
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wt-pse-code_amd")]

from test_clahe_cpu import FIELD, field_fixture, smooth_pictures
from wtpse_hip import ops
from wtpse_hip.input_pipeline import Clahe, DeviceInputPipeline, clahe_host, clahe_luts_host, draw

pytestmark = pytest.mark.gpu


def check(img, clahe, what=""):
    """Device against specification, byte for byte, LUTs included; the input buffer is left as it was.  -> the device's bytes."""
    img = np.ascontiguousarray(img)
    dimg = torch.from_numpy(img.copy()).cuda()
    out, luts = ops.clahe(dimg, clahe, want_luts=True)
    assert out.data_ptr() != dimg.data_ptr() and out.shape == dimg.shape and out.dtype == torch.uint8
    got, want = out.cpu().numpy(), clahe_host(img, clahe)
    bad_luts = luts.cpu().numpy() != clahe_luts_host(img, clahe)
    assert not bad_luts.any(), "%s: %d LUT bytes differ, the first at %s" % (what, int(bad_luts.sum()), tuple(np.argwhere(bad_luts)[0]))
    bad = got != want
    if bad.any():
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        delta = got.astype(np.int16) - want.astype(np.int16)
        raise AssertionError("%s: %d bytes differ (per sample %s), the first at %s: device %d, specification %d; differences from %d to %d"
                             % (what, int(bad.sum()), bad.reshape(len(bad), -1).sum(1).tolist(), first, got[first], want[first],
                                delta.min(), delta.max()))
    assert np.array_equal(dimg.cpu().numpy(), img), "%s: the input was written" % what
    return got


# (N, H, W, tiles, mode): the issue's shapes, then one on either side of the histogram pass's 4096-pixel split and of the apply
# pass's 2048-group split
SHAPES = [(2, 64, 64, (8, 8), "luma"),          # tiles of 64 pixels: smaller than a workgroup
          (3, 37, 53, (3, 5), "rgb"),           # uneven tiles, odd 159-byte rows
          (1, 16, 16, (16, 16), "luma"),        # one-pixel tiles: limit = 1
          (1, 16, 16, (16, 16), "rgb"),
          (2, 40, 40, (1, 1), "luma"),          # no interpolation anywhere
          (1, 600, 700, (2, 2), "luma"),        # tiles of 105 000 pixels: split over workgroups and merged
          (1, 512, 512, (1, 1), "rgb"),         # one tile of 262 144 pixels
          (33, 16, 16, (2, 2), "luma"),         # batch indexing
          (2, 64, 64, (1, 1), "rgb"),           # 4096 pixels: the largest tile of one workgroup
          (2, 64, 65, (1, 1), "luma"),          # 4160 pixels: the smallest tile of two
          (1, 64, 65, (1, 1), "rgb"),
          (2, 37, 53, (3, 5), "luma"),
          (1, 128, 64, (1, 1), "luma"),         # 2048 groups of 4 pixels: the longest band of one workgroup of the apply pass
          (1, 129, 64, (1, 1), "luma"),         # 2064: the shortest band of two
          (2, 128, 64, (1, 1), "rgb"),
          (2, 129, 62, (1, 1), "rgb"),          # 2064 groups again, the last of a row short (62 = 15 * 4 + 2)
          (1, 70, 50, (16, 16), "luma")]        # sixteen bands of uneven heights


@pytest.mark.parametrize("N,H,W,tiles,mode", SHAPES)
def test_shapes(N, H, W, tiles, mode):
    img = smooth_pictures(100 + H + W + N, N, H, W)
    got = check(img, Clahe(2.0, tiles, 0, mode), what="%dx%dx%d %s %s" % (N, H, W, tiles, mode))
    assert not np.array_equal(got, img)


@pytest.mark.parametrize("mode", ["luma", "rgb"])
def test_field_mask(mode):
    img = field_fixture()
    got = check(img, Clahe(2.0, FIELD["tiles"], FIELD["floor"], mode), what="field %s" % mode)
    field = img[0].max(-1) >= FIELD["floor"]
    assert np.array_equal(got[0][~field], img[0][~field]) and not np.array_equal(got[0][field], img[0][field])


@pytest.mark.parametrize("mode", ["luma", "rgb"])
def test_constant_and_two_level_batches(mode):
    const = np.stack([np.full((40, 44, 3), v, np.uint8) for v in (0, 77, 255)])
    got = check(const, Clahe(2.0, (4, 4), 0, mode), what="constant %s" % mode)
    assert all(len(np.unique(g)) == 1 for g in got)
    two = (np.random.RandomState(2).randint(0, 2, (2, 40, 44, 1)) * 255).astype(np.uint8).repeat(3, -1)
    got = check(two, Clahe(2.0, (4, 4), 0, mode), what="0/255 %s" % mode)
    assert (got[two == 255] == 255).all()


@pytest.mark.parametrize("clip", [1.0, 256])
@pytest.mark.parametrize("mode", ["luma", "rgb"])
def test_clip_bounds(clip, mode):
    check(smooth_pictures(21, 2, 64, 64), Clahe(clip, (8, 8), 0, mode), what="clip %r %s" % (clip, mode))
    check(smooth_pictures(22, 2, 64, 64), Clahe(clip, (2, 3), 16, mode), what="clip %r %s floor" % (clip, mode))


def test_same_call_twice_and_an_offset_view():
    img = smooth_pictures(31, 3, 37, 53)
    dimg = torch.from_numpy(img).cuda()
    clahe = Clahe(3.0, (3, 5), 0, "luma")
    a, b = ops.clahe(dimg, clahe), ops.clahe(dimg, clahe)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
    # a contiguous view that starts off a dword (37 * 53 * 3 = 5883 bytes per sample): the byte accesses carry it
    view = dimg[1:]
    assert view.is_contiguous() and view.data_ptr() % 4 != 0
    assert np.array_equal(ops.clahe(view, clahe).cpu().numpy(), clahe_host(img[1:], clahe))
    assert np.array_equal(a.cpu().numpy()[1:], clahe_host(img[1:], clahe))


def test_refusals_on_the_device():
    dimg = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ops.clahe(dimg.to(torch.float32), Clahe())
    with pytest.raises(ValueError):
        ops.clahe(torch.zeros((1, 16, 32, 3), dtype=torch.uint8, device="cuda")[:, :, ::2], Clahe())
    with pytest.raises(ValueError):
        ops.clahe(torch.zeros((1, 4, 16, 3), dtype=torch.uint8, device="cuda"), Clahe(2.0, (8, 8)))       # ty > H
    with pytest.raises(ValueError):
        ops.clahe(torch.zeros((1, 2, 4097, 3), dtype=torch.uint8, device="cuda"), Clahe(2.0, (1, 1)))    # W = 4097
    with pytest.raises(ValueError):
        ops.clahe(dimg.cpu(), Clahe())
    with pytest.raises(ValueError):
        ops.clahe(dimg, dict(clip=2.0))
    with pytest.raises(ValueError):
        ops.clahe(dimg[..., :2].contiguous(), Clahe())


# ---------------------------------------------------------------------------------------------------------------- the fronts
def to_u8(image):
    """The inverse of the normalisation: the fronts hand out fp32 u / 127.5 - 1 for a byte u, so rint((v + 1) * 127.5) recovers u
    exactly (the fp32 error is below 1e-4 of a level).  [N,3,S,S] fp32 -> [N,S,S,3] uint8."""
    v = (image.cpu().numpy().astype(np.float64) + 1.0) * 127.5
    u = np.rint(v)
    assert np.abs(v - u).max() < 1e-4
    return np.ascontiguousarray(u.astype(np.uint8).transpose(0, 2, 3, 1))


def normalised(u8):
    out = u8.astype(np.float32)
    out /= 127.5
    out -= 1.0
    return out.transpose(0, 3, 1, 2)


def _inputs(S, N):
    sizes = [(S + 9, S + 4), (S, S), (2 * S - 3, S + 7), (S + 1, S + 12)][:N]
    imgs = [smooth_pictures(40 + i, 1, h, w)[0] for i, (h, w) in enumerate(sizes)]
    masks = [np.where(np.hypot(*(np.mgrid[0:h, 0:w] - np.array([h / 2, w / 2])[:, None, None])) < min(h, w) * 0.3, 0, 255).astype(np.uint8)
             for h, w in sizes]
    return imgs, masks


def test_pipeline():
    S, N = 32, 4
    imgs, masks = _inputs(S, N)
    draws = [draw(random.Random(i), S) for i in range(N)]
    pipe = DeviceInputPipeline(S, "cuda")
    plain = pipe(imgs, masks, draws)
    off = pipe(imgs, masks, draws, clahe=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, off))
    clahe = Clahe(2.0, (4, 4), 0, "luma")
    got = pipe(imgs, masks, draws, clahe=clahe)
    assert torch.equal(got[1], plain[1]) and torch.equal(got[2], plain[2])           # the masks are not touched
    assert np.array_equal(got[0].cpu().numpy(), normalised(clahe_host(to_u8(plain[0]), clahe)))
    assert not torch.equal(got[0], plain[0])
    with pytest.raises(ValueError):
        pipe(imgs, masks, draws, clahe="luma")


def test_pipeline_runs_behind_the_other_stages():
    """augment, quality, clahe: the batch with all three equals the batch with the first two pushed through the specification."""
    from wtpse_hip.input_pipeline import Augment, ImageQuality, draw_augment, draw_quality
    S, N = 32, 4
    imgs, masks = _inputs(S, N)
    py_rng, np_rng = random.Random(5), np.random.RandomState(5)
    draws = [draw(py_rng, S) for _ in range(N)]
    aug_draws = [draw_augment(py_rng, np_rng, S, Augment()) for _ in range(N)]
    params = draw_quality(np_rng, N, ImageQuality(p_focus=1, p_contrast=1, p_brightness=1, p_noise=1))
    clahe = Clahe(2.5, (3, 5), 10, "rgb")
    two = DeviceInputPipeline(S, "cuda", noise_seed=9)(imgs, masks, draws, aug_draws, quality_draws=params)
    three = DeviceInputPipeline(S, "cuda", noise_seed=9)(imgs, masks, draws, aug_draws, quality_draws=params, clahe=clahe)
    assert torch.equal(two[1], three[1]) and torch.equal(two[2], three[2])
    assert np.array_equal(three[0].cpu().numpy(), normalised(clahe_host(to_u8(two[0]), clahe)))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from oracle.fundus_tree import make_tree
    root = str(tmp_path_factory.mktemp("clahe_tree"))
    make_tree(root, seed=5)
    return root


def test_training_feed(tree):
    """FundusBatches(clahe=...) against the same feed without: the same draws, the pictures pushed through the specification; no
    feed state is added."""
    from wtpse_hip.fundus_data import FundusTree
    from wtpse_hip.trainer import FundusBatches
    sets = [FundusTree(tree, "train", (i,), size=64) for i in (1, 2, 3)]
    clahe = Clahe(2.0, (8, 8), 0, "luma")
    on, off = FundusBatches(sets, 6, "cuda", size=64, clahe=clahe), FundusBatches(sets, 6, "cuda", size=64)
    a, b = on(random.Random(3), np.random.RandomState(3)), off(random.Random(3), np.random.RandomState(3))
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert np.array_equal(a[0].cpu().numpy(), normalised(clahe_host(to_u8(b[0]), clahe)))
    assert on.state() == off.state() and on.clahe_record() == clahe.record() and off.clahe_record() is None
    with pytest.raises(ValueError):
        FundusBatches(sets, 6, "cuda", size=64, clahe="luma")


def test_labelled_test_split(tree):
    from wtpse_hip.fundus_data import FundusTree
    from wtpse_hip.labelled_split import ClaheTestBatches
    from wtpse_hip.test_run import FundusTestBatches
    t = FundusTree(tree, phase="test", splitid=(4,), state="prediction", size=64)
    clahe = Clahe(2.0, (4, 4), 0, "rgb")
    on, off = ClaheTestBatches(t, 1, "cuda", clahe=clahe), FundusTestBatches(t, 1, "cuda")     # (the tree's label sizes differ)
    assert len(on) == len(off) >= 1 and on.clahe_record() == clahe.record() and not hasattr(off, "clahe_record")
    with pytest.raises(ValueError):
        ClaheTestBatches(t, 1, "cuda")
    first = 0
    for (ia, oda, oca, na), (ib, odb, ocb, nb) in zip(on, off):
        assert na == nb and torch.equal(oda, odb) and torch.equal(oca, ocb)
        u8 = np.stack([np.array(off.images[i].resize((64, 64))) for i in range(first, first + len(na))])      # the resize on the host
        assert np.array_equal(ib.cpu().numpy(), normalised(u8))
        assert np.array_equal(ia.cpu().numpy(), normalised(clahe_host(u8, clahe)))
        first += len(na)
    assert first == len(off.images)
    assert [tuple(x.shape) for x in next(iter(on.triples()))] == [tuple(x.shape) for x in next(iter(off.triples()))]


def test_segmenter_front():
    from PIL import Image
    from wtpse_hip.segment import Segmenter
    S = 64
    images = [smooth_pictures(60 + i, 1, h, w)[0] for i, (h, w) in enumerate([(90, 70), (64, 64), (90, 70), (65, 131)])]
    clahe = Clahe(2.0, (8, 8), 24, "luma")
    plain = Segmenter(None, None, None, None, out_dir=None, size=S).front(images)
    got = Segmenter(None, None, None, None, out_dir=None, size=S, clahe=clahe).front(images)
    u8 = np.stack([np.array(Image.fromarray(im).resize((S, S), Image.LANCZOS)) for im in images])           # the resize on the host
    assert np.array_equal(plain.cpu().numpy(), normalised(u8))
    assert np.array_equal(got.cpu().numpy(), normalised(clahe_host(u8, clahe)))
    # a crop that is on the device already (locate's) takes the same path
    dev = [torch.from_numpy(im).cuda() for im in images]
    assert torch.equal(Segmenter(None, None, None, None, out_dir=None, size=S, clahe=clahe).front(dev), got)
    with pytest.raises(ValueError):
        Segmenter(None, None, None, None, out_dir=None, size=4, clahe=clahe)


def test_locator_front_is_the_segmenters():
    from wtpse_hip.locate import Locator
    clahe = Clahe(2.0, (4, 4))
    assert Locator(None, None, size=64, clahe=clahe)._front.clahe == clahe
    assert Locator(None, None, size=64)._front.clahe is None


def test_train_run_writes_the_entry(tree, tmp_path, capsys):
    """Two steps on the synthetic tree with the stage on: the run checkpoint carries "clahe", loads under weights_only, and the
    --clahe checkpoint path of the programs builds a Segmenter that applies it.  A validation feed that disagrees is refused."""
    import argparse

    import bench
    from wtpse_hip.fundus_data import FundusTree
    from wtpse_hip.programs import add_clahe_argument, load_networks, resolve_clahe
    from wtpse_hip.segment import Segmenter
    from wtpse_hip.synth import default_hparams
    from wtpse_hip.labelled_split import ClaheTestBatches
    from wtpse_hip.test_run import FundusTestBatches
    from wtpse_hip.trainer import FundusBatches, TrainRun
    from wtpse_hip.validate import Validator
    dev = torch.device("cuda:0")
    hp = default_hparams(True)
    torch.manual_seed(0)
    nets = list(bench.build_nets(hp, 3, dev, seed=1))          # (programs.load_networks builds per_domain_batch 3)
    for n in nets:
        n.seed_noise(1234)
    sets = [FundusTree(tree, "train", (i,), size=64) for i in (1, 2, 3)]
    clahe = Clahe(2.5, (4, 4), 0, "luma")
    test_tree = FundusTree(tree, phase="test", splitid=(4,), state="prediction", size=64)
    kw = dict(iter_per_epoch=2, max_epoch=1, graph=False, seed=3)
    with pytest.raises(ValueError, match="CLAHE"):
        TrainRun(*nets, hp, FundusBatches(sets, 9, dev, size=64, clahe=clahe), validator=Validator(metrics="device"),
                 val_batches=FundusTestBatches(test_tree, 1, dev).triples, **kw)
    with pytest.raises(ValueError, match="CLAHE"):
        TrainRun(*nets, hp, FundusBatches(sets, 9, dev, size=64), validator=Validator(metrics="device"),
                 val_batches=ClaheTestBatches(test_tree, 1, dev, clahe=clahe).triples, **kw)
    validator = Validator(metrics="device")
    run = TrainRun(*nets, hp, FundusBatches(sets, 9, dev, size=64, clahe=clahe), validator=validator,
                   val_batches=ClaheTestBatches(test_tree, 1, dev, clahe=clahe).triples, **kw)
    assert run.clahe_record == clahe.record() and validator.clahe == clahe.record()
    run.train_epoch()
    path = str(tmp_path / "run.pth.tar")
    run.save(path)
    saved = torch.load(path, map_location="cpu", weights_only=True)
    assert saved["clahe"] == clahe.record() and saved["feed"] == {"order": run.next_batch.order}
    # the best-Dice checkpoint is the validator's: one validation by hand (an untrained network may find no new best)
    validator.best_mean_dice = -1.0
    validator(0, *nets, run.val_batches())
    assert validator.checkpoint["clahe"] == clahe.record() and set(validator.checkpoint) == {"model", "model_shape", "model_oc", "model_oc_shape", "clahe"}
    # a run without the stage writes no entry, and does not continue a run that had it
    plain = TrainRun(*nets, hp, FundusBatches(sets, 9, dev, size=64), **kw)
    assert plain.clahe_record is None and "clahe" not in plain.state()
    with pytest.raises(ValueError, match="CLAHE"):
        plain.restore(saved)
    # the programs' path: --clahe checkpoint picks the record up, without a line; off overrides it with one
    ap = argparse.ArgumentParser()
    add_clahe_argument(ap)
    loaded, _, record = load_networks(path, want_clahe=True)
    capsys.readouterr()
    seg = Segmenter(*loaded, out_dir=None, size=64, clahe=resolve_clahe(ap, ap.parse_args([]).clahe, record))
    assert seg.clahe == clahe and capsys.readouterr().out == ""
    assert resolve_clahe(ap, "off", record) is None and "overrides" in capsys.readouterr().out
    images = [smooth_pictures(70, 1, 80, 72)[0]]
    want = Segmenter(None, None, None, None, out_dir=None, size=64, clahe=clahe).front(images)
    assert torch.equal(seg.front(images), want)
