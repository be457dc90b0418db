"""wtpse_hip/locate.py on the device (-m gpu): ops.locate_cells, ops.crop_u8 and ops.paste_u8 against their host specifications bit for
bit, Segmenter.front on device tensors against the same arrays and the live Pillow, Locator against the host composition, verification
and recentring on injected stage-1 logits, and the driver end to end on synthetic photographs (every comparison is exact)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from test_locate_cpu import PLACEMENTS, host_plan, photo
from test_segment_cpu import content
from test_segment_gpu import _check_row, _host_front, nets  # noqa: F401  (nets: the seeded networks, a module fixture here too)
from test_test_run_cpu import _disc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _field(N, H, W, seed):
    """Random pictures with a black surround: noise inside an ellipse, grey levels 0..5 outside it."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    inside = ((yy - H / 2.0) / (0.45 * H + 1)) ** 2 + ((xx - W / 2.0) / (0.45 * W + 1)) ** 2 < 1.0
    img = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    return np.where(inside[None, :, :, None], img, rng.integers(0, 6, (N, H, W, 1), dtype=np.uint8))


# ---- cell sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("case", [(5, 7, 2), (97, 131, 4), (300, 300, 16), (64, 4099, 64), (257, 33, 256)], ids=str)
def test_locate_cells_matches_host(case, N):
    from wtpse_hip import ops
    from wtpse_hip.locate import cells_host
    H, W, c = case
    img = _field(N, H, W, H * 131 + W + N)
    got = ops.locate_cells(_dev(img), c, 24)
    assert got.dtype == torch.int64 and tuple(got.shape) == (N, -(-H // c), -(-W // c), 2)
    want = cells_host(img, c, 24)
    assert np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())
    assert int(want[..., 0].sum()) not in (0, N * H * W)                    # the threshold decided something


def test_locate_cells_at_every_base_alignment_and_threshold():
    from wtpse_hip import ops
    from wtpse_hip.locate import cells_host
    H, W, c = 37, 53, 6
    img = _field(2, H, W, 9)
    for off, t in ((0, 0), (1, 24), (2, 255), (3, 1), (7, 24), (13, 128)):
        flat = torch.zeros(off + img.size, dtype=torch.uint8, device=DEV)
        flat[off:] = _dev(img).reshape(-1)
        view = flat[off:].view(2, H, W, 3)
        assert view.is_contiguous() and view.data_ptr() % 16 == (flat.data_ptr() + off) % 16
        assert np.array_equal(ops.locate_cells(view, c, t).cpu().numpy(), cells_host(img, c, t)), (off, t)


def test_locate_cells_sums_beyond_32_bits_and_repeatable():
    from wtpse_hip import ops
    from wtpse_hip.locate import cells_host
    white = np.full((1, 300, 512, 3), 255, np.uint8)
    got = ops.locate_cells(_dev(white), 256, 24).cpu().numpy()
    assert np.array_equal(got, cells_host(white, 256, 24))
    assert got[0, 0, 0].tolist() == [65536, 65536 * 65280] and got[0, 0, 0, 1] > 2 ** 31 and got[0, 1, 1].tolist() == [44 * 256, 44 * 256 * 65280]
    img = _dev(_field(2, 300, 300, 5))
    first = ops.locate_cells(img, 16, 24)
    for _ in range(3):
        assert torch.equal(ops.locate_cells(img, 16, 24), first)


def test_locate_cells_argument_checks():
    from wtpse_hip import ops
    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    assert ops.locate_cells(img, 4, 0).cpu().numpy()[..., 0].tolist() == [[[16, 16], [16, 16]]]
    wide = torch.zeros(1, 8, 8, 6, dtype=torch.uint8, device=DEV)
    for bad, c, t in ((img.float(), 4, 24), (img, 1, 24), (img, 257, 24), (img, 4, 256), (img, 4, -1), (wide[..., ::2], 4, 24), (img.cpu(), 4, 24),
                      (img[0], 4, 24), (wide[..., :4], 4, 24)):
        with pytest.raises(ValueError):
            ops.locate_cells(bad, c, t)
    with pytest.raises(ValueError):
        ops.locate_cells(np.zeros((1, 8, 8, 3), np.uint8), 4, 24)


# ---- crop and paste -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("side", [1, 7, 64, 257])
def test_crop_matches_host(side, C):
    from wtpse_hip import ops
    from wtpse_hip.locate import crop_host
    img = np.random.default_rng(side * 3 + C).integers(1, 256, (97, 131, C)).astype(np.uint8)
    boxes = PLACEMENTS + [(-side, 3), (3, -side), (1 - side, 1 - side), (96, 130), (97 - side, 131 - side)]
    got = ops.crop_u8(_dev(img), torch.tensor(boxes, dtype=torch.int32, device=DEV), side)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(boxes), side, side, C)
    assert np.array_equal(got.cpu().numpy(), crop_host(img, boxes, side))
    one = ops.crop_u8(_dev(img), torch.tensor([boxes[3]], dtype=torch.int32, device=DEV), side)      # a single box: the same pixels
    assert torch.equal(one[0], got[3])


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("side", [1, 7, 64, 257])
def test_paste_matches_host_and_restores_a_crop(side, C):
    from wtpse_hip import ops
    from wtpse_hip.locate import crop_host, paste_host
    rng = np.random.default_rng(side * 5 + C)
    img = rng.integers(0, 256, (97, 131, C)).astype(np.uint8)
    patch = rng.integers(0, 256, (side, side + 2, C)).astype(np.uint8)
    for top, left in PLACEMENTS + [(-side, 3), (3, -side - 2), (1 - side, -1 - side), (96, 130)]:
        canvas = _dev(img)
        assert ops.paste_u8(canvas, _dev(patch), top, left) is canvas
        assert np.array_equal(canvas.cpu().numpy(), paste_host(img.copy(), patch, top, left)), (top, left)
        crop = ops.crop_u8(_dev(img), torch.tensor([[top, left]], dtype=torch.int32, device=DEV), side)[0]
        scribbled = _dev(img)
        ops.paste_u8(scribbled, torch.full((side, side, C), 7, dtype=torch.uint8, device=DEV), top, left)
        assert torch.equal(ops.paste_u8(scribbled, crop, top, left), _dev(img)), (top, left)


def test_crop_and_paste_argument_checks():
    from wtpse_hip import ops
    img = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    box = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    ops.crop_u8(img, box, 4)
    for a, b, s in ((img.float(), box, 4), (img, box.long(), 4), (img, box.cpu(), 4), (img, box, 0), (img, box, 8193), (img.cpu(), box, 4),
                    (torch.zeros(8, 8, 2, dtype=torch.uint8, device=DEV), box, 4), (img, box[:, :1], 4), (img.transpose(0, 1), box, 4)):
        with pytest.raises(ValueError):
            ops.crop_u8(a, b, s)
    patch = torch.zeros(2, 2, 3, dtype=torch.uint8, device=DEV)
    for c, p, top in ((img, patch[..., :1], 0), (img, patch.cpu(), 0), (img.float(), patch, 0), (img, patch, 1 << 25), (img[:, ::2], patch, 0)):
        with pytest.raises(ValueError):
            ops.paste_u8(c, p, top, 0)


# ---- the front on device tensors ---------------------------------------------------------------------------------------------------
def test_front_on_device_tensors_equals_front_on_arrays():
    from wtpse_hip.segment import Segmenter
    seg = Segmenter(None, None, None, None, out_dir=None)
    sizes = [(100, 120), (300, 256), (100, 120), (257, 255), (256, 256)]
    imgs = [content(h, w, "random" if i % 2 else "smooth") for i, (h, w) in enumerate(sizes)]
    want = seg.front(imgs)
    assert np.array_equal(want.cpu().numpy(), np.stack([_host_front(im) for im in imgs]))        # the existing Pillow comparison
    assert torch.equal(seg.front([_dev(im) for im in imgs]), want)
    assert torch.equal(seg.front([_dev(im) if i % 2 else im for i, im in enumerate(imgs)]), want)  # a mixed list
    assert torch.equal(seg.front([_dev(imgs[1])]), want[1:2])
    with pytest.raises(ValueError):
        seg.front([_dev(imgs[0]).float()])
    with pytest.raises(ValueError):
        seg.front([_dev(imgs[0]).cpu()])


# ---- Locator ------------------------------------------------------------------------------------------------------------------------
def test_locator_without_a_network_equals_the_host_composition(tmp_path):
    from wtpse_hip import locate as L
    img, _ = photo(600, 800)
    p = host_plan(img, 1)
    assert p["cell"] == 8 and p["window"] == 10 and p["side"] == 250 and len(p["boxes"]) == 1
    loc = L.Locator(None, None, candidates=1, refine=0)
    rows, crops = loc.locate(_dev(img[None]))
    want = dict(L._blank_row(600, 800), fov_area=p["fov_area"], fov_diameter=p["fov_diameter"], cell=8, window=10, located=1, verified=-1,
                candidate=1, score=p["candidates"][0][2], roi_top=p["boxes"][0][0], roi_left=p["boxes"][0][1], roi_side=250, refine_rounds=0)
    L.write_roi_csv(str(tmp_path), [dict(rows[0], index=1, name="a.png")])
    got = L.read_roi_csv(str(tmp_path))[0]
    for k in L.ROI_COLUMNS[2:]:
        assert got[k] == want[k] or (want[k] != want[k] and got[k] != got[k]), (k, got[k], want[k])
    assert np.array_equal(crops[0].cpu().numpy(), L.crop_host(img, p["boxes"], 250)[0])
    # an explicit cell: one pass, the same rule on that table
    rows, _ = L.Locator(None, None, candidates=1, refine=0, cell=16, roi_side=200).locate(_dev(img[None]))
    q = L.plan(L.cells_host(img, 16, 24), 16, 1, side=200)
    assert (rows[0]["roi_top"], rows[0]["roi_left"], rows[0]["roi_side"], rows[0]["window"]) == (*q["boxes"][0], 200, q["window"])
    # a batch whose pictures want different cells, one of them blank
    small = np.zeros((600, 800, 3), np.uint8)
    small[200:400, 300:500] = img[200:400, 300:500]
    rows, crops = loc.locate(_dev(np.stack([img, np.zeros_like(img), small])))
    assert [r["located"] for r in rows][:2] == [1, 0] and crops[1] is None and rows[1]["fov_area"] == 0
    assert rows[0]["roi_top"] == p["boxes"][0][0] and rows[2]["cell"] == host_plan(small, 1)["cell"] != 8


def _injected(blob_for):
    """A stage 1 that answers call n with -30 everywhere and +30 on a disc (centre (100, 150), radius 30) in the maps blob_for[n] names."""
    calls = []

    def stage1(image):
        n = len(calls)
        calls.append(int(image.shape[0]))
        out = np.full((image.shape[0], 1, 256, 256), -30.0, np.float32)
        for b in blob_for[n] if n < len(blob_for) else ():
            out[b, 0][_disc(256, 256, 100, 150, 30) > 0] = 30.0
        return _dev(out)
    return stage1, calls


def test_verification_and_recentring_on_injected_logits():
    from wtpse_hip import locate as L
    from wtpse_hip.segment import mask_geometry_host
    img, _ = photo(600, 800)
    p = host_plan(img, 3)
    assert len(p["boxes"]) == 3
    rec = mask_geometry_host(_disc(256, 256, 100, 150, 30))
    assert L.passes(rec, 256)
    moved = L.recentre(*p["boxes"][1], p["side"], rec, 256)
    assert moved != p["boxes"][1]
    # a disc in candidate 2's crop only, and again in the recentred crop
    loc = L.Locator(None, None, candidates=3, refine=1)
    loc.stage1, calls = _injected([[1], [0]])
    rows, crops = loc.locate(_dev(img[None]))
    assert calls == [3, 1]
    r = rows[0]
    assert (r["candidate"], r["verified"], r["refine_rounds"], r["score"]) == (2, 1, 1, p["candidates"][1][2])
    assert (r["roi_top"], r["roi_left"], r["roi_side"]) == (*moved, p["side"])
    assert np.array_equal(crops[0].cpu().numpy(), L.crop_host(img, [moved], p["side"])[0])
    # the disc is lost after the move: the verified box stays
    loc.stage1, calls = _injected([[1], []])
    rows, crops = loc.locate(_dev(img[None]))
    assert calls == [3, 1] and (rows[0]["roi_top"], rows[0]["roi_left"], rows[0]["refine_rounds"], rows[0]["verified"]) == (*p["boxes"][1], 0, 1)
    assert np.array_equal(crops[0].cpu().numpy(), L.crop_host(img, [p["boxes"][1]], p["side"])[0])
    # two rounds: the second finds the same centroid in the moved crop and moves again; a third call never happens with refine = 2
    loc2 = L.Locator(None, None, candidates=3, refine=2)
    loc2.stage1, calls = _injected([[1], [0], [0]])
    rows, _ = loc2.locate(_dev(img[None]))
    again = L.recentre(*moved, p["side"], rec, 256)
    assert calls == [3, 1, 1] and (rows[0]["roi_top"], rows[0]["roi_left"], rows[0]["refine_rounds"]) == (*again, 2)
    # no disc anywhere: candidate 1, flagged, not moved
    loc.stage1, calls = _injected([[]])
    rows, crops = loc.locate(_dev(img[None]))
    assert calls == [3] and (rows[0]["candidate"], rows[0]["verified"], rows[0]["refine_rounds"]) == (1, 0, 0)
    assert (rows[0]["roi_top"], rows[0]["roi_left"]) == p["boxes"][0]
    assert np.array_equal(crops[0].cpu().numpy(), L.crop_host(img, p["boxes"][:1], p["side"])[0])


# ---- the driver end to end ------------------------------------------------------------------------------------------------------
E2E = (("b right eye.png", 300, 300), ("a.png", 222, 190), ("blank.png", 222, 190))


@pytest.fixture(scope="module")
def whole(nets, tmp_path_factory):  # noqa: F811
    from wtpse_hip import locate as L
    root, out = str(tmp_path_factory.mktemp("photographs")), str(tmp_path_factory.mktemp("located"))
    for name, h, w in E2E:
        Image.fromarray(np.zeros((h, w, 3), np.uint8) if name.startswith("blank") else photo(h, w)[0]).save(os.path.join(root, name))
    for n in nets:
        n.train()
    run = L.WholeImageSegmenter(*nets, out_dir=out, candidates=2, refine=1, batch_size=2)
    summary = run.run(root)
    assert all(n.training for n in nets)
    return root, out, run, summary


def test_end_to_end_files(whole):
    from wtpse_hip import locate as L
    from wtpse_hip.segment import read_measurements
    root, out, run, summary = whole
    rows = L.read_roi_csv(out)
    assert [r["name"] for r in rows] == ["a.png", "b right eye.png", "blank.png"] and [r["index"] for r in rows] == [1, 2, 3]
    assert [r["located"] for r in rows] == [1, 1, 0] and rows[2]["fov_area"] == 0
    assert (summary["n_located"], summary["n_not_located"], summary["n"]) == (2, 1, 2)
    assert summary["n_verified"] == sum(1 for r in rows if r["verified"] == 1)
    mrows, msummary = read_measurements(out)
    assert msummary == summary and [m["name"] for m in mrows] == ["a.png", "b right eye.png"]
    for sub in ("crop", "mask", "overlay", "full_mask", "full_overlay"):
        assert sorted(os.listdir(os.path.join(out, sub))) == ["a.png", "b right eye.png"], sub
    for r, m in zip(rows, mrows):
        img = np.array(Image.open(os.path.join(root, r["name"])).convert("RGB"))
        p = host_plan(img, 2)
        assert (r["height"], r["width"]) == img.shape[:2] and (r["fov_area"], r["cell"], r["window"], r["roi_side"]) == (p["fov_area"], p["cell"], p["window"], p["side"])
        assert r["verified"] in (0, 1) and 1 <= r["candidate"] <= len(p["candidates"]) and r["score"] == p["candidates"][r["candidate"] - 1][2]
        if r["refine_rounds"] == 0:
            assert (r["roi_top"], r["roi_left"]) == p["boxes"][r["candidate"] - 1]
        side, box = r["roi_side"], (r["roi_top"], r["roi_left"])
        crop = np.array(Image.open(os.path.join(out, "crop", r["name"])))
        assert np.array_equal(crop, L.crop_host(img, [box], side)[0])                             # = the device crop (crop_u8 == crop_host)
        mask = np.array(Image.open(os.path.join(out, "mask", r["name"])))
        assert mask.shape == (side, side) and (m["height"], m["width"]) == (side, side)
        want = L.paste_host(np.full(img.shape[:2], 255, np.uint8), mask, *box)
        assert np.array_equal(np.array(Image.open(os.path.join(out, "full_mask", r["name"]))), want)
        over = np.array(Image.open(os.path.join(out, "overlay", r["name"])))
        assert np.array_equal(np.array(Image.open(os.path.join(out, "full_overlay", r["name"]))), L.paste_host(img.copy(), over, *box))
        for name in ("disc", "cup"):
            for axis, origin in (("cy", box[0]), ("cx", box[1])):
                a, b = r[name + "_" + axis], origin + m[name + "_" + axis]
                assert a == b or (a != a and b != b)


def test_end_to_end_measurements_are_segment_on_the_crops(whole, nets, tmp_path):  # noqa: F811
    from wtpse_hip.segment import Segmenter, read_measurements
    _, out, run, summary = whole
    plain = Segmenter(*nets, out_dir=str(tmp_path), batch_size=2).run(os.path.join(out, "crop"))
    rows, _ = read_measurements(out)
    want, _ = read_measurements(str(tmp_path))
    assert len(rows) == len(want) == 2 and {k: summary[k] for k in plain} == plain
    for a, b in zip(rows, want):
        assert (a["index"], a["name"]) == (b["index"], b["name"])
        _check_row(a, b)
        for sub in ("mask", "overlay"):
            assert np.array_equal(np.array(Image.open(os.path.join(out, sub, a["name"]))), np.array(Image.open(os.path.join(str(tmp_path), sub, a["name"]))))


def test_a_folder_of_blank_pictures_is_listed_and_skipped(nets, tmp_path):  # noqa: F811
    from wtpse_hip import locate as L
    root, out = tmp_path / "in", tmp_path / "out"
    root.mkdir()
    Image.fromarray(np.zeros((64, 80, 3), np.uint8)).save(root / "x.png")
    summary = L.WholeImageSegmenter(*nets, out_dir=str(out), batch_size=2).run(str(root))
    rows = L.read_roi_csv(str(out))
    assert len(rows) == 1 and rows[0]["located"] == 0 and rows[0]["verified"] == -1 and (rows[0]["height"], rows[0]["width"]) == (64, 80)
    assert (summary["n"], summary["n_located"], summary["n_not_located"], summary["n_verified"]) == (0, 0, 1, 0)
    assert not os.path.exists(out / "full_mask") and os.listdir(out / "crop") == []
