"""Whole fundus photographs: find the optic disc in what a fundus camera writes — a circular field of view on black, 2000 to 4000
pixels wide, the disc an eighth of its width — cut the region of interest the networks were trained on, and hand the crops to an
unchanged `segment.Segmenter`.  segment.py starts from crops somebody made; this is the step in front of it.

    python -m wtpse_hip.locate --images DIR --checkpoint C --out O [--candidates 3] [--refine 1] [--disc-scale 0.13]
                               [--roi-scale 0.4 | --roi-side PX] [--cell auto|C] [--fov-threshold 24] [--min-area 0.01 --max-area 0.5]
                               [--no-full] + every switch of wtpse_hip.segment (--samples, --views, --morphometry, --batch-size, ...)

    O/roi.csv                ROI_COLUMNS, one row per input image (located or not)
    O/crop/<stem>.png        the final crop, side x side: a dataset-style ROI (segment, test_run and the loaders read a folder of them)
    O/full_mask/<stem>.png   the label map at the photograph's own size: 255 with the crop's label map at the box (--no-full: not written)
    O/full_overlay/<stem>.png   the photograph with the crop's contour overlay at the box (--no-full or --no-overlay: not written)
    O/mask, O/overlay, O/measurements.csv, ... everything segment.py writes for the folder O/crop, in the crop's frame
    O/summary.json           segment's, plus n_located, n_verified, n_not_located
    O/gradability.csv        with --gradability only (gradability.py): per input image, located or not, the focus, exposure and field
                             measures of the photograph (photo_*: ops.gradability_record at --fov-threshold in the visit that makes the
                             cell table, the illumination figures from that table) and of its final crop (roi_*: every pixel in the
                             field), the flags of the thresholds given — they judge the photograph — and focus_rank; summary.json gains
                             gradability.  roi.csv and every other file are the same with and without it

1. Cell sums (`ops.locate_cells`, csrc/locate.hip; `cells_host` is the specification, bit for bit): per c x c cell the count n of the
   pixels with max(R,G,B) >= fov_threshold and the sum s of 77 R + 150 G + 29 B over them.  This is the only pass over the full-size
   picture; with --cell auto it runs twice — once at c = 256 for the field's area, which the cell side depends on, once at that side
   (the second reads what the first left in the Infinity Cache) — with --cell C once.
2. Candidates (`candidates`, host, exact integers): A = sum n, D = 2 sqrt(A / pi), disc_px = disc_scale D, the auto cell the largest power
   of two <= disc_px / 8 (2..256), k = max(1, floor(disc_px / c + 0.5)) cells the window.  For every k x k window (stride one cell) `in`
   is the window and `ring` the centred 3k x 3k window minus it (zeros beyond the table), both from 2-D cumulative sums in int64.  Valid:
   4 n_in >= 3 (k c)^2 and n_ring >= n_in.  Score (s_in / n_in - s_ring / n_ring) / 256.  Greedy picks in the order (score descending,
   row, column); a window within k cells of an earlier pick in BOTH axes is skipped; stop at `count` picks or at the first score <= 0.
   Centre ((i + k/2) c, (j + k/2) c); side = 2 floor(roi_scale D / 2 + 0.5); box top = floor(centre_y - side / 2), left likewise.
3. Crops (`ops.crop_u8`, `crop_host`; zero beyond the photograph) never visit the host: Segmenter.front takes device tensors.
4. Verification (`choose`): the candidates' crops through the front, stage 1 only, ops.postprocess_masks and ops.mask_geometry; the first
   candidate in rank order whose disc has min_area <= area / S^2 <= max_area and a bounding box that touches no border is verified = 1;
   none: candidate 1 with verified = 0 (segmented all the same, and flagged).  candidates = 1 and refine = 0: no network, verified = -1.
   No candidate at all (blank picture, no positive score): located = 0, listed in roi.csv and skipped.
5. Recentring (`recentre`), `refine` times: y = top + (cy + 0.5) side / S - 0.5, top' = floor(y - side / 2 + 0.5), likewise the column;
   crop and stage 1 again.  Stops when the box does not move or the disc no longer passes `choose`'s test, keeping the previous box.

The crops stay on the device until they are segmented (3 side^2 bytes each).  The full-size products decode the photograph a second time
(nothing that size is kept across the run), build mask and overlay on the device with ops.paste_u8 and come back in one copy per size
group."""
import json
import math
import os

import numpy as np
import torch

from . import gradability as GR
from . import ops
from . import tables as T
from . import validate as V
from .packed import fetch
from .segment import ImageFolder, Segmenter, _groups

ROI_INT = ("height", "width", "fov_area")
ROI_INT2 = ("cell", "window", "located", "verified", "candidate")
ROI_INT3 = ("roi_top", "roi_left", "roi_side", "refine_rounds")
ROI_FLOAT = ("disc_cy", "disc_cx", "cup_cy", "cup_cx")
ROI_COLUMNS = ("index", "name") + ROI_INT + ("fov_diameter",) + ROI_INT2 + ("score",) + ROI_INT3 + ROI_FLOAT
_INTS, _FLOATS = ROI_INT + ROI_INT2 + ROI_INT3, ("fov_diameter", "score") + ROI_FLOAT
COARSE_CELL = 256                      # the pass that only measures the field's area (--cell auto)


# ---- the host specifications ----------------------------------------------------------------------------------------------
def cells_host(img, c, t):
    """[H,W,3] (or [N,H,W,3]) uint8 -> int64 [ceil(H/c), ceil(W/c), 2] (or [N, ...]) = per c x c cell (n, s) over its pixels inside the
    picture with max(R,G,B) >= t: their count and the sum of 77 R + 150 G + 29 B.  ops.locate_cells' specification."""
    img = np.asarray(img)
    if img.ndim == 4:
        return np.stack([cells_host(im, c, t) for im in img])
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("img must be [H,W,3] uint8 (got %s %s)" % (img.shape, img.dtype))
    c = int(c)
    H, W = img.shape[:2]
    a = img.astype(np.int64)
    f = (img.max(-1) >= int(t)).astype(np.int64)
    y = (77 * a[..., 0] + 150 * a[..., 1] + 29 * a[..., 2]) * f
    CH, CW = -(-H // c), -(-W // c)
    pool = lambda v: np.pad(v, ((0, CH * c - H), (0, CW * c - W))).reshape(CH, c, CW, c).sum((1, 3))
    return np.stack([pool(f), pool(y)], -1)


def crop_host(img, boxes, side):
    """[H,W,C] and boxes [(top, left)] -> [M,side,side,C]: the boxes' pixels, 0 beyond the picture.  ops.crop_u8's specification."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    out = np.zeros((len(boxes), side, side) + img.shape[2:], img.dtype)
    for m, (top, left) in enumerate(boxes):
        ya, yb, xa, xb = max(top, 0), min(top + side, H), max(left, 0), min(left + side, W)
        if ya < yb and xa < xb:
            out[m, ya - top:yb - top, xa - left:xb - left] = img[ya:yb, xa:xb]
    return out


def paste_host(canvas, patch, top, left):
    """canvas [H,W,C], in place: the patch [h,w,C] with its corner at (top, left), clipped.  ops.paste_u8's specification.  -> canvas."""
    H, W = canvas.shape[:2]
    h, w = patch.shape[:2]
    ya, yb, xa, xb = max(top, 0), min(top + h, H), max(left, 0), min(left + w, W)
    if ya < yb and xa < xb:
        canvas[ya:yb, xa:xb] = patch[ya - top:yb - top, xa - left:xb - left]
    return canvas


def _half_up(x):
    return int(math.floor(x + 0.5))


def fov_diameter(area):
    """The diameter of the circle of `area` pixels (float64)."""
    return 2.0 * math.sqrt(float(area) / math.pi)


def auto_cell(disc_px):
    """The largest power of two <= disc_px / 8, within 2..256."""
    c = 2
    while c * 2 <= disc_px / 8.0 and c < 256:
        c *= 2
    return c


def window_cells(disc_px, c):
    return max(1, _half_up(disc_px / c))


def roi_side(diameter, roi_scale=0.4):
    return max(2, 2 * _half_up(roi_scale * diameter / 2.0))


def _window_sums(table, i0, j0, size, shape):
    """Sums of table over the size x size windows whose corners are (i + i0, j + j0), (i, j) over `shape`, zeros beyond the table."""
    pad = max(size, abs(i0), abs(j0)) + 1
    P = np.pad(table, pad)
    C = np.zeros((P.shape[0] + 1, P.shape[1] + 1), np.int64)
    C[1:, 1:] = P.cumsum(0).cumsum(1)
    ii, jj = np.mgrid[0:shape[0], 0:shape[1]]
    a, b = ii + pad + i0, jj + pad + j0
    return C[a + size, b + size] - C[a, b + size] - C[a + size, b] + C[a, b]


def window_scores(cells, c, k):
    """cells [CH,CW,2] int64 -> (score float64, valid bool), each [CH-k+1, CW-k+1] (empty when the table is smaller than a window)."""
    cells = np.asarray(cells, np.int64)
    CH, CW = cells.shape[:2]
    shape = (max(CH - k + 1, 0), max(CW - k + 1, 0))
    if 0 in shape:
        return np.zeros(shape), np.zeros(shape, bool)
    n, s = cells[..., 0], cells[..., 1]
    n_in, s_in = _window_sums(n, 0, 0, k, shape), _window_sums(s, 0, 0, k, shape)
    n_ring, s_ring = _window_sums(n, -k, -k, 3 * k, shape) - n_in, _window_sums(s, -k, -k, 3 * k, shape) - s_in
    valid = (4 * n_in >= 3 * (k * c) ** 2) & (n_ring >= n_in) & (n_in > 0)
    score = np.where(valid, (s_in / np.maximum(n_in, 1) - s_ring / np.maximum(n_ring, 1)) / 256.0, -np.inf)
    return score, valid


def candidates(cells, c, k, count=3):
    """-> [(i, j, score)], at most `count`, in rank order: the module docstring's step 2."""
    score, valid = window_scores(cells, int(c), int(k))
    if score.size == 0:
        return []
    ii, jj = np.mgrid[0:score.shape[0], 0:score.shape[1]]
    order = np.lexsort((jj.ravel(), ii.ravel(), -score.ravel()))
    out = []
    for o in order:
        i, j = divmod(int(o), score.shape[1])
        if not score[i, j] > 0:
            break
        if all(abs(i - a) >= k or abs(j - b) >= k for a, b, _ in out):
            out.append((i, j, float(score[i, j])))
            if len(out) >= count:
                break
    return out


def centre(i, j, k, c):
    return (i + k / 2.0) * c, (j + k / 2.0) * c


def box_at(cy, cx, side):
    """(top, left) of the side x side box centred at the point (cy, cx) (pixel p covers [p, p + 1))."""
    return int(math.floor(cy - side / 2.0)), int(math.floor(cx - side / 2.0))


def passes(rec, S, min_area=0.01, max_area=0.5):
    """A mask_geometry record of a disc at S x S: its area fraction within the bounds (inclusive) and its box off every border."""
    area, top, bottom, left, right = (int(v) for v in rec[:5])
    return area >= 1 and min_area * S * S <= area <= max_area * S * S and top > 0 and left > 0 and bottom < S - 1 and right < S - 1


def choose(cands, records, S, min_area=0.01, max_area=0.5):
    """-> (position in `cands`, verified): the first candidate in rank order whose record passes, verified = 1; none: (0, 0)."""
    for r in range(len(cands)):
        if passes(records[r], S, min_area, max_area):
            return r, 1
    return 0, 0


def recentre(top, left, side, rec, S):
    """The box moved onto the centroid of the disc record `rec` (taken at S x S from the crop of the box) -> (top, left)."""
    area = int(rec[0])
    cy, cx = float(np.float64(int(rec[5])) / area), float(np.float64(int(rec[6])) / area)
    y = top + (cy + 0.5) * side / S - 0.5
    x = left + (cx + 0.5) * side / S - 0.5
    return int(math.floor(y - side / 2.0 + 0.5)), int(math.floor(x - side / 2.0 + 0.5))


def plan(cells, c, count=3, disc_scale=0.13, roi_scale=0.4, side=None):
    """A cell table at side c -> everything the host decides before a crop is cut: {fov_area, fov_diameter, cell, window, side,
    candidates [(i, j, score)], boxes [(top, left)]}."""
    area = int(np.asarray(cells)[..., 0].sum())
    D = fov_diameter(area)
    k = window_cells(disc_scale * D, c)
    side = int(side) if side else roi_side(D, roi_scale)
    cands = candidates(cells, c, k, count) if area else []
    return {"fov_area": area, "fov_diameter": D, "cell": int(c), "window": k, "side": side, "candidates": cands,
            "boxes": [box_at(*centre(i, j, k, c), side) for i, j, _ in cands]}


# ---- roi.csv ----------------------------------------------------------------------------------------------------------------
def write_roi_csv(out_dir, rows):
    os.makedirs(out_dir, exist_ok=True)
    T.write_csv(os.path.join(out_dir, "roi.csv"), ROI_COLUMNS, rows, ("index",) + _INTS)


def read_roi_csv(out_dir):
    return T.read_csv(os.path.join(out_dir, "roi.csv"), ("index",) + _INTS)


def _blank_row(h, w):
    nan = float("nan")
    row = dict.fromkeys(_INTS, 0)
    row.update(dict.fromkeys(_FLOATS, nan), height=int(h), width=int(w), fov_diameter=0.0, verified=-1)
    return row


# ---- locating -----------------------------------------------------------------------------------------------------------------
class Locator:
    """locate(stack [N,H,W,3] uint8 on the device) -> (rows, crops): per picture its roi.csv row without index, name and the
    centroids, and its final crop [side,side,3] uint8 on the device (None where located = 0).  `stage1(image [B,3,S,S]) -> logits
    [B,1,S,S]` is the disc network (model.predict(model_shape, image)[0]); the caller holds the networks in eval mode."""

    def __init__(self, model, model_shape, candidates=3, refine=1, disc_scale=0.13, roi_scale=0.4, roi_side=None, cell="auto",
                 fov_threshold=24, min_area=0.01, max_area=0.5, batch_size=9, size=256, clahe=None, gradability=None):
        if int(candidates) < 1 or int(refine) < 0 or int(batch_size) < 1:
            raise ValueError("candidates and batch_size must be positive and refine must not be negative")
        if cell != "auto" and not 2 <= int(cell) <= 256:
            raise ValueError("cell must be 'auto' or lie in 2..256 (got %r)" % (cell,))
        if not 0 <= int(fov_threshold) <= 255 or not (disc_scale > 0 and roi_scale > 0) or not 0 <= min_area <= max_area:
            raise ValueError("fov_threshold must lie in 0..255, the scales must be positive and min_area <= max_area")
        if roi_side is not None and not 2 <= int(roi_side) <= 8192:
            raise ValueError("roi_side must lie in 2..8192 (got %r)" % (roi_side,))
        self.model, self.model_shape = model, model_shape
        self.count, self.refine, self.disc_scale, self.roi_scale = int(candidates), int(refine), float(disc_scale), float(roi_scale)
        self.roi_side, self.cell, self.t = (None if roi_side is None else int(roi_side)), (cell if cell == "auto" else int(cell)), int(fov_threshold)
        self.min_area, self.max_area, self.batch_size, self.size = float(min_area), float(max_area), int(batch_size), int(size)
        # (clahe: the candidate crops the disc network verifies are preprocessed as the final crops are; the search for candidates
        # on the full photograph is not)
        self._front = Segmenter(None, None, None, None, out_dir=None, size=size, clahe=clahe)
        self.seconds = None                                 # {"cells", "verify", "refine"} when timing is on (tools/bench_locate.py)
        # a gradability.Gradability: `locate` also takes the photographs' records (ops.gradability_record at the field threshold) in
        # the visit that makes the cell tables and leaves their measures, one per picture of the stack, in `photo_measures`
        self.gradability, self.photo_measures = gradability, None

    def stage1(self, image):
        with torch.no_grad():
            return self.model.predict(self.model_shape, image)[0]

    def _tick(self, key, t0):
        if self.seconds is not None:
            import time
            torch.cuda.synchronize()
            self.seconds[key] = self.seconds.get(key, 0.0) + time.perf_counter() - t0
        return self._now()

    def _now(self):
        if self.seconds is None:
            return 0.0
        import time
        torch.cuda.synchronize()
        return time.perf_counter()

    def cell_tables(self, stack):
        """-> [(cells [CH,CW,2] int64 numpy or None for a picture without a field, c)] per picture."""
        N = stack.shape[0]
        if self.cell != "auto":
            host = ops.locate_cells(stack, self.cell, self.t).cpu().numpy()
            return [(host[i], self.cell) for i in range(N)]
        area = ops.locate_cells(stack, COARSE_CELL, self.t)[..., 0].sum((1, 2)).cpu().numpy()
        cs = [auto_cell(self.disc_scale * fov_diameter(int(a))) if a else 0 for a in area]
        live = sorted(set(c for c in cs if c))
        if len(live) == 1 and all(cs):
            host = ops.locate_cells(stack, live[0], self.t).cpu().numpy()
            return [(host[i], live[0]) for i in range(N)]
        return [(ops.locate_cells(stack[i:i + 1], c, self.t)[0].cpu().numpy(), c) if c else (None, 0) for i, c in enumerate(cs)]

    def records(self, crops):
        """Crops (device [s,s,3] uint8, any sides) -> their disc records [n,8] int64 at S x S, one copy."""
        out = []
        for first in range(0, len(crops), self.batch_size):
            image = self._front.front(crops[first:first + self.batch_size], crops[0].device)
            masks = ops.postprocess_masks(self.stage1(image).contiguous())
            out.append(ops.mask_geometry(masks))
        return torch.cat(out).cpu().numpy()

    def locate(self, stack):
        N, H, W, _ = stack.shape
        dev, S = stack.device, self.size
        t0 = self._now()
        plans, tables = [], self.cell_tables(stack)
        for cells, c in tables:
            plans.append(None if cells is None else plan(cells, c, self.count, self.disc_scale, self.roi_scale, self.roi_side))
        if self.gradability is not None:
            rec = ops.gradability_record(stack, self.t, self.gradability.sat).cpu().numpy()
            self.photo_measures = [self.gradability.measures(rec[i], cells, c or None) for i, (cells, c) in enumerate(tables)]
        t0 = self._tick("cells", t0)
        rows, crops = [_blank_row(H, W) for _ in range(N)], [None] * N
        live = [i for i in range(N) if plans[i] is not None and plans[i]["candidates"]]
        for i, p in enumerate(plans):
            if p is not None:
                rows[i].update(fov_area=p["fov_area"], fov_diameter=p["fov_diameter"], cell=p["cell"], window=p["window"])
        cut = lambda i, boxes: ops.crop_u8(stack[i], torch.tensor(boxes, dtype=torch.int32, device=dev).reshape(-1, 2), plans[i]["side"])
        state = {}                                          # picture -> [position, verified, box, record or None, rounds]
        if self.count == 1 and self.refine == 0:
            for i in live:
                state[i] = [0, -1, plans[i]["boxes"][0], None, 0]
                crops[i] = cut(i, [state[i][2]])[0]
        elif live:
            stacks = [cut(i, plans[i]["boxes"]) for i in live]
            recs = self.records([s[m] for s in stacks for m in range(s.shape[0])])
            at = 0
            for i, s in zip(live, stacks):
                n = s.shape[0]
                pos, ok = choose(plans[i]["candidates"], recs[at:at + n], S, self.min_area, self.max_area)
                state[i] = [pos, ok, plans[i]["boxes"][pos], recs[at + pos], 0]
                crops[i] = s[pos]
                at += n
        t0 = self._tick("verify", t0)
        moving = [i for i in live if state[i][1] == 1]
        for _ in range(self.refine):
            moved = []
            for i in moving:
                box = recentre(state[i][2][0], state[i][2][1], plans[i]["side"], state[i][3], S)
                if box != tuple(state[i][2]):
                    moved.append((i, box))
            if not moved:
                break
            new = [cut(i, [box])[0] for i, box in moved]
            recs = self.records(new)
            moving = []
            for (i, box), crop, rec in zip(moved, new, recs):
                if passes(rec, S, self.min_area, self.max_area):
                    state[i][2], state[i][3], state[i][4] = box, rec, state[i][4] + 1
                    crops[i] = crop
                    moving.append(i)
        self._tick("refine", t0)
        for i in live:
            pos, ok, box, _, rounds = state[i]
            rows[i].update(located=1, verified=ok, candidate=pos + 1, score=plans[i]["candidates"][pos][2], roi_top=box[0], roi_left=box[1],
                           roi_side=plans[i]["side"], refine_rounds=rounds)
        return rows, crops


class CropFolder(ImageFolder):
    """The located pictures' crops as Segmenter.run's feed: `load` returns the device crop."""

    def __init__(self, paths, crops):
        ImageFolder.__init__(self, paths)
        self.crops = list(crops)

    def load(self, i):
        return self.crops[i]


class WholeImageSegmenter:
    """run(folder of photographs): locate every picture (in chunks of `chunk` consecutive ones, by size), write roi.csv and crop/,
    segment the crops with an unchanged Segmenter (every keyword Locator does not take goes to it), write the full-size products.
    -> the summary; `self.roi_rows` keeps roi.csv's rows, `self.segmenter.rows` the measurements."""

    LOCATOR_KEYS = ("candidates", "refine", "disc_scale", "roi_scale", "roi_side", "cell", "fov_threshold", "min_area", "max_area")

    def __init__(self, model, model_shape, model_oc, model_shape_oc, out_dir, full=True, chunk=4, **kw):
        loc = {k: kw.pop(k) for k in self.LOCATOR_KEYS if k in kw}
        self.segmenter = Segmenter(model, model_shape, model_oc, model_shape_oc, out_dir=out_dir, **kw)
        # gradability (a Segmenter keyword): the segmenter scores the crops, the locator the photographs, and `run` joins the two
        self.gradability = self.segmenter.gradability
        self.segmenter.write_gradability = False
        if self.gradability is not None:
            loc["gradability"] = self.gradability
        self.locator = Locator(model, model_shape, batch_size=self.segmenter.batch_size, size=self.segmenter.size,
                               clahe=self.segmenter.clahe, **loc)
        self.out_dir, self.full, self.chunk, self.roi_rows = out_dir, bool(full), max(1, int(chunk)), []
        self.photo_measures, self.grad_rows = [], []

    def _locate_all(self, folder, device):
        from PIL import Image
        rows, crops = [None] * len(folder), [None] * len(folder)
        self.photo_measures = [None] * len(folder)
        os.makedirs(os.path.join(self.out_dir, "crop"), exist_ok=True)
        for first in range(0, len(folder), self.chunk):
            idx = list(range(first, min(first + self.chunk, len(folder))))
            images = [ImageFolder.load(folder, i) for i in idx]
            for _, pos in _groups([im.shape[:2] for im in images]).items():
                stack = torch.from_numpy(np.stack([images[p] for p in pos])).to(device)
                got_rows, got_crops = self.locator.locate(stack)
                host = iter(fetch([c for c in got_crops if c is not None]))         # the one copy
                for p, row, crop in zip(pos, got_rows, got_crops):
                    i = idx[p]
                    rows[i], crops[i] = dict(row, index=i + 1, name=folder.names[i]), crop
                    if self.gradability is not None:
                        self.photo_measures[i] = self.locator.photo_measures[p]
                    if crop is not None:
                        Image.fromarray(next(host)).save(os.path.join(self.out_dir, "crop", folder.names[i]))
        return rows, crops

    def _write_full(self, folder, rows, device):
        """full_mask/ and full_overlay/ of the located pictures: per size group one set of pastes and one copy."""
        from PIL import Image
        overlay = self.segmenter.overlay
        for sub in ("full_mask",) + (("full_overlay",) if overlay else ()):
            os.makedirs(os.path.join(self.out_dir, sub), exist_ok=True)
        todo = [i for i, r in enumerate(rows) if r["located"]]
        read = lambda sub, name: torch.from_numpy(np.ascontiguousarray(np.array(Image.open(os.path.join(self.out_dir, sub, name))))).to(device)
        for first in range(0, len(todo), self.chunk):
            idx = todo[first:first + self.chunk]
            for (H, W), pos in _groups([(rows[i]["height"], rows[i]["width"]) for i in idx]).items():
                n = len(pos)
                masks = torch.full((n, H, W, 1), 255, dtype=torch.uint8, device=device)
                photos = torch.from_numpy(np.stack([ImageFolder.load(folder, idx[p]) for p in pos])).to(device) if overlay else None
                for j, p in enumerate(pos):
                    r = rows[idx[p]]
                    ops.paste_u8(masks[j], read("mask", r["name"]).reshape(r["roi_side"], r["roi_side"], 1), r["roi_top"], r["roi_left"])
                    if overlay:
                        ops.paste_u8(photos[j], read("overlay", r["name"]), r["roi_top"], r["roi_left"])
                host_masks, *host_photos = fetch([masks.reshape(n, H, W)] + ([photos] if overlay else []))        # the one copy
                for j, p in enumerate(pos):
                    name = rows[idx[p]]["name"]
                    Image.fromarray(host_masks[j], "L").save(os.path.join(self.out_dir, "full_mask", name))
                    if overlay:
                        Image.fromarray(host_photos[0][j]).save(os.path.join(self.out_dir, "full_overlay", name))

    def _write_gradability(self, rows, found):
        """gradability.csv: per input picture its photograph-level measures (photo_*) and those of its final crop as the segmenter
        took them (roi_*; a picture that was not located: an empty record's), the flags — they judge the photograph — and
        focus_rank by photo_focus_ratio.  -> summary.json's entry."""
        G = self.gradability
        blank = G.measures(np.zeros(GR.GRAD_REC, np.int64))
        roi = dict(zip(found, self.segmenter.grad_rows))
        table = []
        for i, r in enumerate(rows):
            row = {"index": r["index"], "name": r["name"]}
            row.update({"photo_" + k: self.photo_measures[i][k] for k in GR.MEASURES})
            row.update({"roi_" + k: roi.get(i, blank)[k] for k in GR.MEASURES})
            table.append(row)
        self.grad_rows = GR.finish_rows(table, G, ("photo_", "roi_"))
        GR.write_csv(self.out_dir, self.grad_rows, ("photo_", "roi_"))
        return GR.summarise(self.grad_rows, G)

    def run(self, folder):
        if not isinstance(folder, ImageFolder):
            folder = ImageFolder(folder)
        nets = self.segmenter.nets
        device = next(nets[0].parameters()).device
        with V.eval_mode(nets):
            rows, crops = self._locate_all(folder, device)
        found = [i for i, r in enumerate(rows) if r["located"]]
        summary = self.segmenter.run(CropFolder([folder.paths[i] for i in found], [crops[i] for i in found]))
        for i, m in zip(found, self.segmenter.rows):
            for name in ("disc", "cup"):
                rows[i][name + "_cy"], rows[i][name + "_cx"] = rows[i]["roi_top"] + m[name + "_cy"], rows[i]["roi_left"] + m[name + "_cx"]
        self.roi_rows = rows
        write_roi_csv(self.out_dir, rows)
        summary = dict(summary, n_located=len(found), n_verified=sum(1 for r in rows if r["verified"] == 1), n_not_located=len(rows) - len(found))
        if self.gradability is not None:
            summary = dict(summary, gradability=self._write_gradability(rows, found))
        T.write_json(os.path.join(self.out_dir, "summary.json"), summary, allow_nan=False)
        if self.full and found:
            self._write_full(folder, rows, device)
        return summary


# ---- command line -----------------------------------------------------------------------------------------------------------
def parser():
    import argparse
    from . import segment
    ap = argparse.ArgumentParser(prog="python -m wtpse_hip.locate", description=__doc__.split("\n\n")[0])
    segment.add_arguments(ap, images_help="a directory of whole fundus photographs (%s)" % " ".join(segment.EXTENSIONS))
    ap.add_argument("--candidates", type=int, default=3, help="disc candidates per photograph handed to the disc network")
    ap.add_argument("--refine", type=int, default=1, help="recentring rounds on the verified disc's centroid")
    ap.add_argument("--disc-scale", type=float, default=0.13, help="disc diameter / field-of-view diameter")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--roi-scale", type=float, default=0.4, help="crop side / field-of-view diameter")
    g.add_argument("--roi-side", type=int, default=None, help="the crop side in pixels, whatever the field's size")
    ap.add_argument("--cell", default="auto", help="auto, or the side of the cells the candidates are searched on (2..256)")
    ap.add_argument("--fov-threshold", type=int, default=24, help="a pixel belongs to the field of view when max(R,G,B) reaches this")
    ap.add_argument("--min-area", type=float, default=0.01, help="smallest disc area / crop area that verifies a candidate")
    ap.add_argument("--max-area", type=float, default=0.5, help="largest disc area / crop area that verifies a candidate")
    ap.add_argument("--no-full", action="store_true", help="do not write full_mask/ and full_overlay/")
    return ap


def main(argv=None):
    from . import segment
    from .programs import load_networks, require_gpu, resolve_clahe
    ap = parser()
    args = ap.parse_args(argv)
    kw = segment.segmenter_arguments(ap, args)
    if args.cell != "auto":
        try:
            args.cell = int(args.cell)
        except ValueError:
            ap.error("--cell takes auto or an integer in 2..256")
    require_gpu("locate")
    folder = ImageFolder(args.images)
    if len(folder) < 1:
        raise SystemExit("no image (%s) under %s" % (" ".join(segment.EXTENSIONS), args.images))
    nets, _, record = load_networks(args.checkpoint, want_clahe=True)
    clahe = resolve_clahe(ap, args.clahe, record)
    if clahe is not None:                   # (off: the keywords are what they were)
        kw["clahe"] = clahe
    try:
        run = WholeImageSegmenter(*nets, out_dir=args.out, full=not args.no_full, candidates=args.candidates, refine=args.refine,
                                  disc_scale=args.disc_scale, roi_scale=args.roi_scale, roi_side=args.roi_side, cell=args.cell,
                                  fov_threshold=args.fov_threshold, min_area=args.min_area, max_area=args.max_area, **kw)
    except ValueError as e:
        ap.error(str(e))
    summary = run.run(folder)
    torch.cuda.synchronize()
    print(json.dumps(summary, sort_keys=True))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
