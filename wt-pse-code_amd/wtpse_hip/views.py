"""Test-time views: the eight symmetries of the square (the dihedral group D4) applied to a network input, and the merge of the
predictions the views give back.

The networks are trained under flips and rotations (input_pipeline.Augment) and a mirrored fundus is simply the other eye, so the
prediction of a flipped or rotated picture, flipped or rotated back, is as good an answer as the prediction of the picture itself.
Running several views and merging them steadies the mask and gives a spread that covers the whole network, not only the shape
latent (uncertainty.py varies the latent alone: both U-Nets and the ROI are deterministic there).

A view code c in 0..7 is defined on a 2-D array `a` by numpy:
    t = a.T if c & 4 else a;  rows of t reversed if c & 2;  then columns reversed if c & 1
so 0 is the identity, 1 the horizontal flip, 2 the vertical flip, 3 the half turn and 4..7 the transposing ones (4 the transpose,
5 and 6 the quarter turns, 7 the anti-transpose).  The inverse of c swaps bits 0 and 1 when bit 2 is set.

This module is the host side (numpy only): the group, the named sets of `parse`, and `merge_host`, the specification of the fused
merge launch (ops.views_merge, csrc/views.hip).  The device path sits beside it as uncertainty.shape_samples_host's does.
"""
import numpy as np

NAMED = {"id": (0,), "hflip": (0, 1), "flips": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}
MAX_VIEWS = 8
MAX_MAPS = 64                                   # V * K: the votes are a byte and the per-sample post-processing is one set of launches


def _check_code(c):
    if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) <= 7:
        raise ValueError("a view code is an integer in 0..7 (got %r)" % (c,))
    return int(c)


def inverse(c):
    """The code of the inverse view: bits 0 and 1 swapped when bit 2 is set (the quarter turns are each other's inverse)."""
    c = _check_code(c)
    return c if not c & 4 else 4 | ((c & 1) << 1) | ((c >> 1) & 1)


def view_host(a, c):
    """The view c of `a`, acting on its last two axes (a numpy view: nothing is copied)."""
    c = _check_code(c)
    a = np.asarray(a)
    if c & 4:
        a = np.swapaxes(a, -1, -2)
    if c & 2:
        a = a[..., ::-1, :]
    if c & 1:
        a = a[..., ::-1]
    return a


def unview_host(a, c):
    """The inverse of view_host(., c): unview_host(view_host(x, c), c) is x."""
    c = _check_code(c)
    a = np.asarray(a)
    if c & 1:
        a = a[..., ::-1]
    if c & 2:
        a = a[..., ::-1, :]
    if c & 4:
        a = np.swapaxes(a, -1, -2)
    return a


def parse(spec):
    """A view specification -> the tuple of codes, or None for no views.  None / "none" -> None; a named set ("id", "hflip",
    "flips", "d4"); a comma list of codes ("0,3,5") or a sequence of integers.  The codes must be distinct, with 0 (the picture
    itself) first; anything else raises ValueError."""
    if spec is None:
        return None
    if isinstance(spec, str):
        s = spec.strip().lower()
        if s == "none":
            return None
        if s in NAMED:
            return NAMED[s]
        try:
            codes = [int(p) for p in s.split(",")]
        except ValueError:
            raise ValueError("views: %r is neither none, %s nor a comma list of codes 0..7" % (spec, ", ".join(NAMED))) from None
    else:
        try:
            codes = list(spec)
        except TypeError:
            raise ValueError("views: %r is neither a name, a comma list nor a sequence of codes" % (spec,)) from None
    codes = tuple(_check_code(c) for c in codes)
    if not 1 <= len(codes) <= MAX_VIEWS or len(set(codes)) != len(codes) or codes[0] != 0:
        raise ValueError("views: the codes must be distinct, 1 to 8 of them, with 0 first (got %r)" % (codes,))
    return codes


def merge_host(logits, codes, threshold=0.75):
    """The specification of wtpse_views_merge.  logits [V,B,K,H,W] (H == W), each view's maps in that view's own frame; codes: V view
    codes.  With s = v * K + k the sample index:
      "logits" [B,V*K,H,W]  unview_host of the input maps: a pure permutation, in the input's dtype
      "mean", "std" [B,H,W] float64 running Welford update over p_s = sigmoid(logit_s) in order of s, population standard deviation
                            (the recurrence of uncertainty.shape_samples_host: equal samples give exactly 0)
      "votes" [B,H,W]       uint8, #{s: p_s > threshold}
      "mean_logit" [B,H,W]  float32: the un-viewed float32 logits summed in order of s, starting from the first, one float32 addition
                            each, times float32(1) / float32(V*K) — no fused multiply-add anywhere; the device matches it bit for bit."""
    logits = np.asarray(logits)
    codes = [_check_code(c) for c in codes]
    if logits.ndim != 5 or logits.shape[0] != len(codes) or logits.shape[3] != logits.shape[4]:
        raise ValueError("merge_host: logits must be [V,B,K,S,S] with V = %d codes (got %s)" % (len(codes), logits.shape))
    V, B, K, S, _ = logits.shape
    if not (1 <= V <= MAX_VIEWS and K >= 1 and V * K <= MAX_MAPS):
        raise ValueError("merge_host: 1 <= V <= 8 and V * K <= 64 (got V = %d, K = %d)" % (V, K))
    out = np.empty((B, V * K, S, S), logits.dtype)
    for v, c in enumerate(codes):
        out[:, v * K:(v + 1) * K] = unview_host(logits[v], c)
    mean, m2 = np.zeros((B, S, S), np.float64), np.zeros((B, S, S), np.float64)
    votes = np.zeros((B, S, S), np.int64)
    acc = None
    for s in range(V * K):
        l32 = out[:, s].astype(np.float32)
        acc = l32.copy() if acc is None else (acc + l32).astype(np.float32)
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-out[:, s].astype(np.float64)))
        d = p - mean
        mean = mean + d / (s + 1)
        m2 = m2 + d * (p - mean)
        votes += p > threshold
    inv = np.float32(1.0) / np.float32(V * K)
    return {"logits": out, "mean": mean, "std": np.sqrt(np.maximum(m2, 0.0) / (V * K)), "votes": votes.astype(np.uint8),
            "mean_logit": (acc * inv).astype(np.float32)}
