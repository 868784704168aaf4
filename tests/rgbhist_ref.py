"""numpy restatement of Associator3D's appearance feature, the checker of
test_appearance.py and test_rgbhist_gpu.py (a helper module, no tests here).

Crop: PSN_Rect::cropWithSize (PSNWhere_Types.h:146-153), cv::Rect's (int) casts
(:181), the four clamps of PSNWhere_Associator3D.cpp:1161-1164; an empty crop
is reported as (0, 0, 0, 0). Histogram: GetRGBFeature (:2542-2556) over
psn::histogram (PSNWhere_Utils.cpp:445-460): per channel 16 bins of value >> 4
over the crop's pixels, concatenated R, G, B of a BGR frame. Feature:
count * (1.0 / n_pixels), 0.0 for an empty crop.
"""
import numpy as np

INT_MAX, INT_MIN = 2**31 - 1, -2**31


def _trunc(v: float) -> int:
    """(int)v; beyond the int range the C ABI saturates."""
    if v >= INT_MAX:
        return INT_MAX
    if v <= INT_MIN:
        return INT_MIN
    return int(v)


def appearance_rect(box, W: int, H: int):
    bx, by, bw, bh = (float(v) for v in box)
    cx, cy = max(0.0, bx), max(0.0, by)
    cw, ch = min(W - cx - 1, bw), min(H - cy - 1, bh)
    x, y, w, h = _trunc(cx), _trunc(cy), _trunc(cw), _trunc(ch)
    if x < 0:
        x = 0
    if y < 0:
        y = 0
    if x + w > W:
        w = W - x
    if y + h > H:
        h = H - y
    if w <= 0 or h <= 0:
        return (0, 0, 0, 0)
    return (x, y, w, h)


def clip_rect(rect, W: int, H: int):
    """The clipping psn_lk_box_histograms applies to an integer rect (the four clamps)."""
    x, y, w, h = (int(v) for v in rect)
    x, y = max(x, 0), max(y, 0)
    if x + w > W:
        w = W - x
    if y + h > H:
        h = H - y
    return (0, 0, 0, 0) if w <= 0 or h <= 0 else (x, y, w, h)


def hist_counts(bgr: np.ndarray, rect) -> np.ndarray:
    """48 uint32 counters R[16] G[16] B[16] of rect = (x, y, w, h) inside the BGR frame."""
    x, y, w, h = rect
    if w <= 0 or h <= 0:
        return np.zeros(48, np.uint32)
    patch = bgr[y:y + h, x:x + w]
    assert patch.shape[:2] == (h, w), "rect outside the frame"
    return np.concatenate([np.bincount(patch[..., c].ravel() >> 4, minlength=16) for c in (2, 1, 0)]).astype(np.uint32)


def features(counts: np.ndarray, n_pixels: int) -> np.ndarray:
    if n_pixels == 0:
        return np.zeros(48, np.float64)
    return counts.astype(np.float64) * (np.float64(1.0) / np.float64(n_pixels))
