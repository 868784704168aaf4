"""The level-0 window gradients of a point as the LK kernels see them, and their per-lane
sums, on the CPU: the preconditions of the tests that force the ordered A chains
(tests/test_lk_fw_gpu.py, tests/test_lk_lg_fallback_gpu.py)."""
import numpy as np


def window_grads(oracle_mod, img, x, y, win):
    """(gx, gy) of the window at point (x, y): the oracle's Scharr gradients with the
    window's 14-bit bilinear weights, edge-padded; None when the window is outside."""
    w, h = win
    H, W = img.shape
    pad = max(w, h) + 32
    g = np.pad(oracle_mod.scharr(img).astype(np.int64), ((pad, pad), (pad, pad), (0, 0)), mode="edge")
    px = np.float32(x) - np.float32((w - 1) * 0.5)
    py = np.float32(y) - np.float32((h - 1) * 0.5)
    ix, iy = int(np.floor(px)), int(np.floor(py))
    if ix < -w or iy < -h or ix > W or iy > H:
        return None
    a, b = float(px - np.float32(ix)), float(py - np.float32(iy))
    w00, w01, w10 = round((1 - a) * (1 - b) * 16384), round(a * (1 - b) * 16384), round((1 - a) * b * 16384)
    w11 = 16384 - w00 - w01 - w10
    r = g[iy + pad:iy + pad + h + 1, ix + pad:ix + pad + w + 1]
    v = (r[:-1, :-1] * w00 + r[:-1, 1:] * w01 + r[1:, :-1] * w10 + r[1:, 1:] * w11 + 8192) >> 14
    return v[..., 0], v[..., 1]


def lane_sums(oracle_mod, img, pts, win):
    """Per point the largest per-lane (x & 3) sum of Ix^2, of Iy^2 and of |Ix Iy| over
    the level-0 window."""
    out = []
    for x, y in pts:
        gr = window_grads(oracle_mod, img, x, y, win)
        if gr is None:
            continue
        gx, gy = gr
        out.append([max(int(t[:, l::4].sum()) for l in range(4)) for t in (gx * gx, gy * gy, np.abs(gx * gy))])
    return np.array(out, np.int64)
