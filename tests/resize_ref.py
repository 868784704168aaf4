"""numpy restatement of the ingest resize at a reduced optical-flow scale, the
checker of test_scale.py and test_scale_gpu.py (a helper module, no tests here).

cv::resize(gray, dst, Size(w * s, h * s)) of PSNWhere_Tracker2D.cpp:260-262:
OpenCV 2.4.6 resize(..., INTER_LINEAR) for CV_8UC1 [OCV246
imgproc/src/imgwarp.cpp], restated from its source (OpenCV is not available to
this project's tests, so no test pins this against the library):

  scale = 1.0 / ((double)dst / src)                          double
  f = (float)((d + 0.5) * scale - 0.5); s = floor(f); f -= s  float
  columns only: s < 0 -> s = 0, f = 0; s >= src - 1 -> s = src - 1, f = 0
  c0 = cvRound((1.f - f) * 2048), c1 = cvRound(f * 2048)      float products, ties to even
  D = S[sx] * a0 + S[min(sx + 1, w - 1)] * a1                 int
  rows clamp(sy, 0, h - 1) and clamp(sy + 1, 0, h - 1)
  out = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2
"""
import numpy as np


def scaled_size(width: int, height: int, scale: float):
    """(int)((double)width * scale), (int)((double)height * scale) (:260)."""
    return int(np.float64(width) * np.float64(scale)), int(np.float64(height) * np.float64(scale))


def plan(src: int, dst: int, is_x: bool):
    """(ofs (dst,) int32, coef (dst, 2) int16) of one axis."""
    scale = np.float64(1.0) / (np.float64(dst) / np.float64(src))
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if is_x:
        lo = s < 0
        s[lo], f[lo] = 0, 0
        hi = s >= src - 1
        s[hi], f[hi] = src - 1, 0
    one, k = np.float32(1.0), np.float32(2048.0)
    c0 = np.rint(((one - f) * k).astype(np.float32).astype(np.float64)).astype(np.int16)
    c1 = np.rint((f * k).astype(np.float32).astype(np.float64)).astype(np.int16)
    return s, np.stack([c0, c1], axis=1)


def resize_to(gray: np.ndarray, lw: int, lh: int) -> np.ndarray:
    gray = np.asarray(gray)
    assert gray.ndim == 2 and gray.dtype == np.uint8
    h, w = gray.shape
    xo, xc = plan(w, lw, True)
    yo, yc = plan(h, lh, False)
    S = gray.astype(np.int32)
    x1 = np.minimum(xo + 1, w - 1)
    D = S[:, xo] * xc[:, 0].astype(np.int32)[None, :] + S[:, x1] * xc[:, 1].astype(np.int32)[None, :]  # (h, lw)
    r0, r1 = np.clip(yo, 0, h - 1), np.clip(yo + 1, 0, h - 1)
    b0, b1 = yc[:, 0].astype(np.int32)[:, None], yc[:, 1].astype(np.int32)[:, None]
    out = (((b0 * (D[r0] >> 4)) >> 16) + ((b1 * (D[r1] >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def resize(gray: np.ndarray, scale: float) -> np.ndarray:
    """The gray frame of the ring at `scale` (the LK frame)."""
    h, w = np.asarray(gray).shape
    lw, lh = scaled_size(w, h, scale)
    return resize_to(gray, lw, lh)
