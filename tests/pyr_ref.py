"""A numpy restatement of the ingest and the pyramid (cv::cvtColor BGR2GRAY, then
cv::pyrDown per level as buildOpticalFlowPyramid calls it), and the frame sizes
of tests/test_pyramid_ingest_gpu.py.

Per axis, output i of a length-n axis is sum_k [1 4 6 4 1][k] * in[refl101(2i + k - 2, n)],
the output length is (n + 1) // 2; both axes together are rounded once,
(sum + 128) >> 8. refl101 loops until the index is inside (a 2-pixel level reflects
more than once); n == 1 gives 0. tests/test_pyr_ref.py holds this against
oracle/lk_oracle.c for every (size, cap) below.
"""
import numpy as np

TAPS = np.array([1, 4, 6, 4, 1], np.int64)


def refl101(p: int, n: int) -> int:
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def _axis_index(n: int) -> np.ndarray:
    """((n + 1) // 2, 5) source indices of one axis."""
    return np.array([[refl101(2 * i + k - 2, n) for k in range(5)] for i in range((n + 1) // 2)], np.int64)


def pyr_down(img: np.ndarray) -> np.ndarray:
    h, w = img.shape
    a = img.astype(np.int64)
    rows = (a[:, _axis_index(w)] * TAPS).sum(axis=2)           # (h, ow)
    both = (rows[_axis_index(h), :] * TAPS[None, :, None]).sum(axis=1)  # (oh, ow)
    return ((both + 128) >> 8).astype(np.uint8)


def gray(bgr: np.ndarray) -> np.ndarray:
    """RGB2Gray<uchar> of a (h, w, 3) BGR frame."""
    b, g, r = (bgr[..., c].astype(np.int64) for c in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def pyramid(img: np.ndarray, cap: int) -> list:
    """Levels 0..cap of a gray (h, w) or BGR (h, w, 3) frame."""
    lv = [gray(img) if img.ndim == 3 else np.ascontiguousarray(img, dtype=np.uint8)]
    for _ in range(cap):
        lv.append(pyr_down(lv[-1]))
    return lv


# ---- the sizes of the device sweep -------------------------------------------------

TILE, TILE_DEEP, DEEP_TOP = 8, 4, 5  # PSN_PYR_TILE, kPyrTileDeep: top-level tile edge, from which top
CAPS = range(0, 6)


def tile_edge(cap: int) -> int:
    return TILE if cap < DEEP_TOP else TILE_DEEP


def period(cap: int) -> int:
    """P: the level-0 pixels one top-level tile spans (cap 0: the 64 x 64 ingest tiles)."""
    return 64 if cap == 0 else tile_edge(cap) << cap


def edge_lengths(cap: int) -> list:
    P = period(cap)
    return [1, 2, 3, 4, 5, 7, 8, 9, P - 1, P, P + 1, P + 2, 2 * P - 1, 2 * P + 1, 2 * P + 5]


def sweep_sizes(cap: int) -> list:
    """(w, h) of the size sweep at `cap`: every edge length as a width with heights
    {1, 5, P + 1} and as a height with widths {3, P + 2}."""
    P = period(cap)
    out = []
    for n in edge_lengths(cap):
        out += [(n, h) for h in (1, 5, P + 1)] + [(w, n) for w in (3, P + 2)]
    return list(dict.fromkeys(out))


def sweep_is_bgr(index: int) -> bool:
    """A third of the sweep's sizes are pushed as BGR as well."""
    return index % 3 == 1


# Raw-source frames (w, h, cap): top-level tiles whose level-0 region lies inside the
# frame (3 tiles each way at least). 300 x 270 has such tiles in x only at cap 5 (its
# region is 221 rows from row 66); 300 x 290 has them both ways.
RAW_FRAMES = [(261, 203, 3), (150, 131, 2), (300, 270, 5), (300, 290, 5)]
# (lead bytes, row padding): aligned and contiguous; an odd stride; a misaligned base on a
# stride that is a multiple of 4; both off. "align": lead 0, rows padded up to a multiple of 4
# (the dword path for the widths above that are no multiple of 4).
RAW_LAYOUTS = [(0, 0), (0, "odd"), (1, "mult4"), (3, 5), (0, "align")]


def raw_stride(w: int, ch: int, pad) -> int:
    row = w * ch
    if pad == "odd":
        return row + 1 if row % 2 == 0 else row + 2
    if pad == "mult4":
        return (row + 4 + 3) & ~3
    if pad == "align":
        return (row + 3) & ~3
    return row + pad


def interior_tiles(w: int, h: int, cap: int) -> tuple:
    """Top-level tiles per axis whose level-0 region [s0, s0 + n0) -- widened in x to the
    dwords it is loaded as -- lies inside a w x h frame: (count in x, count in y, tiles x, tiles y)."""
    T, span = tile_edge(cap), 1 << cap
    n0 = span * T + 3 * (span - 1)

    def count(n, dwords):
        tiles = (((n + span - 1) >> cap) + T - 1) // T
        k = 0
        for b in range(tiles):
            s0 = span * T * b - 2 * (span - 1)
            if dwords:
                a0 = s0 & ~3
                end = a0 + 4 * ((s0 - a0 + n0 + 3) >> 2)
            else:
                end = s0 + n0
            k += s0 >= 0 and end <= n
        return k, tiles

    (ix, tx), (iy, ty) = count(w, True), count(h, False)
    return ix, iy, tx, ty
