"""tests/pyr_ref.py (the checker of test_pyramid_ingest_gpu.py) against the CPU oracle,
and the tile conditions its size lists are meant to meet."""
import os
import re

import numpy as np
import pytest

import pyr_ref

KERNELS_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mcmtt_opticalflow_amd", "csrc",
                         "psn_lk_kernels.h")


@pytest.mark.parametrize("cap", pyr_ref.CAPS)
def test_pyr_ref_is_the_oracle_pyramid(oracle_mod, cap):
    sizes = pyr_ref.sweep_sizes(cap) + [(w, h) for w, h, c in pyr_ref.RAW_FRAMES if c == cap]
    for w, h in sizes:
        img = np.random.default_rng(1000 * w + h).integers(0, 256, (h, w), dtype=np.uint8)
        want = oracle_mod.build_pyramid(img, cap + 1)
        got = pyr_ref.pyramid(img, cap)
        assert len(got) == len(want) == cap + 1
        for l, (g, r) in enumerate(zip(got, want)):
            assert g.shape == r.shape == ((h + (1 << l) - 1) >> l, (w + (1 << l) - 1) >> l), (w, h, l)
            np.testing.assert_array_equal(g, r, err_msg=f"{w}x{h} level {l}")


def test_pyr_ref_flat_and_extremes(oracle_mod):
    """All 0, all 255 (the rounding's upper end) and a checkerboard on 2-pixel levels."""
    for img in (np.zeros((9, 7), np.uint8), np.full((9, 7), 255, np.uint8), np.full((2, 2), 255, np.uint8),
                (np.indices((6, 2)).sum(0) % 2 * 255).astype(np.uint8)):
        for g, r in zip(pyr_ref.pyramid(img, 3), oracle_mod.build_pyramid(img, 4)):
            np.testing.assert_array_equal(g, r)


def test_gray_is_the_oracle_bgr2gray(oracle_mod):
    rng = np.random.default_rng(3)
    bgr = rng.integers(0, 256, (67, 53, 3), dtype=np.uint8)
    ends = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)], np.uint8)
    bgr[0, :8] = ends  # 0 and 255 in every channel, every combination
    bgr[1, :3] = [[1, 254, 0], [255, 0, 1], [128, 127, 129]]
    want = oracle_mod.bgr2gray(bgr)
    got = pyr_ref.gray(bgr)
    assert got.dtype == np.uint8 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    assert got[0, 0] == 0 and got[0, 7] == 255
    for g, r in zip(pyr_ref.pyramid(bgr, 2), oracle_mod.build_pyramid(want, 3)):
        np.testing.assert_array_equal(g, r)


def test_tile_constants_are_the_build_defaults():
    """The size lists are placed around T * 2^cap: a changed default tile moves the edges away from them."""
    T, T_DEEP = 8, 4  # tops up to 4, top 5
    src = open(KERNELS_H).read()
    assert re.search(r"^#define PSN_PYR_TILE (\d+)\s*$", src, re.M).group(1) == str(T)
    assert re.search(r"constexpr int kPyrTileDeep = (\d+);", src).group(1) == str(T_DEEP)
    assert re.search(r"constexpr int kPyrMaxTop = (\d+);", src).group(1) == str(max(pyr_ref.CAPS))
    assert re.search(r"pyr_tile_edge\(int top\) \{ return top <= 4 \? kPyrTile : kPyrTileDeep; \}", src)
    assert (pyr_ref.TILE, pyr_ref.TILE_DEEP, pyr_ref.DEEP_TOP) == (T, T_DEEP, 5)
    assert [pyr_ref.period(c) for c in range(6)] == [64, 16, 32, 64, 128, 128]


@pytest.mark.parametrize("cap", range(1, 6))
def test_sweep_sits_on_the_tile_edges(cap):
    T = 8 if cap <= 4 else 4
    P = T << cap
    sizes = pyr_ref.sweep_sizes(cap)
    widths, heights = {w for w, _ in sizes}, {h for _, h in sizes}
    for n in (P - 1, P, P + 1, P + 2, 2 * P - 1, 2 * P + 1):
        assert n in widths and n in heights, n
    assert {1, 2, 3, 4, 5, 7, 8, 9} <= widths and {1, 2, 3, 4, 5, 7, 8, 9} <= heights
    assert any(h == 1 for _, h in sizes) and any(w == 3 for w, _ in sizes)  # strips both ways
    assert sum(pyr_ref.sweep_is_bgr(i) for i in range(len(sizes))) >= len(sizes) // 3


def test_raw_frames_have_interior_tiles():
    """A frame with a fully interior top-level tile (3 tiles each way at least) whose width is no
    multiple of 4, and one for the deep tile (T = 4, top 5)."""
    got = {(w, h, cap): pyr_ref.interior_tiles(w, h, cap) for w, h, cap in pyr_ref.RAW_FRAMES}
    for (w, h, cap), (ix, iy, tx, ty) in got.items():
        assert tx >= 3 and ty >= 3, (w, h, cap)
    assert any(ix and iy and w % 4 for (w, h, cap), (ix, iy, _, _) in got.items())
    assert any(ix and iy and cap == 5 for (w, h, cap), (ix, iy, _, _) in got.items())
    assert got[(261, 203, 3)][:2] == (2, 2) and got[(150, 131, 2)][:2] == (3, 3)
    assert got[(300, 270, 5)][:2] == (1, 0) and got[(300, 290, 5)][:2] == (1, 1)
    # the layouts: which take the dword path (base and stride both multiples of 4)
    for w, _, _ in pyr_ref.RAW_FRAMES:
        for ch in (1, 3):
            dword = [lead % 4 == 0 and pyr_ref.raw_stride(w, ch, pad) % 4 == 0 for lead, pad in pyr_ref.RAW_LAYOUTS]
            assert dword[1:4] == [False, False, False] and dword[4], (w, ch)
            assert pyr_ref.raw_stride(w, ch, "mult4") % 4 == 0 and pyr_ref.raw_stride(w, ch, "odd") % 2 == 1
            assert all(pyr_ref.raw_stride(w, ch, pad) >= w * ch for _, pad in pyr_ref.RAW_LAYOUTS)
