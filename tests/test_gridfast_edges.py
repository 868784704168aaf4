"""The GridFAST edge cases (tests/gridfast_cases.py) on the CPU.

Part one: every case's precondition holds on the oracle, so each case reaches the
kernel branch it is named for (strip 16, list_cap 0, both pass counts on the same
pixels, ties at the cut carried across seams and thread runs, equal responses at a
seam / roi edge / cell border, the 8-bit score's extremes, the select kernel's rank
and sort paths around their boundary, tiny cells).

Part two: `brute_gridfast`, a numpy restatement of the grid layer on top of
test_gridfast.brute_fast (cell bounds floor(i * h / rows), FAST per cell sub-image, the
roi mask, keepStrongest with ties to the earlier keypoint in row-major order, cells in
grid order), equals the oracle on the small cases: the second opinion on the grid, cut
and mask logic for exactly the inputs on which tests/test_gridfast_edges_gpu.py trusts
the oracle."""
import numpy as np
import pytest

import gridfast_cases as gc
from test_gridfast import brute_fast


@pytest.mark.parametrize("case", gc.ALL, ids=gc.case_id)
def test_precondition(oracle_mod, case):
    case.pre(oracle_mod, case)
    w, h = case.size
    assert w * h <= 170_000 and len(case.rois) <= 64


def test_geometry_restatement_known_answers():
    """The plan and the pass rule on the figures of csrc/psn_lk_readers.cpp's comment."""
    assert gc.plan(1920, 1080, (4, 4), [(0, 0, 1919, 1079)]) == (474, 32, 4096)
    assert gc.plan(1030, 70, (2, 1), [(0, 0, 1030, 70)]) == (1024, 16, 4096)
    assert gc.lds_bytes(1024, 16, 4096) == 76016 and gc.lds_bytes(1024, 32, 4096) > gc.MAX_LDS
    # strip 16 from a region wider than 768 px; strip 8 and a smaller list at no width up to kGfMaxRegionW
    assert gc.plan(4096, 100, (1, 4), [(0, 0, 768, 100)])[1] == 32 and gc.plan(4096, 100, (1, 4), [(0, 0, 769, 100)])[1] == 16
    assert min(gc.plan(4096, 100, (1, 4), [(0, 0, rw, 100)])[1:] for rw in range(1, 1025)) == (16, 4096)
    assert gc.plan(4100, 40, (1, 4), [(0, 0, 4099, 39)]) == (1019, 16, 0)
    assert gc.region(300, 300, (2, 2), (0, 0, 299, 299), (1, 1)) == (153, 153, 297, 297)
    assert gc.region(300, 300, (2, 2), (0, 0, 150, 150), (1, 1)) is None
    assert gc.is_single((5, 5, 133, 133), True, 4096) and not gc.is_single((5, 5, 134, 133), True, 4096)
    assert not gc.is_single((5, 5, 133, 133), False, 4096) and not gc.is_single((5, 5, 7, 7), True, 0)


def test_shuffle_hash_restatement(oracle_mod):
    L = oracle_mod.lib()
    for seed, roi in ((0, 0), (7, 3), (0xffffffff, 63)):
        assert gc.shuffle_keys(seed, roi, 64).tolist() == [L.oracle_gridfast_key(seed, roi, k) for k in range(64)]


def test_select_cases_reach_both_paths(oracle_mod):
    """n = 4096 for every cap and seed of the select cases. The rank path takes the caps up
    to 496, at cap 511 a set of exactly 512 keys (its limit, seed 0) and of 513 (the smallest
    sorted set, seed 3); the sort every larger cap. Over the seeds the cap-th key falls into
    at least three histogram bins."""
    c = gc.select_case(100, 0)
    c.pre(oracle_mod, c)
    ns = {(cap, seed): gc.rank_set(seed, 0, 4096, cap) for cap in gc.SELECT_CAPS for seed in gc.SELECT_SEEDS}
    for (cap, seed), n in ns.items():
        assert min(cap, 4096) <= n <= 4096
        assert n <= gc.RANK_MAX if cap <= 496 else n > gc.RANK_MAX if cap >= 513 else True, (cap, seed, n)
    assert ns[511, 0] == gc.RANK_MAX and ns[511, 3] == gc.RANK_MAX + 1
    assert ns[4095, 0] == ns[5000, 0] == 4096
    for cap in (100, 496, 600):
        bins = {int(np.sort(gc.shuffle_keys(seed, 0, 4096))[cap - 1]) >> 24 for seed in gc.SELECT_SEEDS}
        assert len(bins) >= 3, bins
    m = gc.select_mixed(100, 5)
    m.pre(oracle_mod, m)
    # a key of rank cap is in the ranked set of the capped roi before the empty one: a rank test
    # off by one would write it into the empty roi's first row (test_device_call_writes_only_its_rows)
    assert all(gc.rank_set(5, 0, 4096, cap) > cap for cap in (100, 1))


def test_sets_case_is_live(oracle_mod):
    a, b = gc.sets_case()
    assert a.size == b.size and len(a.rois) < 64 < len(a.rois) + len(b.rois)
    for c in (a, b):
        tot = gc.reference(oracle_mod, c)[1]
        assert (tot > c.cap).any() and (tot == 0).any() and ((tot > 0) & (tot < c.cap)).any()


# ------------------------------------------------- the grid layer, restated in numpy

def brute_cells(img, threshold, nonmax, grid):
    """FAST per cell sub-image: {(i, j): (n, 3) frame x, y, response in row-major order}."""
    h, w = img.shape
    t = min(max(threshold, 0), 255)
    out = {}
    for i in range(grid[0]):
        r0, r1 = i * h // grid[0], (i + 1) * h // grid[0]
        for j in range(grid[1]):
            c0, c1 = j * w // grid[1], (j + 1) * w // grid[1]
            out[i, j] = brute_fast(img[r0:r1, c0:c1], t, nonmax) + np.int32([c0, r0, 0])
    return out


def brute_gridfast(cells, roi, max_total, grid):
    """(n, 3) x, y, response: per cell in grid order, the keypoints inside the roi, the
    max_total // cells strongest of them (ties: the earlier), in row-major order."""
    ncell = grid[0] * grid[1]
    if max_total < ncell:
        return np.zeros((0, 3), np.int32)
    out = []
    for i in range(grid[0]):
        for j in range(grid[1]):
            k = cells[i, j]
            k = k[(k[:, 0] >= roi[0]) & (k[:, 0] < roi[0] + roi[2]) & (k[:, 1] >= roi[1]) & (k[:, 1] < roi[1] + roi[3])]
            best = sorted(range(len(k)), key=lambda q: (-k[q, 2], q))[:max_total // ncell]
            out.append(k[sorted(best)])
    return np.concatenate(out)


@pytest.mark.parametrize("case", gc.SMALL, ids=gc.case_id)
def test_brute_gridfast_matches_oracle(oracle_mod, case):
    w, h = case.size
    assert w <= 100 and h <= 100
    cells = brute_cells(case.frame, case.threshold, case.nonmax, case.grid)
    for roi in case.rois:
        np.testing.assert_array_equal(gc.keypoints(oracle_mod, case, roi), brute_gridfast(cells, roi, case.max_total, case.grid),
                                      err_msg=f"{case.name} roi {roi}")


def test_small_cases_cover_the_grid_layer():
    names = {c.name for c in gc.SMALL}
    assert {"seams-small", "roi-edge-stronger-outside", "cell-border", "threshold-5", "binary-threshold254", "tiny28",
            "tiny28-every-cell", "per-cell-0", "lattice100-cut", "lattice100-no-nonmax"} <= names
