"""Edge cases of the GridFAST device kernels (csrc/psn_gridfast.hip): the case table,
the image recipes and the (cached) oracle outputs shared by tests/test_gridfast_edges.py
(CPU) and tests/test_gridfast_edges_gpu.py.

A case is a frame, rois, detector settings, a shuffle seed and a precondition. The
precondition is a predicate on the oracle's output (oracle/gridfast_oracle.c) and the
geometry of the launch: it proves that the case reaches the kernel branch it is named
for, so a change to a recipe cannot silently empty it. The geometry (`plan`, `region`,
`is_single`) restates the host plan of csrc/psn_lk_readers.cpp and the region / pass
rule of gridfast_cell_kernel; `shuffle_keys` / `rank_set` restate the select kernel's
hash and its histogram-bin search.

Most frames are dot lattices: background 20 with isolated bright pixels whose height
over the background comes from a small set, so that a dot of height d is a corner of
response d - 1 and whole classes of keypoints tie exactly."""
from dataclasses import dataclass, field
from typing import Callable

import numpy as np

BG = 20
HEIGHTS = (60, 80, 100)  # responses 59 / 79 / 99
HUGE = 1 << 18           # a max_total that no cell's cut reaches
MAX_LDS = 96 * 1024      # kGfMaxLds
RANK_MAX = 512           # kGfRankMax
THREADS = 256            # kGfThreads


# ---------------------------------------------------------------- image recipes

def lattice(w, h, seed, pitch=4, off=(2, 2), heights=HEIGHTS):
    """Isolated dots every `pitch` px from `off` (x, y), heights drawn from `heights`."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), BG, np.uint8)
    ys, xs = np.arange(off[1], h, pitch), np.arange(off[0], w, pitch)
    img[np.ix_(ys, xs)] = BG + rng.choice(heights, (len(ys), len(xs)))
    return img


def quantised_noise(w, h, seed):
    """Five grey values at random: dense corners, equal responses on neighbouring pixels."""
    return np.random.default_rng(seed).choice(np.uint8([0, 64, 128, 192, 255]), (h, w))


def dots(w, h, pts, bg=BG):
    """Background `bg` with the pixels pts = [(x, y, value), ...]."""
    img = np.full((h, w), bg, np.uint8)
    for x, y, v in pts:
        img[y, x] = v
    return img


# -------------------------------------------- the launch geometry, restated

def lds_bytes(rw_max, strip, list_cap):
    pc, sc = (rw_max + 8 + 3) & ~3, rw_max + 2
    return (strip + 8) * pc + (((strip + 2) * sc + 15) & ~15) + ((strip * rw_max + 15) & ~15) + 4 * list_cap


def plan(w, h, grid, rois):
    """(rw_max, strip, list_cap) of one launch over `rois` (at most 64)."""
    assert len(rois) <= 64
    cell_w = -(-w // grid[1]) - 6
    rw_max = max([1] + [min(r[2], cell_w) for r in rois])
    list_cap = 4096 if w <= 4096 and h <= 4096 else 0
    strip = 32
    while strip > 8 and lds_bytes(rw_max, strip, list_cap) > MAX_LDS:
        strip >>= 1
    while list_cap > 0 and lds_bytes(rw_max, strip, list_cap) > MAX_LDS:
        list_cap >>= 1
    return rw_max, strip, list_cap


def region(w, h, grid, roi, cell):
    """The part (ax0, ay0, ax1, ay1) of cell (i, j)'s detection region inside the roi, or None."""
    (i, j), (rows, cols) = cell, grid
    dy0, dy1 = i * h // rows + 3, (i + 1) * h // rows - 3
    dx0, dx1 = j * w // cols + 3, (j + 1) * w // cols - 3
    x0, y0 = max(roi[0], 0), max(roi[1], 0)
    x1, y1 = min(roi[0] + roi[2], w), min(roi[1] + roi[3], h)
    ax0, ax1, ay0, ay1 = max(dx0, x0), min(dx1, x1), max(dy0, y0), min(dy1, y1)
    if roi[2] <= 0 or roi[3] <= 0 or ax0 >= ax1 or ay0 >= ay1:
        return None
    return ax0, ay0, ax1, ay1


def is_single(reg, nonmax, list_cap):
    """gridfast_cell_kernel's `single`: the region's keypoints surely fit the LDS list."""
    ax0, ay0, ax1, ay1 = reg
    return bool(nonmax) and ((ax1 - ax0 + 1) // 2) * ((ay1 - ay0 + 1) // 2) <= list_cap


def _mix32(x):
    x = x.astype(np.uint64)
    m = np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    return x


def shuffle_keys(seed, roi, n):
    """The 32-bit shuffle hashes of candidates 0..n-1 of roi `roi` (lowbias32, twice)."""
    h0 = _mix32(np.array([(seed + 0x9e3779b9 * (roi + 1)) & 0xffffffff], np.uint64))[0]
    return _mix32(h0 ^ np.arange(n, dtype=np.uint64))


def rank_set(seed, roi, n, cap):
    """How many keys gridfast_select_kernel ranks: those in the top-byte bins up to the
    one that holds the min(n, cap)-th smallest. Above RANK_MAX it sorts all n instead."""
    m = min(n, cap)
    if m <= 0:
        return 0
    top = (shuffle_keys(seed, roi, n) >> np.uint64(24)).astype(np.int64)
    cum = np.cumsum(np.bincount(top, minlength=256))
    return int(cum[np.searchsorted(cum, m)])


# ------------------------------------------------------------------ the case

@dataclass
class Case:
    name: str
    image: Callable[[], np.ndarray]
    rois: list
    pre: Callable = None          # pre(oracle_mod, case): asserts
    threshold: int = 10
    nonmax: bool = True
    max_total: int = 1000
    grid: tuple = (4, 4)
    cap: int = None               # None: max_total (every keypoint comes back)
    seed: int = 0
    _frame: np.ndarray = field(default=None, repr=False)

    def __post_init__(self):
        if self.cap is None:
            self.cap = self.max_total

    @property
    def frame(self):
        if self._frame is None:
            self._frame = np.ascontiguousarray(self.image(), dtype=np.uint8)
            self._frame.setflags(write=False)
        return self._frame

    @property
    def size(self):
        h, w = self.frame.shape
        return w, h

    @property
    def per_cell(self):
        n = self.grid[0] * self.grid[1]
        return self.max_total // n if self.max_total >= n else 0

    def detector(self):
        return dict(threshold=self.threshold, nonmax=self.nonmax, max_total=self.max_total, grid=self.grid)

    def plan(self):
        return plan(*self.size, self.grid, self.rois)


def case_id(c):
    return c.name


def keypoints(o, c, roi, frame=None, **over):
    """The oracle's keypoints of one roi as (n, 3) int rows x, y, response, in its order
    (cells in grid order, row-major inside a cell)."""
    xy, resp = o.gridfast(c.frame if frame is None else frame, roi, **{**c.detector(), **over})
    return np.concatenate([xy.astype(np.int64), resp[:, None].astype(np.int64)], 1).reshape(-1, 3)


def kpset(k):
    return {(int(x), int(y)) for x, y, _ in k}


_refs = {}


def reference(o, c):
    """What psn_gridfast_detect has to return for the case: (points per roi, totals)."""
    if c.name not in _refs:
        pts, tot = o.gridfast_detect(c.frame, c.rois, seed=c.seed, cap=c.cap, **c.detector())
        for a in pts + [tot]:
            a.setflags(write=False)
        _refs[c.name] = (pts, tot)
    return _refs[c.name]


def in_region(k, reg):
    ax0, ay0, ax1, ay1 = reg
    return k[(k[:, 0] >= ax0) & (k[:, 0] < ax1) & (k[:, 1] >= ay0) & (k[:, 1] < ay1)]


# ---------------------------------------------------------- preconditions

def pre_totals(*totals):
    def pre(o, c):
        assert reference(o, c)[1].tolist() == list(totals), reference(o, c)[1]
    return pre


def pre_all(*pres):
    def pre(o, c):
        for p in pres:
            p(o, c)
    return pre


def pre_passes(roi_index, cell, single):
    """Region (roi, cell) takes the single-pass (True) or the two-pass (False) path."""
    def pre(o, c):
        reg = region(*c.size, c.grid, c.rois[roi_index], cell)
        assert reg is not None and is_single(reg, c.nonmax, c.plan()[2]) == single, (reg, c.plan())
        assert len(in_region(keypoints(o, c, c.rois[roi_index]), reg)) > 0
    return pre


def pre_tie_carry(roi_index, cell, single, seam=True):
    """The cell's keepStrongest cut falls strictly inside a tie class; the kept ties lie on
    both sides of a strip seam, at least 3 each, in more than one thread run of a strip
    (two passes) or of the list (single pass); at least 3 ties are dropped. seam False: only
    the cut inside the tie class (a frame too small for the rest)."""
    def pre(o, c):
        roi = c.rois[roi_index]
        reg = region(*c.size, c.grid, roi, cell)
        _, strip, list_cap = c.plan()
        assert is_single(reg, c.nonmax, list_cap) == single
        every = in_region(keypoints(o, c, roi, max_total=HUGE), reg)
        kept = in_region(keypoints(o, c, roi), reg)
        assert len(kept) == c.per_cell < len(every), (len(kept), c.per_cell, len(every))
        t = kept[:, 2].min()
        assert (every[:, 2] > t).sum() < c.per_cell  # the classes above the cut do not fill the cell
        tie_at = np.flatnonzero(every[:, 2] == t)
        ties = every[tie_at]
        need = int((kept[:, 2] == t).sum())
        assert 0 < need and need + 3 <= len(ties), (need, len(ties))
        np.testing.assert_array_equal(kept[kept[:, 2] == t], ties[:need])  # the earlier ones win
        if not seam:
            return
        ax0, ay0, ax1, ay1 = reg
        s = (ties[:need, 1] - ay0) // strip
        assert any((s == i).sum() >= 3 and (s == i + 1).sum() >= 3 for i in range(int(s.max()))), np.bincount(s)
        if single:
            runs = {int(i) // -(-len(every) // THREADS) for i in tie_at[:need]}
        else:
            rw = ax1 - ax0
            runs = set()
            for x, y, _ in ties[:need]:
                y0 = ay0 + (y - ay0) // strip * strip
                n = min(strip, ay1 - y0) * rw
                runs.add((int(y0), int(((y - y0) * rw + x - ax0) // -(-n // THREADS))))
            assert len(runs) > len({y0 for y0, _ in runs})  # two runs of one strip
        assert len(runs) > 1
    return pre


# ------------------------------------------------------------------ the cases

# -- 300 x 300 lattice, grid (2, 2): cells of 1,296 candidates for 1,024 places
def _lat300(seed=1):
    return lambda: lattice(300, 300, seed)


FULL300 = (0, 0, 299, 299)


def _pre_n4096(o, c):
    assert reference(o, c)[1][0] == 4096
    k = keypoints(o, c, c.rois[0])
    assert sorted(set(k[:, 2].tolist())) == [59, 79, 99] and min(np.bincount(k[:, 2])[[59, 79, 99]]) > 500


SELECT_CAPS = (1, 100, 496, 511, 512, 513, 600, 4095, 4096, 5000)
SELECT_SEEDS = (0, 1, 2, 3)
N4096 = Case("lattice300-n4096", _lat300(), [FULL300], max_total=4096, grid=(2, 2),
             pre=pre_all(_pre_n4096, pre_passes(0, (0, 0), False), pre_tie_carry(0, (0, 0), False),
                         pre_tie_carry(0, (1, 1), False)))


def select_case(cap, seed):
    return Case(f"select-cap{cap}-seed{seed}", _lat300(), [FULL300], max_total=4096, grid=(2, 2), cap=cap, seed=seed,
                pre=pre_totals(4096))


# rois of the select launch: 4,096 keypoints, none, 4,096 again, exactly one
SELECT_MIXED_ROIS = [FULL300, (0, 0, 3, 3), FULL300, (5, 5, 2, 2)]


def select_mixed(cap, seed):
    return Case(f"select-mixed-cap{cap}-seed{seed}", _lat300(), SELECT_MIXED_ROIS, max_total=4096, grid=(2, 2),
                cap=cap, seed=seed, pre=pre_totals(4096, 0, 4096, 1))


def _pre_both_paths(cut):
    """The rois lie in cell (0, 0) and take the pass counts of BOTH_SINGLE: a one-pixel step
    in width, height or position moves a roi across the rule. A roi that is not cut holds
    exactly the keypoints of the whole cell that lie in it, whatever its pass count. Both
    pass counts occur among the rois that are cut (cut True) or among those that are not."""
    def pre(o, c):
        lc = c.plan()[2]
        regs = [region(*c.size, c.grid, r, (0, 0)) for r in c.rois]
        assert [is_single(g, c.nonmax, lc) for g in regs] == BOTH_SINGLE
        every = keypoints(o, c, c.rois[-1], max_total=HUGE)
        seen = set()
        for r, g, single in zip(c.rois, regs, BOTH_SINGLE):
            mine, want = in_region(keypoints(o, c, r), g), in_region(every, g)
            assert len(mine) > 0
            if len(want) <= c.per_cell:
                np.testing.assert_array_equal(mine, want)
            else:
                assert len(mine) == c.per_cell
            seen.add((single, len(want) > c.per_cell))
        assert {(True, cut), (False, cut)} <= seen, seen
    return pre


# (5, 5, 128, 128): 64 * 64 = 4096 list entries, the largest single-pass region
BOTH_ROIS = [(5, 5, 128, 128), (5, 5, 129, 128), (5, 5, 128, 129), (4, 5, 129, 128), (6, 5, 127, 128), (0, 0, 100, 100),
             (3, 3, 144, 144)]
BOTH_SINGLE = [True, False, False, False, True, True, False]


def _both(name, image, cut=False, **kw):
    return Case(name, image, BOTH_ROIS, max_total=4096, grid=(2, 2), pre=_pre_both_paths(cut), **kw)


# the noise holds about 380 keypoints per 128 x 128 at threshold 100, 1,100 (a cut) at 40
BOTH = [_both("both-paths-lattice", _lat300(2)),
        _both("both-paths-noise", lambda: quantised_noise(300, 300, 3), threshold=100),
        _both("both-paths-noise-cut", lambda: quantised_noise(300, 300, 3), cut=True, threshold=40)]

# single-pass tie carry: a 100 x 100 region of 625 candidates for 100 places
TIES = [
    Case("ties-single-pass", _lat300(4), [(3, 3, 100, 100), (153, 153, 100, 100)], max_total=400, grid=(2, 2),
         pre=pre_all(pre_tie_carry(0, (0, 0), True), pre_tie_carry(1, (1, 1), True))),
    Case("ties-two-pass-small-cut", _lat300(5), [FULL300], max_total=1600, grid=(2, 2),
         pre=pre_all(pre_tie_carry(0, (0, 0), False), pre_tie_carry(0, (1, 0), False))),
]


def _pre_all_tie(o, c):
    k = keypoints(o, c, c.rois[0], max_total=HUGE)
    assert (k[:, 2] == 0).all() and len(k) == 4 * 1296
    assert reference(o, c)[1][0] == c.max_total
    # the cut keeps the first per_cell candidates of each cell, over several strips
    kept = in_region(keypoints(o, c, c.rois[0]), region(*c.size, c.grid, c.rois[0], (0, 0)))
    np.testing.assert_array_equal(kept, in_region(k, region(*c.size, c.grid, c.rois[0], (0, 0)))[:c.per_cell])
    assert kept[:, 1].max() - 3 > c.plan()[1]


TIES += [Case(f"ties-no-nonmax-{mt}", _lat300(6), [FULL300, (40, 40, 90, 90)], nonmax=False, max_total=mt, grid=(2, 2),
              pre=_pre_all_tie) for mt in (4096, 2000)]

# -- frames wider / taller than 4096: no keypoint list, every region in two passes
WIDE_ROIS = [(0, 0, 4099, 39), (4000, 0, 100, 40), (4090, 10, 10, 20), (1000, 0, 100, 39)]


def _pre_wide(expect_max):
    """list_cap 0 (and, through the width, strip 16); roi 1 would be a single-pass region
    under a 4096-entry list, and holds keypoints up to coordinate expect_max: 4096 does
    not fit the list's 12 bits."""
    def pre(o, c):
        w, h = c.size
        rw_max, strip, list_cap = c.plan()
        assert (rw_max, strip, list_cap) == ((1019, 16, 0) if w > h else (34, 32, 0))
        tot = reference(o, c)[1]
        assert tot[0] == 1000
        axis = 0 if w > h else 1
        cell = (0, 3) if w > h else (3, 0)
        reg = region(w, h, c.grid, c.rois[1], cell)
        assert is_single(reg, True, 4096) and not is_single(reg, True, list_cap)
        k = in_region(keypoints(o, c, c.rois[1]), reg)
        assert k[:, axis].max() == expect_max >= 4094 and tot[2] > 0
        if w > h:  # (the last column of every row; the last rows of a tall cell lose the cut)
            assert keypoints(o, c, c.rois[0])[:, 0].max() == expect_max
    return pre


def _wide(name, image, rois, grid, expect_max):
    return Case(name, image, rois, grid=grid, pre=_pre_wide(expect_max), seed=9)


def _t(rois):
    return [(y, x, h, w) for x, y, w, h in rois]


WIDE = [_wide("wide4100-x4094", lambda: lattice(4100, 40, 7), WIDE_ROIS, (1, 4), 4094),
        _wide("wide4100-x4096", lambda: lattice(4100, 40, 8, off=(0, 2)), WIDE_ROIS, (1, 4), 4096),
        _wide("tall4100-y4096", lambda: lattice(40, 4100, 8, off=(2, 0)), _t(WIDE_ROIS), (4, 1), 4096)]


# -- 1030 x 70, grid (2, 1): region width 1024, strip 16 with the list at 4096
def _pre_1030(o, c):
    assert c.plan() == (1024, 16, 4096) and lds_bytes(1024, 32, 4096) > MAX_LDS
    assert reference(o, c)[1][0] == 1000
    assert keypoints(o, c, c.rois[0])[:, 0].max() >= 1024


W1030 = Case("wide1030-strip16", lambda: lattice(1030, 70, 10), [(0, 0, 1030, 70), (100, 0, 480, 70), (3, 3, 1024, 16)],
             grid=(2, 1), seed=4,
             pre=pre_all(_pre_1030, pre_passes(0, (0, 0), False), pre_passes(1, (0, 0), True), pre_passes(1, (1, 0), True),
                         pre_tie_carry(0, (0, 0), False), pre_tie_carry(1, (0, 0), True), pre_tie_carry(1, (1, 0), True)))


# -- strip seams: equal and unequal responses on vertical and diagonal neighbours
SEAM_HEIGHTS = (31, 32, 33, 64, 65)
SEAM_COLS = {"equal": 20, "upper": 28, "lower": 36, "diag-equal": 44, "diag-lower": 52}


def seam_pairs(ay0, strip, seams, x_off=0):
    """Bright pairs on rows (seam - 1, seam) for seam = ay0 + strip * k: {(kind, k): (upper, lower)}."""
    out = {}
    for k in seams:
        y = ay0 + strip * k
        for kind, x in SEAM_COLS.items():
            x += x_off
            hi, lo = (120, 120) if "equal" in kind else (120, 100) if kind == "upper" else (100, 120)
            out[kind, k] = ((x, y - 1, hi), (x + (1 if "diag" in kind else 0), y, lo))
    return out


def _pre_seams(ay0, strip, seams, roi_index, x_off=0):
    def pre(o, c):
        assert c.plan()[1] == strip and region(*c.size, c.grid, c.rois[roi_index], (0, 0))[1] == ay0
        got = kpset(keypoints(o, c, c.rois[roi_index]))
        for (kind, k), (up, low) in seam_pairs(ay0, strip, seams, x_off).items():
            want = set() if "equal" in kind else {up[:2]} if kind == "upper" else {low[:2]}
            assert got & {up[:2], low[:2]} == want, (kind, k, got & {up[:2], low[:2]})
    return pre


def _seam_image(w, h, ay0, strip, seams, x_offs=(0,)):
    def image():
        img = lattice(w, h, 11, pitch=9, off=(70, 5))  # other keypoints around, clear of the pairs' columns
        img[:, :68 + max(x_offs)] = BG
        for xo in x_offs:
            for up, low in seam_pairs(ay0, strip, seams, xo).values():
                img[up[1], up[0]], img[low[1], low[0]] = up[2], low[2]
        return img
    return image


# 300 x 150, one cell; rois from row 7: seams at rows 39 and 71; the 60-wide rois are
# single-pass regions, the 260-wide ones two-pass from height 64
SEAMS32 = Case("seams-strip32", _seam_image(300, 150, 7, 32, (1, 2)),
               [(10, 7, rw, rh) for rw in (60, 260) for rh in SEAM_HEIGHTS] + [(10, 7, 260, 143)], grid=(1, 1),
               pre=pre_all(_pre_seams(7, 32, (1, 2), 4), _pre_seams(7, 32, (1, 2), 9), pre_passes(4, (0, 0), True),
                           pre_passes(9, (0, 0), False), pre_passes(7, (0, 0), True)))
# 100 x 100: the frame on which tests/test_gridfast_edges.py restates the grid layer in numpy
SEAMS_SMALL = Case("seams-small", _seam_image(100, 100, 7, 32, (1, 2)), [(10, 7, 60, rh) for rh in SEAM_HEIGHTS + (93,)],
                   grid=(1, 1), pre=pre_all(_pre_seams(7, 32, (1, 2), 4), _pre_seams(7, 32, (1, 2), 5)))
# the same pairs in a 1030-wide cell: seams every 16 rows from row 3
SEAMS16 = Case("seams-strip16", _seam_image(1030, 70, 3, 16, (1, 2, 3), (0, 900)),
               [(0, 0, 1030, 70), (10, 0, 60, 70), (900, 0, 130, 70)] + [(0, 3, 1030, rh) for rh in (15, 16, 17, 32, 33)],
               grid=(1, 1),
               pre=pre_all(_pre_seams(3, 16, (1, 2, 3), 0), _pre_seams(3, 16, (1, 2, 3), 1), _pre_seams(3, 16, (1, 2, 3), 2, 900),
                           pre_passes(0, (0, 0), False), pre_passes(1, (0, 0), True)))


# -- roi edges: a stronger dot one pixel outside the roi suppresses the dot inside
EDGE_ROI = (20, 20, 20, 20)
EDGE_PAIRS = {  # name: (inner, outer) positions
    "left": ((20, 27), (19, 27)), "right": ((39, 32), (40, 32)), "top": ((29, 20), (29, 19)),
    "bottom": ((34, 39), (34, 40)), "corner": ((20, 20), (19, 19)), "corner-br": ((39, 39), (40, 40)),
}


def _edge_image(outer=120, inner=100):
    def image():
        pts = [(28, 30, 90)]  # a lone keypoint inside
        for a, b in EDGE_PAIRS.values():
            pts += [a + (inner,)] + ([b + (outer,)] if outer else [])
        return dots(64, 64, pts)
    return image


def _pre_roi_edge(o, c):
    """Stronger dots outside: no inner dot survives; without them, or weaker, every one does."""
    got = kpset(keypoints(o, c, EDGE_ROI, frame=_edge_image()()))
    alone = kpset(keypoints(o, c, EDGE_ROI, frame=_edge_image(0)()))
    weaker = kpset(keypoints(o, c, EDGE_ROI, frame=_edge_image(80)()))
    inner = {a for a, _ in EDGE_PAIRS.values()}
    assert got == {(28, 30)} and alone == weaker == inner | {(28, 30)}, (got, alone, weaker)


ROI_EDGE = [Case(f"roi-edge-{name}-outside", _edge_image(v), [EDGE_ROI, (19, 19, 22, 22), (0, 0, 64, 64)], grid=(1, 1),
                 pre=_pre_roi_edge) for name, v in (("stronger", 120), ("weaker", 80))]

# -- cell borders: 64 x 64, grid (2, 2): cells of 32, detection regions 3..28 and 35..60.
# A dot in a cell's 3-px border scores 0 there, so its weaker neighbour inside survives.
BORDER_PAIRS = {  # (inner, outer)
    "cell0-left": ((3, 10), (2, 10)), "cell0-top": ((12, 3), (12, 2)), "cell0-right": ((28, 16), (29, 16)),
    "cell1-left": ((35, 22), (34, 22)), "cell0-bottom": ((20, 28), (20, 29)), "cell2-top": ((10, 35), (10, 34)),
    "cell3-corner": ((35, 35), (34, 34)), "cell0-corner": ((28, 28), (29, 29)), "cell3-right": ((60, 50), (61, 50)),
    "cell3-bottom": ((48, 60), (48, 61)),
}
BORDER_ROIS = [(0, 0, 64, 64), (20, 20, 24, 24), (26, 10, 12, 40), (3, 3, 26, 26)]


def _border_image():
    pts = []
    for a, b in BORDER_PAIRS.values():
        pts += [a + (100,), b + (120,)]
    return dots(64, 64, pts)


def _pre_cell_border(o, c):
    got = kpset(keypoints(o, c, BORDER_ROIS[0]))
    assert got == {a for a, _ in BORDER_PAIRS.values()}, got
    four = kpset(keypoints(o, c, BORDER_ROIS[1]))  # straddles the four cells
    assert four == {(28, 28), (35, 35), (35, 22), (20, 28)}, four


CELL_BORDER = Case("cell-border", _border_image, BORDER_ROIS, grid=(2, 2), pre=_pre_cell_border)


# -- the 8-bit score's extremes: 255 on 0, a contrast-1 corner, thresholds at and past the ends
def _extreme_image():
    return dots(32, 32, [(10, 12, 255), (20, 18, 1)], bg=0)


def threshold_case(thr, nonmax=True):
    want = [[10, 12, 254]] if thr < 255 else []
    if not nonmax:  # every corner counts, with response 0: the contrast-1 pixel from threshold 0
        want = [[10, 12, 0]] * (thr < 255) + [[20, 18, 0]] * (thr <= 0)

    def pre(o, c):
        assert keypoints(o, c, c.rois[0]).tolist() == want, keypoints(o, c, c.rois[0])
    return Case(f"threshold{thr}{'' if nonmax else '-no-nonmax'}", _extreme_image, [(0, 0, 32, 32), (8, 8, 8, 8)], grid=(1, 1),
                threshold=thr, nonmax=nonmax, pre=pre)


THRESHOLDS = [threshold_case(t) for t in (0, 254, -5, 255, 300)] + [threshold_case(t, False) for t in (0, -5, 1, 255)]


def _pre_all_254(o, c):
    k = keypoints(o, c, c.rois[0], max_total=HUGE)
    assert (k[:, 2] == 254).all() and len(k) > c.max_total == reference(o, c)[1][0]


# black with one pixel in five white: every corner has response 254, every cut is a tie
THRESHOLDS += [Case(f"binary-threshold{t}", lambda: np.random.default_rng(12).choice(np.uint8([0, 255]), (96, 96), p=[0.8, 0.2]),
                    [(0, 0, 96, 96), (17, 9, 40, 70)], grid=(2, 2), threshold=t, max_total=200, pre=_pre_all_254)
               for t in (0, 254)]


# -- tiny frames: cells narrower than 7 px have no detection region, 7-px cells one column
def tiny_case(s, total):
    return Case(f"tiny{s}", lambda: lattice(s, s, 0, pitch=3), [(0, 0, s, s), (0, 0, s - 1, s - 1), (1, 1, s, s)],
                pre=pre_totals(total, total, total))


def _tiny28_every_cell():
    """28 x 28, cells of 7: a dot on every cell's only detection pixel, and on its neighbours."""
    c = [3 + 7 * j for j in range(4)]
    return dots(28, 28, [(x, y, 120) for y in c for x in c] + [(x + 1, y, 140) for y in c for x in c[::2]]
                + [(x, y - 1, 140) for y in c[1:2] for x in c])


TINY = [tiny_case(8, 0), tiny_case(13, 0), tiny_case(27, 0), tiny_case(28, 1),
        Case("tiny28-every-cell", _tiny28_every_cell, [(0, 0, 28, 28), (3, 3, 22, 22), (4, 4, 20, 20)],
             pre=pre_totals(16, 16, 4))]
TINY += [Case("per-cell-0", lambda: lattice(64, 64, 14), [(0, 0, 64, 64), (10, 10, 30, 30)], max_total=15, cap=15,
              pre=pre_totals(0, 0)),
         Case("per-cell-1", lambda: lattice(64, 64, 14), [(0, 0, 64, 64), (10, 10, 30, 30)], max_total=16, cap=16,
              pre=pre_totals(16, 9))]


# -- two sets in one call, 70 rois: the 64-roi launch boundary falls inside the second set
def sets_case():
    """(frames, roi sets, detector Case): the seam image and a lattice on two slots."""
    rng = np.random.default_rng(15)
    boxes = [(int(x), int(y), int(w), int(h)) for x, y, w, h in
             zip(rng.integers(-20, 280, 54), rng.integers(-20, 130, 54), rng.integers(4, 200, 54), rng.integers(4, 150, 54))]
    a = Case("sets-seams", SEAMS32.image, SEAMS32.rois + boxes[:24], grid=(1, 1), max_total=1000, cap=100, seed=21)
    b = Case("sets-lattice", lambda: lattice(300, 150, 16), [(0, 0, 300, 150), (3, 3, 294, 33)] + boxes[24:] + [(0, 0, 0, 0)],
             grid=(1, 1), max_total=1000, cap=100, seed=21)
    return a, b


# the lattice shrunk for the numpy restatement: 4 cells of 121 candidates for 16 places
LATTICE_SMALL = Case("lattice100-cut", lambda: lattice(100, 100, 17), [(0, 0, 99, 99), (3, 3, 44, 44), (30, 20, 50, 70)],
                     max_total=64, grid=(2, 2), pre=pre_all(pre_totals(64, 16, 64), pre_tie_carry(0, (0, 0), True, seam=False)))
LATTICE_SMALL_NO_NONMAX = Case("lattice100-no-nonmax", LATTICE_SMALL.image, LATTICE_SMALL.rois, max_total=64, grid=(2, 2),
                               nonmax=False, pre=pre_totals(64, 16, 64))

ALL = ([N4096] + BOTH + TIES + WIDE + [W1030, SEAMS32, SEAMS16, SEAMS_SMALL] + ROI_EDGE + [CELL_BORDER] + THRESHOLDS + TINY
       + [LATTICE_SMALL, LATTICE_SMALL_NO_NONMAX])
SMALL = [c for c in ALL if c.name.startswith(("seams-small", "roi-edge", "cell-border", "threshold", "binary", "tiny",
                                              "per-cell", "lattice100"))]
