"""Frames on which the border dominates the LK window: the cases, the frame recipe, the
point grid and the (cached) oracle outputs shared by tests/test_lk_small_frames.py (CPU)
and tests/test_lk_small_frames_gpu.py.

OpenCV pads both images by winSize with reflect-101 (the derivatives by zeros). The pad of
a 21 x 21 window around a 16 x 16 frame reflects more than once, but a window around a
point inside the frame ends half a window past the border: its taps reflect twice only
where the frame is at most half the window (class N) or the point lies outside the frame
(outside_grid); second_reflection counts such points. The oracle (oracle/lk_oracle.c)
tracks every case below."""
import numpy as np

from mcmtt_opticalflow_amd import synth
from mcmtt_opticalflow_amd._lib import ACCUM_SCALAR
from test_lk_gpu import oracle_ref

# (W, H, window, requested maxLevel, effective maxLevel)
# A: the top level used is only just larger than the window
CLASS_A = [(180, 178, (21, 21), 3, 3), (83, 131, (9, 15), 3, 3), (104, 74, (12, 8), 3, 3), (328, 264, (40, 32), 3, 3),
           (520, 520, (64, 64), 3, 3), (260, 644, (64, 160), 3, 2), (275, 307, (33, 37), 3, 3),
           (404, 1004, (100, 250), 3, 2), (262, 262, (130, 130), 3, 1)]
# B: the window is at least the frame in one dimension, or the frame is a strip (level 0 only)
CLASS_B = [(16, 16, (21, 21), 3, 0), (20, 40, (21, 21), 3, 0), (64, 64, (64, 64), 3, 0), (65, 65, (64, 64), 3, 0),
           (50, 40, (64, 64), 3, 0), (100, 180, (64, 160), 3, 0), (60, 100, (64, 160), 3, 0),
           (101, 251, (100, 250), 3, 0), (90, 200, (100, 250), 3, 0), (40, 30, (33, 37), 3, 0),
           (400, 7, (5, 5), 3, 0), (7, 300, (5, 5), 3, 0), (300, 4, (3, 3), 3, 0)]
# N: one dimension of the frame is at most half the window, so a window around a point INSIDE
# the frame reaches a frame length past the border: the taps need a second reflection (in
# class B's frames a window around an in-frame point ends within half a window of the
# border, less than the frame: one reflection is enough there -- see outside_grid)
CLASS_N = [(12, 40, (21, 21), 3, 0), (40, 12, (21, 21), 3, 0), (30, 100, (64, 64), 3, 0), (100, 30, (64, 64), 3, 0),
           (30, 170, (64, 160), 3, 0), (45, 300, (100, 250), 3, 0), (15, 60, (33, 37), 3, 0)]
# C: tiny frames (W, H, window, requested maxLevel)
CLASS_C = [(8, 8, (3, 3), 5), (5, 5, (3, 3), 3), (4, 4, (3, 3), 3), (3, 3, (3, 3), 1), (2, 2, (3, 3), 0),
           (1, 1, (3, 3), 0), (1, 50, (3, 3), 2), (50, 1, (3, 3), 2)]
STRIPS = [(400, 7), (7, 300), (300, 4)]

# the kernel the planner gives each window by default (psn_lk_plan.cpp: the class depends
# on the window alone), as _lib.kernel_of_tag names psn_lk_timing_launches' tag; and the
# entry (psn_lk_timing_entries) where it differs
KERNEL = {(21, 21): "lk_kernel_st", (9, 15): "lk_kernel_st", (12, 8): "lk_kernel_st", (5, 5): "lk_kernel_st",
          (3, 3): "lk_kernel_st",
          (40, 32): "lk_kernel_bx<8, true, 128>", (64, 64): "lk_kernel_bx<8, true, 128>",  # two-wave
          (64, 160): "lk_kernel_bx<10, true>",                                              # forward entry
          (33, 37): "lk_kernel_bx<4, false>",                                               # a tail build
          (100, 250): "lk_kernel_lg", (130, 130): "lk_kernel_lg"}
ENTRY = {**KERNEL, (64, 160): "lk_kernel_fw<10, true>"}


def case_id(c):
    return f"{c[0]}x{c[1]}-win{c[2][0]}x{c[2][1]}"


def frames(W, H):
    """Two crops of one texture: the true flow is (2, 1)."""
    tex = synth.texture(W + 8, H + 8, 3)
    return np.ascontiguousarray(tex[4:4 + H, 4:4 + W]), np.ascontiguousarray(tex[3:3 + H, 2:2 + W])


def grid(W, H, win):
    """A grid over the whole frame, corners and edges included, shifted by a quarter pixel."""
    nx, ny = (8, 6) if win[0] * win[1] <= 1024 else (6, 5)
    xs, ys = np.meshgrid(np.linspace(0, W - 1, nx), np.linspace(0, H - 1, ny))
    return (np.stack([xs.ravel(), ys.ravel()], 1) + 0.25).astype(np.float32)


def outside_grid(W, H, win):
    """A 6 x 5 grid reaching half a window less 3 px past every border: the windows of the
    outer points lie mostly outside the frame (calcOpticalFlowPyrLK tracks a point while its
    window's origin is within (-winSize, size))."""
    hx, hy = win[0] // 2 - 3, win[1] // 2 - 3
    xs, ys = np.meshgrid(np.linspace(-hx, W - 1 + hx, 6), np.linspace(-hy, H - 1 + hy, 5))
    return (np.stack([xs.ravel(), ys.ravel()], 1) + 0.25).astype(np.float32)


def second_reflection(W, H, win, pts, nxt, status):
    """Tracked points whose I window (at the point) or J window (at the oracle's nextPt) holds a
    tap at least a frame length past a border: refl101 has to loop for it."""
    def far(p, w, n):
        o = np.floor(p - (w - 1) * 0.5)  # taps o .. o + w
        return (o <= -n) | (o + w >= 2 * n - 1)
    need = np.zeros(len(pts), bool)
    for q in (pts, nxt):
        need |= far(q[:, 0], win[0], W) | far(q[:, 1], win[1], H)
    return need & (status == 1)


_refs = {}


def reference(oracle_mod, W, H, win, ml, scalar=False, outside=False):
    """(f0, f1, points, the oracle's (next, status, err)); computed once per case, point grid
    and accumulation order."""
    key = (W, H, win, ml, scalar, outside)
    if key not in _refs:
        f0, f1 = frames(W, H)
        pts = outside_grid(W, H, win) if outside else grid(W, H, win)
        ref = oracle_ref(oracle_mod, f0, f1, pts, win, ml, flags=ACCUM_SCALAR if scalar else 0)
        for a in (f0, f1, pts) + tuple(ref):
            a.setflags(write=False)
        _refs[key] = (f0, f1, pts, ref)
    return _refs[key]
