"""The cases of tests/test_lk_small_frames_gpu.py are alive on the CPU oracle: it tracks
most grid points of every class A, B and N case (so the device comparison there is not one
of rejections only), their effective pyramid depth is the tabulated one, and the cases
meant to make refl101 loop do hold tracked points whose taps need it. No GPU."""
import pytest

import lk_small_cases as sc


def _share(oracle_mod, case, outside=False):
    W, H, win, ml, eff = case
    assert oracle_mod.effective_max_level(W, H, win[0], win[1], ml) == eff
    _, _, pts, (nxt, status, err) = sc.reference(oracle_mod, W, H, win, ml, outside=outside)
    share = float(status.mean())
    loops = int(sc.second_reflection(W, H, win, pts, nxt, status).sum())
    print(f"{sc.case_id(case)}{' outside grid' if outside else ''}: status-1 share {share:.2f} of {len(pts)} points, "
          f"{loops} tracked with a twice-reflected tap")
    return share, loops


@pytest.mark.parametrize("case", sc.CLASS_A + sc.CLASS_B + sc.CLASS_N, ids=sc.case_id)
def test_oracle_tracks_the_small_frame_cases(oracle_mod, case):
    share, loops = _share(oracle_mod, case)
    assert share >= (0.3 if case[:2] in sc.STRIPS else 0.5)
    if case in sc.CLASS_N:
        assert loops >= 5  # (measured 9..17 of the grid's points)


@pytest.mark.parametrize("case", sc.CLASS_B, ids=sc.case_id)
def test_oracle_tracks_the_points_outside_the_frame(oracle_mod, case):
    share, loops = _share(oracle_mod, case, outside=True)
    assert share >= (0.3 if case[:2] in sc.STRIPS else 0.5)
    if case[:2] in ((16, 16), (50, 40), (60, 100), (90, 200), (40, 30)):  # the window exceeds the frame well
        assert loops >= 5


def test_case_tables():
    assert len(sc.CLASS_A) == 9 and len(sc.CLASS_B) == 13 and len(sc.CLASS_C) == 8
    assert all(c[4] == 0 for c in sc.CLASS_B + sc.CLASS_N)
    assert {c[2] for c in sc.CLASS_A + sc.CLASS_B + [c + (0,) for c in sc.CLASS_C]} == set(sc.KERNEL)
    # the box-window runs do not all fall into one build
    builds = {"lk_kernel_st", "lk_kernel_bx<8, true, 128>", "lk_kernel_fw<10, true>", "lk_kernel_bx<4, false>",
              "lk_kernel_lg"}
    for cases in (sc.CLASS_A, sc.CLASS_B, sc.CLASS_N):
        assert builds <= {sc.ENTRY[c[2]] for c in cases}
