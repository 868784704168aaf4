"""The reduced optical-flow scale (PSN_2D_OPTICALFLOW_SCALE), host side: the
numpy restatement of the ingest resize (tests/resize_ref.py) on known answers,
the library's resize tables (psn_lk_resize_plan) and LK size (psn_lk_scaled_size)
against it, and LocalSearchKLT at a scale (psn_t2d_local_search_klt_scaled)
against oracle/tracker2d_oracle.py with its SCALE set. No GPU."""
import numpy as np
import pytest

import resize_ref
from mcmtt_opticalflow_amd import _lib, lk
from mcmtt_opticalflow_amd import tracker2d as t2d

ORC = pytest.importorskip("tracker2d_oracle")

ERR_ARG = -1


def _random_gray(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


# ---- resize_ref known answers ----

@pytest.mark.parametrize("w,h", [(64, 48), (645, 483), (1, 1), (7, 3)])
def test_ref_identity_at_1(w, h):
    g = _random_gray(w, h, 1)
    np.testing.assert_array_equal(resize_ref.resize(g, 1.0), g)
    xo, xc = resize_ref.plan(w, w, True)
    np.testing.assert_array_equal(xo, np.arange(w))
    assert (xc == np.int16([2048, 0])).all()


@pytest.mark.parametrize("w,h", [(64, 48), (322, 242), (2, 2)])
def test_ref_half_is_rounded_block_mean(w, h):
    g = _random_gray(w, h, 2)
    s = g.astype(np.int32)
    want = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
    np.testing.assert_array_equal(resize_ref.resize(g, 0.5), want.astype(np.uint8))


@pytest.mark.parametrize("scale", [0.3, 0.5, 0.75])
@pytest.mark.parametrize("value", [0, 1, 137, 254, 255])
def test_ref_constant_stays_constant(scale, value):
    out = resize_ref.resize(np.full((483, 645), value, np.uint8), scale)
    assert out.shape == resize_ref.scaled_size(645, 483, scale)[::-1]
    assert (out == value).all()


def test_ref_size_truncates():
    assert resize_ref.scaled_size(645, 483, 0.5) == (322, 241)
    assert resize_ref.scaled_size(200, 134, 0.3) == (60, 40)
    assert resize_ref.scaled_size(322, 242, 0.75) == (241, 181)
    assert resize_ref.resize(np.zeros((483, 645), np.uint8), 0.5).shape == (241, 322)


# ---- the library's tables and LK size ----

@pytest.mark.parametrize("is_x", [True, False])
@pytest.mark.parametrize("src,dst", [(64, 32), (645, 322), (483, 241), (322, 241), (101, 30), (50, 50)])
def test_resize_plan_equals_ref(src, dst, is_x):
    ofs, coef = lk.resize_plan(src, dst, is_x)
    r_ofs, r_coef = resize_ref.plan(src, dst, is_x)
    np.testing.assert_array_equal(ofs, r_ofs)
    np.testing.assert_array_equal(coef, r_coef)
    if is_x:  # the border rule: every column reads inside the row
        assert ofs.min() >= 0 and ofs.max() <= src - 1
        assert (coef[ofs == src - 1] == np.int16([2048, 0])).all()
    assert (np.diff(ofs) >= 0).all()  # (the resize kernel's tiles rely on it)


def test_resize_plan_bad_args():
    L = _lib.load()
    ofs, coef = np.zeros(4, np.int32), np.zeros((4, 2), np.int16)
    assert L.psn_lk_resize_plan(0, 4, ofs.ctypes.data, coef.ctypes.data, 1) == ERR_ARG
    assert L.psn_lk_resize_plan(4, 0, ofs.ctypes.data, coef.ctypes.data, 1) == ERR_ARG
    assert L.psn_lk_resize_plan(4, 4, None, coef.ctypes.data, 1) == ERR_ARG


def test_scaled_size():
    for (w, h, s) in [(645, 483, 0.5), (200, 134, 0.3), (322, 242, 0.75), (1920, 1080, 0.5), (3840, 2160, 0.5),
                      (640, 480, 1.0), (101, 77, 0.999), (10, 10, 0.1)]:
        assert lk.scaled_size(w, h, s) == resize_ref.scaled_size(w, h, s), (w, h, s)
    assert lk.scaled_size(645, 483, 0.5) == (322, 241)
    for bad in (float("nan"), 0.0, -0.5, 1.0000001, 2.0, float("inf")):
        with pytest.raises(lk.PsnLkError) as e:
            lk.scaled_size(640, 480, bad)
        assert e.value.code == ERR_ARG
    with pytest.raises(lk.PsnLkError):  # an LK size below one pixel
        lk.scaled_size(3, 480, 0.3)
    with pytest.raises(lk.PsnLkError):
        lk.scaled_size(0, 480, 0.5)


# ---- LocalSearchKLT at a scale ----

def _klt_sets():
    """(pre_box at full size, pre, cur) cases: seeded sets of 4 to 100 points moving by a
    common shift plus noise and outliers; sets whose vectors are between 0.1 * 0.75 and 0.1 px
    long (they move at the reduced scales only); sets whose spread lies between the scale-s and the
    scale-1 neighbour windows."""
    rng = np.random.default_rng(77)
    cases = []
    for n in (4, 5, 9, 17, 40, 63, 100):
        box = (float(rng.integers(10, 300)), float(rng.integers(10, 200)), float(rng.integers(20, 140)),
               float(rng.integers(40, 300)))
        pre = np.stack([rng.uniform(box[0], box[0] + box[2], n), rng.uniform(box[1], box[1] + box[3], n)], 1)
        shift = rng.uniform(-4, 4, 2)
        cur = pre + shift + rng.normal(0, 0.3, (n, 2))
        out = rng.random(n) < 0.2
        cur[out] += rng.uniform(-30, 30, (int(out.sum()), 2))
        still = rng.random(n) < 0.15
        cur[still] = pre[still]
        cases.append((box, pre.astype(np.float32), cur.astype(np.float32)))
    for n in (8, 31, 100):  # vectors of 0.08 .. 0.095 px: below the 0.1 gate, above 0.1 * 0.75
        box = (50.0, 40.0, 64.0, 160.0)
        pre = np.stack([rng.uniform(60, 100, n), rng.uniform(50, 180, n)], 1).astype(np.float32)
        ang = rng.uniform(0, 2 * np.pi, n)
        r = rng.uniform(0.08, 0.095, n)
        cur = (pre.astype(np.float64) + np.stack([r * np.cos(ang), r * np.sin(ang)], 1)).astype(np.float32)
        cases.append((box, pre, cur))
    for n in (12, 50, 100):  # flow spread over +-0.15 box widths around the shift
        box = (100.0, 80.0, 40.0, 100.0)
        pre = np.stack([rng.uniform(100, 140, n), rng.uniform(80, 180, n)], 1).astype(np.float32)
        cur = (pre + np.float32([3.0, -2.0]) + rng.uniform(-6, 6, (n, 2))).astype(np.float32)
        cases.append((box, pre, cur))
    return cases


@pytest.mark.parametrize("scale", [1.0, 0.5, 0.75])
def test_local_search_klt_scaled_matches_oracle(monkeypatch, scale):
    differ_gate = differ_window = 0
    for k, (box, pre, cur) in enumerate(_klt_sets()):
        sbox = ORC.Rect(*box).scale(scale)  # the reference searches around the scaled box
        monkeypatch.setattr(ORC, "SCALE", scale)
        r_box, r_inl = ORC.local_search_klt(sbox, pre, cur)
        g_box, g_inl = t2d.local_search_klt(sbox.tuple(), pre, cur, scale=scale)
        assert g_box == r_box.tuple(), f"case {k}"
        assert g_inl == r_inl, f"case {k}"
        monkeypatch.setattr(ORC, "SCALE", 1.0)
        one_box, one_inl = ORC.local_search_klt(sbox, pre, cur)
        if scale == 1.0:  # the existing entry point is the scale-1 call
            assert t2d.local_search_klt(sbox.tuple(), pre, cur) == (g_box, g_inl)
        elif (one_box.tuple(), one_inl) != (g_box, g_inl):
            if 7 <= k < 10:
                differ_gate += 1
            elif k >= 10:
                differ_window += 1
    if scale != 1.0:  # the cases do tell the scaled thresholds from the scale-1 ones
        assert differ_gate >= 1 and differ_window >= 1


def test_local_search_klt_scaled_bad_scale():
    pts = np.float32([[1, 1], [2, 2], [3, 3], [4, 4]])
    for bad in (float("nan"), 0.0, -1.0, 1.5):
        with pytest.raises(t2d.T2dError) as e:
            t2d.local_search_klt((0, 0, 10, 10), pts, pts + 1, scale=bad)
        assert e.value.code == ERR_ARG


# ---- ABI ----

def test_new_exports_declared_and_present():
    L, T = _lib.load(), t2d.load()
    for name in ("psn_lk_scaled_size", "psn_lk_resize_plan", "psn_lk_create_scaled", "psn_lk_source_size",
                 "psn_lk_scale"):
        assert name in _lib.header_functions() and hasattr(L, name), name
    for name in ("psn_t2d_create_scaled", "psn_t2d_group_create_scaled", "psn_t2d_local_search_klt_scaled"):
        assert name in t2d.header_functions() and hasattr(T, name), name
    assert L.psn_lk_abi_version() == 5 and T.psn_t2d_abi_version() == 2
