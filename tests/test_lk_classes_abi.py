"""Frame classes at the C ABI, without a GPU: psn_lk_create_classes (include/psn_lk.h)
and psn_t2d_group_create_sizes (include/psn_tracker2d.h) refuse bad arguments with a
code before they touch the device, the new entry points are declared and exported,
the versions stay, and the host-only size rule is the one a class's LK size follows.
"""
import ctypes

import pytest

from mcmtt_opticalflow_amd import _lib, lk
from mcmtt_opticalflow_amd import tracker2d as t2d

ERR_ARG = -1
LK_NEW = ("psn_lk_create_classes", "psn_lk_num_classes", "psn_lk_slot_class", "psn_lk_class_slots",
          "psn_lk_class_source_size", "psn_lk_class_level_size")
T2D_NEW = ("psn_t2d_group_create_sizes", "psn_t2d_group_camera_size")


def _create_classes(classes, scale=1.0, cap=3, n=None):
    L = _lib.load()
    arr = (_lib.LkFrameClass * max(len(classes), 1))(*[_lib.LkFrameClass(*c) for c in classes])
    h = ctypes.c_void_p()
    rc = L.psn_lk_create_classes(0, arr, len(classes) if n is None else n, scale, cap, ctypes.byref(h))
    assert rc != 0 and not h.value  # (these calls must fail: a context made here would need a GPU)
    return rc


def _create_sizes(sizes, scale=1.0):
    T = t2d.load()
    n = len(sizes)
    ids = (ctypes.c_uint * max(n, 1))(*range(n))
    ws = (ctypes.c_int * max(n, 1))(*[s[0] for s in sizes])
    hs = (ctypes.c_int * max(n, 1))(*[s[1] for s in sizes])
    h = ctypes.c_void_p()
    rc = T.psn_t2d_group_create_sizes(0, n, ids, ws, hs, scale, ctypes.byref(h))
    assert rc != 0 and not h.value
    return rc


def test_exports_declared_and_present_versions_stay():
    L, T = _lib.load(), t2d.load()
    for name in LK_NEW:
        assert name in _lib.header_functions() and hasattr(L, name), name
    for name in T2D_NEW:
        assert name in t2d.header_functions() and hasattr(T, name), name
    assert not [n for n in _lib.header_functions() if not hasattr(L, n)]
    assert not [n for n in t2d.header_functions() if not hasattr(T, n)]
    assert L.psn_lk_abi_version() == 5 and T.psn_t2d_abi_version() == 2
    assert _lib.MAX_FRAME_CLASSES == 8
    src = open(_lib.HEADER_PATH).read()
    assert "#define PSN_LK_MAX_FRAME_CLASSES 8" in src and "#define PSN_LK_ABI_VERSION 5" in src


def test_create_classes_argument_errors():
    ok = (320, 240, 4)
    assert _create_classes([]) == ERR_ARG                       # ncls 0
    assert _create_classes([ok] * 9) == ERR_ARG                 # ncls 9 > PSN_LK_MAX_FRAME_CLASSES
    assert _create_classes([ok], n=-1) == ERR_ARG
    for bad in ((0, 240, 4), (320, 0, 4), (-5, 240, 4), (320, 240, 0), (320, 240, -1)):
        assert _create_classes([ok, bad]) == ERR_ARG, bad       # a zero size / no slots, in any class
        assert _create_classes([bad, ok]) == ERR_ARG, bad
    for scale in (float("nan"), 0.0, -0.5, 1.5, float("inf")):
        assert _create_classes([ok, (200, 150, 4)], scale=scale) == ERR_ARG, scale
    assert _create_classes([ok, (3, 3, 4)], scale=0.25) == ERR_ARG  # the second class's LK size is below 1 px
    assert _create_classes([ok], cap=-1) == ERR_ARG and _create_classes([ok], cap=6) == ERR_ARG
    L = _lib.load()
    assert L.psn_lk_create_classes(0, None, 1, 1.0, 3, ctypes.byref(ctypes.c_void_p())) == ERR_ARG
    assert L.psn_lk_create_classes(0, (_lib.LkFrameClass * 1)(_lib.LkFrameClass(*ok)), 1, 1.0, 3, None) == ERR_ARG


def test_class_queries_refuse_a_null_context():
    L = _lib.load()
    i = ctypes.c_int()
    assert L.psn_lk_num_classes(None) == ERR_ARG
    assert L.psn_lk_slot_class(None, 0, ctypes.byref(i)) == ERR_ARG
    assert L.psn_lk_class_slots(None, 0, ctypes.byref(i), ctypes.byref(i)) == ERR_ARG
    assert L.psn_lk_class_source_size(None, 0, ctypes.byref(i), ctypes.byref(i)) == ERR_ARG
    assert L.psn_lk_class_level_size(None, 0, 0, ctypes.byref(i), ctypes.byref(i)) == ERR_ARG
    assert t2d.load().psn_t2d_group_camera_size(None, 0, None, None, None, None) == ERR_ARG


def test_group_create_sizes_argument_errors():
    assert _create_sizes([]) == ERR_ARG
    assert _create_sizes([(320, 240), (0, 150)]) == ERR_ARG
    assert _create_sizes([(320, 240), (200, -1)]) == ERR_ARG
    for scale in (float("nan"), 0.0, 1.5):
        assert _create_sizes([(320, 240), (200, 150)], scale=scale) == ERR_ARG
    # 9 distinct sizes: more than PSN_LK_MAX_FRAME_CLASSES
    assert _create_sizes([(320 + 8 * i, 240) for i in range(9)]) == ERR_ARG
    T = t2d.load()
    one = (ctypes.c_int * 1)(320)
    assert T.psn_t2d_group_create_sizes(0, 1, (ctypes.c_uint * 1)(0), None, one, 1.0, ctypes.byref(ctypes.c_void_p())) == ERR_ARG
    assert T.psn_t2d_group_create_sizes(0, 1, (ctypes.c_uint * 1)(0), one, one, 1.0, None) == ERR_ARG
    with pytest.raises(t2d.T2dError) as e:
        t2d.Group.with_sizes([(320 + 8 * i, 240) for i in range(9)], list(range(9)))
    assert e.value.code == ERR_ARG
    with pytest.raises(ValueError):
        t2d.Group.with_sizes([(320, 240)], [0, 1])


def test_with_classes_reports_the_code():
    with pytest.raises(lk.PsnLkError) as e:
        lk.LKContext.with_classes([(320, 240, 4)] * 9)
    assert e.value.code == ERR_ARG
    with pytest.raises(lk.PsnLkError) as e:
        lk.LKContext.with_classes([(320, 240, 4), (200, 150, 4)], scale=2.0)
    assert e.value.code == ERR_ARG


def test_scaled_size_is_the_class_size_rule():
    """A class's LK size is psn_lk_scaled_size of its own source size (the device half,
    psn_lk_class_level_size of a context, is compared in tests/test_lk_classes_gpu.py)."""
    assert lk.scaled_size(384, 288, 0.5) == (192, 144)
    assert lk.scaled_size(361, 287, 0.5) == (180, 143)  # (int)(w * s): truncated, per class
    assert lk.scaled_size(360, 288, 0.5) == (180, 144)
    assert lk.scaled_size(200, 150, 1.0) == (200, 150)
