"""The context layout (csrc/psn_lk_layout.cpp) on the CPU.

tests/cpp/ctx_layout_dump links the layout unit alone (no libpsn_lk.so, no GPU)
and prints, per case, what psn::ctx_layout gives psn_lk_create_classes: the
return code, the bytes of the pyramid allocation, the class of every slot, the
planner's fields and per frame class its sizes, slots, level table, place in
the allocation, gray planes and resize table (size, FNV-1a checksum, first and
last entry). Every line is checked against the layout's rules as restated here,
not against a record of the code under test.

A case is SCALE/CAP/WxH,SLOTS[/WxH,SLOTS...], one WxH,SLOTS per frame class.
"""
import functools
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS_DIR = os.path.join(HERE, "cpp")
BIN = os.path.join(HARNESS_DIR, "bin", "ctx_layout_dump")

OK, ERR_ARG = 0, -1  # include/psn_lk.h
MAX_TOP = 5  # psn::kPyrMaxTop

EIGHT = "/".join(f"{w}x{h},1" for w, h in [(1920, 1080), (1600, 900), (1366, 768), (1280, 720), (1024, 576), (960, 540),
                                            (640, 480), (320, 240)])
GOOD = [
    "1/3/1920x1080,4",
    "0.5/3/1920x1080,4",
    "1/5/3840x2160,4",
    "1/3/1279x719,3",
    "1/5/5x3,1",
    "1/3/768x576,4/720x576,8",    # PETS
    "0.5/3/768x576,4/720x576,8",  # ... with every class resized
    "1/3/640x480,4/1920x1080,4",  # a larger second class
    "1/3/" + EIGHT,
    "1/3/640x480,2/320x240,4/1280x720,2",  # the second fits the gap, the third does not
    "1/0/641x479,2/333x222,3",  # one level
]
REFUSED = [
    "1/3",                         # no class
    "1/3/" + EIGHT + "/160x120,1",  # nine classes
    "1/3/640x480,0",
    "1/3/640x480,4/640x480,-1",
    "1/3/8x8,1073741823/8x8,1",    # the slot count would pass INT32_MAX / 2
    "1/-1/640x480,4",
    "1/6/640x480,4",
    "1/3/0x480,4",
    "1/3/640x-2,4",
    "0/3/640x480,4",
    "1.5/3/640x480,4",
    "nan/3/640x480,4",
    "0.1/3/5x3,1",                 # scales to 0x0
    "1/3/640x480,4/2x2,1/0x5,1",   # a later class refused
]


def _run(*args):
    subprocess.run(["make", "-s", "-C", HARNESS_DIR, "bin/ctx_layout_dump"], check=True, timeout=300)
    p = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return [json.loads(line) for line in p.stdout.splitlines()]


@pytest.fixture(scope="module")
def lines():
    got = _run(*GOOD, *REFUSED)
    assert [g["case"] for g in got] == GOOD + REFUSED
    return {g["case"]: g for g in got}


@functools.lru_cache(maxsize=None)
def _plan(src, dst, is_x):
    (p,) = _run("--plan", str(src), str(dst), str(is_x))
    return p["ofs"], p["coef"]


def _parse(case):
    scale, cap, *cls = case.split("/")
    return float(scale), int(cap), [tuple(int(v) for v in c.replace("x", ",").split(",")) for c in cls]


def _up(v, a):
    return (v + a - 1) // a * a


def _fnv1a(ints):
    h = 1469598103934665603
    for x in ints:
        for b in (x & 0xFFFFFFFF).to_bytes(4, "little"):
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def _i32(u):
    return u - (1 << 32) if u >= 1 << 31 else u


def _extents(g):
    """(class, slot, begin, end) of every slot: class 0 owns the scratch slots too."""
    us = g["cfg"]["user_slots"]
    out = []
    for k, f in enumerate(g["classes"]):
        own = list(range(f["first_slot"], f["first_slot"] + f["nslots"])) + ([us, us + 1] if k == 0 else [])
        for s in own:
            b = f["place"] + f["slot_bytes"] * (s - f["first_slot"])
            out.append((k, s, b, b + f["slot_bytes"]))
    return out


@pytest.mark.parametrize("case", GOOD)
def test_sizes_slots_and_planner_fields(lines, case):
    g = lines[case]
    scale, cap, cls = _parse(case)
    assert g["rc"] == OK
    fs = g["classes"]
    assert len(fs) == len(cls)
    first = 0
    for f, (w, h, n) in zip(fs, cls):
        assert (f["src_w"], f["src_h"]) == (w, h)
        assert (f["w"], f["h"]) == (int(w * scale), int(h * scale))
        assert f["rz"] == ((f["w"], f["h"]) != (w, h))
        assert (f["first_slot"], f["nslots"]) == (first, n)  # user slots are numbered class after class
        first += n
    assert g["slot_fcls"] == [k for k, (_, _, n) in enumerate(cls) for _ in range(n)] + [0, 0]
    c = g["cfg"]
    assert (c["width"], c["height"]) == (fs[0]["w"], fs[0]["h"])
    assert (c["user_slots"], c["nslots"], c["nlevels"]) == (first, first + 2, cap + 1)
    if len(cls) == 1:  # the planner's width x height over every slot
        assert c["ncls"] == 0 and c["cls"] == []
    else:
        assert c["ncls"] == len(cls)
        assert c["cls"] == [[f["w"], f["h"], f["first_slot"], f["nslots"]] for f in fs]


@pytest.mark.parametrize("case", GOOD)
def test_levels(lines, case):
    g = lines[case]
    nl = g["cfg"]["nlevels"]
    for f in g["classes"]:
        assert len(f["lw"]) == len(f["lh"]) == len(f["pitch"]) == len(f["off"]) == nl
        assert (f["lw"][0], f["lh"][0]) == (f["w"], f["h"])
        total = 0
        for l in range(nl):
            if l:
                assert f["lw"][l] == (f["lw"][l - 1] + 1) // 2 and f["lh"][l] == (f["lh"][l - 1] + 1) // 2
            assert f["pitch"][l] == _up(f["lw"][l], 256)
            assert f["off"][l] == total
            total += f["pitch"][l] * f["lh"][l]
        assert f["slot_bytes"] == _up(total, 4096)


@pytest.mark.parametrize("case", GOOD)
def test_every_slot_has_its_own_bytes(lines, case):
    g = lines[case]
    ext = _extents(g)
    assert sorted(s for _, s, _, _ in ext) == list(range(g["cfg"]["nslots"]))  # every slot number once
    assert all(0 <= b and e <= g["pyr_bytes"] for _, _, b, e in ext)
    by_begin = sorted(ext, key=lambda x: x[2])
    for a, b in zip(by_begin, by_begin[1:]):
        assert a[3] <= b[2], (a, b)


@pytest.mark.parametrize("case", GOOD)
def test_places(lines, case):
    g = lines[case]
    fs = g["classes"]
    sb0, n0 = fs[0]["slot_bytes"], fs[0]["nslots"]
    us, ns = g["cfg"]["user_slots"], g["cfg"]["nslots"]
    assert fs[0]["place"] == 0
    if len(fs) == 1:  # the layout of a context before frame classes
        assert g["pyr_bytes"] == sb0 * ns
    behind = [k for k in range(1, len(fs)) if fs[k]["place"] >= sb0 * us]
    for k, f in enumerate(fs[1:], 1):
        if k not in behind:  # in the gap between class 0's user and scratch slots
            assert sb0 * n0 <= f["place"] and f["place"] + f["slot_bytes"] * f["nslots"] <= sb0 * us
        else:  # behind the scratch slots
            assert f["place"] >= sb0 * ns
    # no class larger than class 0: all in the gap, nothing behind the scratch slots
    if all(f["slot_bytes"] <= sb0 for f in fs):
        assert not behind and g["pyr_bytes"] == sb0 * ns
    # a class goes behind only when the gap has no room for it after the classes before it
    room = sb0 * (us - n0)
    for k, f in enumerate(fs[1:], 1):
        need = f["slot_bytes"] * f["nslots"]
        assert (k in behind) == (need > room)
        if k not in behind:
            room -= need
    assert g["pyr_bytes"] == sb0 * ns + sum(fs[k]["slot_bytes"] * fs[k]["nslots"] for k in behind)


def test_named_placements(lines):
    pets = lines["1/3/768x576,4/720x576,8"]
    assert pets["pyr_bytes"] == pets["classes"][0]["slot_bytes"] * 14  # 720x576 lies in the gap
    big = lines["1/3/640x480,4/1920x1080,4"]
    sb0 = big["classes"][0]["slot_bytes"]
    assert big["classes"][1]["place"] == sb0 * 10  # right behind the scratch slots 8 and 9
    assert big["pyr_bytes"] == sb0 * 10 + big["classes"][1]["slot_bytes"] * 4
    eight = lines["1/3/" + EIGHT]
    assert eight["pyr_bytes"] == eight["classes"][0]["slot_bytes"] * 10
    three = lines["1/3/640x480,2/320x240,4/1280x720,2"]
    sb0 = three["classes"][0]["slot_bytes"]
    assert three["classes"][1]["place"] == sb0 * 2 and three["classes"][2]["place"] == sb0 * 10


@pytest.mark.parametrize("case", GOOD)
def test_resize_tables_and_gray_planes(lines, case):
    g = lines[case]
    for k, f in enumerate(g["classes"]):
        if not f["rz"]:
            assert (f["gray_pitch"], f["gray_bytes"], f["rz_n"]) == (0, 0, 0)
            continue
        assert f["gray_pitch"] == _up(f["w"], 256)
        assert f["gray_bytes"] == f["gray_pitch"] * f["h"] * (f["nslots"] + (2 if k == 0 else 0))
        tab = []  # xofs[w] | xcoef[w] | yofs[h] | ycoef[h], as resize_gray_kernel reads it
        for src, dst, is_x in ((f["src_w"], f["w"], 1), (f["src_h"], f["h"], 0)):
            ofs, coef = _plan(src, dst, is_x)
            assert len(ofs) == dst and len(coef) == 2 * dst
            tab += ofs + [_i32((coef[2 * i] & 0xFFFF) | (coef[2 * i + 1] & 0xFFFF) << 16) for i in range(dst)]
        assert f["rz_n"] == len(tab) == 2 * (f["w"] + f["h"])
        assert (f["rz_first"], f["rz_last"]) == (tab[0], tab[-1])
        assert f["rz_sum"] == _fnv1a(tab)


def test_resize_plan_entry_is_the_bilinear_table():
    """The second entry of the dump gives psn_lk_resize_plan's tables: at 1/2 every
    output pixel is the mean of two source pixels (OpenCV's 2048-scaled weights)."""
    ofs, coef = _plan(1920, 960, 1)
    assert ofs == [2 * d for d in range(960)]
    assert coef == [1024, 1024] * 960
    ofs, coef = _plan(3, 1, 0)
    assert ofs == [1] and coef == [2048, 0]


@pytest.mark.parametrize("case", REFUSED)
def test_refused_inputs_leave_no_layout(lines, case):
    g = lines[case]
    assert g["rc"] == ERR_ARG and g["touched"] is False
    assert set(g) == {"case", "rc", "touched"}


def test_lds_guard_is_behind_the_level_cap():
    """PSN_LK_ERR_UNSUPPORTED (the pyramid tiles' LDS plan) cannot be reached in a
    library that compiles: psn_lk_kernels.h asserts the plan of every top level up
    to kPyrMaxTop at build time, and a cap past it is PSN_LK_ERR_ARG. Every cap in
    range lays out."""
    got = _run(*[f"1/{cap}/640x480,2" for cap in range(MAX_TOP + 1)])
    assert [g["rc"] for g in got] == [OK] * (MAX_TOP + 1)


def test_layout_binary_stands_alone():
    """ctx_layout_dump has no part of the library behind it."""
    _run("1/3/64x64,1")
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True, timeout=60).stdout
    assert "libpsn" not in out, out
