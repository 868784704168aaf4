"""The LK launch planner with frame classes (csrc/psn_lk_plan.cpp), on the CPU.

tests/cpp/lk_plan_classes.cpp links the planner alone and plans calls on a
context of two frame classes, 320x240 in slots 0-3 and 200x150 in slots 4-7
(scratch slots 8, 9: class 0). A launch carries one ring geometry, so the
planner groups by (kernel class, build key, frame class); a query's level
truncation comes from its own class; a query across classes fails the call.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "mcmtt_opticalflow_amd", "csrc")
ST, BX, TILED, LG = 0, 1, 2, 3  # psn::LkClass

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="hipcc absent")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = tmp_path_factory.mktemp("planclasses") / "lk_plan_classes"
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(ROOT, "tests", "cpp"),
                        os.path.join(ROOT, "tests", "cpp", "lk_plan_classes.cpp"), os.path.join(CSRC, "psn_lk_plan.cpp"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout.splitlines()[-1])


def test_launches_are_split_by_frame_class(plans):
    m = plans["mixed"]
    assert m["rc"] == 0 and m["tag"] >= 1000
    ls = m["launches"]
    # one launch per (kernel class, build key, frame class) ...
    groups = [(l["cls"], l["key"], l["fcls"]) for l in ls]
    assert len(set(groups)) == len(groups)
    # ... whose queries all lie in the launch's class, both slots
    for l in ls:
        assert l["q"] and all(q["prev_cls"] == l["fcls"] == q["next_cls"] for q in l["q"])
    # both kernel classes run in both frame classes: 21x21 and 32x32 in the single-tile
    # kernel, 32x80 (2,560 px > 1,024) in the box kernel
    assert {(l["cls"], l["fcls"]) for l in ls} >= {(ST, 0), (ST, 1), (BX, 0), (BX, 1)}
    for l in ls:
        wins = {(q["w"], q["h"]) for q in l["q"]}
        if l["cls"] == ST:
            assert wins == {(21, 21), (32, 32)}
        elif (32, 80) in wins:
            assert l["cls"] == BX and wins == {(32, 80)}
        else:  # the 70x201 window: class 0 only, a launch of its own
            assert wins == {(70, 201)} and l["fcls"] == 0
    # every point of every query is launched once
    assert sum(l["wgs"] for l in ls) == 13 * 12
    assert m["used"] == [0, 1, 4, 5, 2, 6]
    # at most one launch may take a deferred build along
    assert sum(l["fuse"] for l in ls) == 1


def test_max_level_comes_from_the_querys_class(plans):
    assert plans["levels"] == [1, 0]  # 32x80 at 320x240 and at 200x150
    got = {(l["fcls"], q["max_level"]) for l in plans["mixed"]["launches"] for q in l["q"] if (q["w"], q["h"]) == (32, 80)}
    assert got == {(0, 1), (1, 0)}
    # 21x21 keeps max_level 3 at 320x240 (level 3 is 40x30) and stops at 2 at 200x150 (level 3 would be 25x19: 19 <= 21)
    got = {(l["fcls"], q["max_level"]) for l in plans["mixed"]["launches"] for q in l["q"] if (q["w"], q["h"]) == (21, 21)}
    assert got == {(0, 3), (1, 2)}
    # the scratch slots are class 0's
    s = plans["scratch"]
    assert s["rc"] == 0 and [(l["fcls"], q["max_level"]) for l in s["launches"] for q in l["q"]] == [(0, 1)]


def test_no_merged_query_spans_classes(plans):
    m = plans["merge"]
    assert m["rc"] == 0
    qs = [(l["fcls"], q) for l in m["launches"] for q in l["q"]]
    # four uniform queries per class merge into one query of four sub-queries each
    assert sorted((f, q["sub_pts"], q["num_pts"], q["qidx"]) for f, q in qs) == [(0, 100, 400, 0), (1, 100, 400, 4)]
    assert all(q["prev_cls"] == f == q["next_cls"] for f, q in qs)
    assert len(m["launches"]) == 2


def test_cross_class_query_is_refused(plans):
    c = plans["cross"]
    assert c["rc"] == -1 and not c["launches"]  # PSN_LK_ERR_ARG, nothing planned for launch
    assert "3" in c["err"] and "4" in c["err"] and "class" in c["err"], c["err"]


def test_one_entry_table_plans_what_no_table_plans(plans):
    s = plans["sweep"]
    assert s["cases"] >= 250 and s["differ"] == 0, s
