"""The LK launch planner (csrc/psn_lk_plan.cpp) on the CPU.

tests/cpp/lk_plan_dump links the planner alone (no libpsn_lk.so, no GPU) and
prints, for every call of the sweep in tests/cpp/lk_plan_sweep.h, what
psn::plan_call plans: per launch the kernel, its template parameters, grid, LDS
and every LkQueryDev field of every query (min_eig / eps2 as hex floats), and
for a bad call its error code and text; the first line names the values of the
arrays. tests/golden/lk_plan_parent.jsonl holds
the same lines recorded from the commit before the planner left
psn_lk_abi.cpp (that commit's track_device_impl, run with the kernel launchers
stubbed). Every line must be equal: a planner change shows as a diff of the record.
"""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS_DIR = os.path.join(HERE, "cpp")
BIN = os.path.join(HARNESS_DIR, "bin", "lk_plan_dump")
RECORD = os.path.join(HERE, "golden", "lk_plan_parent.jsonl")


def _dump_lines():
    subprocess.run(["make", "-s", "-C", HARNESS_DIR, "bin/lk_plan_dump"], check=True, timeout=300)
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return p.stdout.splitlines()


def test_plans_equal_the_record():
    got = _dump_lines()
    with open(RECORD) as f:
        want = f.read().splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            jg, jw = json.loads(g), json.loads(w)
            keys = [k for k in jw if jg.get(k) != jw[k]]
            raise AssertionError(f"line {i + 1} ({jw.get('case')}): differs in {keys}\n got: {g}\nwant: {w}")
    assert len(got) == len(want)


def test_planner_binary_stands_alone():
    """lk_plan_dump has no part of the library behind it."""
    _dump_lines()
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True, timeout=60).stdout
    assert "libpsn" not in out, out


def test_record_covers_the_planner():
    """The record holds every kernel class, every planner error code and the
    multi-query rules (not a property of the code under test: a guard against a
    record that was cut down)."""
    with open(RECORD) as f:
        legend, *calls = [json.loads(line) for line in f]
    shape = legend["legend"]["shape"].split(",")
    qf = legend["legend"]["q"].split(",")
    assert len(calls) >= 250
    launches = [l for c in calls for l in c["launches"]]
    assert all(len(l["shape"]) == len(shape) and all(len(q) == len(qf) for q in l["q"]) for l in launches)
    assert {l["kernel"] for l in launches} == {"st", "bx", "tiled", "lg"}
    # PSN_LK_ERR_ARG, _WINSIZE, _SLOT, _LEVEL_CAP, _UNSUPPORTED
    assert {c["rc"] for c in calls} == {0, -1, -2, -5, -6, -8}
    assert all(not c["launches"] for c in calls if c["rc"])
    assert any(q[qf.index("sub_pts")] for l in launches for q in l["q"])  # merged sub-queries
    assert any(len(l["q"]) == 32 for l in launches)  # a split at kMaxQueries
    assert any(l["shape"][shape.index("occ")] == 3 for l in launches)  # three single-tile workgroups per CU
    assert any(l["shape"][shape.index("fuse")] for l in launches)
    assert any(c["counted"] and c["stride"] == 3 for c in calls)
    assert {tuple(c["frame"][:2]) for c in calls} >= {(1920, 1080), (640, 480), (3840, 2160), (960, 540)}
