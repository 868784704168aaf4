"""bench.py's multi-GPU plumbing on CPU: `--gpus N` starts N rank processes
itself (one per GPU, RANK / LOCAL_RANK / WORLD_SIZE set before anything touches
a GPU), the ranks join the gloo control plane, shard the cameras (weak: C per
GPU; strong, SURVEY 8(e): --total-cameras M split over the ranks, index ==
camID order as Associator3D requires, PSNWhere_Associator3D.cpp:1105-1116) and
time with barrier + max-over-ranks. --dry-run skips the GPU work."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*argv, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                       timeout=240, env=e, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout  # rank 0 only
    return json.loads(lines[0])


def test_launcher_world2_weak():
    out = _run("--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1")
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["steps"] == 3
    assert out["cameras_by_rank"] == [[0, 1, 2, 3], [4, 5, 6, 7]]  # configs[2] per GPU


@pytest.mark.parametrize("n", [2, 4])
def test_launcher_strong_configs3(n):
    out = _run("--gpus", str(n), "--dry-run", "--total-cameras", "8", "--points", "2048", "--boxes", "32")
    assert out["n_gpus"] == n and out["scaling"] == "strong"
    per = 8 // n
    assert out["cameras_by_rank"] == [list(range(r * per, r * per + per)) for r in range(n)]


def test_launcher_single_and_bad_split():
    out = _run("--dry-run", "--total-cameras", "8")
    assert out["n_gpus"] == 1 and out["cameras_by_rank"] == [list(range(8))]
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--dry-run",
                        "--total-cameras", "8"], capture_output=True, text=True, timeout=240, env=e, cwd=ROOT)
    assert p.returncode != 0  # 8 cameras do not split over 3 ranks: every rank fails, the launcher reports it


def test_plain_run_is_the_headline_alone():
    """Without --full nothing beside the timed steps runs; --full keeps every
    leg, and the --no-* options still drop their part of it."""
    sys.path.insert(0, ROOT)
    import bench

    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.measure_steps, a.isolated) == (7, 2, 0, False)
    assert a.no_cpu_baseline and a.no_secondary and a.no_legs and not a.full and a.dump_outputs is None
    f = bench.parse_args(["--full"])
    assert f.measure_steps == 20 and f.isolated
    assert not (f.no_cpu_baseline or f.no_secondary or f.no_legs)
    g = bench.parse_args(["--full", "--no-legs", "--no-isolated", "--measure-steps", "5"])
    assert g.no_legs and not g.isolated and g.measure_steps == 5 and not g.no_secondary
    # every leg is a --full line of its own process, without legs of its own
    c = bench.parse_args(bench.child_args(f, steps=3))
    assert c.full and c.measure_steps == 20 and c.no_legs and c.no_secondary and c.no_cpu_baseline and c.steps == 3


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: the packed result slots of a step, unpacked into float64 .npy files."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench
    from mcmtt_opticalflow_amd import tracker2d as t2d

    rng = np.random.default_rng(5)
    nb = t2d.result_slot_bytes(4, 1)
    rows = np.zeros((2, nb), np.uint8)
    results = []
    for cam in range(2):
        objs = [{"id": 10 * cam + k, "box": (1.0 + k, 2.0, 64.0, 160.0), "head": (17.0, 2.0, 32.0, 20.0),
                 "score": 0.25 * k, "prev": rng.uniform(0, 1900, (3 + k, 2)).astype(np.float32),
                 "curr": rng.uniform(0, 1900, (2 + k, 2)).astype(np.float32)} for k in range(2 + cam)]
        results.append({"cam_id": cam, "frame_idx": 6, "objects": objs, "detection_rects": [], "tracker_rects": []})
        t2d.pack_result(results[-1], rows[cam])
    bench.dump_tracker_outputs(str(tmp_path / "out"), {"timed_last": rows, "max_obj": 4})
    got = {n: np.load(tmp_path / "out" / (n + ".npy")) for n in ("objects", "points_prev", "points_curr")}
    assert all(a.dtype == np.float64 for a in got.values())
    objs = [(r["cam_id"], o) for r in results for o in r["objects"]]
    assert got["objects"].shape == (5, 14)
    for row, (cam, o) in zip(got["objects"], objs):
        assert row.tolist() == [cam, 6, o["id"], *o["box"], *o["head"], o["score"], len(o["prev"]), len(o["curr"])]
    for name, key in (("points_prev", "prev"), ("points_curr", "curr")):
        exp = np.concatenate([np.column_stack([np.full(len(o[key]), cam), np.full(len(o[key]), o["id"]), o[key]])
                              for cam, o in objs])
        np.testing.assert_array_equal(got[name], exp)


def _bench_with_dump(out_dir, *argv):
    """One bench.py run in a process of its own: (the JSON line, the dumped arrays)."""
    import numpy as np

    line = _run(*argv, "--dump-outputs", str(out_dir))
    return line, {n: np.load(os.path.join(out_dir, n + ".npy")) for n in ("objects", "points_prev", "points_curr")}


@pytest.mark.gpu
def test_plain_line_and_dump_outputs_gpu(tmp_path):
    """A plain run on the GPU: --steps sets the timed steps, the line carries the
    headline fields and none of --full's legs, and two runs with the same
    arguments dump the same outputs (seeded inputs, bit-exact kernels)."""
    import numpy as np

    argv = ("--gpus", "1", "--steps", "3", "--warmup", "2", "--cameras", "2")
    line, a = _bench_with_dump(tmp_path / "a", *argv)
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (3, 2, 1)
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "u8+f32"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(2 * 1e3 / line["ms_per_step"], rel=1e-3)  # 2 cameras per step
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert "legs" not in line and "secondary" not in line
    # the last timed frame (index warm-up + steps - 1) of both cameras
    assert set(a["objects"][:, 0]) == {0.0, 1.0} and set(a["objects"][:, 1]) == {4.0}
    assert len(a["objects"]) > 0 and len(a["points_curr"]) == a["objects"][:, 13].sum()
    assert len(a["points_prev"]) == a["objects"][:, 12].sum()
    assert all(np.isfinite(v).all() for v in a.values())
    _, b = _bench_with_dump(tmp_path / "b", *argv)
    for name in a:
        np.testing.assert_array_equal(a[name], b[name])


def test_algorithmic_bytes_match_survey():
    """SURVEY 8(d)'s per-camera-frame figures (gray input)."""
    sys.path.insert(0, ROOT)
    import bench

    for (w, h, lv, n), exp in [((640, 480, 3, 64), 1902144), ((1920, 1080, 4, 512), 13067952),
                               ((1920, 1080, 4, 2048), 13100208), ((3840, 2160, 5, 4096), 52541616)]:
        pyr, lk = bench.algorithmic_bytes(w, h, lv, n)
        assert pyr + lk == exp
