"""The batch planner (psn_jpeg_batch_plan, csrc/psn_jpeg_parse.cpp) under
AddressSanitizer + UndefinedBehaviorSanitizer, on a machine without a GPU.

tests/cpp/jpeg_batch_check.cpp is compiled with psn_jpeg_parse.cpp only into a
program of its own (nothing is loaded into this process). It hands every batch
to psn_jpeg_batch_plan with each stream in a malloc block of exactly its length
and the item and plan arrays as exact. What it prints is compared with what the
shared library returns for the same batches: the same source in two builds, so
the two are equal exactly.

The batches: the item lists of tests/test_jpeg_batch.py with their refusals, and
every prefix of two small files placed mid-batch between intact files."""
import ctypes
import os
import shutil
import struct
import subprocess

import pytest

import jpeg_synth as js
import jpeg_variants as jv
from mcmtt_opticalflow_amd import _lib, lk
from test_jpeg_batch import FIXTURES, SYNTH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmtt_opticalflow_amd", "csrc")
# the flags of test_jpeg_host.py
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fsanitize=float-cast-overflow",
       "-static-libasan", "-static-libubsan"]
NULL_DATA, NULL_OUT = 1, 2
WIDE = 1 << 20
SWEPT = ("420_tiny", "geometry_gray_7x9")


def _batches():
    """(name, [(stream, flags, stride)], n handed to the library)."""
    fx = [jv.fixture(n)[0] for n in FIXTURES]
    sy = [js.case(n).data for n in SYNTH]
    plain = lambda fs: [(f, 0, WIDE) for f in fs]  # noqa: E731
    out = [("all", plain(fx + sy), None), ("reversed", plain((fx + sy)[::-1]), None), ("one", plain(fx[:1]), None),
           ("largest", plain([fx[1]] * _lib.JPEG_MAX_BATCH), None),
           ("too many", plain([fx[1]] * (_lib.JPEG_MAX_BATCH + 1)), None), ("n 0", plain(fx[:2]), 0),
           ("n -1", plain(fx[:2]), -1), ("fewer than given", plain(fx[:4]), 3),
           ("null data", plain(fx[:1]) + [(b"", NULL_DATA, WIDE)] + plain(fx[1:2]), None),
           ("null out", plain(fx[:2]) + [(fx[2], NULL_OUT, WIDE)], None)]
    w = lk.JpegDecoder.info(fx[1])[0]
    out.append(("short stride", [(fx[0], 0, WIDE), (fx[1], 0, 3 * w - 1), (fx[2], 0, WIDE)], None))
    out.append(("exact stride", [(fx[0], 0, WIDE), (fx[1], 0, 3 * w), (fx[2], 0, WIDE)], None))
    bad = fx[2][:2] + b"\x00\x00" + fx[2][4:]
    out.append(("corrupt header at 2 of 4", plain([fx[0], fx[1], bad, fx[3]]), None))
    for name in SWEPT:
        data = jv.fixture(name)[0] if name in FIXTURES else js.case(name).data
        e0, _ = jv.entropy_range(data)
        out += [(f"prefix {k} of {name}", plain([fx[0], data[:k], fx[4]]), None) for k in range(e0 + 4)]
    return out


def _library_lines(idx, items, n):
    """What jpeg_batch_check prints for the batch, from the shared library."""
    L = _lib.load()
    keep = [ctypes.create_string_buffer(d, len(d)) for d, _, _ in items]
    arr = (_lib.JpegItem * len(items))()
    for i, (d, flags, stride) in enumerate(items):
        arr[i] = _lib.JpegItem(None if flags & NULL_DATA else ctypes.addressof(keep[i]), len(d),
                               None if flags & NULL_OUT else 16, stride)
    lay, plans = _lib.JpegBatchLayout(), (_lib.JpegPlan * len(items))()
    rc = L.psn_jpeg_batch_plan(arr, n, ctypes.byref(lay), plans)
    tot = [lay.ent_args, lay.jpeg_args, lay.lists, lay.blob_size, lay.scratch_size, lay.coef_size, lay.planes_size]
    mx = [lay.max_sequences, lay.max_parallel_components, lay.max_segment_groups, lay.max_block_groups, lay.max_width,
          lay.max_height]
    sp = lambda xs: "".join(f" {x}" for x in xs)  # noqa: E731
    lines = [f"batch {idx} rc {rc} bad {lay.bad_item} n {lay.n} lists {lay.n_parallel} {lay.n_serial} totals{sp(tot)} "
             f"maxima{sp(mx)} par{sp(lay.parallel[:lay.n_parallel])} ser{sp(lay.serial[:lay.n_serial])}"]
    for i in range(lay.n if rc == 0 else 0):
        b, p = lay.item[i], plans[i]
        lines.append(f"item {idx} {i} path {b.path} {b.list_index} blob {b.tables} {b.segments} {b.bytes} {b.segments_size} "
                     f"{b.bytes_size} scratch {b.stats} {b.states} {b.counts} {b.prefix} {b.rounds} {b.states_size} "
                     f"{b.counts_size} {b.prefix_size} {b.rounds_size} out {b.coef} {b.coef_size} {b.planes} {b.planes_size} "
                     "plan " + " ".join(str(v) for v in _lib.struct_dict(p).values()))
    return lines, rc, lay.bad_item


@pytest.fixture(scope="module")
def batch_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("jpeg_batch_host")
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no host C++ compiler")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = tmp / "jpeg_batch_check"
    srcs = [os.path.join(ROOT, "tests", "cpp", "jpeg_batch_check.cpp"), os.path.join(CSRC, "psn_jpeg_parse.cpp")]
    objs = [str(tmp / (os.path.basename(s) + ".o")) for s in srcs]
    # no ROCm include path: plain host C++, as in test_jpeg_host.py
    jobs = [subprocess.Popen([cxx, "-O0", "-g", "-std=c++17", "-Wall", "-Wextra", "-D_GLIBCXX_ASSERTIONS", *SAN,
                              "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c", s, "-o", o])
            for s, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0, 0]
    subprocess.run([cxx, *SAN, *objs, "-o", str(exe)], check=True)
    return exe


def test_batch_planner_sanitized_equals_library(batch_exe, tmp_path):
    batches = _batches()
    case = tmp_path / "batches.bin"
    blob = b""
    for _, items, n in batches:
        blob += struct.pack("<Ii", len(items), len(items) if n is None else n)
        blob += b"".join(struct.pack("<IIi", len(d), fl, st) + d for d, fl, st in items)
    case.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(batch_exe), str(case)], capture_output=True, text=True, env=env, timeout=600)
    got = r.stdout.splitlines()
    if r.returncode != 0:
        seen = sum(ln.startswith("batch ") for ln in got)
        pytest.fail(f"ended in batch '{batches[min(seen, len(batches) - 1)][0]}'\n" + r.stdout[-1000:] + r.stderr[-6000:])
    assert got[-1] == f"jpeg batch check: ok {len(batches)}"
    want, answers = [], {}
    for idx, (name, items, n) in enumerate(batches):
        lines, rc, bad = _library_lines(idx, items, len(items) if n is None else n)
        want += [(name, ln) for ln in lines]
        answers[name] = (rc, bad)
    assert len(got) - 1 == len(want)
    for g, (name, w) in zip(got, want):
        assert g == w, name
    # the case set has not gone soft
    assert answers["all"] == answers["largest"] == answers["exact stride"] == answers["fewer than given"] == (0, -1)
    assert answers["too many"] == answers["n 0"] == answers["n -1"] == (-1, -1)
    assert answers["null data"] == (-1, 1) and answers["null out"] == (-1, 2) and answers["short stride"] == (-1, 1)
    assert answers["corrupt header at 2 of 4"] == (-1, 2)
    for name in SWEPT:
        swept = [v for k, v in answers.items() if k.startswith("prefix ") and k.endswith(" of " + name)]
        assert (0, -1) in swept and (-1, 1) in swept and {bad for rc, bad in swept if rc} == {1}
