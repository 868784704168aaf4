"""The JPEG host side (csrc/psn_jpeg_parse.cpp: marker parser, Huffman table
builder, planner; csrc/psn_jpeg_model.cpp: the CPU model of the entropy decode)
under AddressSanitizer + UndefinedBehaviorSanitizer, on a machine without a GPU.

tests/cpp/jpeg_host_check.cpp is compiled with those two units only into a
program of its own (nothing is loaded into this process). It hands every stream
to psn_jpeg_info, psn_jpeg_entropy_plan and psn_jpeg_entropy_model from a malloc
block of exactly the stream's length, so a read of one byte past a stream -- which
a bytes object's slack hides from ctypes -- ends the run. What it prints is
compared with what the shared library returns for the same bytes: the same source
in two builds, so the two are equal exactly.

The streams: every case of jpeg_synth, every golden fixture with the variants of
jpeg_variants, every prefix of two small files to two bytes past the first entropy
byte, and headers written by hand around each length check of the parser. That
the set still reaches an accepted stream, both refusals and both planner paths is
asserted from the library's own answers."""
import ctypes
import functools
import os
import shutil
import struct
import subprocess

import pytest

import jpeg_synth as js
import jpeg_variants as jv
from mcmtt_opticalflow_amd import _lib, lk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmtt_opticalflow_amd", "csrc")
# the flags of test_flow_steps.py
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fsanitize=float-cast-overflow",
       "-static-libasan", "-static-libubsan"]
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -8
MODELS = [(1, 0), (2, 4), (2, 64), (2, 1024)]  # (mode, sub_bytes) of psn_jpeg_entropy_model
NO_MODEL = 1  # case file flag: psn_jpeg_info and psn_jpeg_entropy_plan only
SWEPT = ("fixture 420_tiny", "synth geometry_gray_7x9")

SOI = b"\xff\xd8"
SOF_16x16_3 = bytes.fromhex("08 0010 0010 03 01 22 00 02 11 01 03 11 01")


def _hand_made():
    """(name, stream, flags): each ends where the length check it is for has to stop the parser."""
    seg = js._segment
    frame = SOI + seg(0xC0, SOF_16x16_3)
    first = bytes.fromhex("FF D8  FF C0 00 11 08 00 10 00 10 03 01 22 00 02 11 01 03 11 01  FF DA 00 03 03")
    assert first == frame + seg(0xDA, b"\x03") and len(first) == 26
    gray = SOI + seg(0xC0, bytes.fromhex("08 0010 0010 01 01 11 00"))
    spec = js._std_spec(16, 16, 3, (2, 2))
    return [
        ("sos_count_only", first, 0),
        ("sos_one_short_3", frame + seg(0xDA, bytes.fromhex("03 01 00 02 11 03")), 0),
        ("sos_one_short_1", gray + seg(0xDA, bytes.fromhex("01 01")), 0),
        ("sof_one_short", SOI + seg(0xC0, SOF_16x16_3[:-1]), 0),
        ("dht_counts_past_segment", SOI + seg(0xC4, bytes([0x00] + [0, 2, 3, 7] + [0] * 12 + [0, 1, 2, 3, 4])), 0),
        ("dht_counts_cut", SOI + seg(0xC4, bytes([0x10] + [0, 1, 2])), 0),
        ("dqt16_cut", SOI + seg(0xDB, bytes([0x10]) + bytes(range(1, 65))), 0),
        ("dri_empty", frame + seg(0xDD, b""), 0),
        ("fill_bytes_to_end", SOI + b"\xff" * 9, 0),
        ("four_bytes", SOI + jv.EOI, 0),
        ("frame_65535", js._headers(spec, (65535, 65535)) + b"\x12\x34", NO_MODEL),
    ]


@functools.lru_cache(maxsize=None)
def _streams():
    out = [(f"synth {n}", js.case(n).data, 0) for n in list(js._BUILDERS) + js.ILL_FORMED_CASES]
    for name in sorted(jv.PLAIN) + list(jv.RESTART):
        data, _ = jv.fixture(name)
        out.append((f"fixture {name}", data, 0))
        e0, e1 = jv.entropy_range(data)
        for variant in (jv.truncated, jv.corrupted, jv.with_fill_byte, jv.ending_in_ff):
            if variant is jv.corrupted and name == "420_tiny":  # 23 entropy bytes: no room for its eight bytes, 37 apart
                continue
            if variant in (jv.with_fill_byte, jv.ending_in_ff) and data.find(b"\xff\x00", e0, e1) < 0:
                continue
            out.append((f"{variant.__name__} {name}", variant(data), 0))
    by_name = {n: d for n, d, _ in out}
    for name in SWEPT:
        data = by_name[name]
        e0, _ = jv.entropy_range(data)
        out += [(f"prefix {k} of {name}", data[:k], 0) for k in range(e0 + 4)]  # to two bytes past the first entropy byte
    return out + [(f"hand {n}", d, f) for n, d, f in _hand_made()]


@functools.lru_cache(maxsize=64)
def _fnv(data: bytes) -> int:
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _library_lines(idx, data, flags):
    """What jpeg_host_check prints for the stream, from the shared library."""
    L = _lib.load()
    w, h, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    info = L.psn_jpeg_info(data, len(data), ctypes.byref(w), ctypes.byref(h), ctypes.byref(c))
    try:
        plan, p = OK, lk.JpegDecoder.plan(data)
    except lk.PsnLkError as e:
        plan, p = e.code, _lib.struct_dict(_lib.JpegPlan())
    lines = [f"stream {idx} len {len(data)} info {info} {w.value} {h.value} {c.value} plan {plan} "
             + " ".join(str(v) for v in p.values())]
    for mode, sub in () if flags & NO_MODEL else MODELS:
        try:
            coef, st = lk.JpegDecoder.model(data, mode, sub)
            lines.append(f"model {idx} {mode} {sub} rc 0 stats " + " ".join(str(v) for v in st.values())
                         + f" fnv {_fnv(coef.tobytes()):016x}")
        except lk.PsnLkError as e:
            lines.append(f"model {idx} {mode} {sub} rc {e.code}")
    return lines, info, (p["path"] if plan == OK else None)


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("jpeg_host")
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no host C++ compiler")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = tmp / "jpeg_host_check"
    srcs = [os.path.join(ROOT, "tests", "cpp", "jpeg_host_check.cpp"), os.path.join(CSRC, "psn_jpeg_parse.cpp"),
            os.path.join(CSRC, "psn_jpeg_model.cpp")]
    objs = [str(tmp / (os.path.basename(s) + ".o")) for s in srcs]
    # no ROCm include path: the two units are plain host C++. -O0 leaves every load and store to the
    # sanitizers; _GLIBCXX_ASSERTIONS: an index past a vector's size may stay inside its capacity
    jobs = [subprocess.Popen([cxx, "-O0", "-g", "-std=c++17", "-Wall", "-Wextra", "-D_GLIBCXX_ASSERTIONS", *SAN,
                              "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c", s, "-o", o])
            for s, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0, 0, 0]
    subprocess.run([cxx, *SAN, *objs, "-o", str(exe)], check=True)
    return exe


def test_jpeg_host_side_sanitized_equals_library(host_exe, tmp_path):
    streams = _streams()
    case = tmp_path / "streams.bin"
    case.write_bytes(b"".join(struct.pack("<II", len(d), f) + d for _, d, f in streams))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(host_exe), str(case)], capture_output=True, text=True, env=env, timeout=600)
    got = r.stdout.splitlines()
    if r.returncode != 0:  # a stream's line follows its info and plan calls and precedes its model calls
        seen = sum(ln.startswith("stream ") for ln in got)
        pytest.fail(f"ended in the model of '{streams[seen - 1][0] if seen else None}' or the headers of "
                    f"'{streams[min(seen, len(streams) - 1)][0]}'\n" + r.stdout[-1000:] + r.stderr[-6000:])
    assert got[-1] == f"jpeg host check: ok {len(streams)}"
    want, infos, paths, accepted = [], set(), set(), set()
    for idx, (name, data, flags) in enumerate(streams):
        lines, info, path = _library_lines(idx, data, flags)
        want += [(name, ln) for ln in lines]
        infos.add(info)
        paths.add(path)
        if info == OK and name.startswith("prefix "):
            accepted.add(name.split(" of ", 1)[1])
    assert len(got) - 1 == len(want)
    for g, (name, w) in zip(got, want):
        assert g == w, name
    # the case set has not gone soft
    assert infos == {OK, ERR_ARG, ERR_UNSUPPORTED}
    assert {_lib.JPEG_PATH_SERIAL, _lib.JPEG_PATH_PARALLEL} <= paths
    assert accepted == set(SWEPT)
    by_name = {n: i for i, (n, _, _) in enumerate(streams)}
    hand = {n: _library_lines(0, streams[i][1], NO_MODEL)[1] for n, i in by_name.items() if n.startswith("hand ")}
    assert hand["hand frame_65535"] == ERR_UNSUPPORTED
    assert {v for n, v in hand.items() if n != "hand frame_65535"} == {ERR_ARG, ERR_UNSUPPORTED}
    assert hand["hand sos_count_only"] == hand["hand sos_one_short_3"] == hand["hand sos_one_short_1"] == ERR_ARG
