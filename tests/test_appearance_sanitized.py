"""The host-only appearance code (crop arithmetic, 'PT2A' pack / unpack) under
AddressSanitizer + UndefinedBehaviorSanitizer: tracker2d_appearance.cpp and the
stand-alone caller tests/cpp/appearance_host_check.cpp are compiled together
into one program of their own and that program is run (no GPU, nothing loaded
into this process)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the runtimes are linked into the program, so nothing about it depends on the order in
# which the dynamic loader maps other libraries
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fsanitize=float-cast-overflow",
       "-static-libasan", "-static-libubsan"]


def test_appearance_host_code_sanitized(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no host C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = tmp_path / "appearance_host_check"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", *SAN, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "appearance_host_check.cpp"),
                    os.path.join(ROOT, "mcmtt_opticalflow_amd", "host", "tracker2d_appearance.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "appearance host check: ok" in r.stdout
