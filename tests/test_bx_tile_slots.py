"""The fallback tile geometry of the box kernel (CPU, no GPU): the chain slots of a
tile's unit range, csrc/psn_lk_kernels.h. In the no-tail builds (SSE2 order,
w % 8 == 0: every quad feeds the four lane chains, no tail chain) the short form
bx_tile_slots_nt -- the unit range itself, no division -- must equal the general
bx_tile_slots for every tile of every window such a build can take, and a full
tile must be whole 16-float blocks in every instantiated build, so that only a
window's last tile has a pad to zero."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = os.path.join(ROOT, "mcmtt_opticalflow_amd", "csrc", "psn_lk_bx.hip")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="hipcc absent")

PROGRAM = r"""
#include <cstdio>
#include "psn_lk_kernels.h"
using namespace psn;
int main() {
    const int builds[][2] = {%s};  // units per thread, tile threads
    long tiles = 0, bad = 0, padded_not_last = 0;
    for (auto &b : builds) {
        const int upt = b[0], tg = b[1], nt = tg == kBxTile2 ? kBxNT2 : kBxNT;
        for (int w = 8; w <= 256; w += 8)
            for (int h = 1; h <= 256; h++) {
                const int qw = bx_qw(w), U = h * qw;
                if (U > nt * upt) break;
                for (int hw = 1; hw <= (tg == kBxTile2 ? 1 : 8); hw++) {
                    const int g_last = (U - 1) / (tg * upt);
                    for (int h0 = 0; h0 < 8 && h0 * (kBxTile / tg) <= g_last; h0++)  // the chains start at a half wave
                        for (int g = h0 * (kBxTile / tg); g <= g_last; g += hw) {
                            const int ua = tg * upt * g, ub = ua + tg * upt * hw < U ? ua + tg * upt * hw : U;
                            int s[4], t[4];
                            // no tail: nq = qw SSE2 quads per row, no tail pixels from n4 = w on
                            bx_tile_slots(ua, ub, qw, qw, w, 0, s[0], s[1], s[2], s[3]);
                            bx_tile_slots_nt(ua, ub, t[0], t[1], t[2], t[3]);
                            tiles++;
                            bad += s[0] != t[0] || s[1] != t[1] || s[2] != t[2] || s[3] != t[3];
                            padded_not_last += (t[2] %% 16 != 0) && ub != U;
                        }
                }
            }
    }
    // a tail window keeps the general form: 44 x 40 (11 quads per row, 10 of them SSE2 at the b
    // chains' 8-pixel steps, 4 tail pixels), the tile of units [128, 256)
    int sa, ta, nsse, ntail;
    bx_tile_slots(128, 256, 11, 10, 40, 4, sa, ta, nsse, ntail);
    std::printf("{\"tiles\": %%ld, \"bad\": %%ld, \"padded_not_last\": %%ld, \"tail\": [%%d, %%d, %%d, %%d]}\n", tiles, bad,
                padded_not_last, sa, ta, nsse, ntail);
    return 0;
}
"""


def _builds():
    """The instantiated no-tail builds, from the kernel list of the source: (units
    per thread, tile threads) -- half-wave tiles, quarter waves in the two-wave build."""
    src = open(KERNELS).read()
    hdr = open(os.path.join(os.path.dirname(KERNELS), "psn_lk_kernels.h")).read()
    const = {k: int(v) for k, v in re.findall(r"\b(kBx(?:NT2?|UPT2|Tile2?)) = (\d+)[,;]", hdr)}
    body = re.search(r"#define PSN_BX_KERNELS\(X\)((?:.*\\\n)*.*)\n", src).group(1)
    out = []
    for upt, notail, nt in re.findall(r"X\((\w+), (true|false), (\w+)\)", body):
        if notail == "true":
            upt = const.get(upt) or int(upt)
            out.append((upt, const["kBxTile2"] if const[nt] == const["kBxNT2"] else const["kBxTile"]))
    return out


def test_full_no_tail_tiles_are_whole_blocks():
    builds = _builds()
    print("no-tail builds (units per thread, tile threads):", builds)
    assert len(builds) == 6 and (8, 16) in builds and (10, 32) in builds
    for upt, tg in builds:
        assert (upt * tg) % 16 == 0, (upt, tg)


def test_short_form_equals_general_form(tmp_path):
    src, exe = tmp_path / "slots.hip", tmp_path / "slots"
    src.write_text(PROGRAM % ", ".join("{%d, %d}" % b for b in _builds()))
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mcmtt_opticalflow_amd", "csrc"),
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    p = json.loads(out.stdout)
    print(p)
    assert p["tiles"] > 100000 and p["bad"] == 0
    assert p["padded_not_last"] == 0  # only a window's last tile has a pad
    # 44 x 40, units [128, 256): rows 11 r + q; 128 = row 11 quad 7, 256 = row 23 quad 3
    #   SSE2 slots before: 11 * 10 + 7 = 117, in the tile: 23 * 10 + 3 - 117 = 116
    #   tail pixels before: 11 * 4 + 0 = 44, in the tile: 23 * 4 + 0 - 44 = 48
    assert p["tail"] == [117, 44, 116, 48]
