"""The tile arithmetic of the chain lanes' straight-line tile step (CPU, no GPU):
lk_kernel_fw<10, true> sums a FULL fallback tile (all tile threads x units per
thread units inside the window) by chain_sum_nt<NB> with the region stride S and
the plane pitch P taken once per fallback (bx_nt_tile_blocks / _S / _P,
csrc/psn_lk_kernels.h); a partial last tile keeps bx_tile_slots_nt and
chain_sum_pl. The same arithmetic is checked for the two-wave build
lk_kernel_bx<8, true, 128>, whose tiles it describes as well (that build keeps
chain_sum_pl: the straight-line sum measured no gain there). For every window
either build accepts:
NB whole blocks are exactly a tile's terms per lane chain, the kernel's test of a
full tile (tile units x (g + 1) <= U) picks exactly the tiles whose unit range is
whole, every such tile's per-tile values (bx_tile_slots_nt, bx_region) equal the
hoisted constants, and the partial tile is what is left. The windows of
tests/test_bx_chain_tile_step_gpu.py are checked by name."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="hipcc absent")

PROGRAM = r"""
#include <cstdio>
#include "psn_lk_kernels.h"
using namespace psn;
struct Build { int upt, tg, nt; };
// the windows a build accepts (no tail: SSE2 order, w a multiple of 8), as plan_query takes them
static bool accepts(const Build &b, int w, int h) {
    const long U = (long)h * bx_qw(w);
    if (b.nt == kBxNT2) return bx_two_wave_fits(w, h, true);
    const long need = (U + kBxNT - 1) / kBxNT;
    return need > 8 && need <= kBxFwUPT && BxLayout(w, h, b.upt).total <= bx_max_lds(b.upt, true) &&
           (long)st_jreg_h(h) * bx_jrp(w) < 65536;
}
int main() {
    const Build builds[2] = {{kBxFwUPT, kBxTile, kBxNT}, {kBxUPT2, kBxTile2, kBxNT2}};
    std::printf("{");
    for (int bi = 0; bi < 2; bi++) {
        const Build &b = builds[bi];
        const int TU = b.tg * b.upt, NB = bx_nt_tile_blocks(b.upt, b.tg), SF = bx_nt_tile_S(b.upt, b.tg),
                  PF = bx_nt_tile_P(b.upt, b.tg);
        long windows = 0, tiles = 0, full = 0, partial = 0, bad = 0;
        for (int w = 8; w <= 512; w += 8)
            for (int h = 3; h <= 1024; h++) {
                if (!accepts(b, w, h)) continue;
                windows++;
                const int U = h * bx_qw(w), g_last = (U - 1) / TU;
                long nfull = 0;
                for (int g = 0; g <= g_last; g++) {
                    const int ua = TU * g, ub = ua + TU < U ? ua + TU : U;
                    int sa, ta, nsse, ntail;
                    bx_tile_slots_nt(ua, ub, sa, ta, nsse, ntail);
                    const int S = bx_region(nsse), P = 4 * S + bx_region(ntail);
                    const bool is_full = TU * (g + 1) <= U;  // the kernel's test
                    tiles++;
                    bad += is_full != (ub - ua == TU);
                    if (is_full) {
                        nfull++;
                        // the slot base is the tile's unit range; S, P and the block count are the build's
                        bad += sa != ua || ta != 0 || ntail != 0 || nsse != TU || S != SF || P != PF ||
                               ((nsse + 15) >> 4) != NB;
                    } else {
                        partial++;
                        bad += g != g_last || nsse != U %% TU || nsse <= 0;
                    }
                }
                full += nfull;
                bad += nfull != U / TU;
            }
        std::printf("%%s\"%%d\": {\"nb\": %%d, \"tile_units\": %%d, \"S\": %%d, \"P\": %%d, \"windows\": %%ld, \"tiles\": %%ld, "
                    "\"full\": %%ld, \"partial\": %%ld, \"bad\": %%ld}",
                    bi ? ", " : "", b.nt, NB, TU, SF, PF, windows, tiles, full, partial, bad);
    }
    const int named[][2] = {%s};
    std::printf(", \"named\": [");
    for (unsigned i = 0; i < sizeof(named) / sizeof(named[0]); i++) {
        const int w = named[i][0], h = named[i][1];
        const Build &b = accepts(builds[1], w, h) ? builds[1] : builds[0];
        const int U = h * bx_qw(w), TU = b.tg * b.upt;
        std::printf("%%s[%%d, %%d, %%d, %%d, %%d, %%d]", i ? ", " : "", w, h, accepts(b, w, h) ? b.nt : 0, U, U / TU, U %% TU);
    }
    std::printf("]}\n");
    return 0;
}
"""

# window -> (workgroup threads of the build that takes it, units, full tiles, units of the partial tile)
NAMED = {(64, 160): (256, 2560, 8, 0), (56, 160): (256, 2240, 7, 0), (64, 129): (256, 2064, 6, 144),
         (64, 64): (128, 1024, 8, 0), (32, 32): (128, 256, 2, 0), (24, 24): (128, 144, 1, 16)}


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("chain_tile_step")
    src, exe = d / "tiles.hip", d / "tiles"
    src.write_text(PROGRAM % ", ".join("{%d, %d}" % k for k in NAMED))
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mcmtt_opticalflow_amd", "csrc"),
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    p = json.loads(out.stdout)
    print(p)
    return p


def test_block_counts_are_the_tiles_terms(model):
    fw, two = model["256"], model["128"]
    assert (fw["nb"], fw["tile_units"]) == (20, 320) and (two["nb"], two["tile_units"]) == (8, 128)
    for b in (fw, two):
        assert b["nb"] * 16 == b["tile_units"]
        # a region of whole blocks + 4 floats, a plane of four lane regions + the empty tail region
        assert b["S"] == b["tile_units"] + 4 and b["P"] == 4 * b["S"] + 4


def test_hoisted_geometry_equals_every_full_tiles(model):
    for b in (model["256"], model["128"]):
        assert b["windows"] > 50 and b["full"] > b["windows"] and b["partial"] > 0
        assert b["full"] + b["partial"] == b["tiles"]
        assert b["bad"] == 0


def test_named_windows(model):
    got = {(w, h): (nt, u, nfull, part) for w, h, nt, u, nfull, part in model["named"]}
    assert got == NAMED
