"""The batch planner (psn_jpeg_batch_plan, csrc/psn_jpeg_parse.cpp; host only):
where psn_jpeg_decode_batch_device puts every item's tables, segment offsets,
entropy bytes, scratch, coefficients and planes, the two path lists and the
launches' grid maxima -- on the golden fixtures and on jpeg_synth cases."""
import numpy as np
import pytest

import jpeg_synth as js
import jpeg_variants as jv
from mcmtt_opticalflow_amd import _lib, lk

OK, ERR_ARG = 0, -1
FIXTURES = sorted(jv.PLAIN) + list(jv.RESTART)
SYNTH = ["ambiguous444", "ladder_ff", "geometry_gray_7x9", "geometry_420_17x9", "truncated_ladder_ff", "multipass"]

BLOB = [("tables", None), ("segments", "segments_size"), ("bytes", "bytes_size")]
SCRATCH = [("stats", None), ("states", "states_size"), ("counts", "counts_size"), ("prefix", "prefix_size"),
           ("rounds", "rounds_size")]


def _files():
    return [jv.fixture(n)[0] for n in FIXTURES] + [js.case(n).data for n in SYNTH]


def _disjoint(ranges, total):
    ranges = sorted(r for r in ranges if r[1] > r[0])
    for (a0, a1), (b0, b1) in zip(ranges, ranges[1:]):
        assert a1 <= b0, (a0, a1, b0, b1)
    assert not ranges or ranges[-1][1] <= total


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_layout(order):
    files = _files() if order == "forward" else _files()[::-1]
    r = lk.JpegDecoder.batch_plan(files)
    assert r["rc"] == OK
    L, plans = r["layout"], r["plans"]
    assert L["n"] == len(files) and L["bad_item"] == -1
    singles = [lk.JpegDecoder.plan(f) for f in files]
    assert plans == singles  # the planner's choice per file is the single file's
    blob, scratch, coef, planes = [], [], [], []
    for i, (f, it, p) in enumerate(zip(files, L["item"], plans)):
        for k, v in it.items():
            if k not in ("path", "list_index"):
                assert v % 16 == 0, (i, k, v)
        assert it["path"] == p["path"]
        assert it["bytes_size"] >= p["entropy_bytes"] + 16  # the item's own slack
        assert it["segments_size"] >= 4 * p["segments"]
        w, h, nc = lk.JpegDecoder.info(f)
        blocks = it["planes_size"] // 64
        assert it["coef_size"] == 128 * blocks and blocks >= jv.scan_blocks(f) - 0 and blocks > 0
        if p["path"] == _lib.JPEG_PATH_PARALLEL:
            assert it["states_size"] >= 8 * p["subsequences"] and it["counts_size"] >= 4 * p["subsequences"]
            assert it["prefix_size"] >= 4 * p["subsequences"] and it["rounds_size"] >= 4 * p["sequences"]
        else:
            assert it["states_size"] == it["counts_size"] == it["prefix_size"] == it["rounds_size"] == 0
        blob += [(it["tables"], it["segments"])] + [(it[o], it[o] + it[s]) for o, s in BLOB[1:]]
        scratch += [(it["stats"], it["stats"] + 16)] + [(it[o], it[o] + it[s]) for o, s in SCRATCH[1:]]
        coef.append((it["coef"], it["coef"] + it["coef_size"]))
        planes.append((it["planes"], it["planes"] + it["planes_size"]))
    n = len(files)
    assert L["ent_args"] < L["jpeg_args"] < L["lists"] and L["lists"] + 8 * n <= L["blob_size"]
    for k in ("ent_args", "jpeg_args", "lists", "blob_size", "scratch_size", "coef_size", "planes_size"):
        assert L[k] % 16 == 0
    _disjoint(blob + [(L["ent_args"], L["jpeg_args"]), (L["jpeg_args"], L["lists"]), (L["lists"], L["lists"] + 8 * n)],
              L["blob_size"])
    _disjoint(scratch, L["scratch_size"])
    _disjoint(coef, L["coef_size"])
    _disjoint(planes, L["planes_size"])
    # the two lists partition the items, each ascending, and list_index is the position
    par = [i for i, p in enumerate(plans) if p["path"] == _lib.JPEG_PATH_PARALLEL]
    ser = [i for i, p in enumerate(plans) if p["path"] == _lib.JPEG_PATH_SERIAL]
    assert L["parallel"] == par and L["serial"] == ser and par and ser
    assert (L["n_parallel"], L["n_serial"]) == (len(par), len(ser))
    for lst in (par, ser):
        assert [L["item"][i]["list_index"] for i in lst] == list(range(len(lst)))
    # grid maxima
    info = [lk.JpegDecoder.info(f) for f in files]
    assert L["max_sequences"] == max(plans[i]["sequences"] for i in par)
    assert L["max_parallel_components"] == max(info[i][2] for i in par)
    assert L["max_segment_groups"] == max(-(-plans[i]["segments"] // 64) for i in ser)
    assert L["max_block_groups"] == max(-(-(it["planes_size"] // 64) // 256) for it in L["item"])
    assert (L["max_width"], L["max_height"]) == (max(i[0] for i in info), max(i[1] for i in info))


def test_one_path_only():
    r = lk.JpegDecoder.batch_plan([jv.fixture("420_q85_rstrow")[0]] * 2)
    assert r["rc"] == OK and r["layout"]["n_parallel"] == 0 and r["layout"]["max_sequences"] == 0
    r = lk.JpegDecoder.batch_plan([jv.fixture("420_tiny")[0]])
    assert r["rc"] == OK and r["layout"]["n_serial"] == 0 and r["layout"]["max_segment_groups"] == 0


def test_refusals():
    f = [jv.fixture(n)[0] for n in ("420_q75", "gray_q80", "444_q95", "420_tiny")]
    plan = lk.JpegDecoder.batch_plan
    r = plan(f, n=0)
    assert r["rc"] == ERR_ARG and r["layout"]["bad_item"] == -1
    r = plan([f[3]] * (_lib.JPEG_MAX_BATCH + 1))
    assert r["rc"] == ERR_ARG and r["layout"]["bad_item"] == -1
    assert plan([f[3]] * _lib.JPEG_MAX_BATCH)["rc"] == OK
    L = _lib.load()
    lay = _lib.JpegBatchLayout()
    assert L.psn_jpeg_batch_plan(None, 2, lay, None) == ERR_ARG and lay.bad_item == -1  # a null item list
    items, keep = lk.JpegDecoder._items(f)
    assert L.psn_jpeg_batch_plan(items, 4, None, None) == ERR_ARG
    r = plan([f[0], None, f[2]])  # a null data pointer
    assert r["rc"] == ERR_ARG and r["layout"]["bad_item"] == 1
    items[3].d_bgr = None  # a null output pointer
    assert L.psn_jpeg_batch_plan(items, 4, lay, None) == ERR_ARG and lay.bad_item == 3
    w = lk.JpegDecoder.info(f[1])[0]
    r = plan(f, strides=[1 << 20, 3 * w - 1, 1 << 20, 1 << 20])  # a short stride
    assert r["rc"] == ERR_ARG and r["layout"]["bad_item"] == 1
    assert plan(f, strides=[1 << 20, 3 * w, 1 << 20, 1 << 20])["rc"] == OK
    bad = list(f)
    bad[2] = bad[2][:2] + b"\x00\x00" + bad[2][4:]  # a corrupt header at item 2 of 4
    r = plan(bad)
    assert r["rc"] == ERR_ARG and r["layout"]["bad_item"] == 2
    prog = bytearray(f[0])
    sof = prog.find(b"\xff\xc0")
    prog[sof + 1] = 0xC2  # progressive: unsupported, not malformed
    r = plan([f[0], f[1], f[2], bytes(prog)])
    assert r["rc"] == -8 and r["layout"]["bad_item"] == 3
