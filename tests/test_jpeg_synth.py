"""The entropy decode's CPU model on synthesised streams (tests/jpeg_synth.py): the
corners PIL-encoded files never reach -- rounds at their caps, two passes of
jpeg_chain_kernel, 16-bit codes, symbols across two subsequence boundaries,
FF 00 pairs on every kind of boundary, ill-formed scans. The reference of an
intact case is the coefficient array it was written from; of an ill-formed one,
the serial decode. Every case also asserts, from the writer's symbol map or the
model's stats, that it has the property it is named for."""
import io

import numpy as np
import pytest

import jpeg_synth as js
import jpeg_variants as jv
from mcmtt_opticalflow_amd import _lib, lk

SUBS = [4, 8, 16, 64, 128, 256, 1024]


def _serial(data):
    coef, st = lk.JpegDecoder.model(data, 1, 0)
    assert st["path"] == _lib.JPEG_PATH_SERIAL and st["blocks"] == jv.scan_blocks(data) == coef.shape[0]
    return coef


def _parallel(data, ref, s):
    coef, st = lk.JpegDecoder.model(data, 2, s)
    nsub = -(-len(_entropy(data)) // s)
    assert st["path"] == _lib.JPEG_PATH_PARALLEL and st["sub_bytes"] == s
    assert st["subsequences"] == nsub and st["sequences"] == -(-nsub // 256)
    assert st["blocks"] == jv.scan_blocks(data)
    assert 1 <= st["sync_rounds"] <= 256 and 1 <= st["chain_rounds"] <= st["sequences"]
    np.testing.assert_array_equal(coef, ref, err_msg=f"sub_bytes {s}")
    return st


def _entropy(data):
    e0, e1 = jv.entropy_range(data)
    return data[e0:e1]


def _check_intact(c):
    assert c.stream.entropy == _entropy(c.data)
    p = lk.JpegDecoder.plan(c.data)
    assert p["plain"] == 1 and p["path"] == _lib.JPEG_PATH_PARALLEL
    np.testing.assert_array_equal(_serial(c.data), c.coefs)
    for s in SUBS:
        _parallel(c.data, c.coefs, s)


def _pil(data):
    from PIL import Image

    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])


@pytest.fixture(scope="module")
def multipass():
    return js.case("multipass")


# ------------------------------------------------------------------ every case

@pytest.mark.parametrize("name", js.SMALL_INTACT)
def test_intact_model_equals_input(name):
    _check_intact(js.case(name))


def test_multipass_model_equals_input(multipass):
    """592x592, 16-bit AC codes, every coefficient set: at 4-byte subsequences more
    than 1024 sequences, two passes of the chain with a carry between them."""
    _check_intact(multipass)
    _, st = lk.JpegDecoder.model(multipass.data, 2, 4)
    print("multipass at S=4:", st)
    assert st["sequences"] > 1024 and st["subsequences"] > 1024 * 256
    assert len(multipass.stream.entropy) > 1 << 20


@pytest.mark.parametrize("name", js.ILL_FORMED_CASES)
def test_ill_formed_parallel_equals_serial(oracle_mod, name):
    c = js.case(name)
    w, h, _ = lk.JpegDecoder.info(c.data)
    assert oracle_mod.jpeg_decode_bgr(c.data).shape == (h, w, 3)  # decodes without error
    assert lk.JpegDecoder.plan(c.data)["path"] == _lib.JPEG_PATH_PARALLEL  # still plain
    ref = _serial(c.data)
    for s in SUBS:
        _parallel(c.data, ref, s)


@pytest.mark.parametrize("name", js.ILL_FORMED_CASES)
def test_ill_formed_model_decodes_what_the_oracle_decodes(oracle_mod, name):
    """The oracle hands out pixels only, so the serial model's coefficients are
    written out again as an intact file: the oracle's pixels of that file are its
    pixels of the ill-formed one. (overwritten_ladder_ff holds codes no length
    accepts; libjpeg, and the oracle, have read 17 bits when they give up on one.)"""
    c = js.case(name)
    w, h, _ = lk.JpegDecoder.info(c.data)
    again = js.encode(js.dataclasses.replace(c.spec, width=w, height=h), _serial(c.data)).data
    np.testing.assert_array_equal(oracle_mod.jpeg_decode_bgr(again), oracle_mod.jpeg_decode_bgr(c.data))


@pytest.mark.parametrize("name", js.IN_RANGE)
def test_in_range_pixels_oracle_equals_pil(oracle_mod, name):
    """Intact files whose samples stay in range: the one regime in which PIL's
    decode is a reference for the oracle's pixels."""
    pytest.importorskip("PIL")
    c = js.case(name)
    assert c.in_range
    np.testing.assert_array_equal(oracle_mod.jpeg_decode_bgr(c.data), _pil(c.data))


# ------------------------------------------------------------------ the property of each case

def test_ambiguous444_rounds_at_their_caps():
    """One Huffman slot for all three components: a cold decoder finds the symbol
    and block boundaries but never which block of the MCU it is in, so only the
    true state, handed on one thread a round, ends the rounds."""
    c = js.case("ambiguous444")
    assert len({*c.spec.dc_slot, *c.spec.ac_slot}) == 1
    _, st = lk.JpegDecoder.model(c.data, 2, 4)
    print("ambiguous444 at S=4:", st)
    assert st["sync_rounds"] == 256 and st["chain_rounds"] == st["sequences"] >= 4
    _, st8 = lk.JpegDecoder.model(c.data, 2, 8)
    assert st8["sync_rounds"] == 256 and st8["sequences"] >= 2


def test_ambiguous_gray_pair_rounds_come_from_block_phase():
    """The same blocks in the same scan order with the same tables, as a three- and
    as a one-component file (only the DC differences differ, predicted per
    component or not). One component has no block phase to miss: its rounds stay
    under half the cap -- a decoder off by symbol or coefficient phase corrects
    itself within a few blocks of some 24 bytes, 128 rounds are 512 bytes -- while
    the three-component file sits at the cap."""
    a, g = js.case("ambiguous444"), js.case("ambiguous_gray")
    np.testing.assert_array_equal(g.coefs, a.coefs[js.layout(64, 64, 3).scan_block])
    assert (g.spec.dc_tables, g.spec.ac_tables) == (a.spec.dc_tables, a.spec.ac_tables)
    _, sa = lk.JpegDecoder.model(a.data, 2, 4)
    _, sg = lk.JpegDecoder.model(g.data, 2, 4)
    print("ambiguous pair at S=4: rounds", sa["sync_rounds"], "against", sg["sync_rounds"])
    assert sa["sync_rounds"] == 256 and sg["sync_rounds"] <= 128 and sg["chain_rounds"] == 1


def test_flat_many_blocks_in_one_subsequence():
    c = js.case("flat")
    assert not c.coefs.any()
    starts = c.stream.sym_start[c.stream.sym_dc]
    assert len(starts) == 96 and np.bincount(starts // 32).max() >= 5
    assert lk.JpegDecoder.model(c.data, 2, 1024)[1]["subsequences"] == 1


def _dense_properties(c):
    st = c.stream
    assert (c.coefs != 0).all() and np.abs(c.coefs[:, 1:]).max() == 1023
    assert (st.sym_code_len[~st.sym_dc] == 16).all()  # beyond the 9-bit lookahead: Reader::decode's loop
    assert js.canonical_codes(c.spec.ac_tables[0])[0x00][1] == 16 and 0x00 not in st.counts[(1, 0)]  # no EOB
    first, last = st.sym_start // 32, (st.sym_start + st.sym_bits - 1) // 32
    nsub = -(-len(st.entropy) // 4)
    assert (last - first >= 2).any()  # a symbol over two 4-byte boundaries (a stuffed zero inside it)
    assert len(np.unique(first)) < nsub  # a subsequence in which no symbol starts
    assert 2 * len(np.unique(first[st.sym_dc])) < nsub  # most subsequences complete no block (cnt == 0)


def test_deep_dense_long_codes_and_empty_subsequences():
    _dense_properties(js.case("deep_dense"))


def test_multipass_is_built_like_deep_dense(multipass):
    _dense_properties(multipass)


def test_ladder_ff_stuffing_on_every_boundary():
    assert js.ladder_seed() is not None, "no seed of 0..63 has every placement property"
    c = js.case("ladder_ff")
    props = js.ladder_properties(c.stream)
    assert all(props.values()), props
    # the same from the file's bytes alone
    e = np.frombuffer(_entropy(c.data), np.uint8)
    ff = np.flatnonzero(e == 0xFF)
    assert (e[ff + 1] == 0).all()
    assert len(ff) >= 0.30 * (len(e) - len(ff))  # 30 % of the unstuffed bytes
    for s in (4, 16, 128):
        assert (ff % s == s - 1).any(), s  # FF ends a subsequence, its zero starts the next
    assert (ff % 1024 == 1023).any()  # ... ends a sequence (workgroup) at S=4
    assert any(((ff >= w - 2) & (ff <= w)).any() for w in range(256 * 4 + 64, len(e), 1024))  # staged window's end
    dc = c.coefs[:, 0].astype(int)
    assert set(np.abs(np.diff(dc))) == {2047}
    assert set(np.abs(c.coefs[:, 1:]).ravel()) == {0, 511, 1023}


def test_stuffed_starts_cold_state_is_the_true_state():
    """Every 4-byte subsequence starts at a block boundary, every other one behind a
    stuffed zero: a cold decoder (block 0, DC next, past the stuffed zero) is in
    the true state everywhere, so round 0 is right and one round confirms it.
    A cold start on the stuffed zero itself would read eight bits that are not
    in the stream, and take further rounds to repair."""
    c = js.case("stuffed_starts")
    e = np.frombuffer(c.stream.entropy, np.uint8)
    assert len(e) == 144 * 8 > 1024  # two sequences at S=4
    at = np.arange(4, len(e), 4)
    zero = (e[at] == 0) & (e[at - 1] == 0xFF)
    assert zero[0::2].all() and not zero[1::2].any()
    blocks = set(c.stream.sym_start[c.stream.sym_dc].tolist())
    assert all(8 * (o + z) in blocks for o, z in zip(at.tolist(), zero.tolist()))
    _, st = lk.JpegDecoder.model(c.data, 2, 4)
    assert (st["sequences"], st["sync_rounds"], st["chain_rounds"]) == (2, 2, 1), st


def test_undefined_code_takes_17_bits():
    """Sixteen ones are a code of no valid table (the all-ones code of any length
    is ruled out). The blocks behind one decode as written only if 17 bits went
    with it; the intact-case tests hold model, oracle and PIL to that."""
    c = js.case("undefined_code")
    st = c.stream
    bad = np.flatnonzero(st.sym_code_len == 17)
    assert len(bad) == 2 and st.counts[(1, 0)][js.UNDEFINED] == 2 and (st.sym_bits[bad] >= 17).all()
    assert st.sym_dc[bad + 1].all()  # each followed by a block's DC symbol
    for table in (js.STD_AC_LUMA, js.ac_ladder16(), js.ac_all_at(16)):
        assert max(code for code, n in js.canonical_codes(table).values() if n == 16) < 0xFFFF


def test_zrl_runs_and_blocks_without_eob():
    c = js.case("zrl")
    counts = c.stream.counts[(1, 0)]
    assert counts[0xF0] == 6 * (1 + 2 + 3 + 3 + 1 + 1) and counts[0x00] == 6 * 4  # ZRLs per kind of block
    assert (c.coefs[:, 63] != 0).sum() == 12


@pytest.mark.parametrize("name", ["optimised_q50", "optimised_q95"])
def test_optimised_tables_differ_from_the_standard(name):
    c = js.case(name)
    std = {(0, 0): js.STD_DC_LUMA, (0, 1): js.STD_DC_CHROMA, (1, 0): js.STD_AC_LUMA, (1, 1): js.STD_AC_CHROMA}
    for (cls, slot), table in std.items():
        mine = (c.spec.ac_tables if cls else c.spec.dc_tables)[slot]
        assert mine != table
        assert set(mine[1]) == set(c.stream.counts[(cls, slot)])  # exactly the symbols the scan uses
    # optimal: no longer than with the standard's tables
    spec = js.dataclasses.replace(c.spec, dc_tables={0: js.STD_DC_LUMA, 1: js.STD_DC_CHROMA},
                                  ac_tables={0: js.STD_AC_LUMA, 1: js.STD_AC_CHROMA})
    assert len(c.stream.entropy) < len(js.encode(spec, c.coefs).entropy)


def test_sof1_q16_headers():
    c = js.case("sof1_q16")
    assert b"\xff\xc1" in c.data[:jv.entropy_range(c.data)[0]] and b"\xff\xc0" not in c.data[:c.stream.ent0]
    at = c.data.index(b"\xff\xdb")
    assert c.data[at + 4] >> 4 == 1  # Pq = 1
    assert max(int(q.max()) for q in c.spec.qtabs) > 255
    assert lk.JpegDecoder.info(c.data) == (24, 16, 3)


@pytest.mark.parametrize("name", [n for n in js.SMALL_INTACT if n.startswith("extreme_idct")])
def test_extreme_idct_saturates(oracle_mod, name):
    c = js.case(name)
    q = int(c.spec.qtabs[0][0])
    assert set(np.abs(c.coefs).ravel()) == ({1023} if q == 1 else {16}) and q in (1, 255)
    out = oracle_mod.jpeg_decode_bgr(c.data)
    assert out.min() == 0 and out.max() == 255


def test_geometry_cases_cover_the_edges():
    assert len([n for n in js.SMALL_INTACT if n.startswith("geometry_")]) == 4 * 7
    for mode, (nc, samp) in js.GEOMETRY_MODES.items():
        for w, h in js.GEOMETRY_SIZES:
            c = js.case(f"geometry_{mode}_{w}x{h}")
            assert lk.JpegDecoder.info(c.data) == (w, h, nc)
            assert c.coefs.shape[0] == jv.scan_blocks(c.data) == js.layout(w, h, nc, samp).nblocks


def test_ill_formed_cases_are_what_they_are_named():
    for base in ("ambiguous444", "ladder_ff"):
        b = js.case(base)
        n, blocks = len(b.stream.entropy), b.coefs.shape[0]
        good = _serial(b.data)
        t = _entropy(js.case(f"truncated_{base}").data)
        assert 0.38 * n <= len(t) <= 0.4 * n and b.stream.entropy.startswith(t)
        o = _entropy(js.case(f"overwritten_{base}").data)
        assert len(o) == n and b"\xfe" * 598 in o and b"\xfe" * 598 not in b.stream.entropy
        r = js.case(f"run_overflow_{base}").data
        assert not np.array_equal(_serial(r)[::3, 63], good[::3, 63])  # the guard entries land on coefficient 63
        assert jv.scan_blocks(js.case(f"excess_blocks_{base}").data) == blocks // 2
        assert jv.scan_blocks(js.case(f"short_scan_{base}").data) == blocks * 2
        for kind in js.ILL_FORMED:
            bad = _serial(js.case(f"{kind}_{base}").data)
            assert bad.shape != good.shape or not np.array_equal(bad, good), kind


# ------------------------------------------------------------------ the synthesiser itself

def _flowchart_decode(table, bits):
    """DECODE of the standard's figure F.16 over a list of bits: (symbol, bits read)."""
    counts, vals = table
    mincode, maxcode, valptr, code, k = [0] * 17, [-1] * 17, [0] * 17, 0, 0
    for l in range(1, 17):
        if counts[l - 1]:
            valptr[l], mincode[l] = k, code
            k += counts[l - 1]
            code += counts[l - 1]
            maxcode[l] = code - 1
        code <<= 1
    i, code = 1, bits[0]
    while code > maxcode[i]:
        code = (code << 1) | bits[i]
        i += 1
    return vals[valptr[i] + code - mincode[i]], i


@pytest.mark.parametrize("table", [js.STD_DC_LUMA, js.STD_DC_CHROMA, js.STD_AC_LUMA, js.STD_AC_CHROMA,
                                   js.dc_ladder(), js.ac_ladder16()] + [js.ac_all_at(l) for l in range(8, 17)])
def test_canonical_codes_round_trip(table):
    codes = js.canonical_codes(js.check_table(table))
    assert sorted(codes) == sorted(table[1])
    for sym, (code, length) in codes.items():
        bits = [(code >> (length - 1 - i)) & 1 for i in range(length)] + [1] * 16
        assert _flowchart_decode(table, bits) == (sym, length)


def test_standard_tables_are_the_fixtures():
    """The four tables typed in from the standard are the ones PIL wrote into the golden files."""
    data, found, p = jv.fixture("444_q95")[0], {}, 2
    while data[p + 1] != 0xDA:
        n = int.from_bytes(data[p + 2:p + 4], "big")
        s, o = data[p + 4:p + 2 + n], 0
        while data[p + 1] == 0xC4 and o < len(s):
            k = sum(s[o + 1:o + 17])
            found[s[o]] = (list(s[o + 1:o + 17]), list(s[o + 17:o + 17 + k]))
            o += 17 + k
        p += 2 + n
    assert found == {0x00: js.STD_DC_LUMA, 0x01: js.STD_DC_CHROMA, 0x10: js.STD_AC_LUMA, 0x11: js.STD_AC_CHROMA}


def test_builder_rejects_bad_tables():
    with pytest.raises(ValueError):  # 256 codes of 8 bits: the last is all ones
        js.check_table(([0] * 7 + [256] + [0] * 8, list(range(256))))
    with pytest.raises(ValueError):  # two codes of one bit
        js.check_table(([2] + [0] * 15, [0, 1]))
    with pytest.raises(ValueError):
        js.check_table(([0, 1] + [0] * 14, [16]), dc=True)
    with pytest.raises(ValueError):  # the scan uses a symbol the table lacks
        spec = js._std_spec(8, 8)
        spec.ac_tables = {0: ([1] + [0] * 15, [0x00]), 1: js.STD_AC_CHROMA}
        js.encode(spec, np.ones((1, 64), np.int16))
    with pytest.raises(lk.PsnLkError):  # and the decoder's parser agrees about the all-ones code
        spec = js._std_spec(8, 8)
        data = js.encode(spec, np.zeros((1, 64), np.int16)).data
        at = data.index(b"\xff\xc4") + 5
        lk.JpegDecoder.info(data[:at] + bytes([2]) + data[at + 1:])  # two DC codes of one bit


def test_symbol_map_matches_the_bytes():
    """The map's positions are those of a bit-serial read of the stuffed bytes."""
    c = js.case("ladder_ff")
    st, e = c.stream, c.stream.entropy
    assert (st.sym_start[1:] == st.sym_start[:-1] + st.sym_bits[:-1]).all() and st.sym_start[0] == 0
    at = st.sym_start // 8
    assert (np.frombuffer(e, np.uint8)[at[at > 0] - 1] != 0xFF).all()  # never inside a stuffed zero
    for i in (0, 1, len(st.sym_start) // 2, len(st.sym_start) - 1):  # the code at that position decodes
        pos, bits = int(st.sym_start[i]), []
        while len(bits) < 16:
            byte = pos >> 3
            if byte >= len(e):  # past the last symbol
                bits.append(1)
                continue
            if e[byte] == 0 and byte and e[byte - 1] == 0xFF:
                pos += 8
                continue
            bits.append((e[byte] >> (7 - (pos & 7))) & 1)
            pos += 1
        table = c.spec.dc_tables[0] if st.sym_dc[i] else c.spec.ac_tables[0]
        assert _flowchart_decode(table, bits)[1] == st.sym_code_len[i]
