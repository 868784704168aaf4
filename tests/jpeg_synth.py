"""A baseline-JPEG writer driven by quantised coefficients, for the entropy decoder's
tests: the stream's content is chosen, not encoded from an image, so a test can
put every symbol where it wants it and compare the decoder with the one reference
that depends on no decoder -- the coefficients that went in.

encode() takes a Spec (geometry, quantisation and Huffman tables, table slots) and
an (nblocks, 64) int16 array in natural order, laid out as psn_jpeg_entropy_model
returns it (component planes stacked, blk0 + row * bw + col), and returns a Stream:
the file and a symbol map (start bit and bit length of every symbol in the stuffed
entropy bytes; a symbol is a Huffman code with its value bits, as the decoder's
step reads it). Table builders, a natural mode (image -> coefficients) and the
deliberately ill-formed variants follow; the named cases of test_jpeg_synth.py and
test_jpeg_synth_gpu.py are at the end. Everything is generated from seeds."""
import dataclasses
import functools

import numpy as np

import jpeg_variants as jv
from mcmtt_opticalflow_amd import synth

# zigzag index -> natural index
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                   41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# ---------------------------------------------------------------- Huffman tables
# A table is (bits, vals): bits[l - 1] codes of length l, vals in code order.

_AC_LUMA = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435"
    "363738393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798"
    "999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4"
    "f5f6f7f8f9fa")
_AC_CHROMA = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a"
    "35363738393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a9293949596"
    "9798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4"
    "f5f6f7f8f9fa")

# the standard's typical tables (ITU-T T.81 Annex K.3)
STD_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
STD_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
STD_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], list(_AC_LUMA))
STD_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(_AC_CHROMA))

# every AC symbol of 8-bit baseline: EOB, ZRL, run 0..15 x size 1..10
AC_SYMBOLS = sorted([0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)])

STD_Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                       14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113,
                       92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
STD_Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                         47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)


def check_table(table, dc=False):
    """Raises ValueError for a table the decoder's parser rejects: a code that
    overflows its length (the all-ones code included), a DC symbol above 15; also
    for a vals list that does not match bits or repeats a symbol."""
    bits, vals = table
    if len(bits) != 16 or sum(bits) != len(vals) or len(set(vals)) != len(vals) or len(vals) > 256:
        raise ValueError("bits / vals do not describe one table")
    code = 0
    for l in range(1, 17):
        code += bits[l - 1]
        if code >= (1 << l):
            raise ValueError(f"codes of length {l} overflow (the all-ones code is not allowed)")
        code <<= 1
    if dc and any(v > 15 for v in vals):
        raise ValueError("DC symbol above 15")
    return table


def canonical_codes(table):
    """symbol -> (code, length), the canonical assignment of Annex C."""
    bits, vals = table
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


def ac_all_at(length):
    """Every AC symbol at one code length, 8..16."""
    bits = [0] * 16
    bits[length - 1] = len(AC_SYMBOLS)
    return check_table((bits, list(AC_SYMBOLS)))


def dc_ladder():
    """Unary ladder: size s has the code of s ones and a zero (lengths 1..12)."""
    return check_table(([1] * 12 + [0] * 4, list(range(12))), dc=True)


LADDER_SHORT = [0x01, 0x02, 0x03, 0x04, 0x00, 0xF0, 0x09, 0x0A]  # the AC ladder's symbols of length 1..8


def ac_ladder16():
    """One code each at lengths 1..8 (the last two: a value of 9 and of 10 bits),
    every other AC symbol at length 16 -- those codes start with eight ones."""
    rest = [s for s in AC_SYMBOLS if s not in LADDER_SHORT]
    return check_table(([1] * 8 + [0] * 7 + [len(rest)], LADDER_SHORT + rest))


def optimal_table(counts, dc=False):
    """The table Annex K.2 derives from symbol counts (what optimize=True gives):
    Huffman's merge with one reserved code point, lengths limited to 16."""
    freq = [0] * 257
    for s, n in counts.items():
        freq[s] = n
    freq[256] = 1  # reserves the all-ones code
    size, other = [0] * 257, [-1] * 257

    def least(skip):
        best, at = None, -1
        for i in range(257):
            if freq[i] and i != skip and (best is None or freq[i] <= best):
                best, at = freq[i], i
        return at

    while True:
        c1 = least(-1)
        c2 = least(c1)
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        # every symbol of both subtrees gets one bit longer; c1's chain then continues with c2's
        size[c1] += 1
        while other[c1] >= 0:
            c1 = other[c1]
            size[c1] += 1
        other[c1] = c2
        size[c2] += 1
        while other[c2] >= 0:
            c2 = other[c2]
            size[c2] += 1
    bits = [0] * 34
    for i in range(257):
        if size[i]:
            bits[size[i]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1  # the reserved code point
    vals = [s for l in range(1, 33) for s in range(256) if size[s] == l]
    return check_table((bits[1:17], vals), dc=dc)


# ---------------------------------------------------------------- geometry

@dataclasses.dataclass
class Spec:
    width: int
    height: int
    ncomp: int = 1
    sampling: tuple = (1, 1)        # luma h, v (3 components; chroma is 1x1)
    qtabs: tuple = ()               # quantisation tables, 64 values each in natural order
    qsel: tuple = (0, 1, 1)         # table per component
    q16: bool = False               # write the tables with Pq = 1
    sof: int = 0xC0                 # 0xC0 (SOF0) or 0xC1 (SOF1)
    dc_slot: tuple = (0, 1, 1)
    ac_slot: tuple = (0, 1, 1)
    dc_tables: dict = None          # slot -> (bits, vals)
    ac_tables: dict = None


@dataclasses.dataclass
class Layout:
    comps: list          # (h, v, bw, bh, blk0) per component, h and v as the scan interleaves them
    nblocks: int
    scan_block: list     # coefficient block of every block of the scan, in scan order
    scan_comp: list


def layout(width, height, ncomp, sampling=(1, 1)):
    if ncomp == 1:
        dims = [(1, 1, -(-width // 8), -(-height // 8))]
        mcux, mcuy = dims[0][2], dims[0][3]
    else:
        h, v = sampling
        mcux, mcuy = -(-width // (8 * h)), -(-height // (8 * v))
        dims = [(h, v, mcux * h, mcuy * v), (1, 1, mcux, mcuy), (1, 1, mcux, mcuy)]
    comps, blk0 = [], 0
    for h, v, bw, bh in dims:
        comps.append((h, v, bw, bh, blk0))
        blk0 += bw * bh
    blocks, cis = [], []
    for my in range(mcuy):
        for mx in range(mcux):
            for ci, (h, v, bw, _, b0) in enumerate(comps):
                for by in range(v):
                    for bx in range(h):
                        blocks.append(b0 + (my * v + by) * bw + mx * h + bx)
                        cis.append(ci)
    return Layout(comps, blk0, blocks, cis)


# ---------------------------------------------------------------- the writer

@dataclasses.dataclass
class Stream:
    data: bytes              # the file
    ent0: int                # offset of the first entropy byte
    entropy: bytes           # the stuffed entropy bytes (data[ent0:ent0 + len(entropy)])
    unstuffed: bytes
    sym_start: np.ndarray    # per symbol: first bit, in the stuffed entropy bytes
    sym_bits: np.ndarray     # bits to the next symbol's start there (stuffed zeros inside count)
    sym_code_len: np.ndarray  # length of the symbol's Huffman code
    sym_dc: np.ndarray       # True: a DC size symbol
    counts: dict             # (class, slot) -> {symbol: count}


UNDEFINED = 256  # pseudo-symbol: sixteen ones, a code no valid table holds, and the 17th bit libjpeg reads with it


def _symbols(spec, lay, coefs, overflow, undefined=()):
    """The scan as (table, symbol, size, value bits) lists. `overflow`: scan positions
    whose block ends, in place of EOB, with run 15 + a one-bit value that carries
    the coefficient index past 63; `undefined`: those that end with UNDEFINED."""
    zz = np.asarray(coefs, np.int64)[:, ZIGZAG]
    tab, sym, size, val = [], [], [], []
    pred = [0] * spec.ncomp
    for at, (blk, ci) in enumerate(zip(lay.scan_block, lay.scan_comp)):
        row = zz[blk].tolist()
        d = row[0] - pred[ci]
        pred[ci] = row[0]
        s = abs(d).bit_length()
        if s > 11:
            raise ValueError(f"DC difference {d} needs {s} bits")
        tab.append(spec.dc_slot[ci])
        sym.append(s)
        size.append(s)
        val.append(d if d >= 0 else d + (1 << s) - 1)
        t, run = 4 + spec.ac_slot[ci], 0
        for k in range(1, 64):
            v = row[k]
            if v == 0:
                run += 1
                continue
            while run > 15:  # ZRL
                tab.append(t)
                sym.append(0xF0)
                size.append(0)
                val.append(0)
                run -= 16
            s = abs(v).bit_length()
            if s > 10:
                raise ValueError(f"AC coefficient {v} needs {s} bits")
            tab.append(t)
            sym.append((run << 4) | s)
            size.append(s)
            val.append(v if v > 0 else v + (1 << s) - 1)
            run = 0
        if run:  # coefficient 63 is zero: the block needs an end
            tab.append(t)
            if at in undefined:
                sym.append(UNDEFINED)
                size.append(0)
                val.append(0)
            elif at in overflow:
                if run > 15:
                    raise ValueError("an overflowing run needs a non-zero coefficient at index 48 or later")
                sym.append(0xF1)
                size.append(1)
                val.append(1)
            else:
                sym.append(0x00)
                size.append(0)
                val.append(0)
    return np.array(tab), np.array(sym), np.array(size), np.array(val)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def _headers(spec, size):
    w, h = size
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    for i, q in enumerate(spec.qtabs):
        q = np.asarray(q)[ZIGZAG]
        body = b"".join(int(x).to_bytes(2, "big") for x in q) if spec.q16 else bytes(int(x) for x in q)
        out += _segment(0xDB, bytes([(16 if spec.q16 else 0) | i]) + body)
    hv = [spec.sampling if spec.ncomp == 3 else (1, 1)] + [(1, 1)] * 2
    sof = bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([spec.ncomp])
    for c in range(spec.ncomp):
        sof += bytes([c + 1, (hv[c][0] << 4) | hv[c][1], spec.qsel[c]])
    out += _segment(spec.sof, sof)
    for cls, tables in ((0, spec.dc_tables), (1, spec.ac_tables)):
        for slot in sorted(tables):
            bits, vals = check_table(tables[slot], dc=cls == 0)
            out += _segment(0xC4, bytes([(cls << 4) | slot]) + bytes(bits) + bytes(vals))
    sos = bytes([spec.ncomp])
    for c in range(spec.ncomp):
        sos += bytes([c + 1, (spec.dc_slot[c] << 4) | spec.ac_slot[c]])
    return out + _segment(0xDA, sos + b"\0\x3f\0")


def symbol_counts(spec, coefs):
    """(class, slot) -> {symbol: count} of the scan encode() would write."""
    lay = layout(spec.width, spec.height, spec.ncomp, spec.sampling)
    tab, sym, _, _ = _symbols(spec, lay, coefs, ())
    return _counts(tab, sym)


def _counts(tab, sym):
    out = {}
    for t in np.unique(tab):
        s, n = np.unique(sym[tab == t], return_counts=True)
        out[(int(t) >> 2, int(t) & 3)] = dict(zip(s.tolist(), n.tolist()))
    return out


def encode(spec, coefs, header_size=None, overflow=(), undefined=()):
    """The file of `coefs` under `spec`. header_size: the (width, height) the frame
    header states when it is not the one the blocks were laid out for; overflow,
    undefined: scan positions of blocks that end ill-formed (_symbols)."""
    lay = layout(spec.width, spec.height, spec.ncomp, spec.sampling)
    coefs = np.asarray(coefs)
    if coefs.shape != (lay.nblocks, 64):
        raise ValueError(f"coefficients {coefs.shape}, the geometry has {lay.nblocks} blocks")
    tab, sym, size, val = _symbols(spec, lay, coefs, frozenset(overflow), frozenset(undefined))
    code, clen = np.zeros((8, 257), np.int64), np.zeros((8, 257), np.int64)
    code[4:, UNDEFINED], clen[4:, UNDEFINED] = 0x1FFFF, 17
    for cls, tables in ((0, spec.dc_tables), (1, spec.ac_tables)):
        for slot, table in tables.items():
            for s, (c, l) in canonical_codes(check_table(table, dc=cls == 0)).items():
                code[4 * cls + slot, s], clen[4 * cls + slot, s] = c, l
    hl = clen[tab, sym]
    if (hl == 0).any():
        bad = np.flatnonzero(hl == 0)[0]
        raise ValueError(f"symbol {sym[bad]:#x} has no code in table {tab[bad] >> 2}/{tab[bad] & 3}")
    word = ((code[tab, sym] << size) | val).astype(np.int64)  # at most 16 + 11 bits
    nbit = hl + size
    start = np.cumsum(nbit) - nbit
    total = int(nbit.sum())
    # every bit of every symbol, then packed: the bits past the last symbol are ones
    j = np.arange(total, dtype=np.int64) - np.repeat(start, nbit)
    bit = ((np.repeat(word, nbit) >> (np.repeat(nbit, nbit) - 1 - j)) & 1).astype(np.uint8)
    bit = np.concatenate([bit, np.ones(-total % 8, np.uint8)])
    raw = np.packbits(bit)
    # position of an unstuffed bit in the stuffed stream: one more byte per 0xFF before its byte
    ff_before = np.concatenate([[0], np.cumsum(raw == 0xFF)])
    edge = np.concatenate([start, [total]])
    stuffed = 8 * ((edge >> 3) + ff_before[edge >> 3]) + (edge & 7)
    entropy = raw.tobytes().replace(b"\xff", b"\xff\x00")
    head = _headers(spec, header_size or (spec.width, spec.height))
    return Stream(head + entropy + jv.EOI, len(head), entropy, raw.tobytes(), stuffed[:-1], np.diff(stuffed), hl,
                  tab < 4, _counts(tab, sym))


# ---------------------------------------------------------------- natural mode

def quality_tables(quality):
    """The standard's two tables scaled as libjpeg's quality setting scales them."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * scale + 50) // 100, 1, 255) for t in (STD_Q_LUMA, STD_Q_CHROMA))


_DCT = np.array([[(np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)]
                 for u in range(8)])


def _plane_blocks(plane, bw, bh, q):
    """Level shift, float64 forward DCT and quantisation of a (bh * 8, bw * 8) plane."""
    b = plane.astype(np.float64).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8) - 128.0
    f = _DCT @ b @ _DCT.T
    c = np.rint(f.reshape(-1, 64) / np.asarray(q, np.float64)[None, :])
    return np.clip(c, -1023, 1023).astype(np.int16)


def natural(bgr, ncomp, sampling=(1, 1), qtabs=None, quality=85):
    """(Spec, coefficients) of an 8-bit (H, W, 3) BGR image: YCbCr, chroma box-
    downsampled, float64 DCT, quantised -- samples stay in range by construction.
    The Spec carries the standard's Huffman tables."""
    height, width = bgr.shape[:2]
    qtabs = quality_tables(quality) if qtabs is None else qtabs
    lay = layout(width, height, ncomp, sampling)
    b, g, r = (bgr[..., i].astype(np.float64) for i in range(3))
    planes = [0.299 * r + 0.587 * g + 0.114 * b]
    if ncomp == 3:
        planes += [128 - 0.168736 * r - 0.331264 * g + 0.5 * b, 128 + 0.5 * r - 0.418688 * g - 0.081312 * b]
    hmax, vmax = sampling if ncomp == 3 else (1, 1)
    out = []
    for ci, (h, v, bw, bh, _) in enumerate(lay.comps):
        fx, fy = (hmax // h, vmax // v) if ncomp == 3 else (1, 1)
        full = np.pad(planes[ci], ((0, bh * 8 * fy - height), (0, bw * 8 * fx - width)), mode="edge")
        small = full.reshape(bh * 8, fy, bw * 8, fx).mean(axis=(1, 3))
        out.append(_plane_blocks(np.clip(np.rint(small), 0, 255), bw, bh, qtabs[(0, 1, 1)[ci]]))
    spec = Spec(width, height, ncomp, sampling, qtabs=tuple(qtabs), dc_tables={0: STD_DC_LUMA, 1: STD_DC_CHROMA},
                ac_tables={0: STD_AC_LUMA, 1: STD_AC_CHROMA})
    return spec, np.concatenate(out)


def image(width, height, seed):
    return synth.to_bgr(synth.texture(width, height, seed))


# ---------------------------------------------------------------- ill-formed output

def cut(data, fraction):
    """The entropy data cut at a fraction (not after an FF) and closed with EOI."""
    e0, e1 = jv.entropy_range(data)
    at = e0 + int((e1 - e0) * fraction)
    while data[at - 1] == 0xFF:
        at -= 1
    return data[:at] + jv.EOI


def overwrite(data, lo, hi, value):
    """Entropy bytes [lo, hi) (offsets in the entropy data) set to `value`; the
    range starts after a byte that is not FF, so the stream stays plain."""
    assert value != 0xFF
    e0, e1 = jv.entropy_range(data)
    lo, hi = e0 + lo, min(e0 + hi, e1)
    while data[lo - 1] == 0xFF:
        lo += 1
    assert lo < hi
    return data[:lo] + bytes([value]) * (hi - lo) + data[hi:]


def run_overflow(spec, coefs, every=3):
    """Every `every`-th block of the scan ends at zigzag index 55 and closes with a
    run that carries the index past 63 (the guard entries of the natural-order table)."""
    coefs = np.array(coefs)
    lay = layout(spec.width, spec.height, spec.ncomp, spec.sampling)
    at = range(0, len(lay.scan_block), every)
    for i in at:
        blk = lay.scan_block[i]
        coefs[blk, ZIGZAG[55]] = 1
        coefs[blk, ZIGZAG[56:]] = 0
    return encode(spec, coefs, overflow=at).data


def excess_blocks(spec, coefs):
    """The header states about half the height: the scan holds more blocks than the frame."""
    return encode(spec, coefs, header_size=(spec.width, max(8, spec.height // 16 * 8))).data


def short_scan(spec, coefs):
    """The header states twice the height: the scan ends before the frame's blocks do."""
    return encode(spec, coefs, header_size=(spec.width, spec.height * 2)).data


# ---------------------------------------------------------------- the cases

@dataclasses.dataclass
class Case:
    name: str
    data: bytes
    coefs: np.ndarray = None     # the coefficients the stream holds by construction; None: the serial decode defines them
    in_range: bool = False       # samples stay in range: PIL is a valid pixel reference
    stream: Stream = None
    spec: Spec = None

    @property
    def intact(self):
        return self.coefs is not None


def _std_spec(width, height, ncomp=1, sampling=(1, 1), q=1, **kw):
    return Spec(width, height, ncomp, sampling, qtabs=(np.full(64, q), np.full(64, q)),
                dc_tables={0: STD_DC_LUMA, 1: STD_DC_CHROMA}, ac_tables={0: STD_AC_LUMA, 1: STD_AC_CHROMA}, **kw)


def _intact(name, spec, coefs, in_range=False, **ill):
    coefs = np.asarray(coefs, np.int16)
    st = encode(spec, coefs, **ill)
    return Case(name, st.data, coefs, in_range, st, spec)


def _ambiguous_coefs(nblocks, seed=3):
    """Sparse AC of amplitude up to 12 and a DC random walk: samples stay in range.
    (The seed is one at which no sequence of the 4:4:4 file guesses its block phase
    right by chance, one in three: the tests assert what follows from that.)"""
    rng = np.random.default_rng(seed)
    c = np.zeros((nblocks, 64), np.int16)
    for b in range(nblocks):
        k = rng.choice(np.arange(1, 64), size=12, replace=False)
        c[b, ZIGZAG[k]] = rng.integers(1, 13, 12) * rng.choice([-1, 1], 12)
    c[:, 0] = np.clip(np.cumsum(rng.integers(-40, 41, nblocks)), -300, 300)
    return c


def _ambiguous_spec(width, height, ncomp):
    return _std_spec(width, height, ncomp, dc_slot=(0, 0, 0), ac_slot=(0, 0, 0), qsel=(0, 0, 0))


def _ambiguous444():
    return _ambiguous_spec(64, 64, 3), _ambiguous_coefs(192)


def _ambiguous_gray():
    """ambiguous444's blocks in its scan order, as the 192 blocks of a one-component file."""
    spec, c = _ambiguous444()
    order = layout(64, 64, 3).scan_block
    return _ambiguous_spec(192, 64, 1), c[order]


def _dense_coefs(nblocks, seed):
    """All 64 coefficients non-zero; a third of the AC ones are +-1023."""
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 1024, (nblocks, 64)) * rng.choice([-1, 1], (nblocks, 64))
    c = np.where(rng.random((nblocks, 64)) < 1 / 3, 1023 * rng.choice([-1, 1], (nblocks, 64)), c)
    dc = rng.integers(-1024, 1024, nblocks)
    c[:, 0] = np.where(dc == 0, 1, dc)
    return c.astype(np.int16)


def _deep_spec(side):
    return Spec(side, side, qtabs=(np.ones(64, int),), dc_tables={0: STD_DC_LUMA}, ac_tables={0: ac_all_at(16)})


def _ladder_coefs(seed):
    """Amplitudes 1023 and 511 (value bits all ones) at random positions, DC
    alternating between the extremes: differences of +-2047."""
    rng = np.random.default_rng(seed)
    c = np.zeros((36, 64), np.int16)
    for b in range(36):
        n = int(rng.integers(24, 64))
        k = rng.choice(np.arange(1, 64), size=n, replace=False)
        c[b, ZIGZAG[k]] = rng.choice([1023, 511, 1023, -1023], n)
    c[:, 0] = np.where(np.arange(36) % 2 == 0, 1023, -1024)
    return c


def _ladder_spec():
    return Spec(48, 48, qtabs=(np.ones(64, int),), dc_tables={0: dc_ladder()}, ac_tables={0: ac_ladder16()})


def ff_offsets(stream):
    """Offsets of the FF bytes (each followed by its stuffed zero) in the entropy bytes."""
    e = np.frombuffer(stream.entropy, np.uint8)
    return np.flatnonzero(e == 0xFF)


def ladder_properties(stream):
    """ladder_ff's placement properties, by name."""
    ff, n = ff_offsets(stream), len(stream.entropy)
    raw = np.frombuffer(stream.unstuffed, np.uint8)
    ends = [w for w in range(256 * 4 + 64, n, 1024)]  # staged window ends at 4-byte subsequences
    return {
        "ff_share": float((raw == 0xFF).mean()) >= 0.30,
        "sub4": bool((ff % 4 == 3).any()), "sub16": bool((ff % 16 == 15).any()), "sub128": bool((ff % 128 == 127).any()),
        "seq4": bool((ff % 1024 == 1023).any()),
        "window4": any(bool(((ff >= w - 2) & (ff <= w)).any()) for w in ends),
    }


@functools.lru_cache(maxsize=None)
def ladder_seed():
    """The first seed of 0..63 whose stream has every placement property, or None."""
    for seed in range(64):
        if all(ladder_properties(encode(_ladder_spec(), _ladder_coefs(seed))).values()):
            return seed
    return None


def _ladder():
    seed = ladder_seed()
    assert seed is not None, "no seed of 0..63 gives ladder_ff its placement properties"
    return _ladder_spec(), _ladder_coefs(seed)


def _zrl_coefs():
    c = np.zeros((36, 64), np.int16)
    for b in range(36):
        kind = b % 6
        if kind < 4:  # one, two or three ZRLs before the value
            c[b, ZIGZAG[(17, 33, 49, 63)[kind]]] = (3, -2, 7, -1)[kind]
        elif kind == 4:  # every stop at once; ends exactly at 63
            c[b, ZIGZAG[[17, 33, 49, 63]]] = [1, -5, 2, 9]
        else:  # EOB-terminated neighbour
            c[b, ZIGZAG[[1, 2, 20]]] = [4, -4, 1]
        c[b, 0] = 10 * (b % 5) - 20
    return c


def _stuffed_starts():
    """Blocks of 32 and 24 bits in turn, the first ending in a byte of ones (the
    eight value bits of coefficient 63 = 255, no EOB): eight stuffed bytes a pair,
    so every 4-byte subsequence starts at a block boundary, and every other one
    with the stuffed zero in front of it. Eight zero bits are no whole block under
    these tables (DC size 0, then two coefficients of -1)."""
    # (0, 1) 00, ZRL 010, EOB 0110, (14, 8) 0111000000000
    ac = check_table(([0, 1, 1, 1] + [0] * 8 + [1, 0, 0, 0], [0x01, 0xF0, 0x00, 0xE8]))
    spec = Spec(128, 144, qtabs=(np.ones(64, int),), dc_tables={0: STD_DC_LUMA}, ac_tables={0: ac})
    c = np.zeros((288, 64), np.int16)
    c[0::2, 63] = 255                                                   # 2 + 3 * 3 + 13 + 8 bits
    c[1::2, ZIGZAG[1:7][:, None]] = np.array([1, -1, -1, 1, -1, -1])[:, None]  # 2 + 6 * 3 + 4 bits
    return spec, c


def _undefined_code():
    """Blocks 0 and 2 of four end with sixteen ones in place of EOB: a decoder
    that has read 17 bits when it gives up (jdhuff.c's jpeg_huff_decode, whose
    sentinel is maxcode[17]) yields 0 -- an EOB -- and finds the next block."""
    spec = _std_spec(32, 8)
    c = np.zeros((4, 64), np.int16)
    c[:, 0] = [40, -25, 60, 10]
    c[:, ZIGZAG[[1, 2, 5]]] = [[9, -3, 2], [-7, 4, 1], [5, 5, -6], [-2, 8, 3]]
    return spec, c, dict(undefined=(0, 2))


def _extreme(ncomp, q):
    spec = _std_spec(32, 32, ncomp, (2, 2) if ncomp == 3 else (1, 1), q=q)
    n = layout(32, 32, ncomp, spec.sampling).nblocks
    rng = np.random.default_rng(5 + ncomp + q)
    amp = 1023 if q == 1 else 16
    c = amp * rng.choice([-1, 1], (n, 64))
    c[::3] = amp  # every third block: all positive
    c[1::3] = -amp
    return spec, c


def _optimised(quality):
    spec, c = natural(image(40, 24, 11), 3, (2, 2), quality=quality)
    counts = symbol_counts(spec, c)
    spec.dc_tables = {s: optimal_table(counts[(0, s)], dc=True) for s in (0, 1)}
    spec.ac_tables = {s: optimal_table(counts[(1, s)]) for s in (0, 1)}
    return spec, c


def _sof1_q16():
    q = tuple(np.minimum(t * 3, 65535) for t in quality_tables(50))  # luma up to 363, chroma 297
    spec, c = natural(image(24, 16, 3), 3, (2, 1), qtabs=q)
    spec.q16, spec.sof = True, 0xC1
    return spec, c


GEOMETRY_SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 9), (2, 33), (33, 2)]
GEOMETRY_MODES = {"gray": (1, (1, 1)), "444": (3, (1, 1)), "422": (3, (2, 1)), "420": (3, (2, 2))}
ILL_FORMED = ("truncated", "overwritten", "run_overflow", "excess_blocks", "short_scan")

_BUILDERS = {
    "ambiguous444": (_ambiguous444, True),
    "ambiguous_gray": (_ambiguous_gray, True),
    "flat": (lambda: (_std_spec(64, 64, 3, (2, 2)), np.zeros((96, 64), np.int16)), True),
    "deep_dense": (lambda: (_deep_spec(48), _dense_coefs(36, 2)), False),
    "ladder_ff": (_ladder, False),
    "zrl": (lambda: (_std_spec(48, 48), _zrl_coefs()), True),
    "stuffed_starts": (_stuffed_starts, True),
    "undefined_code": (_undefined_code, True),
    "optimised_q50": (lambda: _optimised(50), True),
    "optimised_q95": (lambda: _optimised(95), True),
    "sof1_q16": (_sof1_q16, True),
    "extreme_idct_gray_q1": (lambda: _extreme(1, 1), False),
    "extreme_idct_gray_q255": (lambda: _extreme(1, 255), False),
    "extreme_idct_420_q1": (lambda: _extreme(3, 1), False),
    "extreme_idct_420_q255": (lambda: _extreme(3, 255), False),
    "multipass": (lambda: (_deep_spec(592), _dense_coefs(74 * 74, 3)), False),
}
for _mode, (_nc, _samp) in GEOMETRY_MODES.items():
    for _w, _h in GEOMETRY_SIZES:
        _BUILDERS[f"geometry_{_mode}_{_w}x{_h}"] = (
            lambda w=_w, h=_h, nc=_nc, samp=_samp: natural(image(w, h, w + 2 * h), nc, samp, quality=85), True)

SMALL_INTACT = [n for n in _BUILDERS if n != "multipass"]
IN_RANGE = [n for n in SMALL_INTACT if _BUILDERS[n][1]]  # samples stay in range: PIL is a valid pixel reference
ILL_FORMED_CASES = [f"{kind}_{base}" for base in ("ambiguous444", "ladder_ff") for kind in ILL_FORMED]


def _ill_formed(name):
    kind = next(k for k in ILL_FORMED if name.startswith(k + "_"))
    base = case(name[len(kind) + 1:])
    if kind == "truncated":
        data = cut(base.data, 0.4)
    elif kind == "overwritten":
        data = overwrite(base.data, 1000, 1600, 0xFE)
    else:
        data = {"run_overflow": run_overflow, "excess_blocks": excess_blocks, "short_scan": short_scan}[kind](
            base.spec, base.coefs)
    return Case(name, data, spec=base.spec)


@functools.lru_cache(maxsize=None)
def case(name):
    """The named case (built once per process; treat it as read-only)."""
    if name in _BUILDERS:
        build, in_range = _BUILDERS[name]
        spec, coefs, *ill = build()
        return _intact(name, spec, coefs, in_range, **(ill[0] if ill else {}))
    return _ill_formed(name)
