"""Helpers of the parallel entropy decode's tests: the golden JPEG fixtures, where
a file's entropy bytes lie, and the damaged / non-plain variants the tests use."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_fixtures.npz")

# restart-less fixtures -> entropy bytes (all plain: every FF is followed by 00)
PLAIN = {"420_q75": 1326, "422_q90": 3205, "444_q95": 7292, "gray_q80": 546, "420_tiny": 23}
RESTART = ("420_q30_rst3", "420_q85_rstrow", "422_q60_rst5")
EOI = b"\xff\xd9"


def fixture(name):
    z = np.load(GOLDEN)
    return z[name + "_jpeg"].tobytes(), z[name + "_bgr"]


def entropy_range(data: bytes):
    """[ent0, ent1): the bytes after the SOS header up to the marker that ends the scan."""
    p = 2
    while data[p + 1] != 0xDA:
        p += 2 + int.from_bytes(data[p + 2:p + 4], "big")
    q = ent0 = p + 2 + int.from_bytes(data[p + 2:p + 4], "big")
    while q + 1 < len(data):
        if data[q] == 0xFF and data[q + 1] not in (0x00, 0xFF) and not 0xD0 <= data[q + 1] <= 0xD7:
            break
        q += 1
    return ent0, q


def scan_blocks(data: bytes) -> int:
    """nmcu x blocks per MCU, from the frame header."""
    p = 2
    while data[p + 1] not in (0xC0, 0xC1):
        p += 2 + int.from_bytes(data[p + 2:p + 4], "big")
    s = data[p + 4:]
    h, w, nc = int.from_bytes(s[1:3], "big"), int.from_bytes(s[3:5], "big"), s[5]
    if nc == 1:
        return ((w + 7) // 8) * ((h + 7) // 8)
    samp = [(s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15) for c in range(nc)]
    hmax, vmax = max(a for a, _ in samp), max(b for _, b in samp)
    nmcu = ((w + 8 * hmax - 1) // (8 * hmax)) * ((h + 8 * vmax - 1) // (8 * vmax))
    return nmcu * sum(a * b for a, b in samp)


def truncated(data: bytes) -> bytes:
    """The entropy data cut at 60 % (not after an FF) and closed with EOI."""
    e0, e1 = entropy_range(data)
    cut = e0 + (e1 - e0) * 6 // 10
    while data[cut - 1] == 0xFF:
        cut -= 1
    return data[:cut] + EOI


def corrupted(data: bytes) -> bytes:
    """Eight entropy bytes XOR 0x55, from a third of the way in, 37 bytes apart;
    positions are passed over where the byte or its predecessor is FF or the result
    would be FF, so the stream stays plain."""
    e0, e1 = entropy_range(data)
    b = bytearray(data)
    p, done = e0 + (e1 - e0) // 3, 0
    while done < 8 and p < e1:
        if b[p] != 0xFF and b[p - 1] != 0xFF and b[p] ^ 0x55 != 0xFF:
            b[p] ^= 0x55
            done += 1
        p += 37
    assert done == 8
    return bytes(b)


def _first_stuffed(data: bytes) -> int:
    e0, e1 = entropy_range(data)
    at = data.find(b"\xff\x00", e0, e1)
    assert at > 0, "the fixture has no stuffed byte"
    return at


def with_fill_byte(data: bytes) -> bytes:
    """FF FF 00 in place of an FF 00: a fill byte in front of a stuffed FF."""
    at = _first_stuffed(data)
    return data[:at] + b"\xff" + data[at:]


def ending_in_ff(data: bytes) -> bytes:
    """Cut between an FF and its stuffed zero, closed with EOI: the entropy data ends in FF."""
    at = _first_stuffed(data)
    return data[:at + 1] + EOI
