"""The lossless PNG encoder's test images and decoders, shared by the host
twin's tests (test_png_encode.py) and the device's (test_png_encode_gpu.py).

A case is (name, format, width, rows): `rows` a tight (height, row bytes)
uint8 array in the project's own sense of the format (MONOWHITE: 1 = black).
"""
import io
import struct
import zlib

import numpy as np

from unpaper_hip import ctypes_abi as A
from helpers import page_array

SEG = 256  # kSegBytes of csrc/png_enc_core.h
CHANNELS = {A.FMT_GRAY8: 1, A.FMT_RGB24: 3, A.FMT_Y400A: 2}
MONO = (A.FMT_MONOWHITE, A.FMT_MONOBLACK)
ALL_FORMATS = [A.FMT_GRAY8, A.FMT_RGB24, A.FMT_Y400A, A.FMT_MONOWHITE, A.FMT_MONOBLACK]
NAMES = {A.FMT_GRAY8: "gray", A.FMT_RGB24: "rgb", A.FMT_Y400A: "ya", A.FMT_MONOWHITE: "monow",
         A.FMT_MONOBLACK: "monob"}
COLOUR_TYPE = {A.FMT_GRAY8: 0, A.FMT_RGB24: 2, A.FMT_Y400A: 4, A.FMT_MONOWHITE: 0, A.FMT_MONOBLACK: 0}


def row_bytes(fmt, width):
    return (width + 7) // 8 if fmt in MONO else width * CHANNELS[fmt]


def stored_bound(fmt, width, height):
    total = (row_bytes(fmt, width) + 1) * height
    return total + 5 * -(-total // 65535) + 6


def _sketch(fmt, width, height, seed):
    """Text-like content: flat paper, short dark runs, a little noise."""
    rng = np.random.default_rng(seed)
    if fmt in MONO:
        bits = rng.random((height, width)) < 0.2
        bits[:, : width // 3] = False
        rows = np.packbits(bits, axis=1, bitorder="big")
        return rows
    ch = CHANNELS[fmt]
    px = np.full((height, width, ch), 250, np.uint8)
    px[rng.random((height, width)) < 0.3] = rng.integers(0, 256, ch)
    px[::3] = np.minimum(px[::3], rng.integers(0, 256, (1, width, ch)).astype(np.uint8))
    return px.reshape(height, width * ch)


def _cases():
    out = []
    seed = 0
    for fmt in ALL_FORMATS:
        for w in (1, 2, 3, 7, 8, 9, 31, 32, 33):
            seed += 1
            out.append(("%s_%dx2" % (NAMES[fmt], w), fmt, w, _sketch(fmt, w, 2, seed)))
        for h in (1, 64, 65):
            seed += 1
            out.append(("%s_33x%d" % (NAMES[fmt], h), fmt, 33, _sketch(fmt, 33, h, seed)))
    # runs that end at, before and after the 258 cap
    for w in (257, 258, 259, 260, 261, 517):
        out.append(("gray_run_%d" % w, A.FMT_GRAY8, w, np.full((3, w), 7, np.uint8)))
        rgb = np.tile(np.array([9, 200, 31], np.uint8), (2, w))
        out.append(("rgb_run_%d" % w, A.FMT_RGB24, w, rgb))
    out.append(("monob_run_2072", A.FMT_MONOBLACK, 2072, np.full((2, 259), 0xFF, np.uint8)))
    # two segments and a byte, and more
    out.append(("gray_2segs_plus", A.FMT_GRAY8, 2 * SEG, _sketch(A.FMT_GRAY8, 2 * SEG, 1, 901)))
    out.append(("gray_2049x2", A.FMT_GRAY8, 2049, _sketch(A.FMT_GRAY8, 2049, 2, 902)))
    # scanned-page-like content
    out.append(("page_gray_203x131", A.FMT_GRAY8, 203, page_array(203, 131, seed=5)))
    out.append(("page_rgb_203x131", A.FMT_RGB24, 203, page_array(203, 131, seed=6, color=True).reshape(131, 609)))
    out.append(("white_gray", A.FMT_GRAY8, 203, np.full((131, 203), 255, np.uint8)))
    out.append(("black_gray", A.FMT_GRAY8, 203, np.zeros((131, 203), np.uint8)))
    out.append(("white_monow", A.FMT_MONOWHITE, 203, np.zeros((131, 26), np.uint8)))
    out.append(("black_monow", A.FMT_MONOWHITE, 203, np.full((131, 26), 0xFF, np.uint8)))
    rng = np.random.default_rng(77)
    out.append(("noise_gray", A.FMT_GRAY8, 300, rng.integers(0, 256, (200, 300), dtype=np.uint8)))
    out.append(("noise_rgb", A.FMT_RGB24, 100, rng.integers(0, 256, (70, 300), dtype=np.uint8)))
    # rows equal to the row above; rows of period bpp
    out.append(("same_rows_gray", A.FMT_GRAY8, 150, np.tile(rng.integers(0, 256, (1, 150), dtype=np.uint8), (9, 1))))
    out.append(("same_rows_rgb", A.FMT_RGB24, 50, np.tile(rng.integers(0, 256, (1, 150), dtype=np.uint8), (9, 1))))
    out.append(("period_rgb", A.FMT_RGB24, 90,
                np.stack([np.tile(rng.integers(0, 256, 3, dtype=np.uint8), 90) for _ in range(5)])))
    out.append(("period_ya", A.FMT_Y400A, 90,
                np.stack([np.tile(rng.integers(0, 256, 2, dtype=np.uint8), 90) for _ in range(5)])))
    # the row above lies beyond the 32 KiB window
    out.append(("gray_32769x3", A.FMT_GRAY8, 32769,
                np.tile(_sketch(A.FMT_GRAY8, 32769, 1, 903), (3, 1))))
    return out


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]
# the cases that also run in a pitch with garbage around the pixels
EMBED_IDS = ["gray_33x65", "rgb_33x65", "ya_33x65", "monow_33x65", "monob_33x65", "monow_7x2", "monob_9x2",
             "page_gray_203x131", "monob_run_2072"]


def embed(fmt, width, rows, seed=11):
    """The image inside rows of an odd, larger pitch filled with garbage:
    bilevel pixels start 5 bits into a row.  Returns (array, byte offset of
    pixel 0's byte for byte formats, bit offset for bilevel ones)."""
    rng = np.random.default_rng(seed)
    h = rows.shape[0]
    if fmt in MONO:
        bits = np.unpackbits(rows, axis=1, bitorder="big")[:, :width]
        pitch = (width + 5 + 7) // 8 + 4
        pitch += 1 - pitch % 2
        big = rng.integers(0, 2, (h, pitch * 8), dtype=np.uint8)
        big[:, 5:5 + width] = bits
        return np.packbits(big, axis=1, bitorder="big"), 0, 5
    pitch = rows.shape[1] + 6
    pitch += 1 - pitch % 2
    big = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    big[:, 3:3 + rows.shape[1]] = rows
    return big, 3, 0


def tight(fmt, width, rows):
    """The rows with the pad bits of a bilevel format cleared, as a fresh copy."""
    rows = np.ascontiguousarray(rows).copy()
    if fmt in MONO and width % 8:
        rows[:, -1] &= (0xFF00 >> (width % 8)) & 0xFF
    return rows


def png_samples(fmt, width, rows):
    """What the file must hold: the rows' sample bytes in PNG sense (MONOWHITE
    inverted, pad bits 0)."""
    rows = tight(fmt, width, rows)
    if fmt == A.FMT_MONOWHITE:
        rows = tight(fmt, width, ~rows)
    return rows


def chunks(png):
    """[(type, data)] of a PNG file; checks the signature and every CRC."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    out, at = [], 8
    while at < len(png):
        n, = struct.unpack(">I", png[at:at + 4])
        typ, data = png[at + 4:at + 8], png[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", png[at + 8 + n:at + 12 + n])
        assert zlib.crc32(typ + data) == crc, typ
        out.append((typ, data))
        at += 12 + n
    assert at == len(png) and out[-1] == (b"IEND", b"")
    return out


def idat(png):
    d = [c[1] for c in chunks(png) if c[0] == b"IDAT"]
    assert len(d) == 1
    return d[0]


def unfilter(fmt, width, height, stream):
    """zlib.decompress (which checks the Adler-32) and the filters undone in
    numpy: (sample rows, the filter numbers)."""
    rb = row_bytes(fmt, width)
    bpp = 1 if fmt in MONO else CHANNELS[fmt]
    f = np.frombuffer(zlib.decompress(stream), np.uint8)
    assert f.size == (rb + 1) * height
    f = f.reshape(height, rb + 1)
    out = np.zeros((height, rb), np.uint8)
    for y in range(height):
        t, line = int(f[y, 0]), f[y, 1:]
        if t == 0:
            out[y] = line
        elif t == 1:
            for c in range(bpp):
                out[y, c::bpp] = np.cumsum(line[c::bpp], dtype=np.uint8)
        elif t == 2:
            out[y] = line + (out[y - 1] if y else 0)
        else:
            raise AssertionError("row %d: filter %d" % (y, t))
    return out, f[:, 0].copy()


def pil_samples(png, fmt, width):
    from PIL import Image
    im = Image.open(io.BytesIO(png))
    im.load()
    assert im.mode == {A.FMT_GRAY8: "L", A.FMT_RGB24: "RGB", A.FMT_Y400A: "LA"}.get(fmt, "1")
    a = np.asarray(im)
    if fmt in MONO:
        return np.packbits(a.astype(bool), axis=1, bitorder="big")
    return a.reshape(a.shape[0], -1)


def is_stored(stream):
    """The Deflate data starts with a stored block (BTYPE = 00)."""
    return (stream[2] >> 1) & 3 == 0
