"""The TIFF encoder's test images and a hand decoder of its files, shared by
test_tiff_encode.py (host twin) and test_tiff_encode_gpu.py (device)."""
import io
import struct
import zlib

import numpy as np

from unpaper_hip import ctypes_abi as A

CHANNELS = {A.FMT_GRAY8: 1, A.FMT_RGB24: 3, A.FMT_Y400A: 2}
SEG = 256  # pngenc::kSegBytes


def rows_per_strip(row_bytes, height):
    return max(1, min(65536 // row_bytes, height))


def stored_size(total):
    return total + 5 * ((total + 65534) // 65535) + 6


def _text(rng, h, rb):
    """Mostly white with dark runs: matches, literals and a skewed histogram."""
    a = np.full((h, rb), 0xF0, np.uint8)
    m = rng.random((h, rb)) < 0.2
    a[m] = rng.integers(0, 256, int(m.sum()), dtype=np.uint8)
    return a


def _make():
    rng = np.random.default_rng(1234)
    cases = []

    def add(name, fmt, width, rows):
        cases.append((name, fmt, width, np.ascontiguousarray(rows, np.uint8)))

    add("gray_1x1", A.FMT_GRAY8, 1, np.array([[77]], np.uint8))
    for rb in (255, 256, 257):
        rps = 65536 // rb
        add("gray_%d_one_strip" % rb, A.FMT_GRAY8, rb, _text(rng, 10, rb))
        add("gray_%d_exact" % rb, A.FMT_GRAY8, rb, _text(rng, 2 * rps, rb))
        add("gray_%d_short_last" % rb, A.FMT_GRAY8, rb, _text(rng, 2 * rps + 3, rb))
    # the last strip is one row of 100 bytes: shorter than a segment
    add("gray_strip_below_segment", A.FMT_GRAY8, 100, _text(rng, 65536 // 100 + 1, 100))
    # a row over 65,536 bytes: one row a strip, no row-distance candidate
    add("gray_70000x3", A.FMT_GRAY8, 70000, np.tile(_text(rng, 1, 70000), (3, 1)))
    add("gray_32769x4", A.FMT_GRAY8, 32769, np.tile(_text(rng, 1, 32769), (4, 1)))
    for fmt, tag in ((A.FMT_RGB24, "rgb"), (A.FMT_Y400A, "ya")):
        ch = CHANNELS[fmt]
        for w in (85, 86, 87):
            rps = 65536 // (w * ch)
            # identical rows across the strip boundary: a row-distance match
            # there would reach into the previous strip
            add("%s_%d_equal_rows" % (tag, w), fmt, w, np.tile(_text(rng, 1, w * ch), (rps + 40, 1)))
        add("%s_86_text" % tag, fmt, 86, _text(rng, 50, 86 * ch))
    # one strip of random bytes between flat strips: stored and coded streams in one page
    a = np.full((768, 256), 0xFF, np.uint8)
    a[256:512] = rng.integers(0, 256, (256, 256), dtype=np.uint8)
    add("gray_stored_between_flat", A.FMT_GRAY8, 256, a)
    return cases


CASES = _make()
CASE_IDS = [c[0] for c in CASES]
TIFF_TYPES = {3: "H", 4: "I"}


def embed(rows, pad, seed):
    """The rows inside rows `pad` bytes longer, garbage in the padding."""
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (rows.shape[0], rows.shape[1] + pad), dtype=np.uint8)
    big[:, :rows.shape[1]] = rows
    return big


def ifds(data):
    """The file's IFDs: a list of {tag: (type, [values])}, rationals as
    (numerator, denominator) pairs, and each IFD's offset."""
    assert data[:4] == b"II*\x00"
    out, offs = [], []
    at = struct.unpack_from("<I", data, 4)[0]
    while at:
        assert at % 2 == 0 and at + 2 <= len(data)
        offs.append(at)
        n = struct.unpack_from("<H", data, at)[0]
        tags = {}
        last = 0
        for k in range(n):
            tag, typ, cnt, val = struct.unpack_from("<HHII", data, at + 2 + 12 * k)
            assert tag > last, "tags ascend"
            last = tag
            size = {3: 2, 4: 4, 5: 8}[typ] * cnt
            if size <= 4:
                raw = data[at + 2 + 12 * k + 8: at + 2 + 12 * k + 8 + size]
            else:
                assert val % 2 == 0, "values lie on even offsets"
                raw = data[val: val + size]
                assert len(raw) == size
            if typ == 5:
                v = [struct.unpack_from("<II", raw, 8 * i) for i in range(cnt)]
            else:
                v = list(struct.unpack("<%d%s" % (cnt, TIFF_TYPES[typ]), raw))
            tags[tag] = (typ, v)
        out.append(tags)
        at = struct.unpack_from("<I", data, at + 2 + 12 * n)[0]
    return out, offs


def hand_decode(data, tags):
    """A Deflate page decoded by hand: every strip inflated on its own (so a
    match that reached into the previous strip fails), Predictor 2 undone.
    Returns (rows as height x row_bytes, the strips' (offset, count, stored))."""
    w, h = tags[256][1][0], tags[257][1][0]
    spp = tags[277][1][0]
    assert tags[259][1] == [8] and tags[317][1] == [2] and tags[284][1] == [1]
    assert tags[258][1] == [8] * spp
    rps = tags[278][1][0]
    offs, cnts = tags[273][1], tags[279][1]
    rb = w * spp
    nstrips = (h + rps - 1) // rps
    assert len(offs) == len(cnts) == nstrips
    rows = np.zeros((h, rb), np.uint8)
    strips = []
    for k in range(nstrips):
        z = data[offs[k]: offs[k] + cnts[k]]
        assert len(z) == cnts[k] and z[:2] == b"\x78\x01"
        n = min(rps, h - k * rps)
        assert cnts[k] <= stored_size(n * rb)
        d = zlib.decompressobj()
        raw = d.decompress(z)
        assert d.eof and not d.unused_data and len(raw) == n * rb
        a = np.frombuffer(raw, np.uint8).reshape(n, w, spp)
        rows[k * rps: k * rps + n] = np.cumsum(a, axis=1, dtype=np.uint8).reshape(n, rb)
        strips.append((offs[k], cnts[k], (z[2] & 6) == 0))
    return rows, strips


def pil_pages(data):
    """Every page through PIL (libtiff): a list of height x row_bytes arrays."""
    from PIL import Image
    out = []
    with Image.open(io.BytesIO(data)) as im:
        for i in range(getattr(im, "n_frames", 1)):
            im.seek(i)
            a = np.array(im)
            if im.mode == "1":
                a = np.packbits(a, axis=1)
            out.append(a.reshape(a.shape[0], -1))
    return out
