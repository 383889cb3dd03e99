"""What the TIFF tests share: page makers, a writer through PIL (libtiff), a
hand writer for the files PIL does not make (big-endian, FillOrder 2, hostile
headers) and the mapping of PIL's pixels to the library's formats.

The expected pixels of a file are always numpy.asarray(Image.open(...)):
  mode 1, Photometric 0 -> MONOWHITE, stored bit = not PIL's pixel
  mode 1, Photometric 1 -> MONOBLACK, stored bit = PIL's pixel
  L -> GRAY8, LA -> Y400A, RGB -> RGB24, P -> RGB24 through the palette.
Bilevel pages are compared pixel by pixel (the pad bits of a row's last byte
are not pixels)."""
import struct

import numpy as np
from PIL import Image

from unpaper_hip import ctypes_abi as A

COMP = {"raw": 1, "packbits": 32773, "tiff_lzw": 5, "tiff_adobe_deflate": 8, "group3": 3, "group4": 4}


def _mix(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def noise(n, seed):
    """n bytes of integer-hash noise, the same on every machine."""
    with np.errstate(over="ignore"):
        idx = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x100000001B3)
        return (_mix(_mix(idx)) >> np.uint64(24)).astype(np.uint8)


def page(mode, w, h, seed=1):
    """A PIL image of `mode`: a ramp with a band of noise and flat stretches,
    so that every coder meets runs, repeats and literals."""
    ch = {"1": 1, "L": 1, "P": 1, "LA": 2, "RGB": 3}[mode]
    y, x = np.mgrid[0:h, 0:w]
    a = np.empty((h, w, ch), np.uint8)
    nz = noise(h * w * ch, seed).reshape(h, w, ch)
    for c in range(ch):
        base = ((x * (3 + c) + y * 7) // 4) & 0xFF
        a[:, :, c] = np.where((y % 16) < 5, nz[:, :, c], np.where((x % 64) < 24, 200 - 40 * c, base))
    if mode == "1":
        return Image.fromarray(a[:, :, 0] > 127)
    if mode == "P":
        im = Image.fromarray(a[:, :, 0] % 200, "P")
        pal = noise(768, seed + 99)
        im.putpalette(bytes(pal))
        return im
    return Image.fromarray(a[:, :, 0] if ch == 1 else a, mode)


def save(path, im, compression, rps=None, predictor=None, tags=None, more=None):
    """Write `im` (and the images `more` as further IFDs) through PIL."""
    info = dict(tags or {})
    if rps is not None:
        info[278] = rps
    if predictor is not None:
        info[317] = predictor
    kw = dict(format="TIFF", compression=compression, tiffinfo=info)
    if more:
        kw.update(save_all=True, append_images=list(more))
    im.save(path, **kw)
    return path


def strips(path, page=0):
    """(offsets, byte counts, RowsPerStrip) of a page, as PIL reads the tags."""
    with Image.open(path) as im:
        im.seek(page)
        off, cnt = im.tag_v2[273], im.tag_v2[279]
        return list(off), list(cnt), im.tag_v2.get(278, im.size[1])


def expected(path, page=0):
    """(format, width, height, pixels): pixels (h, w) stored bits for bilevel
    pages, (h, row bytes) for the byte formats."""
    with Image.open(path) as im:
        im.seek(page)
        phot = im.tag_v2.get(262)
        mode = im.mode
        w, h = im.size
        a = np.asarray(im.convert("RGB") if mode == "P" else im)
    if mode == "1":
        a = a.astype(bool)
        return (A.FMT_MONOWHITE, w, h, (~a).astype(np.uint8)) if phot == 0 else \
            (A.FMT_MONOBLACK, w, h, a.astype(np.uint8))
    fmt = {"L": A.FMT_GRAY8, "LA": A.FMT_Y400A, "RGB": A.FMT_RGB24, "P": A.FMT_RGB24}[mode]
    return fmt, w, h, np.ascontiguousarray(a, np.uint8).reshape(h, -1)


def pixels(fmt, w, rows):
    """A decoded page's rows (h, >= row bytes) in the form of expected()."""
    rows = np.asarray(rows)
    if fmt in (A.FMT_MONOWHITE, A.FMT_MONOBLACK):
        return np.unpackbits(rows[:, :(w + 7) // 8], axis=1)[:, :w]
    return rows[:, :w * {A.FMT_GRAY8: 1, A.FMT_Y400A: 2, A.FMT_RGB24: 3}[fmt]]


def row_bytes(fmt, w):
    return (w + 7) // 8 if fmt in (A.FMT_MONOWHITE, A.FMT_MONOBLACK) else \
        w * {A.FMT_GRAY8: 1, A.FMT_Y400A: 2, A.FMT_RGB24: 3}[fmt]


def build(w, h, strip_data, rps, tags, big_endian=False, magic=42, next_ifd=0, counts=True):
    """A classic TIFF by hand: header, the strips, one IFD, its out-of-line
    values.  tags: {tag: (type, [values])} with type 3 SHORT, 4 LONG,
    5 RATIONAL ([(num, den)]); ImageWidth, ImageLength, RowsPerStrip,
    StripOffsets and StripByteCounts are added.  next_ifd: the offset written
    after the IFD ("self" = the IFD's own)."""
    e = ">" if big_endian else "<"
    out = bytearray((b"MM" if big_endian else b"II") + struct.pack(e + "HI", magic, 0))
    offs = []
    for s in strip_data:
        offs.append(len(out))
        out += s
    if len(out) & 1:
        out += b"\0"
    t = {256: (4, [w]), 257: (4, [h]), 278: (4, [rps]), 273: (4, offs)}
    if counts:
        t[279] = (4, [len(s) for s in strip_data])
    t.update(tags)
    ifd = len(out)
    struct.pack_into(e + "I", out, 4, ifd)
    extra_at = ifd + 2 + 12 * len(t) + 4
    body, extra = bytearray(struct.pack(e + "H", len(t))), bytearray()
    for tag in sorted(t):
        typ, vals = t[tag]
        if typ == 5:
            data = b"".join(struct.pack(e + "II", *v) for v in vals)
        else:
            data = b"".join(struct.pack(e + ("H" if typ == 3 else "I"), v) for v in vals)
        body += struct.pack(e + "HHI", tag, typ, len(vals))
        if len(data) <= 4:
            body += data.ljust(4, b"\0")
        else:
            body += struct.pack(e + "I", extra_at + len(extra))
            extra += data
            if len(extra) & 1:
                extra += b"\0"
    body += struct.pack(e + "I", ifd if next_ifd == "self" else next_ifd)
    return bytes(out + body + extra)


def packbits_literal(rows):
    """Rows (h, n) as PackBits literals, a row at a time (as encoders do)."""
    out = bytearray()
    for r in rows:
        r = bytes(r)
        for i in range(0, len(r), 128):
            c = r[i:i + 128]
            out += bytes([len(c) - 1]) + c
    return bytes(out)


BITREV = np.array([int("{:08b}".format(i)[::-1], 2) for i in range(256)], np.uint8)


def patch_array(raw, page, tag, index, value):
    """`raw` (a little-endian classic TIFF, bytearray) with element `index` of
    the SHORT / LONG array of `tag` in IFD `page` set to `value`."""
    ifd = struct.unpack_from("<I", raw, 4)[0]
    for _ in range(page):
        n = struct.unpack_from("<H", raw, ifd)[0]
        ifd = struct.unpack_from("<I", raw, ifd + 2 + 12 * n)[0]
    n = struct.unpack_from("<H", raw, ifd)[0]
    for i in range(n):
        e = ifd + 2 + 12 * i
        t, typ, count = struct.unpack_from("<HHI", raw, e)
        if t != tag:
            continue
        size = {3: 2, 4: 4}[typ]
        at = e + 8 if count * size <= 4 else struct.unpack_from("<I", raw, e + 8)[0]
        struct.pack_into("<H" if typ == 3 else "<I", raw, at + size * index, value)
        return
    raise KeyError(tag)
