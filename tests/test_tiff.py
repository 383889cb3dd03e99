"""Host TIFF reader (uphip_tiff_*, uphip_image_*; csrc/tiff.cpp and the strip
decoder of csrc/tiff_strip.h, the device kernels' host twin): runs on the CPU.

Files are written here by PIL (libtiff) or by the hand writer of
tests/tiff_cases.py; the expected pixels are PIL's for the same file.

- every mode x every compression it takes, Predictor 2 on L / LA / RGB, widths
  1, 7, 8, 9, 333 and 2481, heights 1 and 50, RowsPerStrip 1, 3 and the height
  (a short last strip included);
- LZW: a noise strip that fills the table and takes a Clear mid-strip, an
  all-white page (KwKwK, strings thousands of bytes long), strips of 65,536
  and 65,537 bytes and pages of 7 and 8 strips against the routing rule;
- big-endian, FillOrder 2 (raw, PackBits and Group 4), MinIsWhite, three IFDs,
  a file of uphip_tiff_g4_write read back;
- every refusal names its tag; hostile headers; truncations and byte flips
  return an error or pixels and never write outside the page;
- the same files through tests/c/tiff_main.cpp under ASan / UBSan.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import tiff_cases as T
from unpaper_hip import ctypes_abi as A
from unpaper_hip.device import UnpaperHipError, load_library
from unpaper_hip.pipeline import TiffDocument, g4_encode_host, image_read, tiff_g4_write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COMPS = {"1": ["raw", "packbits", "tiff_lzw", "tiff_adobe_deflate", "group3", "group4"],
         "L": ["raw", "packbits", "tiff_lzw", "tiff_adobe_deflate"],
         "LA": ["raw", "packbits", "tiff_lzw", "tiff_adobe_deflate"],
         "RGB": ["raw", "packbits", "tiff_lzw", "tiff_adobe_deflate"],
         "P": ["raw", "packbits", "tiff_lzw", "tiff_adobe_deflate"]}
MATRIX = [(m, c, 1) for m in COMPS for c in COMPS[m]] + \
         [(m, c, 2) for m in ("L", "LA", "RGB") for c in ("tiff_lzw", "tiff_adobe_deflate")]
SHAPES = [(w, h, rps) for w in (1, 7, 8, 9, 333, 2481) for h, rr in ((1, (1,)), (50, (1, 3, 50)))
          for rps in rr]


@pytest.fixture(scope="module")
def case_dir(tmp_path_factory):
    """Every file the tests below write: the sanitizer program reads them all."""
    return str(tmp_path_factory.mktemp("tiff_cases"))


def _last_error(L):
    e = L.uphip_last_error()
    L.uphip_clear_error()
    return e.decode() if e else ""


def check_file(path, npages=1):
    """The library's pages of `path` equal PIL's."""
    d = TiffDocument(path)
    try:
        assert d.page_count == npages
        for p in range(npages):
            fmt, w, h, want = T.expected(path, p)
            assert d.probe(p)[:3] == (w, h, fmt), path
            got = d.read_page(p)
            assert np.array_equal(T.pixels(fmt, w, got.data), want), (path, p)
    finally:
        d.close()


@pytest.mark.parametrize("mode,comp,pred", MATRIX, ids=["%s-%s-p%d" % t for t in MATRIX])
def test_format_matrix(case_dir, mode, comp, pred):
    for w, h, rps in SHAPES:
        path = os.path.join(case_dir, "m_%s_%s_%d_%dx%d_%d.tif" % (mode, comp, pred, w, h, rps))
        T.save(path, T.page(mode, w, h, seed=w + h), comp, rps=rps, predictor=pred if pred == 2 else None)
        with Image.open(path) as im:
            assert im.tag_v2[259] == T.COMP[comp] and im.tag_v2.get(317, 1) == pred
            assert len(im.tag_v2[273]) == (h + rps - 1) // rps
        check_file(path)


# ---- LZW corners -------------------------------------------------------------

def test_lzw_noise_fills_the_table_and_clears(case_dir):
    """One strip of 60,000 noise bytes: about 40,000 codes, so libtiff's coder
    fills the 4,094 entries and emits Clear about ten times inside the strip."""
    path = os.path.join(case_dir, "lzw_noise.tif")
    a = T.noise(300 * 200, 5).reshape(200, 300)
    T.save(path, Image.fromarray(a, "L"), "tiff_lzw", rps=200)
    off, cnt, _ = T.strips(path)
    assert len(off) == 1 and cnt[0] > 4094 * 12 // 8
    check_file(path)


def test_lzw_all_white(case_dir):
    """KwKwK on every code; the strings grow to thousands of bytes."""
    path = os.path.join(case_dir, "lzw_white.tif")
    T.save(path, Image.new("L", (2481, 26), 255), "tiff_lzw", rps=26)
    off, cnt, _ = T.strips(path)
    assert len(off) == 1 and cnt[0] < 1000
    check_file(path)


@pytest.mark.parametrize("w,rps,h,device", [(256, 256, 2048, True), (65537, 1, 8, False),
                                            (333, 3, 21, False), (333, 3, 22, True)],
                         ids=["65536-byte-strips", "65537-byte-strips", "7-strips", "8-strips"])
def test_lzw_strip_size_and_routing(case_dir, w, rps, h, device):
    path = os.path.join(case_dir, "route_%d_%d_%d.tif" % (w, rps, h))
    T.save(path, T.page("L", w, h, seed=3), "tiff_lzw", rps=rps)
    off, _, r = T.strips(path)
    assert r == rps and len(off) == (h + rps - 1) // rps
    check_file(path)
    d = TiffDocument(path)
    try:
        assert d.on_device(0) is device
    finally:
        d.close()


def test_routing_by_compression(case_dir):
    for comp, want in (("packbits", True), ("tiff_adobe_deflate", False), ("raw", False)):
        path = os.path.join(case_dir, "route_%s.tif" % comp)
        T.save(path, T.page("L", 100, 40), comp, rps=2)
        d = TiffDocument(path)
        try:
            assert d.on_device(0) is want, comp
        finally:
            d.close()


# ---- container cases -----------------------------------------------------------

def _hand(case_dir, name, data):
    path = os.path.join(case_dir, name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def _bilevel_rows(w, h, seed):
    bits = (T.noise(h * w, seed).reshape(h, w) > 150).astype(np.uint8)
    return bits, np.packbits(bits, axis=1)


@pytest.mark.parametrize("big", [False, True], ids=["II", "MM"])
@pytest.mark.parametrize("phot", [0, 1])
def test_hand_built_raw_bilevel(case_dir, big, phot):
    w, h, rps = 701, 9, 4
    bits, rows = _bilevel_rows(w, h, 11)
    data = T.build(w, h, [rows[i:i + rps].tobytes() for i in range(0, h, rps)], rps,
                   {258: (3, [1]), 259: (3, [1]), 262: (3, [phot]), 277: (3, [1]),
                    282: (5, [(300, 1)]), 283: (5, [(600, 2)]), 296: (3, [2])}, big_endian=big)
    path = _hand(case_dir, "hand_raw_%d_%d.tif" % (big, phot), data)
    check_file(path)
    d = TiffDocument(path)
    try:
        assert d.probe(0) == (w, h, A.FMT_MONOWHITE if phot == 0 else A.FMT_MONOBLACK, (300.0, 300.0))
        assert np.array_equal(T.pixels(A.FMT_MONOWHITE, w, d.read_page(0).data), bits)  # bits as stored
    finally:
        d.close()


@pytest.mark.parametrize("big", [False, True], ids=["II", "MM"])
def test_big_endian_gray_lzw(case_dir, big):
    """PIL's LZW strips in a hand-built container of either byte order, SHORT
    offsets and counts."""
    src = T.save(os.path.join(case_dir, "be_src.tif"), T.page("L", 333, 20), "tiff_lzw", rps=3, predictor=2)
    off, cnt, _ = T.strips(src)
    raw = open(src, "rb").read()
    data = T.build(333, 20, [raw[o:o + c] for o, c in zip(off, cnt)], 3,
                   {258: (3, [8]), 259: (3, [5]), 262: (3, [1]), 277: (3, [1]), 317: (3, [2])}, big_endian=big)
    path = _hand(case_dir, "be_lzw_%d.tif" % big, data)
    check_file(path)
    assert np.array_equal(image_read(path).payload(), T.expected(src)[3])


@pytest.mark.parametrize("comp", ["raw", "packbits", "group4"])
def test_fill_order_2(case_dir, comp):
    w, h = 701, 90
    bits, rows = _bilevel_rows(w, h, 12)
    tags = {258: (3, [1]), 262: (3, [0]), 266: (3, [2]), 277: (3, [1])}
    if comp == "group4":
        stream = np.frombuffer(g4_encode_host(rows, w), np.uint8)
        strip, tags[259], tags[293] = T.BITREV[stream].tobytes(), (3, [4]), (4, [0])
    elif comp == "raw":
        strip, tags[259] = T.BITREV[rows].tobytes(), (3, [1])
    else:
        packed = np.frombuffer(T.packbits_literal(rows), np.uint8)
        strip, tags[259] = T.BITREV[packed].tobytes(), (3, [32773])
    path = _hand(case_dir, "fill2_%s.tif" % comp, T.build(w, h, [strip], h, tags))
    check_file(path)
    d = TiffDocument(path)
    try:
        assert np.array_equal(T.pixels(A.FMT_MONOWHITE, w, d.read_page(0).data), bits)
    finally:
        d.close()


@pytest.mark.parametrize("mode,comp", [("L", "tiff_lzw"), ("L", "raw"), ("1", "group4"), ("1", "packbits")])
def test_min_is_white(case_dir, mode, comp):
    path = os.path.join(case_dir, "miw_%s_%s.tif" % (mode, comp))
    T.save(path, T.page(mode, 77, 30), comp, rps=7, tags={262: 0})
    with Image.open(path) as im:
        assert im.tag_v2[262] == 0
    check_file(path)


def test_three_ifds(case_dir):
    path = os.path.join(case_dir, "three.tif")
    T.save(path, T.page("L", 120, 40, 1), "tiff_lzw", rps=5,
           more=[T.page("RGB", 64, 33, 2), T.page("1", 203, 17, 3)])
    check_file(path, 3)
    d = TiffDocument(path)
    try:
        assert [d.probe(p)[:3] for p in range(3)] == [(120, 40, A.FMT_GRAY8), (64, 33, A.FMT_RGB24),
                                                      (203, 17, A.FMT_MONOBLACK)]
        with pytest.raises(UnpaperHipError, match="out of range"):
            d.probe(3)
    finally:
        d.close()
    # the single-image entries read the first
    assert np.array_equal(image_read(path).payload(), T.expected(path, 0)[3])


def test_g4_write_reads_back(case_dir):
    w, h = 203, 131
    bits, rows = _bilevel_rows(w, h, 13)
    path = os.path.join(case_dir, "g4_written.tif")
    tiff_g4_write(path, g4_encode_host(rows, w), w, h, dpi=150)
    d = TiffDocument(path)
    try:
        assert d.probe(0) == (w, h, A.FMT_MONOWHITE, (150.0, 150.0))
        assert np.array_equal(T.pixels(A.FMT_MONOWHITE, w, d.read_page(0).data), bits)
    finally:
        d.close()
    check_file(path)


def test_group3_two_dimensional(case_dir):
    path = os.path.join(case_dir, "g3_2d.tif")
    T.save(path, T.page("1", 333, 50), "group3", rps=7, tags={292: 1})
    with Image.open(path) as im:
        assert im.tag_v2[292] & 1
    check_file(path)


# ---- refusals and hostile files -------------------------------------------------

GRAY = {258: (3, [8]), 259: (3, [1]), 262: (3, [1]), 277: (3, [1])}


def _gray_file(tags, **kw):
    t = dict(GRAY)
    t.update(tags)
    return T.build(16, 4, [bytes(256)], 4, t, **kw)


REFUSALS = [
    ("bigtiff", lambda: _gray_file({}, magic=43), "BigTIFF"),
    ("tiles", lambda: _gray_file({322: (3, [16]), 323: (3, [16])}), "TileWidth"),
    ("planar", lambda: _gray_file({258: (3, [8, 8, 8]), 262: (3, [2]), 277: (3, [3]), 284: (3, [2])}),
     "PlanarConfiguration 2"),
    ("bits2", lambda: _gray_file({258: (3, [2])}), "BitsPerSample 2"),
    ("bits4", lambda: _gray_file({258: (3, [4])}), "BitsPerSample 4"),
    ("bits16", lambda: _gray_file({258: (3, [16])}), "BitsPerSample 16"),
    ("rgba", lambda: _gray_file({258: (3, [8, 8, 8, 8]), 262: (3, [2]), 277: (3, [4]), 338: (3, [2])}),
     "SamplesPerPixel 4"),
    ("extra2", lambda: _gray_file({258: (3, [8, 8, 8]), 277: (3, [3]), 338: (3, [2, 2])}), "ExtraSamples"),
    ("ycbcr", lambda: _gray_file({258: (3, [8, 8, 8]), 262: (3, [6]), 277: (3, [3])}),
     "PhotometricInterpretation 6"),
    ("cmyk", lambda: _gray_file({258: (3, [8, 8, 8, 8]), 262: (3, [5]), 277: (3, [4])}),
     "PhotometricInterpretation 5"),
    ("cielab", lambda: _gray_file({258: (3, [8, 8, 8]), 262: (3, [8]), 277: (3, [3])}),
     "PhotometricInterpretation 8"),
    ("predictor_1bit", lambda: _gray_file({258: (3, [1]), 259: (3, [5]), 317: (3, [2])}),
     "Predictor 2 with BitsPerSample 1"),
] + [("comp%d" % c, lambda c=c: _gray_file({259: (3, [c])}), "Compression %d" % c)
     for c in (2, 6, 7, 34925, 34712)]


@pytest.mark.parametrize("name,make,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_tag(case_dir, name, make, word):
    L = load_library()
    path = _hand(case_dir, "refuse_%s.tif" % name, make())
    info = A.PnmInfo()
    assert L.uphip_tiff_probe(path.encode(), C.byref(info)) == -1
    assert word in _last_error(L)
    assert L.uphip_image_probe(path.encode(), C.byref(info)) == -1
    assert word in _last_error(L)


def _read_guarded(L, path, info):
    """uphip_tiff_read into a buffer with sentinel bytes between the rows and
    around the page; returns the status after checking the sentinel."""
    rb = T.row_bytes(info.format, info.width)
    ls = rb + 7
    buf = np.full((info.height + 2) * ls, 0xA5, np.uint8)
    page = buf[ls:ls + info.height * ls].reshape(info.height, ls)
    r = L.uphip_tiff_read(path.encode(), page.ctypes.data, ls, None)
    L.uphip_clear_error()
    assert (buf[:ls] == 0xA5).all() and (buf[ls + info.height * ls:] == 0xA5).all(), path
    assert (page[:, rb:] == 0xA5).all(), path
    return r


def test_hostile_files(case_dir):
    L = load_library()
    info = A.PnmInfo()

    def probe(name, data):
        path = _hand(case_dir, "hostile_%s.tif" % name, data)
        r = L.uphip_tiff_probe(path.encode(), C.byref(info))
        return r, _last_error(L), path

    # an IFD whose next pointer is itself: one page, and the walk ends
    r, _, path = probe("loop", _gray_file({}, next_ifd="self"))
    assert r == 0
    d = TiffDocument(path)
    assert d.page_count == 1
    d.close()
    # strip offsets past the end of the file
    r, e, _ = probe("offsets", _gray_file({273: (4, [1 << 20])}))
    assert r == -1 and "StripOffsets" in e
    # a header claiming 2^31 pixels over a few bytes: refused, nothing decoded
    r, e, _ = probe("huge_raw", T.build(46340, 46340, [bytes(64)], 46340, GRAY))
    assert r == -1 and "StripByteCounts" in e
    lz = dict(GRAY)
    lz[259] = (3, [5])
    r, e, _ = probe("huge_lzw", T.build(46340, 46340, [bytes(64)], 46340, lz))
    assert r == -1 and "StripByteCounts" in e
    r, e, _ = probe("huge_side", T.build((1 << 20) + 1, 4, [bytes(64)], 4, GRAY))
    assert r == -1 and "ImageWidth" in e
    # a wrong strip count
    r, e, _ = probe("nstrips", T.build(16, 4, [bytes(64), bytes(64), bytes(64)], 2, GRAY))
    assert r == -1 and "StripOffsets has 3 entries for 2 strips" in e
    # StripByteCounts missing: one uncompressed strip only
    r, _, path = probe("nocounts", T.build(16, 4, [bytes(range(64))], 4, GRAY, counts=False))
    assert r == 0
    assert np.array_equal(image_read(path).payload().ravel(), np.arange(64, dtype=np.uint8))
    r, e, _ = probe("nocounts_lzw", T.build(16, 4, [bytes(64)], 4, lz, counts=False))
    assert r == -1 and "StripByteCounts" in e
    # old-style LZW (first byte 0, second odd)
    r, _, path = probe("old_lzw", T.build(16, 4, [b"\x00\x01" + bytes(62)], 4, lz))
    assert r == 0
    assert _read_guarded(L, path, info) == -1
    buf = np.zeros(64, np.uint8)
    assert L.uphip_tiff_read(path.encode(), buf.ctypes.data, 16, None) == -1
    assert "old-style" in _last_error(L)


# ---- corruption -------------------------------------------------------------------

CORRUPT = [("1", "raw"), ("L", "packbits"), ("RGB", "tiff_lzw"), ("LA", "tiff_adobe_deflate"),
           ("1", "group3"), ("1", "group4")]


@pytest.mark.parametrize("mode,comp", CORRUPT, ids=[c for _, c in CORRUPT])
def test_truncations_and_flips(case_dir, mode, comp):
    """Every truncation at a multiple of 97 bytes and 200 seeded single-byte
    flips: an error or pixels, and nothing written outside the page."""
    L = load_library()
    src = os.path.join(case_dir, "corrupt_src_%s.tif" % comp)
    T.save(src, T.page(mode, 333, 50, seed=9), comp, rps=7, predictor=2 if comp == "tiff_lzw" else None)
    good = open(src, "rb").read()
    fmt, w, h, _ = T.expected(src)
    info = A.PnmInfo(w, h, fmt)
    variants = [("t%05d" % n, good[:n]) for n in range(0, len(good), 97)]
    rng = np.random.default_rng(1234)
    for k in range(200):
        at = int(rng.integers(0, len(good)))
        b = bytearray(good)
        b[at] ^= int(rng.integers(1, 256))
        variants.append(("f%03d" % k, bytes(b)))
    ok = 0
    for name, data in variants:
        path = _hand(case_dir, "corrupt_%s_%s.tif" % (comp, name), data)
        probe = A.PnmInfo()
        if L.uphip_tiff_probe(path.encode(), C.byref(probe)) != 0:
            L.uphip_clear_error()
            continue
        if (probe.width, probe.height, probe.format) != (w, h, fmt):
            continue  # the flip hit the geometry: the sanitizer program reads these
        ok += _read_guarded(L, path, info) == 0
    assert ok > 0  # some flips leave a readable file


# ---- the sanitizer program ---------------------------------------------------------

def test_reader_under_sanitizers(case_dir):
    """tests/c/tiff_main.cpp, a stand-alone host program built with
    -fsanitize=address,undefined (make sanitize_tiff), over every file the
    tests above wrote, or over a set of its own when run alone."""
    if len(os.listdir(case_dir)) < 50:
        for mode, comp, pred in MATRIX:
            T.save(os.path.join(case_dir, "s_%s_%s_%d.tif" % (mode, comp, pred)), T.page(mode, 333, 50), comp,
                   rps=3, predictor=pred if pred == 2 else None)
    r = subprocess.run(["make", "-s", "sanitize_tiff", "TIFF_DIR=" + case_dir], cwd=ROOT, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "tiff_main: ok" in r.stdout
