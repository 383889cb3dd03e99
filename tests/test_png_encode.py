"""CPU tests of the lossless PNG encoder's host twin (uphip_png_encode_host,
csrc/png_enc_core.h), of uphip_png_wrap and of the PDF writer's Flate pages.
Every file is decoded three ways: zlib plus the filters undone in numpy, PIL,
and the project's own PNG reader."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from unpaper_hip import ctypes_abi as A
from unpaper_hip import pipeline as P
from unpaper_hip.device import load_library
from unpaper_hip.pdf import PdfDocument, PdfWriter

import png_cases as K
from helpers import page_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def encode(fmt, width, rows, offset=0, dpi=0):
    return P.png_encode_host(rows, width, fmt, offset=offset, dpi=dpi)


@pytest.mark.parametrize("case", K.CASES, ids=K.CASE_IDS)
def test_decodes_three_ways(case, tmp_path):
    name, fmt, width, rows = case
    height = rows.shape[0]
    png = encode(fmt, width, rows)
    want = K.png_samples(fmt, width, rows)
    ch = K.chunks(png)
    assert [c[0] for c in ch] == [b"IHDR", b"IDAT", b"IEND"]
    assert ch[0][1] == struct.pack(">IIBBBBB", width, height, 1 if fmt in K.MONO else 8, K.COLOUR_TYPE[fmt], 0, 0, 0)
    stream = ch[1][1]
    assert stream[:2] == b"\x78\x01"
    assert len(stream) <= K.stored_bound(fmt, width, height)
    got, filters = K.unfilter(fmt, width, height, stream)
    assert np.array_equal(got, want)  # the pad bits of bilevel rows included: 0
    if fmt in K.MONO:
        assert not filters.any()
    assert np.array_equal(K.pil_samples(png, fmt, width), want)
    path = tmp_path / "a.png"
    path.write_bytes(png)
    img = P.image_read(str(path))
    assert (img.width, img.height) == (width, height)
    assert img.format == (A.FMT_MONOBLACK if fmt in K.MONO else fmt)
    assert np.array_equal(img.data[:, :want.shape[1]], want)


@pytest.mark.parametrize("name", K.EMBED_IDS)
def test_pitch_and_offset_do_not_matter(name):
    _, fmt, width, rows = K.CASES[K.CASE_IDS.index(name)]
    big, byte_off, bit_off = K.embed(fmt, width, rows)
    L = load_library()
    h = rows.shape[0]
    buf = np.zeros(K.stored_bound(fmt, width, h) + 200, np.uint8)
    n = L.uphip_png_encode_host(big.ctypes.data + byte_off, big.shape[1], bit_off, width, h, fmt, 0,
                                buf.ctypes.data, buf.size)
    assert n > 0
    assert buf[:n].tobytes() == encode(fmt, width, K.tight(fmt, width, rows))


def test_noise_is_stored():
    for name in ("noise_gray", "noise_rgb"):
        _, fmt, width, rows = K.CASES[K.CASE_IDS.index(name)]
        stream = K.idat(encode(fmt, width, rows))
        assert K.is_stored(stream)
        assert len(stream) <= K.stored_bound(fmt, width, rows.shape[0])
    _, fmt, width, rows = K.CASES[K.CASE_IDS.index("page_gray_203x131")]
    assert not K.is_stored(K.idat(encode(fmt, width, rows)))


def test_filters_are_chosen_per_row():
    """Rows equal to the row above take Up, a flat row takes Sub, noise None."""
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 256, (1, 64), dtype=np.uint8)
    rows = np.concatenate([noise, noise, np.full((1, 64), 9, np.uint8),
                           rng.integers(0, 256, (1, 64), dtype=np.uint8)])
    _, filters = K.unfilter(A.FMT_GRAY8, 64, 4, K.idat(encode(A.FMT_GRAY8, 64, rows)))
    assert list(filters) == [0, 2, 1, 0]


def test_wide_rows_do_not_match_beyond_the_window():
    """32769 gray pixels a row: the byte above is 32770 back, past Deflate's
    window; zlib refuses a stream that points there."""
    _, fmt, width, rows = K.CASES[K.CASE_IDS.index("gray_32769x3")]
    rows = rows.copy()
    rows[1, 5] ^= 0x55  # rows 1 and 2 then differ from the row above in places
    rows[2, 9] ^= 0x33
    got, _ = K.unfilter(fmt, width, 3, K.idat(encode(fmt, width, rows)))
    assert np.array_equal(got, rows)


@pytest.mark.parametrize("dpi", [72, 300, 600])
def test_phys_chunk(dpi):
    rows = np.full((3, 5), 200, np.uint8)
    ch = K.chunks(encode(A.FMT_GRAY8, 5, rows, dpi=dpi))
    assert [c[0] for c in ch] == [b"IHDR", b"pHYs", b"IDAT", b"IEND"]
    ppm = round(dpi / 0.0254)
    assert ch[1][1] == struct.pack(">IIB", ppm, ppm, 1)


def test_wrap_makes_the_same_file():
    _, fmt, width, rows = K.CASES[K.CASE_IDS.index("page_rgb_203x131")]
    png = encode(fmt, width, rows, dpi=300)
    assert P.png_wrap(K.idat(png), width, rows.shape[0], fmt, dpi=300) == png


# ---- size conditions ------------------------------------------------------

def test_white_a4_page_shrinks_to_a_hundredth():
    rows = np.full((1754, 1240), 255, np.uint8)
    assert len(encode(A.FMT_GRAY8, 1240, rows)) <= rows.size // 100


@pytest.mark.parametrize("size", [(203, 131), (1240, 1754)])
def test_scanned_page_shrinks_to_a_half(size):
    w, h = size
    rows = page_array(w, h, seed=1)
    png = encode(A.FMT_GRAY8, w, rows)
    print("page_array %dx%d: %d bytes, %.1f %% of raw" % (w, h, len(png), 100.0 * len(png) / rows.size))
    assert len(png) <= rows.size // 2
    got, _ = K.unfilter(A.FMT_GRAY8, w, h, K.idat(png))
    assert np.array_equal(got, rows)


# ---- PDF ------------------------------------------------------------------

def test_pdf_flate_pages_read_back(tmp_path):
    path = str(tmp_path / "a.pdf")
    names = ["page_gray_203x131", "page_rgb_203x131", "monow_33x65", "monob_33x65", "noise_gray"]
    w = PdfWriter.create(path, dpi=150)
    streams = []
    for name in names:
        _, fmt, width, rows = K.CASES[K.CASE_IDS.index(name)]
        streams.append(K.idat(encode(fmt, width, rows)))
        w.add_page_flate(streams[-1], width, rows.shape[0], fmt)
    w.close()
    with PdfDocument.open(path) as doc:
        assert doc.page_count == len(names)
        for i, name in enumerate(names):
            _, fmt, width, rows = K.CASES[K.CASE_IDS.index(name)]
            img = doc.read_page(i)
            want = K.png_samples(fmt, width, rows)
            assert (img.width, img.height) == (width, rows.shape[0])
            # bilevel samples are in PNG sense (1 = white): DeviceGray's own
            assert img.format == (A.FMT_MONOBLACK if fmt in K.MONO else fmt)
            assert np.array_equal(img.data[:, :want.shape[1]], want), name
            assert abs(doc.page_info(i)[0] - width * 72.0 / 150) < 0.01
            assert doc.extract_page_image(i).data == streams[i]
    _pil_sees_streams(path, streams)


def _pil_sees_streams(path, streams):
    """PIL's PdfParser walks the page tree to each image and returns the same
    stream bytes (it inflates /FlateDecode itself)."""
    from PIL import PdfParser
    with PdfParser.PdfParser(path) as pdf:
        assert len(pdf.pages) == len(streams)
        for ref, s in zip(pdf.pages, streams):
            page = pdf.read_indirect(ref)
            im = page[b"Resources"][b"XObject"][b"Im0"]
            if isinstance(im, PdfParser.IndirectReference):
                im = pdf.read_indirect(im)
            assert im.dictionary[b"Filter"] == b"FlateDecode" or str(im.dictionary[b"Filter"]) == "FlateDecode"
            assert im.dictionary[b"DecodeParms"][b"Predictor"] == 15
            assert im.decode() == zlib.decompress(s)


def test_pdf_flate_refuses_alpha(tmp_path):
    w = PdfWriter.create(str(tmp_path / "a.pdf"))
    _, fmt, width, rows = K.CASES[K.CASE_IDS.index("ya_33x65")]
    L = load_library()
    s = K.idat(encode(fmt, width, rows))
    assert L.uphip_pdf_writer_add_page_flate(w.handle, s, len(s), width, 65, fmt, 0) == -1
    assert b"alpha" in L.uphip_last_error()
    L.uphip_clear_error()
    w.abort()


# ---- argument errors ------------------------------------------------------

def test_argument_errors():
    L = load_library()
    rows = np.zeros((4, 16), np.uint8)
    out = np.zeros(4096, np.uint8)
    p, o = rows.ctypes.data, out.ctypes.data
    bad = [
        (None, 16, 0, 8, 4, A.FMT_GRAY8, 0, o, 4096),     # null pixels
        (p, 16, 0, 0, 4, A.FMT_GRAY8, 0, o, 4096),        # zero width
        (p, 16, 0, 8, 0, A.FMT_GRAY8, 0, o, 4096),        # zero height
        (p, 16, 0, 8, 4, 17, 0, o, 4096),                 # bad format
        (p, 16, 3, 8, 4, A.FMT_GRAY8, 0, o, 4096),        # offset on a byte format
        (p, 16, 3, 4, 4, A.FMT_RGB24, 0, o, 4096),
        (p, 16, -1, 8, 4, A.FMT_MONOWHITE, 0, o, 4096),   # negative offset
        (p, 16, 125, 8, 4, A.FMT_MONOBLACK, 0, o, 4096),  # pixels past the row
        (p, 7, 0, 8, 4, A.FMT_GRAY8, 0, o, 4096),         # stride below a row
        (p, 16, 0, 8, 4, A.FMT_GRAY8, -5, o, 4096),       # negative dpi
        (p, 16, 0, 8, 4, A.FMT_GRAY8, 0, o, 10),          # buffer too small
    ]
    for args in bad:
        assert L.uphip_png_encode_host(*args) == -1, args
        assert L.uphip_last_error()
        L.uphip_clear_error()
    assert L.uphip_png_encode_host(p, 16, 0, 8, 4, A.FMT_GRAY8, 0, None, 0) > 0  # sizes a buffer
    z = b"\x78\x01\x03\x00\x00\x00\x00\x01"
    for args in [(None, 8, 1, 1, A.FMT_GRAY8, 0, o, 4096), (z, 0, 1, 1, A.FMT_GRAY8, 0, o, 4096),
                 (z, 8, 0, 1, A.FMT_GRAY8, 0, o, 4096), (z, 8, 1, 1, 9, 0, o, 4096),
                 (z, 8, 1, 1, A.FMT_GRAY8, 0, o, 20)]:
        assert L.uphip_png_wrap(*args) == -1, args
        assert L.uphip_last_error()
        L.uphip_clear_error()


# ---- the host twin under ASan / UBSan ---------------------------------------

def test_host_twin_under_sanitizers():
    """tests/c/png_enc_main.cpp: a stand-alone program that runs the host twin
    over its own list of the cases above, inflates every stream with zlib and
    compares the samples (make sanitize_png builds and runs it)."""
    r = subprocess.run(["make", "-s", "sanitize_png"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "png_enc_main: ok" in r.stdout
