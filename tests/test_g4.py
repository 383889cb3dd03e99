"""CPU tests of the CCITT Group 4 encoder: the host form of the coder the
device kernels share (csrc/g4_row.h) against libtiff's streams
(tests/golden/g4, written by make_g4_fixtures.py), the PDF and TIFF
containers around a stream, and the argument checks.  Every comparison is
exact."""
import ctypes as C

import numpy as np
import pytest

import g4_cases
from unpaper_hip import ctypes_abi as A
from unpaper_hip.device import load_library
from unpaper_hip.pipeline import g4_encode_host, tiff_g4_write


def _err():
    L = load_library()
    e = L.uphip_last_error()
    L.uphip_clear_error()
    return e.decode() if e else ""


def test_every_case_has_a_fixture():
    assert sorted(g4_cases.manifest()) == sorted(g4_cases.NAMES)


@pytest.mark.parametrize("name", g4_cases.NAMES)
def test_host_encoder_equals_libtiff(name):
    bits, want = g4_cases.load(name)
    got = g4_encode_host(g4_cases.pack(bits), bits.shape[1])
    assert len(got) == len(want) and got == want


@pytest.mark.parametrize("offset", [1, 7, 8, 13, 37])
@pytest.mark.parametrize("name", g4_cases.NAMES)
def test_host_encoder_bit_offset_and_padding(name, offset):
    """The page `offset` bits into rows whose every other bit is 1: the bits
    before the page, the padding after it and whole slack bytes must not be
    read as pixels."""
    bits, want = g4_cases.load(name)
    h, w = bits.shape
    rows = np.ones((h, offset + w + 19), np.uint8)
    rows[:, offset:offset + w] = bits
    got = g4_encode_host(np.packbits(rows, axis=1), w, bit_offset=offset)
    assert got == want


@pytest.mark.parametrize("name", g4_cases.NAMES)
def test_pdf_page_round_trip(name, tmp_path):
    """A stream wrapped by add_page_g4 and read back by the project's own
    reader and T.6 decoder: black (1) comes back as gray 0, white as 255."""
    from unpaper_hip.pdf import PdfDocument, PdfWriter
    bits, stream = g4_cases.load(name)
    h, w = bits.shape
    path = str(tmp_path / "page.pdf")
    wr = PdfWriter.create(path, dpi=300)
    wr.add_page_g4(stream, w, h)
    wr.close()
    raw = open(path, "rb").read()
    for key in (b"/Filter /CCITTFaxDecode", b"/K -1", b"/Columns %d" % w, b"/Rows %d" % h,
                b"/BlackIs1 true", b"/BitsPerComponent 1", b"/DeviceGray", b"/Decode [1 0]"):
        assert key in raw, key
    d = PdfDocument.open(path)
    try:
        assert d.page_count == 1
        im = d.extract_page_image(0)
        assert (im.width, im.height, im.bits_per_component) == (w, h, 1) and im.data == stream
        page = d.read_page(0)
    finally:
        d.close()
    assert (page.width, page.height, page.format) == (w, h, A.FMT_GRAY8)
    assert np.array_equal(page.payload(), np.where(bits, 0, 255).astype(np.uint8))


def test_tiff_container_opens_in_pil(tmp_path):
    from PIL import Image, features
    if not features.check("libtiff"):
        pytest.skip("PIL without libtiff cannot read Group 4")
    for name in ("rand_64x333", "blobs_24x96", "one_2x5300", "width_1"):
        bits, stream = g4_cases.load(name)
        h, w = bits.shape
        path = str(tmp_path / (name + ".tif"))
        tiff_g4_write(path, stream, w, h, 200)
        with Image.open(path) as im:
            t = im.tag_v2
            assert (t[256], t[257], t[258], t[259], t[262], t[266]) == (w, h, (1,), 4, 0, 1)
            assert (t[277], t[278], t[279], t[293], t[296]) == (1, h, (len(stream),), 0, 2)
            assert float(t[282]) == 200.0 and float(t[283]) == 200.0
            px = np.array(im.convert("L"))
        assert np.array_equal(px, np.where(bits, 0, 255).astype(np.uint8)), name


def test_argument_errors(tmp_path):
    L = load_library()
    rows = np.zeros((4, 2), np.uint8)
    out = np.zeros(64, np.uint8)
    p, o = rows.ctypes.data, out.ctypes.data
    assert L.uphip_g4_encode_host(None, 2, 0, 16, 4, o, 64) == -1 and "null" in _err()
    for w, h in ((0, 4), (-3, 4), (16, 0), (16, -1)):
        assert L.uphip_g4_encode_host(p, 2, 0, w, h, o, 64) == -1
        assert "invalid size" in _err()
    assert L.uphip_g4_encode_host(p, 2, -1, 16, 4, o, 64) == -1 and "do not fit" in _err()
    assert L.uphip_g4_encode_host(p, 2, 1, 16, 4, o, 64) == -1 and "do not fit" in _err()
    # too small a buffer: the size comes back and nothing is written
    out[:] = 0xAA
    n = L.uphip_g4_encode_host(p, 2, 0, 16, 4, o, 2)
    assert n == 4 and (out == 0xAA).all() and _err() == ""
    assert L.uphip_g4_encode_host(p, 2, 0, 16, 4, None, 0) == n
    assert L.uphip_g4_encode_host(p, 2, 0, 16, 4, o, n) == n and (out[n:] == 0xAA).all()
    # four white rows: four V0 codes, EOFB
    assert out[:n].tobytes() == bytes([0xF0, 0x01, 0x00, 0x10])
    assert L.uphip_tiff_g4_write(None, o, 4, 16, 4, 0) == -1 and "null" in _err()
    path = str(tmp_path / "x.tif").encode()
    assert L.uphip_tiff_g4_write(path, o, 4, 0, 4, 0) == -1 and "invalid size" in _err()
    assert L.uphip_tiff_g4_write(path, o, 4, 16, 4, -5) == -1 and "dpi" in _err()
    assert L.uphip_pdf_writer_add_page_g4(None, o, 4, 16, 4, 0) == -1 and _err()
    assert L.uphip_sink_tiff_g4(None, 0, 0) is None and "null pattern" in _err()
    assert L.uphip_sink_tiff_g4(b"out%d%d.tif", 0, 0) is None and _err()
    assert L.uphip_sink_tiff_g4(b"out%d.tif", 0, -1) is None and "dpi" in _err()
    assert L.uphip_sink_pdf_bilevel(None, None, 0) is None and "null path" in _err()
    assert L.uphip_sink_pdf_bilevel(str(tmp_path / "y.pdf").encode(), None, 5000) is None and "dpi" in _err()
    assert L.uphip_batch_encode_g4_async(None) == -1 and _err()
    assert L.uphip_batch_g4_sizes(None, None, 0) == -1 and _err()
    assert L.uphip_batch_g4_download_async(None, o, 64) == -1 and _err()


def test_pdf_sink_destroyed_unfinished_leaves_no_file(tmp_path):
    import os
    L = load_library()
    path = str(tmp_path / "doc.pdf")
    k = L.uphip_sink_pdf_bilevel(path.encode(), None, 0)
    assert k
    L.uphip_sink_destroy(k)
    assert not os.path.exists(path) and not os.path.exists(path + ".part")
    k = L.uphip_sink_pdf_bilevel(path.encode(), None, 0)
    assert L.uphip_sink_finish(k) == 0
    L.uphip_sink_destroy(k)
    assert os.path.exists(path)
