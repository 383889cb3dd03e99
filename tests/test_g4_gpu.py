"""GPU tests of the bilevel output branch: the device CCITT Group 4 encoder
(csrc/kernels_g4.hip) against the host encoder over the same row coder, the
batch encode and the runner's TIFF / PDF sinks.  Every comparison is exact.
The host encoder itself is pinned to libtiff's bytes by test_g4.py."""
import numpy as np
import pytest

import g4_cases
from helpers import page_array
from unpaper_hip import ctypes_abi as A
from unpaper_hip.hostimage import HostImage
from unpaper_hip.pipeline import (Batch, DeviceBuffer, Runner, g4_encode, g4_encode_host, pnm_read,
                                  sink_pdf_bilevel, sink_pnm, sink_tiff_g4, source_memory)

pytestmark = pytest.mark.gpu


def _upload(rows):
    rows = np.ascontiguousarray(rows, np.uint8)
    buf = DeviceBuffer(rows.nbytes)
    assert buf.lib.uphip_memcpy_htod(buf.ptr, rows.ctypes.data, rows.nbytes) == 0
    return buf


@pytest.mark.parametrize("name", g4_cases.NAMES)
def test_device_encoder_equals_host(hip, name):
    """Every fixture from a device buffer: packed rows as they are, then 5
    bits into rows of a larger, odd pitch whose other bits are garbage (rows
    start at every alignment of a dword)."""
    bits, want = g4_cases.load(name)
    h, w = bits.shape
    packed = g4_cases.pack(bits)
    assert g4_encode_host(packed, w) == want
    buf = _upload(packed)
    try:
        assert g4_encode(buf.ptr, packed.shape[1], w, h) == want, "packed rows"
    finally:
        buf.close()
    off = 5
    pitch = ((off + w + 7) // 8 + 6) | 1
    wide = (g4_cases.noise(h, pitch * 8, 500000, 99)).astype(np.uint8)
    wide[:, off:off + w] = bits
    rows = np.packbits(wide, axis=1)
    assert g4_encode_host(rows, w, bit_offset=off) == want
    buf = _upload(rows)
    try:
        assert g4_encode(buf.ptr, pitch, w, h, bit_offset=off) == want, "pitch %d, bit offset %d" % (pitch, off)
    finally:
        buf.close()


def test_device_encoder_wide_rows(hip):
    """9000-pixel rows: 64 rows and their reference no longer fit the block's
    LDS, so a block takes fewer (56) and the 70 rows span two blocks whose
    edge is not at row 64."""
    h, w = 70, 9000
    bits = g4_cases.noise(h, w, 1000, 77)
    bits[20:60, 4000:4400] = 1
    packed = g4_cases.pack(bits)
    want = g4_encode_host(packed, w)
    buf = _upload(packed)
    try:
        assert g4_encode(buf.ptr, packed.shape[1], w, h) == want
    finally:
        buf.close()


def test_device_encoder_argument_errors(hip):
    L = hip.lib
    buf = DeviceBuffer(64)
    try:
        # a row too wide for the block's LDS is refused before any launch
        assert L.uphip_g4_encode(buf.ptr, 1 << 17, 0, 1 << 20, 1, None, 0) == -1
        assert b"k_g4_rows" in L.uphip_last_error()
        L.uphip_clear_error()
        for args in ((None, 2, 0, 16, 4), (buf.ptr, 2, 0, 0, 4), (buf.ptr, 2, 0, 16, 0),
                     (buf.ptr, 2, 1, 16, 4), (buf.ptr, 2, -1, 16, 4)):
            assert L.uphip_g4_encode(*args, None, 0) == -1
            assert L.uphip_last_error()
            L.uphip_clear_error()
    finally:
        buf.close()


def _gray_pages(n, w, h, seed):
    return [HostImage.from_array(page_array(w, h, seed + i, specks=30), A.FMT_GRAY8) for i in range(n)]


def _plain_options(oracle, output_count):
    """The pages as they are, thresholded to MONOWHITE: what the sheets hold
    is then known to be neither empty nor full."""
    opts = oracle.default_options()
    opts.disable = A.NO_PROCESSING
    opts.output_pixel_format = A.FMT_MONOWHITE
    if output_count == 2:
        opts.layout = A.LAYOUT_DOUBLE
        opts.output_count = 2
    return opts


@pytest.mark.parametrize("output_count", [1, 2])
def test_batch_encode_equals_host(hip, oracle, output_count):
    """Four 96 x 130 sheets (pages 65 wide in the double layout: page 1 of a
    sheet starts inside a byte).  Sheet 2 is overwritten with a checkerboard
    on the device after the run: three bits a pixel is more than a page's
    share of the encode buffer, so its pages come back -1 and are re-encoded
    alone.  Every stream equals the host encoder on the sheet's own bits."""
    w, h, n = 130, 96, 4
    pw = w // output_count
    opts = _plain_options(oracle, output_count)
    b = Batch(opts, n, w, h, A.FMT_GRAY8)
    try:
        assert (b.out_width, b.out_height, b.out_format) == (w, h, A.FMT_MONOWHITE)
        for s, p in enumerate(_gray_pages(n, w, h, 40)):
            b.set_input(s, 0, p)
        b.run(n)
        b.wait()
        ptr, pitch = b.output_ptr(2)
        board = np.zeros((h, pitch), np.uint8)
        board[:, :(w + 7) // 8] = g4_cases.pack(g4_cases.checker(h, w))
        assert b.lib.uphip_memcpy_htod(ptr, board.ctypes.data, board.nbytes) == 0
        b.encode_g4()
        files = b.g4_files(n * output_count)
        sheets = [b.output(s) for s in range(n)]
        assert np.array_equal(sheets[2].payload(), board[:, :(w + 7) // 8])
        for s in (0, 1, 3):
            px = np.unpackbits(sheets[s].payload(), axis=1)[:, :w]
            assert 0 < px.sum() < px.size, "sheet %d is blank" % s
        for i, f in enumerate(files):
            s, j = divmod(i, output_count)
            want = g4_encode_host(sheets[s].data, pw, bit_offset=j * pw)
            if s == 2:
                assert f is None, "page %d fits its share" % i
                ptr, pitch = b.output_ptr(s)
                f = g4_encode(ptr, pitch, pw, h, bit_offset=j * pw)
            assert f == want, "page %d" % i
        # a second encode on the same buffers gives the same streams
        b.encode_g4()
        assert b.g4_files(n * output_count) == files
    finally:
        b.close()


def test_batch_encode_needs_bilevel_output(hip, oracle):
    opts = oracle.default_options()
    opts.disable = A.NO_PROCESSING
    b = Batch(opts, 1, 130, 96, A.FMT_GRAY8)
    try:
        b.set_input(0, 0, _gray_pages(1, 130, 96, 7)[0])
        b.run(1)
        b.wait()
        with pytest.raises(Exception, match="MONOWHITE"):
            b.encode_g4()
    finally:
        b.close()


def _runner_jobs(w, h, n):
    """n GRAY8 pages; page 1 a checkerboard (its Group 4 stream is larger than
    a page's share, the runner re-encodes it alone)."""
    pages = _gray_pages(n, w, h, 60)
    board = np.where(g4_cases.checker(h, w), 0, 255).astype(np.uint8)
    pages[1] = HostImage.from_array(board, A.FMT_GRAY8)
    return pages


def _run(opts, pages, w, h, sink):
    host_in = np.stack([p.payload() for p in pages])
    r = Runner(opts, 2, w, h, A.FMT_GRAY8, devices=(0,), streams=2, host_threads=2)
    try:
        src = source_memory(host_in.ctypes.data, w, w * h, len(pages), keep=host_in)
        return r.run_host(len(pages), src, sink)
    finally:
        r.close()


@pytest.mark.parametrize("output_count", [1, 2])
def test_runner_g4_sinks_equal_pnm(hip, oracle, tmp_path, output_count):
    """Five jobs (three chunks of two sheets on two streams) through sink_pnm,
    sink_tiff_g4 and sink_pdf_bilevel: the TIFF files decode in PIL, and the
    PDF's pages in the project's reader, to exactly the PBM pages, in order."""
    from PIL import Image, features
    from unpaper_hip.pdf import PdfDocument
    w, h, n = 203, 131, 5
    pw = w // output_count
    opts = _plain_options(oracle, output_count)
    pages = _runner_jobs(w, h, n)
    failed, err = _run(opts, pages, w, h, sink_pnm(str(tmp_path / "p%03d.pbm")))
    assert failed == 0, err
    failed, err = _run(opts, pages, w, h, sink_tiff_g4(str(tmp_path / "t%03d.tif"), dpi=150))
    assert failed == 0, err
    pdf_sink = sink_pdf_bilevel(str(tmp_path / "doc.pdf"), dpi=150)
    failed, err = _run(opts, pages, w, h, pdf_sink)
    assert failed == 0, err
    pdf_sink.finish()
    d = PdfDocument.open(str(tmp_path / "doc.pdf"))
    try:
        assert d.page_count == n * output_count
        seen = set()
        for i in range(n * output_count):
            pbm = pnm_read(str(tmp_path / ("p%03d.pbm" % i)))
            assert (pbm.width, pbm.height, pbm.format) == (pw, h, A.FMT_MONOWHITE)
            gray = pbm.to_gray()
            seen.add(gray.tobytes())
            page = d.read_page(i)
            assert (page.width, page.height, page.format) == (pw, h, A.FMT_GRAY8)
            assert np.array_equal(page.payload(), gray), "PDF page %d" % i
            pt_w, pt_h, _ = d.page_info(i)
            assert abs(pt_w - pw * 72.0 / 150) < 0.01 and abs(pt_h - h * 72.0 / 150) < 0.01
            if features.check("libtiff"):
                with Image.open(str(tmp_path / ("t%03d.tif" % i))) as im:
                    assert im.size == (pw, h) and im.tag_v2[259] == 4 and float(im.tag_v2[282]) == 150.0
                    assert np.array_equal(np.array(im.convert("L")), gray), "TIFF page %d" % i
            # the stream in the file is the host encoder's for the page's bits
            with open(str(tmp_path / ("t%03d.tif" % i)), "rb") as f:
                assert f.read()[198:] == g4_encode_host(pbm.data, pw), "TIFF strip %d" % i
        assert len(seen) == n * output_count  # every page differs: the order check means something
    finally:
        d.close()


def test_runner_g4_sink_refuses_gray_output(hip, oracle, tmp_path):
    import os
    w, h = 203, 131
    opts = oracle.default_options()
    opts.disable = A.NO_PROCESSING
    pages = _gray_pages(2, w, h, 60)
    failed, err = _run(opts, pages, w, h, sink_tiff_g4(str(tmp_path / "t%03d.tif")))
    assert failed != 0 and "output_pixel_format" in err
    assert os.listdir(str(tmp_path)) == []
    failed, err = _run(opts, pages, w, h, sink_pdf_bilevel(str(tmp_path / "doc.pdf")))
    assert failed != 0 and "output_pixel_format" in err
