"""GPU tests of the lossless output branch: the device PNG encoder
(csrc/kernels_png.hip) against its host twin over the same core, the batch
encode and the runner's PNG / lossless-PDF sinks.  Every comparison is exact.
The host twin itself is checked against zlib, PIL and the project's PNG reader
by test_png_encode.py."""
import ctypes as C
import os

import numpy as np
import pytest

import png_cases as K
from helpers import page_array
from unpaper_hip import ctypes_abi as A
from unpaper_hip.hostimage import HostImage
from unpaper_hip.pipeline import (Batch, DeviceBuffer, Runner, png_encode, png_encode_host, pnm_read,
                                  sink_pdf_lossless, sink_png, sink_pnm, source_memory)

pytestmark = pytest.mark.gpu


def _upload(rows):
    rows = np.ascontiguousarray(rows, np.uint8)
    buf = DeviceBuffer(rows.nbytes)
    assert buf.lib.uphip_memcpy_htod(buf.ptr, rows.ctypes.data, rows.nbytes) == 0
    return buf


@pytest.mark.parametrize("case", K.CASES, ids=K.CASE_IDS)
def test_device_encoder_equals_host(hip, case):
    name, fmt, width, rows = case
    want = png_encode_host(rows, width, fmt, dpi=200)
    buf = _upload(rows)
    try:
        assert png_encode(buf.ptr, rows.shape[1], width, rows.shape[0], fmt, dpi=200) == want
    finally:
        buf.close()


@pytest.mark.parametrize("name", K.EMBED_IDS)
def test_device_encoder_pitch_and_offset(hip, name):
    """The image inside rows of an odd pitch with garbage around it: byte
    formats 3 bytes into the buffer (rows start at every alignment of a
    dword), bilevel ones 5 bits into a row."""
    _, fmt, width, rows = K.CASES[K.CASE_IDS.index(name)]
    want = png_encode_host(K.tight(fmt, width, rows), width, fmt)
    big, byte_off, bit_off = K.embed(fmt, width, rows)
    buf = _upload(big)
    try:
        got = png_encode(buf.ptr + byte_off, big.shape[1], width, rows.shape[0], fmt, offset=bit_off)
        assert got == want
    finally:
        buf.close()


def test_device_encoder_argument_errors(hip):
    L = hip.lib
    buf = DeviceBuffer(1 << 17)
    try:
        # a row too wide for the block's LDS is refused before any launch
        assert L.uphip_png_encode(buf.ptr, 100000, 0, 100000, 1, A.FMT_GRAY8, 0, None, 0) == -1
        assert b"k_png_filter" in L.uphip_last_error()
        L.uphip_clear_error()
        for args in ((None, 16, 0, 16, 4, A.FMT_GRAY8), (buf.ptr, 16, 0, 0, 4, A.FMT_GRAY8),
                     (buf.ptr, 16, 0, 16, 0, A.FMT_GRAY8), (buf.ptr, 16, 0, 16, 4, 12),
                     (buf.ptr, 16, 2, 8, 4, A.FMT_GRAY8), (buf.ptr, 2, 1, 16, 4, A.FMT_MONOWHITE),
                     (buf.ptr, 2, -1, 16, 4, A.FMT_MONOBLACK)):
            assert L.uphip_png_encode(*args, 0, None, 0) == -1, args
            assert L.uphip_last_error()
            L.uphip_clear_error()
    finally:
        buf.close()


def _pages(n, w, h, seed, fmt):
    return [HostImage.from_array(page_array(w, h, seed + i, specks=30, color=fmt == A.FMT_RGB24), fmt)
            for i in range(n)]


def _plain_options(oracle, output_count, out_fmt):
    """The pages as they are (thresholded for MONOWHITE output)."""
    opts = oracle.default_options()
    opts.disable = A.NO_PROCESSING
    if out_fmt == A.FMT_MONOWHITE:
        opts.output_pixel_format = A.FMT_MONOWHITE
    if output_count == 2:
        opts.layout = A.LAYOUT_DOUBLE
        opts.output_count = 2
    return opts


def _page_stream(sheet, fmt, pw, j):
    """The host twin's stream for page j (pw wide) of a downloaded sheet."""
    if fmt in K.MONO:
        return K.idat(png_encode_host(sheet.data, pw, fmt, offset=j * pw))
    bpp = K.CHANNELS[fmt]
    return K.idat(png_encode_host(sheet.data[:, j * pw * bpp:], pw, fmt))


@pytest.mark.parametrize("out_fmt", [A.FMT_GRAY8, A.FMT_RGB24, A.FMT_MONOWHITE], ids=["gray", "rgb", "mono"])
@pytest.mark.parametrize("output_count", [1, 2])
def test_batch_encode_equals_host(hip, oracle, output_count, out_fmt):
    """Four 130 x 96 sheets (pages 65 wide in the double layout: a bilevel
    page 1 starts inside a byte).  Sheet 2 is overwritten with random bytes on
    the device after the run, so its GRAY8 and RGB24 pages leave as stored
    blocks.  Every
    stream equals the host twin on the sheet's own pixels."""
    w, h, n = 130, 96, 4
    pw = w // output_count
    in_fmt = A.FMT_RGB24 if out_fmt == A.FMT_RGB24 else A.FMT_GRAY8
    b = Batch(_plain_options(oracle, output_count, out_fmt), n, w, h, in_fmt)
    try:
        assert (b.out_width, b.out_height, b.out_format) == (w, h, out_fmt)
        for s, p in enumerate(_pages(n, w, h, 40, in_fmt)):
            b.set_input(s, 0, p)
        b.run(n)
        b.wait()
        before = C.c_int64()
        assert b.lib.uphip_batch_device_bytes(b.handle, C.byref(before)) == 0
        ptr, pitch = b.output_ptr(2)
        noise = np.random.default_rng(8).integers(0, 256, (h, pitch), dtype=np.uint8)
        assert b.lib.uphip_memcpy_htod(ptr, noise.ctypes.data, noise.nbytes) == 0
        b.encode_png()
        streams = b.png_files(n * output_count)
        after = C.c_int64()
        assert b.lib.uphip_batch_device_bytes(b.handle, C.byref(after)) == 0
        # the encode buffers are counted: at least the filtered bytes and the streams' bound
        assert after.value - before.value >= 2 * n * output_count * (K.row_bytes(out_fmt, pw) + 1) * h
        sheets = [b.output(s) for s in range(n)]
        rb = K.row_bytes(out_fmt, w)
        assert np.array_equal(sheets[2].data[:, :rb], noise[:, :rb])
        for i, z in enumerate(streams):
            s, j = divmod(i, output_count)
            assert z == _page_stream(sheets[s], out_fmt, pw, j), "page %d" % i
            if out_fmt not in K.MONO:  # (noise in bilevel rows still has its filter bytes and pad bits)
                assert K.is_stored(z) == (s == 2), "page %d" % i
            assert len(z) <= K.stored_bound(out_fmt, pw, h)
        assert len(set(streams)) == len(streams)
        # a second encode on the same buffers gives the same streams
        b.encode_png()
        assert b.png_files(n * output_count) == streams
    finally:
        b.close()


def _run(opts, pages, w, h, sink, fmt=A.FMT_GRAY8):
    host_in = np.stack([p.payload() for p in pages])
    r = Runner(opts, 2, w, h, fmt, devices=(0,), streams=2, host_threads=2)
    try:
        src = source_memory(host_in.ctypes.data, host_in.shape[2], host_in.shape[1] * host_in.shape[2],
                            len(pages), keep=host_in)
        return r.run_host(len(pages), src, sink)
    finally:
        r.close()


@pytest.mark.parametrize("output_count,out_fmt", [(1, A.FMT_GRAY8), (2, A.FMT_GRAY8), (2, A.FMT_MONOWHITE),
                                                  (1, A.FMT_RGB24)],
                         ids=["gray1", "gray2", "mono2", "rgb1"])
def test_runner_png_sinks_equal_pnm(hip, oracle, tmp_path, output_count, out_fmt):
    """Five jobs (three chunks of two sheets on two streams) through sink_pnm,
    sink_png and sink_pdf_lossless: the PNG files decode in PIL, and the PDF's
    pages in the project's reader, to exactly the PNM pages, in order."""
    from PIL import Image
    from unpaper_hip.pdf import PdfDocument
    w, h, n = 203, 131, 5
    pw = w // output_count
    in_fmt = A.FMT_RGB24 if out_fmt == A.FMT_RGB24 else A.FMT_GRAY8
    opts = _plain_options(oracle, output_count, out_fmt)
    pages = _pages(n, w, h, 60, in_fmt)
    failed, err = _run(opts, pages, w, h, sink_pnm(str(tmp_path / "p%03d.pnm")), in_fmt)
    assert failed == 0, err
    failed, err = _run(opts, pages, w, h, sink_png(str(tmp_path / "q%03d.png"), dpi=150), in_fmt)
    assert failed == 0, err
    pdf_sink = sink_pdf_lossless(str(tmp_path / "doc.pdf"), dpi=150)
    failed, err = _run(opts, pages, w, h, pdf_sink, in_fmt)
    assert failed == 0, err
    pdf_sink.finish()
    d = PdfDocument.open(str(tmp_path / "doc.pdf"))
    try:
        assert d.page_count == n * output_count
        seen = set()
        for i in range(n * output_count):
            pnm = pnm_read(str(tmp_path / ("p%03d.pnm" % i)))
            assert (pnm.width, pnm.height, pnm.format) == (pw, h, out_fmt)
            want = pnm.to_rgb()
            seen.add(want.tobytes())
            page = d.read_page(i)
            assert (page.width, page.height) == (pw, h)
            assert page.format == (A.FMT_MONOBLACK if out_fmt == A.FMT_MONOWHITE else out_fmt)
            assert np.array_equal(page.to_rgb(), want), "PDF page %d" % i
            pt_w, pt_h, _ = d.page_info(i)
            assert abs(pt_w - pw * 72.0 / 150) < 0.01 and abs(pt_h - h * 72.0 / 150) < 0.01
            path = str(tmp_path / ("q%03d.png" % i))
            with Image.open(path) as im:
                assert im.size == (pw, h)
                assert im.mode == {A.FMT_GRAY8: "L", A.FMT_RGB24: "RGB", A.FMT_MONOWHITE: "1"}[out_fmt]
                assert abs(im.info["dpi"][0] - 150) < 0.05
                assert np.array_equal(np.array(im.convert("RGB")), want), "PNG page %d" % i
            # the file is the host twin's for the page's pixels
            with open(path, "rb") as f:
                assert f.read() == png_encode_host(pnm.data, pw, out_fmt, dpi=150), "PNG file %d" % i
        assert len(seen) == n * output_count  # every page differs: the order check means something
    finally:
        d.close()


def test_runner_pdf_lossless_refuses_alpha(hip, oracle, tmp_path):
    w, h = 203, 131
    opts = oracle.default_options()
    opts.disable = A.NO_PROCESSING
    opts.output_pixel_format = A.FMT_Y400A
    pages = _pages(2, w, h, 60, A.FMT_GRAY8)
    sink = sink_pdf_lossless(str(tmp_path / "doc.pdf"))
    failed, err = _run(opts, pages, w, h, sink)
    assert failed != 0 and "output_pixel_format" in err
    sink.close()
    assert os.listdir(str(tmp_path)) == []
