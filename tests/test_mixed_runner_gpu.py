"""The runner in the fixed-sheet mode (options.sheet_size fully set, no
pre_rotate): its geometry is the largest page of the source
(uphip_source_max_geometry), every page of that format and at most that size
is admitted and centred in the sheet, a larger one fails its own job.  The
expected sheets are the oracle's process_sheet on the pages as PIL, or the
project's host readers, decode them."""
import io
import os

import numpy as np
import pytest

import mixed_cases as M
from helpers import assert_same
from unpaper_hip import ctypes_abi as A
from unpaper_hip.hostimage import HostImage
from unpaper_hip.pipeline import (Runner, TiffDocument, pnm_read, pnm_write, sink_pdf_lossless, sink_pnm,
                                  sink_tiff_multipage, source_max_geometry, source_pdf, source_pnm, source_tiff)

pytestmark = pytest.mark.gpu

SIZES3 = [(601, 850), (653, 800), (620, 877)]


def _pil(page):
    from PIL import Image
    return Image.fromarray(page.payload())


def _write_pgms(tmp_path, pages, stem="p"):
    paths = []
    for i, p in enumerate(pages):
        paths.append(str(tmp_path / ("%s%02d.pgm" % (stem, i))))
        pnm_write(paths[-1], p)
    return paths


def _run(opts, src, n, sink, geometry=None, sheets=4):
    gw, gh, fmt = geometry or source_max_geometry(src)
    r = Runner(opts, sheets, gw, gh, fmt, devices=(0,), streams=2, host_threads=3)
    try:
        failed, err = r.run_host(n, src, sink)
        return failed, err, r.stats().jobs_done
    finally:
        r.close()


def _expect(oracle, opts, page, key):
    exp, _ = M.expected(oracle, opts, [page], key)
    assert (exp.width, exp.height) == M.SHEET
    return exp


def test_path_list_of_many_sizes_and_codecs(hip, oracle, tmp_path):
    opts = M.sheet_options(oracle, M.SHEET)
    pages = M.pages_of(M.LIST1)
    paths = _write_pgms(tmp_path, pages)
    png, jpg = str(tmp_path / "x.png"), str(tmp_path / "y.jpg")
    _pil(pages[2]).save(png)                      # 601 x 850
    _pil(pages[9]).save(jpg, quality=90)          # 587 x 877: no multiple of 8 either way, baseline
    paths += [png, jpg]
    src = source_pnm(paths)
    assert source_max_geometry(src) == (700, 911, A.FMT_GRAY8)
    failed, err, done = _run(opts, src, len(paths), sink_pnm(str(tmp_path / "o%02d.pgm")))
    assert failed == 0 and done == len(paths), err
    from PIL import Image
    with Image.open(jpg) as im:
        assert im.size == (587, 877) and im.mode == "L"
        decoded = HostImage.from_array(np.asarray(im), A.FMT_GRAY8)
    want = [_expect(oracle, opts, p, ("list1", A.FMT_GRAY8, i)) for i, p in enumerate(pages)]
    want += [want[2], _expect(oracle, opts, decoded, ("runner jpeg",))]
    for i, exp in enumerate(want):
        assert_same(pnm_read(str(tmp_path / ("o%02d.pgm" % i))), exp, "job %d (%s)" % (i, os.path.basename(paths[i])))


def _mixed_tiff(path, pages):
    """One file, LZW and PackBits pages in turn."""
    from PIL import TiffImagePlugin
    with TiffImagePlugin.AppendingTiffWriter(path, True) as tf:
        for i, p in enumerate(pages):
            _pil(p).save(tf, format="TIFF", compression=("tiff_lzw", "packbits")[i % 2])
            tf.newFrame()


@pytest.mark.parametrize("flags", [A.TIFF_HOST_DECODE, A.TIFF_DEVICE_DECODE])
def test_multipage_tiff_to_multipage_tiff(hip, oracle, tmp_path, flags):
    opts = M.sheet_options(oracle, M.SHEET)
    pages = M.pages_of(SIZES3 + SIZES3, seed0=2)   # page 0 is list 1's page 2
    path, out = str(tmp_path / "in.tif"), str(tmp_path / "out.tif")
    _mixed_tiff(path, pages)
    src = source_tiff(path, flags)
    assert source_max_geometry(src) == (653, 877, A.FMT_GRAY8)
    sink = sink_tiff_multipage(out)
    failed, err, done = _run(opts, src, len(pages), sink)
    assert failed == 0 and done == len(pages), err
    sink.finish()
    d = TiffDocument(out)
    try:
        assert d.page_count == len(pages)
        for i, p in enumerate(pages):
            exp = _expect(oracle, opts, p, ("list1", A.FMT_GRAY8, 2) if i == 0 else ("runner tiff", i))
            assert_same(d.read_page(i), exp, "page %d" % i)
    finally:
        d.close()


def test_multipage_pdf_to_lossless_pdf(hip, oracle, tmp_path):
    from PIL import Image
    from unpaper_hip.pdf import PdfDocument
    opts = M.sheet_options(oracle, M.SHEET)
    ims = [_pil(p) for p in M.pages_of(SIZES3, seed0=2)]
    path, out = str(tmp_path / "in.pdf"), str(tmp_path / "out.pdf")
    ims[0].save(path, format="PDF", save_all=True, append_images=ims[1:])
    src = source_pdf(path)
    assert source_max_geometry(src) == (653, 877, A.FMT_GRAY8)
    sink = sink_pdf_lossless(out)
    failed, err, done = _run(opts, src, len(ims), sink)
    assert failed == 0 and done == len(ims), err
    sink.finish()
    din, dout = PdfDocument.open(path), PdfDocument.open(out)
    try:
        assert dout.page_count == len(ims)
        for i in range(len(ims)):
            with Image.open(io.BytesIO(din.extract_page_image(i).data)) as im:   # PIL wrote JPEG pages
                assert im.size == SIZES3[i]
                page = HostImage.from_array(np.asarray(im), A.FMT_GRAY8)
            exp = _expect(oracle, opts, page, ("runner pdf", i))
            assert_same(dout.read_page(i), exp, "page %d" % i)
    finally:
        din.close()
        dout.close()


LIST_OVER = [(601, 850), (653, 800), (700, 911), (620, 877)]


def test_a_page_above_the_maximum_fails_alone(hip, oracle, tmp_path):
    opts = M.sheet_options(oracle, M.SHEET)
    pages = M.pages_of(LIST_OVER, seed0=2)
    src = source_pnm(_write_pgms(tmp_path, pages))
    failed, err, done = _run(opts, src, 4, sink_pnm(str(tmp_path / "o%02d.pgm")), geometry=(653, 877, A.FMT_GRAY8))
    assert failed == 1 and done == 3
    assert "could not be loaded" in err and "p02.pgm" in err and "700x911" in err and "653x877" in err
    assert not os.path.exists(str(tmp_path / "o02.pgm"))
    for i in (0, 1, 3):
        exp = _expect(oracle, opts, pages[i], ("list1", A.FMT_GRAY8, 2) if i == 0 else ("runner over", i))
        assert_same(pnm_read(str(tmp_path / ("o%02d.pgm" % i))), exp, "job %d" % i)


def test_without_sheet_size_other_sizes_fail_as_before(hip, oracle, tmp_path):
    opts = oracle.default_options()
    pages = M.pages_of(LIST_OVER, seed0=2)
    src = source_pnm(_write_pgms(tmp_path, pages))
    failed, err, done = _run(opts, src, 4, sink_pnm(str(tmp_path / "o%02d.pgm")), geometry=(601, 850, A.FMT_GRAY8))
    assert failed == 3 and done == 1
    assert "could not be loaded" in err and "sheet_size" in err
    exp, _ = M.expected(oracle, opts, [pages[0]], ("runner unset", 0))
    assert_same(pnm_read(str(tmp_path / "o00.pgm")), exp, "job 0")
    assert not any(os.path.exists(str(tmp_path / ("o%02d.pgm" % i))) for i in (1, 2, 3))
