"""CPU tests of the fixed-sheet mode: uphip_source_max_geometry (the geometry
of a runner that takes every page of a source), and that no sheet of the size
lists the GPU tests compare is a no-op: the cleanup changes each of them, so a
pipeline that did nothing after the decode would not pass them."""
import ctypes as C

import numpy as np
import pytest

import mixed_cases as M
from unpaper_hip import ctypes_abi as A
from unpaper_hip.device import UnpaperHipError
from unpaper_hip.pipeline import (pnm_write, source_callback, source_max_geometry, source_pdf, source_pnm,
                                  source_tiff)

SIZES = [(601, 850), (653, 800), (620, 877)]


def _pil_pages():
    from PIL import Image
    return [Image.fromarray(p.payload()) for p in M.pages_of(SIZES)]


def test_max_geometry_pnm_list(tmp_path):
    paths = []
    for i, p in enumerate(M.pages_of(SIZES)):
        paths.append(str(tmp_path / ("p%d.pgm" % i)))
        pnm_write(paths[-1], p)
    assert source_max_geometry(source_pnm(paths)) == (653, 877, A.FMT_GRAY8)


def test_max_geometry_tiff(tmp_path):
    im = _pil_pages()
    path = str(tmp_path / "doc.tif")
    im[0].save(path, format="TIFF", save_all=True, append_images=im[1:], compression="tiff_lzw")
    assert source_max_geometry(source_tiff(path)) == (653, 877, A.FMT_GRAY8)


def test_max_geometry_pdf(tmp_path):
    im = _pil_pages()
    path = str(tmp_path / "doc.pdf")
    im[0].save(path, format="PDF", save_all=True, append_images=im[1:])
    assert source_max_geometry(source_pdf(path)) == (653, 877, A.FMT_GRAY8)


def test_max_geometry_names_the_page_of_another_format(tmp_path):
    from helpers import make_image
    gray, rgb = str(tmp_path / "a.pgm"), str(tmp_path / "b.ppm")
    pnm_write(gray, make_image(40, 30, A.FMT_GRAY8))
    pnm_write(rgb, make_image(40, 30, A.FMT_RGB24))
    with pytest.raises(UnpaperHipError, match="b.ppm"):
        source_max_geometry(source_pnm([gray, rgb]))


def test_max_geometry_refuses_a_callback_source():
    src = source_callback(lambda job, page, dst, linesize: 1)
    with pytest.raises(UnpaperHipError, match="callback"):
        source_max_geometry(src)


def _sheets():
    for sheet, sizes in ((M.SHEET, M.LIST1), (M.SHEET_OFFSETS, M.LIST_OFFSETS), (M.SHEET_TAIL, M.LIST_TAIL)):
        for i, p in enumerate(M.pages_of(sizes)):
            yield sheet, 1, [p], "%dx%d page %d" % (sheet + (i,))
    for i, pair in enumerate(M.LIST_DOUBLE):
        yield M.SHEET_DOUBLE, 2, M.pages_of(pair, seed0=10 * i), "double %d" % i


def test_no_sheet_is_a_noop(oracle):
    """Every sheet of the batch-level lists differs from the same sheet with
    all the cleanup off (NO_PROCESSING)."""
    for sheet, n, pages, what in _sheets():
        fields = dict(input_count=n, layout=A.LAYOUT_DOUBLE) if n == 2 else {}
        on = M.sheet_options(oracle, sheet, **fields)
        off = M.copy_options(on)
        off.disable = A.NO_PROCESSING
        a, fa, _ = oracle.process_sheet(on, pages)
        b, fb, _ = oracle.process_sheet(off, pages)
        assert (a.width, a.height) == sheet and (b.width, b.height) == sheet, what
        assert not np.array_equal(a.payload(), b.payload()), what
