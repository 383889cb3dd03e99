"""The fixed-sheet mode of the batch (options.sheet_size fully set): pages of
any size up to the batch geometry's, a size per input slot
(uphip_batch_set_page_size), every page centred in its sheet as the
reference's sheet_stage_decode does with center_image (cropped where larger).
Byte for byte against the oracle's process_sheet on the saved frame, as
test_pipeline_gpu.py::check; uphip_batch_decode_route tells which decode ran:
0 fill + k_copy, 1 k_decode_gray, 2 k_decode_gray_fit.
test_mixed_sizes.py shows that none of these sheets is a no-op."""
import numpy as np
import pytest

import mixed_cases as M
from helpers import assert_same, make_image
from unpaper_hip import ctypes_abi as A
from unpaper_hip.device import UnpaperHipError
from unpaper_hip.pipeline import Batch, DeviceBuffer

pytestmark = pytest.mark.gpu


def run_batch(opts, geometry, fmt, sheets):
    """sheets: one page list per sheet, pages of any size within `geometry`.
    Returns (outputs, reports, route)."""
    b = Batch(opts, len(sheets), geometry[0], geometry[1], fmt)
    try:
        for s, pages in enumerate(sheets):
            for j, p in enumerate(pages):
                b.set_input(s, j, p)
        b.run(len(sheets))
        b.wait()
        return ([b.output(s) for s in range(len(sheets))], [b.report(s) for s in range(len(sheets))],
                b.decode_route())
    finally:
        b.close()


def check_list(oracle, name, sheet, sizes, route, fmt=A.FMT_GRAY8):
    opts = M.sheet_options(oracle, sheet)
    pages = M.pages_of(sizes, fmt)
    outs, reps, got = run_batch(opts, M.max_size(sizes), fmt, [[p] for p in pages])
    assert got == route
    for i, p in enumerate(pages):
        exp, erep = M.expected(oracle, opts, [p], (name, fmt, i))
        assert (exp.width, exp.height) == sheet
        assert_same(outs[i], exp, "%s page %d %dx%d" % ((name, i) + sizes[i]))
        M.assert_report(reps[i], erep)


def test_fit_route_every_placement_class(hip, oracle):
    assert M.max_size(M.LIST1) == (700, 911)
    check_list(oracle, "list1", M.SHEET, M.LIST1, 2)


def test_fit_route_every_byte_offset(hip, oracle):
    """tx = 16..0, then sx = 1..16: every shift of the source bytes against
    the sheet's words, and both edges of the row's last word."""
    check_list(oracle, "offsets", M.SHEET_OFFSETS, M.LIST_OFFSETS, 2)


def test_fit_route_last_word_of_29(hip, oracle):
    check_list(oracle, "tail", M.SHEET_TAIL, M.LIST_TAIL, 2)


def test_uniform_pages_in_a_sheet_of_another_size(hip, oracle):
    """No set_page_size call: the plan's own placement, now on the fit route."""
    opts = M.sheet_options(oracle, M.SHEET)
    pages = [make_image(601, 850, A.FMT_GRAY8, seed=2), make_image(601, 850, A.FMT_GRAY8, seed=40)]
    outs, reps, route = run_batch(opts, (601, 850), A.FMT_GRAY8, [[p] for p in pages])
    assert route == 2
    for i, p in enumerate(pages):
        # seed 2 at 601 x 850 is list 1's page 2
        exp, erep = M.expected(oracle, opts, [p], ("list1", A.FMT_GRAY8, 2) if i == 0 else ("uniform", i))
        assert_same(outs[i], exp, "uniform page %d" % i)
        M.assert_report(reps[i], erep)


@pytest.mark.parametrize("fmt", [A.FMT_RGB24, A.FMT_Y400A, A.FMT_MONOWHITE, A.FMT_MONOBLACK])
def test_copy_route_other_formats(hip, oracle, fmt):
    check_list(oracle, "formats", M.SHEET, M.LIST_FORMATS, 0, fmt)


def test_two_inputs_a_sheet(hip, oracle):
    opts = M.sheet_options(oracle, M.SHEET_DOUBLE, input_count=2, layout=A.LAYOUT_DOUBLE)
    sheets = [M.pages_of(pair, seed0=10 * i) for i, pair in enumerate(M.LIST_DOUBLE)]
    geometry = M.max_size([s for pair in M.LIST_DOUBLE for s in pair])
    outs, reps, route = run_batch(opts, geometry, A.FMT_GRAY8, sheets)
    assert route == 0
    for i, pages in enumerate(sheets):
        exp, erep = M.expected(oracle, opts, pages, ("double", i))
        assert_same(outs[i], exp, "double sheet %d" % i)
        M.assert_report(reps[i], erep)


@pytest.mark.parametrize("pitch,route", [(768, 2), (700 + 3, 0)])
def test_run_device(hip, oracle, pitch, route):
    """The pages in a device buffer of the caller's: rows 16-byte aligned take
    the fit decode, any other pitch the copy."""
    opts = M.sheet_options(oracle, M.SHEET)
    pages = M.pages_of(M.LIST1)
    gw, gh = M.max_size(M.LIST1)
    n, stride = len(pages), pitch * gh
    host = np.full((n, gh, pitch), 0x55, np.uint8)   # not the background: a stray read shows
    for i, p in enumerate(pages):
        host[i, :p.height, :p.width] = p.payload()
    buf = DeviceBuffer(host.nbytes + 64)
    b = Batch(opts, n, gw, gh, A.FMT_GRAY8)
    try:
        assert buf.lib.uphip_memcpy_htod(buf.ptr, host.ctypes.data, host.nbytes) == 0
        for i, p in enumerate(pages):
            b.set_page_size(i, 0, p.width, p.height)
        b.run_device(n, buf.ptr, pitch, stride)
        b.wait()
        assert b.decode_route() == route
        for i, p in enumerate(pages):
            exp, erep = M.expected(oracle, opts, [p], ("list1", A.FMT_GRAY8, i))
            assert_same(b.output(i), exp, "pitch %d page %d" % (pitch, i))
            M.assert_report(b.report(i), erep)
    finally:
        b.close()
        buf.close()


def test_sizes_hold_until_changed(hip, oracle):
    opts = M.sheet_options(oracle, M.SHEET)
    sizes = M.LIST1
    gw, gh = M.max_size(sizes)
    small = M.pages_of(sizes)
    full = [make_image(gw, gh, A.FMT_GRAY8, seed=70 + i) for i in range(len(sizes))]
    fresh, _, route = run_batch(opts, (gw, gh), A.FMT_GRAY8, [[p] for p in full])
    assert route == 2   # 700 x 911 pages cropped into 620 x 877
    b = Batch(opts, len(sizes), gw, gh, A.FMT_GRAY8)
    try:
        def run():
            b.run(len(sizes))
            b.wait()
            return [b.output(s) for s in range(len(sizes))]
        for s, p in enumerate(small):
            b.set_input(s, 0, p)
        first = run()
        for s, p in enumerate(small):
            exp, _ = M.expected(oracle, opts, [p], ("list1", A.FMT_GRAY8, s))
            assert_same(first[s], exp, "sized sheet %d" % s)
        # back to the geometry's size: as a batch that was never sized
        for s, p in enumerate(full):
            b.set_page_size(s, 0, 0, 0)
            b.set_input(s, 0, p)
        again = run()
        for s in range(len(sizes)):
            assert_same(again[s], fresh[s], "reset sheet %d" % s)
        # one slot's size alone: only its sheet changes
        b.set_page_size(3, 0, 333, 250)
        third = run()
        exp3, _ = M.expected(oracle, opts, [_top_left(full[3], 333, 250)], ("crop", 3))
        for s in range(len(sizes)):
            assert_same(third[s], exp3 if s == 3 else fresh[s], "slot 3 resized, sheet %d" % s)
        assert not np.array_equal(third[3].payload(), fresh[3].payload())
    finally:
        b.close()


def _top_left(page, w, h):
    """The w x h page that a slot holding `page` is once its size is (w, h):
    rows at the slot's pitch from its origin."""
    from unpaper_hip.hostimage import HostImage
    return HostImage.from_array(page.payload()[:h, :w], page.format)


def test_set_page_size_errors(hip, oracle):
    def refused(opts, field, slot=0, w=100, h=100):
        b = Batch(opts, 2, 320, 200, A.FMT_GRAY8)
        try:
            with pytest.raises(UnpaperHipError, match=field):
                b.set_page_size(slot, 0, w, h)
        finally:
            b.close()
    refused(oracle.default_options(), "sheet_size")
    half = oracle.default_options()
    half.sheet_size = A.RectangleSize(320, -1)
    refused(half, "sheet_size")
    refused(M.sheet_options(oracle, (320, 200), pre_rotate=90), "pre_rotate")
    refused(M.sheet_options(oracle, (320, 200)), "width", w=321)
    refused(M.sheet_options(oracle, (320, 200)), "height", h=201)
    refused(M.sheet_options(oracle, (320, 200)), "slot", slot=2)
