"""The batch with more than two mask-scan points against the oracle, as
test_multi_mask_gpu.assert_sheet compares: the saved frame byte for byte,
mask_count, every mask and every rotation's float bits against
mask_cases.expected, and the report's first two entries.  Every case on the
one-launch mask scan (k_mask_sums_points) and again on the looped route
(uphip_batch_set_mask_scan_route), the stage switches, the limits, the scan
kernel's corners, and the device memory of one- and two-point batches, which
this must not change."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import assert_same
from unpaper_hip import ctypes_abi as A
from unpaper_hip.device import UnpaperHipError
from unpaper_hip.pipeline import Batch
from test_multi_mask_gpu import assert_sheet, bits
import mask_batch_cases as BC
import mask_cases as MC
import mixed_cases as M

pytestmark = pytest.mark.gpu

ONE_LAUNCH, LOOPED = 0, 1


def run_sheets(b, c, order, fmt=A.FMT_GRAY8):
    for slot, s in enumerate(order):
        b.set_input(slot, 0, c.page(s, fmt))
    b.run(len(order))
    b.wait()
    return [(b.output(slot), b.report(slot), b.masks(slot)) for slot in range(len(order))]


@functools.lru_cache(maxsize=None)
def case_on(name, route, fmt=A.FMT_GRAY8, interp=A.INTERP_CUBIC):
    """The case's three sheets through one batch on `route`, run once."""
    c = MC.CASES[name]
    b = Batch(c.options(interp), MC.SHEETS, *c.size, fmt)
    try:
        b.set_mask_scan_route(route)
        return run_sheets(b, c, range(MC.SHEETS), fmt)
    finally:
        b.close()


def check_case(name, route, fmt=A.FMT_GRAY8, interp=A.INTERP_CUBIC):
    got, exp = case_on(name, route, fmt, interp), MC.expected(name, fmt, interp)
    for s in range(MC.SHEETS):
        assert_sheet(got[s], exp[s], "%s fmt %d interp %d route %d sheet %d" % (name, fmt, interp, route, s))
    return got


@pytest.mark.parametrize("name", list(MC.CASES))
def test_case_one_launch(hip, name):
    """GRAY8, cubic, three sheets in one batch (f-two-none's two points take
    the parent's launches whatever the route)."""
    check_case(name, ONE_LAUNCH)


@pytest.mark.parametrize("name", list(MC.CASES))
def test_case_looped(hip, name):
    """The looped route: the same expectations, and the frames of the
    one-launch route."""
    got = check_case(name, LOOPED)
    one = case_on(name, ONE_LAUNCH)
    for s in range(MC.SHEETS):
        assert_same(got[s][0], one[s][0], "%s sheet %d: the routes differ" % (name, s))
        assert [m.tuple() for m in got[s][2][1]] == [m.tuple() for m in one[s][2][1]]


@pytest.mark.parametrize("fmt", [A.FMT_RGB24, A.FMT_Y400A, A.FMT_MONOWHITE, A.FMT_MONOBLACK])
@pytest.mark.parametrize("name", MC.FORMAT_CASES)
def test_formats(hip, name, fmt):
    check_case(name, ONE_LAUNCH, fmt)


def test_rgb_looped(hip):
    """The generic (RGB24 plane) path of the scan kernel against its looped twin."""
    got = check_case("d-mixed6", LOOPED, A.FMT_RGB24)
    one = case_on("d-mixed6", ONE_LAUNCH, A.FMT_RGB24)
    for s in range(MC.SHEETS):
        assert_same(got[s][0], one[s][0], "sheet %d: the routes differ" % s)


@pytest.mark.parametrize("interp", MC.INTERPS)
@pytest.mark.parametrize("name", ["a-row3", "d-mixed6"])
def test_interpolations(hip, name, interp):
    """The general loop (each mask detected on the sheet as the masks before
    it left it) under every interpolation, the bilinear kernel of the linear
    plan included.  d-mixed6 depends on that order at all three
    interpolations, on sheets 0 and 1 (test_multi_mask_batch.py shows it on
    the CPU with test_multi_mask.rotated_from_undeskewed's method)."""
    check_case(name, ONE_LAUNCH, A.FMT_GRAY8, interp)


def test_reruns(hip):
    """One batch run on sheets (0, 1, 2), then on (2, 0): each run's answer
    is its own sheets'."""
    name = "d-mixed6"
    c, exp = MC.CASES[name], MC.expected(name)
    b = Batch(c.options(), MC.SHEETS, *c.size, A.FMT_GRAY8)
    try:
        for order in [(0, 1, 2), (2, 0)]:
            got = run_sheets(b, c, order)
            for slot, s in enumerate(order):
                assert_sheet(got[slot], exp[s], "%s order %r slot %d" % (name, order, slot))
    finally:
        b.close()


@pytest.mark.parametrize("flag", [A.NO_MASK_SCAN, A.NO_DESKEW, A.NO_MASK_CENTER])
def test_stage_switches(hip, oracle, flag):
    """Each stage switch alone on b-grid4, against the oracle's process_sheet
    with the same options: the saved frame and the report's two entries."""
    c = MC.CASES["b-grid4"]
    opts = c.options(disable=flag)
    b = Batch(opts, MC.SHEETS, *c.size, A.FMT_GRAY8)
    try:
        got = run_sheets(b, c, range(MC.SHEETS))
    finally:
        b.close()
    for s in range(MC.SHEETS):
        sheet, ofmt, erep = oracle.process_sheet(opts, [c.page(s)])
        out, rep, (count, masks, rots) = got[s]
        what = "b-grid4 disable 0x%x sheet %d" % (flag, s)
        assert_same(out, oracle.convert_for_save(sheet, ofmt), what)
        assert rep.mask_count == erep.mask_count == count, what
        assert rep.mask_count == (0 if flag == A.NO_MASK_SCAN else c.npoints), what
        for i in range(min(count, A.MAX_PAGES)):
            assert rep.masks[i].tuple() == erep.masks[i].tuple() == masks[i].tuple(), what
            assert bits(rep.rotation[i]) == bits(erep.rotation[i]) == bits(rots[i]), what


def test_limit_capacities(hip):
    """g-limit, UPHIP_MAX_POINTS points: get_masks with room for all, for
    seven and for none."""
    name = "g-limit"
    c, exp = MC.CASES[name], MC.expected(name)
    assert c.npoints == A.MAX_POINTS == 100
    b = Batch(c.options(), 1, *c.size, A.FMT_GRAY8)
    try:
        out, rep, (count, masks, rots) = run_sheets(b, c, (0,))[0]
        assert count == 100 and len(masks) == 100 and len(rots) == 100
        assert [m.tuple() for m in masks] == exp[0][3]
        n7, m7, r7 = b.masks(0, capacity=7)
        assert n7 == 100 and len(m7) == 7 and len(r7) == 7
        assert [m.tuple() for m in m7] == exp[0][3][:7]
        assert [bits(r) for r in r7] == [bits(r) for r in exp[0][4][:7]]
        assert b.lib.uphip_batch_get_masks(b.handle, 0, None, None, 0) == 100
    finally:
        b.close()


def test_limit_refusals(hip):
    c = MC.CASES["g-limit"]
    opts = c.options()
    opts.point_count = A.MAX_POINTS + 1
    with pytest.raises(UnpaperHipError, match="point_count"):
        Batch(opts, 1, *c.size, A.FMT_GRAY8)
    b = Batch(c.options(), 1, *c.size, A.FMT_GRAY8)
    try:
        with pytest.raises(UnpaperHipError, match="batch_set_mask_scan_route"):
            b.set_mask_scan_route(2)
        with pytest.raises(UnpaperHipError, match="batch_set_mask_scan_route"):
            b.set_mask_scan_route(-1)
        b.set_mask_scan_route(LOOPED)
        b.set_mask_scan_route(ONE_LAUNCH)
    finally:
        b.close()


# uphip_batch_device_bytes of three batches of one or two points, measured on
# the parent build (commit ca1f60e) on an MI355X: such a batch allocates the
# same buffers with the same sizes as before
PARENT_BYTES = {"default": 40823420, "f-two-none": 61188356, "list1": 224203316}


def test_device_bytes_of_small_batches_unchanged(hip, oracle):
    def of(opts, cap, w, h):
        b = Batch(opts, cap, w, h, A.FMT_GRAY8)
        try:
            return b.device_bytes()
        finally:
            b.close()
    c = MC.CASES["f-two-none"]
    assert c.npoints == 2
    gw, gh = M.max_size(M.LIST1)
    got = {"default": of(oracle.default_options(), 2, 620, 877),
           "f-two-none": of(c.options(), 3, *c.size),
           "list1": of(M.sheet_options(oracle, M.SHEET), len(M.LIST1), gw, gh)}
    assert got == PARENT_BYTES


@pytest.mark.parametrize("route", [ONE_LAUNCH, LOOPED])
@pytest.mark.parametrize("fmt", [A.FMT_GRAY8, A.FMT_RGB24])
@pytest.mark.parametrize("depth", list(BC.DEPTHS))
def test_scan_corners(hip, oracle, depth, fmt, route):
    """The scan kernel's own corners (mask_batch_cases.py): a band clipped by
    the top edge, one that ends in the last row with its vertical band in the
    last column, one inside, at a finite depth and at depth -1, both scan
    directions on.  Masks only, against oracle.detect_masks on the page;
    filters and deskew are off, and the centring stage is what detects (with
    it off as well nothing detects a mask, in the oracle as here)."""
    opts = BC.corner_options(BC.DEPTHS[depth])
    page = BC.corner_page(fmt)
    b = Batch(opts, 2, *BC.CORNER_SIZE, fmt)
    try:
        b.set_mask_scan_route(route)
        for slot in range(2):
            b.set_input(slot, 0, page)
        b.run(2)
        b.wait()
        n, emasks = BC.corner_expected(oracle, BC.DEPTHS[depth], fmt)
        for slot in range(2):
            count, masks, _ = b.masks(slot)
            assert count == n == 3
            assert [m.tuple() for m in masks] == emasks, "slot %d" % slot
    finally:
        b.close()
