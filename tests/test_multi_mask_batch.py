"""What test_multi_mask_batch_gpu.py relies on, shown on the CPU: the scan
corner sheet gives three different masks, none the fallback, and the
whole-sheet depth another answer than the finite one; d-mixed6 depends on the
order of its masks at every interpolation; the route entry is in the ctypes
mirror; the PDF tool takes its points."""
import os
import sys

import numpy as np
import pytest

from unpaper_hip import ctypes_abi as A
import mask_batch_cases as BC
import mask_cases as MC

FMTS = (A.FMT_GRAY8, A.FMT_RGB24)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("depth", list(BC.DEPTHS))
def test_corner_masks_are_distinct(oracle, depth, fmt):
    n, masks = BC.corner_expected(oracle, BC.DEPTHS[depth], fmt)
    assert n == len(BC.CORNER_POINTS) == 3
    assert len(set(masks)) == 3
    for m, f in zip(masks, BC.corner_fallback()):
        # neither axis fell back to the maximum size about the point
        assert (m[0], m[2]) != (f[0], f[2]) and (m[1], m[3]) != (f[1], f[3]), (m, f)


@pytest.mark.parametrize("fmt", FMTS)
def test_corner_depths_differ(oracle, fmt):
    """A scan that summed the whole sheet where the depth is finite (or the
    reverse) gives another mask for point 2."""
    finite = BC.corner_expected(oracle, BC.DEPTHS["finite"], fmt)[1]
    whole = BC.corner_expected(oracle, BC.DEPTHS["whole"], fmt)[1]
    assert finite[2] != whole[2]


def test_corner_bands_touch_the_edges():
    w, h = BC.CORNER_SIZE
    dv, dh = BC.CORNER_DEPTH
    (x0, y0), (x1, y1), (x2, y2) = BC.CORNER_POINTS
    assert y0 - dh // 2 < 0                                   # clipped by the top edge
    assert y1 - dh // 2 + dh - 1 == h - 1                     # ends in the last row
    assert x1 - dv // 2 + dv - 1 == w - 1                     # ends in the last column
    assert 0 < y2 - dh // 2 and y2 - dh // 2 + dh - 1 < h - 1
    assert all(0 <= x < w and 0 <= y < h for x, y in BC.CORNER_POINTS)


@pytest.mark.parametrize("interp", MC.INTERPS)
def test_mixed6_depends_on_the_order(oracle, interp):
    """test_multi_mask.rotated_from_undeskewed's comparison at every
    interpolation: on two of d-mixed6's three sheets a mask reads what an
    earlier one wrote, whichever kernel interpolates."""
    c = MC.CASES["d-mixed6"]
    differ = []
    for s in range(MC.SHEETS):
        opts = c.options(interp)
        plain, _, _ = oracle.process_sheet(c.options(interp, A.NO_DESKEW | A.NO_MASK_CENTER), [c.page(s)])
        n, masks = oracle.detect_masks(plain, opts.mask_detection_parameters,
                                       [A.Point(*p) for p in c.points])
        out = plain.copy()
        for i in range(n):
            r = oracle.detect_rotation(plain, masks[i], opts.deskew_parameters)
            if r != 0.0:
                tmp = plain.copy()
                oracle.deskew(tmp, masks[i], r, interp)
                oracle.copy_rectangle(tmp, out, masks[i], masks[i].vertex[0])
        deskewed = oracle.process_sheet(c.options(interp, A.NO_MASK_CENTER), [c.page(s)])[0]
        differ.append(bool((out.payload() != deskewed.payload()).any()))
    assert differ == [True, True, False]


def test_set_mask_scan_route_in_ctypes_mirror():
    import ctypes as C
    from unpaper_hip.device import EXPORTED, load_library
    from unpaper_hip.pipeline import Batch
    assert "uphip_batch_set_mask_scan_route" in EXPORTED
    L = load_library()
    f = L.uphip_batch_set_mask_scan_route
    assert f.restype is C.c_int and len(f.argtypes) == 2
    assert f(None, 0) == -1
    assert b"batch_set_mask_scan_route" in L.uphip_last_error()
    L.uphip_clear_error()
    assert callable(Batch.set_mask_scan_route)


def test_pdf_pipeline_takes_mask_scan_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import pdf_pipeline
    finally:
        sys.path.pop(0)
    args = pdf_pipeline.parse_args(["in.pdf", "out.pdf", "--mask-scan-point", "100,200",
                                    "--mask-scan-point", "300,400", "--mask-scan-point", "5,6"])
    o = A.Options()
    pdf_pipeline.apply_mask_scan_points(o, args.mask_scan_point)
    assert o.point_count == 3
    assert [(o.points[i].x, o.points[i].y) for i in range(3)] == [(100, 200), (300, 400), (5, 6)]
    with pytest.raises(SystemExit):
        pdf_pipeline.parse_args(["in.pdf", "out.pdf", "--mask-scan-point", "100"])
    with pytest.raises(ValueError, match="mask-scan-point"):
        pdf_pipeline.apply_mask_scan_points(A.Options(), [(1, 1)] * (A.MAX_POINTS + 1))
