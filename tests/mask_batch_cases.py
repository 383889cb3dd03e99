"""The corners of the one-launch mask scan (k_mask_sums_points): a small sheet
whose three points put a scan band over the top edge, into the last row and
the last column, and inside the sheet, at a finite scan depth and at depth -1
(the whole sheet).  test_multi_mask_batch.py checks on the CPU that the
oracle's masks on it are three different ones and none the maximum-size
fallback; test_multi_mask_batch_gpu.py compares the batch's masks with them."""
import numpy as np

from unpaper_hip import ctypes_abi as A
import filter_cases as FC
import mask_cases as MC

CORNER_SIZE = (200, 120)
CORNER_DEPTH = (50, 40)     # the vertical scan's columns, the horizontal scan's rows
# the depth's band of point 0 starts 8 rows above the sheet; point 1's ends in
# the last row (100 - 20 + 40 - 1 = 119) and its vertical band in the last
# column (175 - 25 + 50 - 1 = 199); point 2's lie inside
CORNER_POINTS = [(40, 12), (175, 100), (105, 60)]
CORNER_BLOCKS = [(24, 3, 62, 25), (160, 86, 194, 116), (88, 47, 118, 71)]   # x0, y0, x1, y1
# dark paper below point 2's finite band, left of its block's columns: the
# whole-sheet depth sees it, the finite depth must not
CORNER_DISTRACTORS = [(70, 92, 84, 116)]
CORNER_MAX = (90, 70)
DEPTHS = {"finite": CORNER_DEPTH, "whole": (-1, -1)}


def corner_options(depth, disable=0):
    """Filters and deskew off, both scan directions on.  The centring stays:
    its detection is the one uphip_batch_get_masks returns (with the deskew
    and the centring both off no stage detects a mask, in the reference as in
    the batch), and its moves come after the masks are kept."""
    o = FC.default_options()
    o.layout = A.LAYOUT_NONE
    o.disable = MC.FILTERS | A.NO_DESKEW | disable
    o.point_count = len(CORNER_POINTS)
    for i, (x, y) in enumerate(CORNER_POINTS):
        o.points[i] = A.Point(x, y)
    mp = o.mask_detection_parameters
    mp.scan_direction = A.Direction(True, True)
    mp.scan_size = A.RectangleSize(6, 6)
    mp.scan_step = A.Delta(2, 2)
    mp.scan_depth.vertical, mp.scan_depth.horizontal = depth
    mp.scan_threshold.horizontal = mp.scan_threshold.vertical = 0.4   # tinted paper ends a scan
    mp.minimum_width = mp.minimum_height = 10
    mp.maximum_width, mp.maximum_height = CORNER_MAX
    return o


def corner_page(fmt):
    w, h = CORNER_SIZE
    rng = np.random.default_rng(41)
    g = np.full((h, w), 255, np.uint8)
    for x0, y0, x1, y1 in CORNER_BLOCKS + CORNER_DISTRACTORS:
        g[y0:y1 + 1, x0:x1 + 1] = rng.integers(0, 60, size=(y1 - y0 + 1, x1 - x0 + 1))
    return FC.as_format(g, fmt, rng)


def corner_fallback():
    """detect_mask's answer where it finds nothing: the maximum size about
    each point (masks.c:165-180)."""
    mw, mh = CORNER_MAX
    return [(x - mw // 2, y - mh // 2, x + mw // 2, y + mh // 2) for x, y in CORNER_POINTS]


def corner_expected(oracle, depth, fmt):
    o = corner_options(depth)
    n, masks = oracle.detect_masks(corner_page(fmt), o.mask_detection_parameters,
                                   [A.Point(*p) for p in CORNER_POINTS])
    return n, [m.tuple() for m in masks]
