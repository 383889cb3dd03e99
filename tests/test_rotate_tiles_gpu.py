"""The GRAY8 bicubic rotation reading its per-sheet and per-tile records
(csrc/rot_tiles.h, written by k_rot_tiles once per launch) instead of deriving
them in every tile: whole sheets, and the rotation's float bits, byte for byte
against the oracle, on the shapes where a wrong record shows.

  * sheets of 129 x 49, 127 x 47 and 300 x 200: the 128 x 48 tiles cross the
    right and bottom edge, and the mask is the whole sheet, so the corner
    tiles' windows start outside the image (posc false, edge staging);
  * 400 x 560 pages skewed by 0.3, -2.0, 2.6 and 2.8 degrees (and 2.2 / 2.35,
    next to the small-window class bound), mixed with blank sheets: both
    launches take sheets; with the default pipeline (the rotation's fused
    column sums feed the next mask scan) and with mask centring disabled;
  * one batch of 66 sheets, large-window sheets at both ends, so the
    large-window launch's sheet walk crosses a 64-sheet group;
  * the single-image deskew op, which takes its records from the same kernel.
"""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_pipeline_gpu import assert_same, gpu_sheets, oracle_sheet, skewed_page
from unpaper_hip import ctypes_abi as A
from unpaper_hip.hostimage import HostImage

pytestmark = pytest.mark.gpu


def _need_rows(rotation):
    """Window rows a 128 x 48 tile needs at this rotation (the class test)."""
    return 48 + int(np.ceil(np.float32(127) * np.abs(np.sin(np.float32(rotation))))) + 5


def _block(w, h, deg, seed):
    """White page, a block of dark noise rotated by `deg` about the centre:
    edges that the rotation detection finds even on a sheet of one tile."""
    rng = np.random.default_rng(seed)
    t = math.radians(deg)
    yy, xx = np.mgrid[0:h, 0:w]
    dx, dy = xx - w / 2, yy - h / 2
    u = math.cos(t) * dx + math.sin(t) * dy
    v = -math.sin(t) * dx + math.cos(t) * dy
    inside = (abs(u) < w * 0.3) & (abs(v) < h * 0.25)
    out = np.full((h, w), 255, np.uint8)
    out[inside] = rng.integers(0, 80, size=int(inside.sum()))
    return out


def _check(oracle, opts, arrays, what):
    """Every sheet and detected angle against the oracle (run once per distinct
    page); returns the oracle's rotations."""
    sheets = [[HostImage.from_array(a, A.FMT_GRAY8)] for a in arrays]
    outs, reps = gpu_sheets(opts, sheets)
    first = {}
    for s, a in enumerate(arrays):
        first.setdefault(id(a), s)
    todo = sorted(first.values())
    with ThreadPoolExecutor(8) as ex:
        exps = dict(zip(todo, ex.map(lambda s: oracle_sheet(oracle, opts, sheets[s]), todo)))
    rots = []
    for s, a in enumerate(arrays):
        exp, erep = exps[first[id(a)]]
        assert_same(outs[s], exp, "%s sheet %d" % (what, s))
        assert reps[s].mask_count == erep.mask_count
        assert np.float32(reps[s].rotation[0]).tobytes() == \
            np.float32(erep.rotation[0]).tobytes(), "%s rotation of sheet %d" % (what, s)
        rots.append(float(erep.rotation[0]))
    return rots


@pytest.mark.parametrize("w,h,degs", [(129, 49, (2.0, -2.6, None)), (127, 47, (4.5, None, 4.5)),
                                      (300, 200, (2.6, -2.0, 4.0, None))])
def test_small_sheets_edge_tiles(hip, oracle, w, h, degs):
    opts = oracle.default_options()
    if w < 200:
        # one-tile sheets: a scan the sheet can hold, and no deviation veto
        opts.deskew_parameters.deskewScanSize = 30
        opts.deskew_parameters.deskewScanDepth = 0.5
        opts.deskew_parameters.deskewScanDeviationRad = np.float32(10 * math.pi / 180)
        pages = [np.full((h, w), 255, np.uint8) if d is None else _block(w, h, d, 3) for d in degs]
    else:
        pages = [np.full((h, w), 255, np.uint8) if d is None else skewed_page(w, h, d, 7)
                 for d in degs]
    rots = _check(oracle, opts, pages, "%dx%d" % (w, h))
    # the oracle rotates every non-blank sheet: the rotation kernel ran
    assert all((r != 0.0) == (d is not None) for r, d in zip(rots, degs)), rots


@pytest.mark.parametrize("disable", [0, A.NO_MASK_CENTER])
def test_window_classes_and_column_sums(hip, oracle, disable):
    opts = oracle.default_options()
    opts.disable = disable
    w, h = 400, 560
    degs = [0.3, None, -2.0, 2.6, 2.8, None, 2.2, 2.35]
    pages = [np.full((h, w), 255, np.uint8) if d is None else skewed_page(w, h, d, i)
             for i, d in enumerate(degs)]
    rots = _check(oracle, opts, pages, "classes, disable %#x" % disable)
    need = [_need_rows(r) for r in rots if r]
    assert len(need) == 6, rots
    # sheets on both sides of the small-window bound (58 or 59 rows, by the
    # launcher's LDS budget: either way)
    assert min(need) <= 58 and max(need) >= 60, need


def test_large_window_walk_crosses_sheet_group(hip, oracle):
    opts = oracle.default_options()
    w, h = 300, 200
    kinds = {d: skewed_page(w, h, d, 7) for d in (2.6, -2.0, 4.0)}
    kinds[None] = np.full((h, w), 255, np.uint8)
    order = [4.0, -2.0, None, 2.6]
    pages = [kinds[order[i % 4]] for i in range(66)]   # sheets 64 and 65: 4.0 and -2.0
    pages[65] = kinds[4.0]
    rots = _check(oracle, opts, pages, "66 sheets")
    assert _need_rows(rots[0]) >= 60 and _need_rows(rots[64]) >= 60 and \
        _need_rows(rots[65]) >= 60 and _need_rows(rots[1]) <= 58, (rots[:4], rots[64:])


@pytest.mark.parametrize("deg,mask", [(2.0, (30, 40, 370, 520)), (-2.8, (0, 0, 399, 559))])
def test_single_image_deskew_op(hip, oracle, deg, mask):
    w, h = 400, 560
    img = HostImage.from_array(skewed_page(w, h, deg, 11), A.FMT_GRAY8)
    rad = np.float32(deg * math.pi / 180.0)
    d = hip.upload(img)
    hip.deskew(d, A.rect(*mask), float(rad), A.INTERP_CUBIC)
    oracle.deskew(img, A.rect(*mask), float(rad), A.INTERP_CUBIC)
    assert_same(d.to_host(), img)
