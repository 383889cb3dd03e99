"""The GRAY8 bicubic rotation with a tile's rows dealt to its eight waves
round-robin (csrc/rot_tiles.h rot_wave_row: wave w takes tile rows w, w + 8,
..., w + 40): whole sheets, and the rotation's float bits, byte for byte
against the oracle, on the smallest shapes at which a wrong row mapping shows.

  * sheets of 200 x 53 and 200 x 95: the bottom tile has 5 and 47 rows inside
    the image, so waves own rows on both sides of the image's last row (the
    stores' row test, the partial copy's clamp, the column sums' break);
  * 400 x 560 pages skewed by 2.0 and -2.6 degrees, whose detected mask is
    smaller than the sheet (partial tiles: rows above and below the mask
    inside one wave), with the default pipeline (the rotation's fused column
    sums decide the next mask, so a row counted twice or not at all changes
    the sheet) and with mask centring disabled;
  * a page of horizontal bands, 11 dark rows every 24, skewed by 1 degree: in
    every tile some rows of every wave are white and some are not, so the
    white flag of a wave's row k must belong to the image row that k means.
"""
import math

import numpy as np
import pytest

from test_pipeline_gpu import skewed_page
from test_rotate_tiles_gpu import _block, _check
from unpaper_hip import ctypes_abi as A

pytestmark = pytest.mark.gpu


def _bands(w, h, deg, seed):
    """White page, a block of dark noise bands (11 rows every 24) rotated by
    `deg` degrees about the centre (nearest neighbour)."""
    rng = np.random.default_rng(seed)
    cw, ch = int(w * 0.8), int(h * 0.8)
    g = np.full((ch, cw), 255, np.uint8)
    dark = (np.arange(ch) % 24) < 11
    g[dark] = rng.integers(0, 90, size=(int(dark.sum()), cw))
    out = np.full((h, w), 255, np.uint8)
    t = math.radians(deg)
    yy, xx = np.mgrid[0:h, 0:w]
    dx, dy = xx - w / 2, yy - h / 2
    u = (math.cos(t) * dx + math.sin(t) * dy + cw / 2).astype(np.int64)
    v = (-math.sin(t) * dx + math.cos(t) * dy + ch / 2).astype(np.int64)
    ok = (u >= 0) & (u < cw) & (v >= 0) & (v < ch)
    out[ok] = g[v[ok], u[ok]]
    return out


@pytest.mark.parametrize("w,h,degs", [(200, 53, (2.0, -2.6, None)), (200, 95, (2.6, None, -2.0))])
def test_bottom_tile_rows_on_both_sides_of_the_last_row(hip, oracle, w, h, degs):
    opts = oracle.default_options()
    # short sheets: a scan the sheet can hold, and no deviation veto
    opts.deskew_parameters.deskewScanSize = 30
    opts.deskew_parameters.deskewScanDepth = 0.5
    opts.deskew_parameters.deskewScanDeviationRad = np.float32(10 * math.pi / 180)
    pages = [np.full((h, w), 255, np.uint8) if d is None else _block(w, h, d, 3) for d in degs]
    rots = _check(oracle, opts, pages, "%dx%d" % (w, h))
    # the oracle rotates every non-blank sheet: the rotation kernel ran
    assert all((r != 0.0) == (d is not None) for r, d in zip(rots, degs)), rots


@pytest.mark.parametrize("disable", [0, A.NO_MASK_CENTER])
def test_partial_tiles_and_column_sums(hip, oracle, disable):
    opts = oracle.default_options()
    opts.disable = disable
    w, h = 400, 560
    degs = [2.0, None, -2.6]
    pages = [np.full((h, w), 255, np.uint8) if d is None else skewed_page(w, h, d, 5 + i)
             for i, d in enumerate(degs)]
    rots = _check(oracle, opts, pages, "partial tiles, disable %#x" % disable)
    assert all((r != 0.0) == (d is not None) for r, d in zip(rots, degs)), rots


def test_bands_white_and_inked_rows_in_every_wave(hip, oracle):
    opts = oracle.default_options()
    w, h = 400, 560
    pages = [_bands(w, h, 1.0, 21), _bands(w, h, -1.0, 22)]
    rots = _check(oracle, opts, pages, "bands")
    assert all(r != 0.0 for r in rots), rots
