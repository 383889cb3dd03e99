"""The multi-mask cases: sheets with several mask-scan points (up to
UPHIP_MAX_POINTS, the reference's MAX_POINTS), their options, what each case
is for and the oracle's results on them.  The batch and the runner take at
most two points today; these are the cases their parity tests need once they
take more, and test_multi_mask.py checks on the CPU that the oracle really
works on them.

Every sheet is SIZE (the deskew cases' size of test_pipeline_gpu.py), layout
none, with one block of synthetic text per point, each at its own visible
skew: the deskew stage rotates every mask and the centring stage moves it, so
no case is a no-op.  A case has three sheets whose skews differ, so that one
batch holds sheets that rotate differently.
"""
import functools
import math

import numpy as np

from unpaper_hip import ctypes_abi as A
from unpaper_hip.hostimage import HostImage
import filter_cases as FC

SIZE = (620, 877)
SHEETS = 3
FILTERS = A.NO_BLACKFILTER | A.NO_NOISEFILTER | A.NO_BLURFILTER | A.NO_GRAYFILTER


def text_block(bw, bh, rng):
    """bw x bh of left-aligned text lines made of 3 x 3 cells (the page of
    test_pipeline_gpu.skewed_page, one block of it)."""
    g = np.full((bh, bw), 255, np.uint8)
    for y in range(0, bh - 8, 18):
        cells = rng.random((3, bw // 3)) < 0.5
        cells[:, :2] = True          # a solid left edge for the rotation scan
        cells[:, -2:] = True
        vals = rng.integers(0, 41, size=cells.shape)
        blk = np.where(cells, vals, 255).astype(np.uint8)
        g[y:y + 9, :cells.shape[1] * 3] = np.repeat(np.repeat(blk, 3, 0), 3, 1)
    return g


def draw_block(out, cx, cy, bw, bh, deg, rng):
    """A text block of bw x bh rotated by `deg` degrees about (cx, cy)."""
    h, w = out.shape
    blk = text_block(bw, bh, rng)
    t = math.radians(deg)
    r = int(math.hypot(bw, bh) / 2) + 2
    y0, y1, x0, x1 = max(cy - r, 0), min(cy + r, h), max(cx - r, 0), min(cx + r, w)
    yy, xx = np.mgrid[y0:y1, x0:x1]
    dx, dy = xx - cx, yy - cy
    u = np.floor(math.cos(t) * dx + math.sin(t) * dy + bw / 2).astype(np.int64)
    v = np.floor(-math.sin(t) * dx + math.cos(t) * dy + bh / 2).astype(np.int64)
    ok = (u >= 0) & (u < bw) & (v >= 0) & (v < bh)
    sub = out[y0:y1, x0:x1]
    sub[ok] = blk[v[ok], u[ok]]


class MaskCase:
    """points: the options' points.  blocks: (cx, cy, bw, bh) of the text
    block of each point, None for a point over blank paper.  degs[sheet][i]:
    block i's skew on that sheet.  cell: the masks' maximum size.  specks:
    dark 3 x 3 specks over the whole sheet (what a rotation moves where the
    paper between the blocks would otherwise be white before and after).
    scan: mask scan size and step."""

    def __init__(self, name, points, blocks, degs, cell, disable=0, specks=0, scan=(20, 5),
                 size=SIZE, seed=1, about=""):
        self.name, self.points, self.blocks, self.degs = name, points, blocks, degs
        self.cell, self.disable, self.specks, self.scan = cell, disable, specks, scan
        self.size, self.seed, self.about = size, seed, about

    @property
    def npoints(self):
        return len(self.points)

    def options(self, interp=A.INTERP_CUBIC, disable=0):
        o = FC.default_options()
        o.layout = A.LAYOUT_NONE
        o.interpolate_type = interp
        o.disable = self.disable | disable
        o.point_count = len(self.points)
        for i, (x, y) in enumerate(self.points):
            o.points[i] = A.Point(x, y)
        mp = o.mask_detection_parameters
        mp.scan_direction = A.Direction(True, True)
        mp.scan_size = A.RectangleSize(self.scan[0], self.scan[0])
        mp.scan_step = A.Delta(self.scan[1], self.scan[1])
        # each point's bars span its own cell only
        mp.scan_depth.horizontal = self.cell[1]
        mp.scan_depth.vertical = self.cell[0]
        mp.minimum_width = mp.minimum_height = min(50, self.cell[0] // 2, self.cell[1] // 2)
        mp.maximum_width, mp.maximum_height = self.cell
        return o

    def gray(self, sheet):
        w, h = self.size
        rng = np.random.default_rng(self.seed * 100 + sheet)
        g = np.full((h, w), 255, np.uint8)
        for i, b in enumerate(self.blocks):
            if b is not None:
                draw_block(g, *b, self.degs[sheet][i], rng)
        for _ in range(self.specks):
            x, y = int(rng.integers(0, w - 3)), int(rng.integers(0, h - 3))
            g[y:y + 3, x:x + 3] = rng.integers(0, 60)
        return g, rng

    def page(self, sheet, fmt=A.FMT_GRAY8):
        g, rng = self.gray(sheet)
        return FC.as_format(g, fmt, rng)


def _grid(cols, rows, bw, bh, size=SIZE, dx=0, dy=0):
    """Blocks of bw x bh at the centres of a cols x rows grid, row by row."""
    w, h = size
    return [(w * (2 * c + 1) // (2 * cols) + dx, h * (2 * r + 1) // (2 * rows) + dy, bw, bh)
            for r in range(rows) for c in range(cols)]


def _points(blocks, off=(0, 0)):
    return [(b[0] + off[0], b[1] + off[1]) for b in blocks]


def _degs(n, base):
    """Three sheets: each block at its own skew, the sheets' skews differing
    in size and sign."""
    out = []
    for s in range(SHEETS):
        out.append([(base[(i + s) % len(base)]) * (1 if (i + s) % 2 == 0 else -1) for i in range(n)])
    return out


BASE_DEGS = (1.5, 2.4, 3.1, 0.9, 2.0, 3.6)


def case_row3():
    b = _grid(3, 1, 120, 420)
    return MaskCase("a-row3", _points(b, (6, -9)), b, _degs(3, BASE_DEGS), (200, 520),
                    about="3 points in a row")


def case_grid4():
    b = _grid(2, 2, 170, 250)
    return MaskCase("b-grid4", _points(b, (-7, 8)), b, _degs(4, BASE_DEGS), (290, 400),
                    about="2 x 2 grid, well separated regions")


def case_overlap4():
    # blocks 70 px apart and bars of 50, which end some 45 px past a block:
    # every mask reaches into its neighbours'
    w, h = SIZE
    b = [(w // 2 - 130, h // 2 - 180, 190, 290), (w // 2 + 130, h // 2 - 180, 190, 290),
         (w // 2 - 130, h // 2 + 180, 190, 290), (w // 2 + 130, h // 2 + 180, 190, 290)]
    return MaskCase("c-overlap4", _points(b, (5, 5)), b, _degs(4, BASE_DEGS), (300, 420),
                    disable=FILTERS, specks=500, scan=(50, 5), seed=3,
                    about="4 points whose masks overlap pairwise")


def case_mixed6():
    # a 2 x 3 grid; the blocks of points 1 and 4 share the left column's upper
    # two cells and are pushed together, the others keep their cells' centres
    w, h = SIZE
    g = _grid(2, 3, 150, 170)
    left_top, right_top, left_mid, right_mid, left_bot, right_bot = g
    near = 38
    b = [right_top,
         (left_top[0], left_top[1] + near, 150, 170),      # point 1
         right_mid, left_bot,
         (left_mid[0], left_mid[1] - near, 150, 170),      # point 4
         right_bot]
    degs = _degs(6, BASE_DEGS)
    for s in range(SHEETS):   # the two near blocks at the largest skews: the widest windows
        degs[s][1], degs[s][4] = (4.4, -4.1, 3.9)[s], (-4.2, 4.5, 4.3)[s]
    return MaskCase("d-mixed6", _points(b, (4, -6)), b, degs, (260, 250),
                    disable=FILTERS, specks=500, seed=4,
                    about="6 points, mask 1's rotation window reaches into mask 4")


def case_blank3():
    b = _grid(1, 3, 300, 170)
    blocks = [b[0], None, b[2]]
    return MaskCase("e-blank3", [(b[0][0] + 5, b[0][1]), (b[1][0], b[1][1]), (b[2][0] - 8, b[2][1] + 6)],
                    blocks, _degs(3, BASE_DEGS), (420, 260), seed=5,
                    about="a point over blank paper: its mask is the maximum size about it")


def case_two_none():
    b = _grid(1, 2, 360, 260)
    return MaskCase("f-two-none", _points(b, (10, -5)), b, _degs(2, BASE_DEGS), (560, 400), seed=6,
                    about="2 points given explicitly, layout none")


def case_limit():
    # UPHIP_MAX_POINTS points on a 10 x 10 grid of 40 x 40 cells; each cell
    # holds a dark blob off its centre, which the centring moves there
    size = (400, 400)
    pts = [(40 * c + 20, 40 * r + 20) for r in range(10) for c in range(10)]
    assert len(pts) == A.MAX_POINTS
    case = MaskCase("g-limit", pts, [None] * len(pts), [[0] * len(pts)] * SHEETS, (36, 36),
                    disable=FILTERS | A.NO_DESKEW, scan=(6, 2), size=size, seed=7,
                    about="UPHIP_MAX_POINTS points, deskew off, centring on")

    def gray(sheet):
        rng = np.random.default_rng(700 + sheet)
        g = np.full((size[1], size[0]), 255, np.uint8)
        for i, (x, y) in enumerate(pts):
            ox, oy = int(rng.integers(-4, 5)), int(rng.integers(-4, 5))
            if ox == 0 and oy == 0:
                ox = 3
            g[y + oy - 7:y + oy + 7, x + ox - 7:x + ox + 7] = rng.integers(0, 50, size=(14, 14))
        return g, rng
    case.gray = gray
    return case


def all_cases():
    return [case_row3(), case_grid4(), case_overlap4(), case_mixed6(), case_blank3(),
            case_two_none(), case_limit()]


CASES = {c.name: c for c in all_cases()}
DEPENDENT = ("c-overlap4", "d-mixed6")
FORMAT_CASES = ("b-grid4", "c-overlap4", "d-mixed6")
INTERPS = (A.INTERP_NN, A.INTERP_LINEAR, A.INTERP_CUBIC)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle_py import Oracle
    return Oracle()


def deskew_stage(o, c, s, fmt=A.FMT_GRAY8, interp=A.INTERP_CUBIC):
    """The deskew stage restated with the oracle's per-op calls, each mask
    detected on the sheet as the masks before it left it: (the sheet after
    the stage, every mask's rotation -- the oracle's report keeps two)."""
    opts = c.options(interp)
    cur, _, _ = o.process_sheet(c.options(interp, A.NO_DESKEW | A.NO_MASK_CENTER), [c.page(s, fmt)])
    if opts.disable & A.NO_DESKEW:
        return cur, [0.0] * c.npoints
    n, masks = o.detect_masks(cur, opts.mask_detection_parameters, [A.Point(*p) for p in c.points])
    rots = []
    for i in range(n):
        r = o.detect_rotation(cur, masks[i], opts.deskew_parameters)
        rots.append(r)
        if r != 0.0:
            o.deskew(cur, masks[i], r, interp)
    return cur, rots


@functools.lru_cache(maxsize=None)
def expected(name, fmt=A.FMT_GRAY8, interp=A.INTERP_CUBIC):
    """The oracle on the case's sheets, computed once: per sheet (saved frame,
    report, mask count and masks of the centring stage's detection, every
    mask's rotation).  The masks are detect_masks on deskew_stage's sheet,
    the image the centring stage's detection sees; test_multi_mask.py checks
    that sheet against the oracle's own with the centring disabled."""
    from concurrent.futures import ThreadPoolExecutor
    o, c = _oracle(), CASES[name]
    opts = c.options(interp)

    def one(s):
        sheet, ofmt, rep = o.process_sheet(opts, [c.page(s, fmt)])
        pre, rots = deskew_stage(o, c, s, fmt, interp)
        n, masks = o.detect_masks(pre, opts.mask_detection_parameters, [A.Point(*p) for p in c.points])
        return o.convert_for_save(sheet, ofmt), rep, n, [m.tuple() for m in masks], rots
    with ThreadPoolExecutor(SHEETS) as ex:
        return list(ex.map(one, range(SHEETS)))
