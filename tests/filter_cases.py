"""The filter suite's cases: pages, parameters and what each case is for,
shared by the device parity tests (test_filters_gpu.py: HIP == oracle) and the
CPU check that the oracle really works on them (test_filter_cases.py).

A parity case proves something only where the oracle changes the page: a case
states the work it expects of the oracle (`work`: lower bounds on changed
pixels and on oracle.stats() counters), or why there is none (`noop`).  A case
made for one arm of a launcher (a kernel picked by sheet size or geometry)
names the arm (`arms`), as uphip_filter_arms reports it.

The parameter lists (GRAY_SIZES, BLUR_PARAMS, ...) are the tables the
parametrized tests are built from; the builders below make the case of one
combination.
"""
import ctypes as C
import functools
import io

import numpy as np

from unpaper_hip import ctypes_abi as A
from unpaper_hip.hostimage import HostImage
from helpers import BYTE_FORMATS, FORMATS, make_image, page_array

MONO = (A.FMT_MONOWHITE, A.FMT_MONOBLACK)
NAMES = {A.FMT_GRAY8: "gray", A.FMT_RGB24: "rgb", A.FMT_Y400A: "ya", A.FMT_MONOWHITE: "monow",
         A.FMT_MONOBLACK: "monob"}


class Case:
    """filter: grayfilter / blurfilter / noisefilter / blackfilter / masks /
    border.  page(): a fresh HostImage.  args: what follows the image in the
    backend's call.  work: {"changed": n} and oracle.stats() names, each a
    lower bound (">="); for a detection {"edges": n}: sides of its result that
    are not the page's own."""

    def __init__(self, filter, name, fmt, page, args, work=None, noop=None, arms=(), fused=False):
        self.filter, self.name, self.fmt, self.page, self.args = filter, name, fmt, page, args
        self.work = dict(work or {})
        self.noop = noop
        self.arms = tuple(arms)
        self.fused = fused
        if not noop and filter not in ("masks", "border"):
            self.work.setdefault("changed", 1)

    @property
    def id(self):
        return "%s-%s-%s" % (self.filter, self.name, NAMES[self.fmt])

    def run(self, backend, image):
        """The case's operation on `image` (a HostImage for the oracle, a
        device image for the HIP backend); detections return their result."""
        return getattr(backend, {"masks": "detect_masks", "border": "detect_border"}
                       .get(self.filter, self.filter))(image, *self.args)


def both(hip, oracle, case):
    """HIP == oracle on the case: the filtered page byte for byte, or the
    detection's result."""
    from helpers import assert_same
    h = case.page()
    d = hip.upload(h)
    r1 = case.run(hip, d)
    r2 = case.run(oracle, h)
    if case.filter == "masks":
        assert r1[0] == r2[0] and [m.tuple() for m in r1[1]] == [m.tuple() for m in r2[1]]
    elif case.filter == "border":
        assert r1.tuple() == r2.tuple()
    else:
        assert_same(d.to_host(), h, case.id)


@functools.lru_cache(maxsize=None)
def _defaults():
    from oracle_py import Oracle
    return Oracle().default_options()


def default_options():
    o = A.Options()
    C.memmove(C.byref(o), C.byref(_defaults()), C.sizeof(o))
    return o


# ------------------------------------------------------------------ formats
def as_format(g, fmt, rng, thr=None):
    """A gray array in `fmt`: RGB24 channels tinted apart (as the C4 pages),
    Y400A with a random alpha, 1-bit white where gray >= 128."""
    kw = {} if thr is None else {"abs_black_threshold": thr}
    if fmt == A.FMT_RGB24:
        t = rng.integers(0, 9, size=3)
        rgb = np.stack([np.maximum(g.astype(np.int16) - int(t[c]), 0) for c in range(3)], axis=2)
        return HostImage.from_array(rgb.astype(np.uint8), fmt, **kw)
    if fmt == A.FMT_Y400A:
        a = rng.integers(0, 256, size=g.shape, dtype=np.uint8)
        return HostImage.from_array(np.stack([g, a], axis=2), fmt, **kw)
    if fmt in MONO:
        return HostImage.from_array(g >= 128, fmt, **kw)
    return HostImage.from_array(g, fmt, **kw)


def gray3(g, fmt):
    """A gray array as GRAY8, or as RGB24 with three equal channels."""
    return HostImage.from_array(np.repeat(g[:, :, None], 3, axis=2) if fmt == A.FMT_RGB24 else g, fmt)


# --------------------------------------------------------------- grayfilter
GRAY_SIZES = [(300, 200), (1001, 777), (50, 50), (7, 3)]
GRAY_PARAMS = [((50, 50), (20, 20), 127), ((30, 20), (15, 8), 127),
               ((50, 50), (20, 20), 200), ((13, 7), (5, 3), 60)]


def gray_params(size, step, thr):
    return A.GrayfilterParameters(A.RectangleSize(*size), A.Delta(*step), thr)


def cloud_array(w, h, seed, strokes=None):
    """Light-gray clouds (185..249: above the black threshold in every format,
    the RGB24 tint included, so the grayfilter wipes what carries no dark
    pixel) with sparse dark strokes (the tiles it must leave alone)."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(200, 236, size=((h + 15) // 16 + 1, (w + 15) // 16 + 1))
    g = np.kron(coarse, np.ones((16, 16), np.int64))[:h, :w] + rng.integers(-15, 14, size=(h, w))
    g = np.clip(g, 185, 249).astype(np.uint8)
    n = w * h // 2500 if strokes is None else strokes
    for _ in range(n):
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        if rng.integers(0, 2):
            g[y, x:x + int(rng.integers(2, 12))] = rng.integers(0, 60)
        else:
            g[y:y + int(rng.integers(2, 12)), x] = rng.integers(0, 60)
    return g, rng


def cloud_page(w, h, fmt, seed=5, strokes=None):
    g, rng = cloud_array(w, h, seed, strokes)
    return as_format(g, fmt, rng)


def gray_page_case(fmt, size, params):
    name = "%dx%d-%dx%d-%d" % (size + params[0] + (params[2],))
    if fmt in MONO:
        # the pages these cases always had
        return Case("grayfilter", name, fmt, lambda: make_image(*size, fmt, seed=5),
                    (gray_params(*params),),
                    noop="1-bit page: the grayfilter has nothing to wipe (a tile without a "
                         "black pixel is white already)")
    return Case("grayfilter", name, fmt, lambda: cloud_page(*size, fmt), (gray_params(*params),))


def gray_scene_case():  # cuda_filters_test.c:296-331
    def page():
        g = np.full((8, 8), 255, np.uint8)
        g[0:4, 0:4] = 150
        g[0:4, 4:8] = 80
        return HostImage.from_array(g, A.FMT_GRAY8, abs_black_threshold=50)
    return Case("grayfilter", "scene", A.FMT_GRAY8, page, (gray_params((4, 4), (4, 4), 127),))


GRAY_FEEDBACK_BLACK = [40, 100, 170]
GRAY_FEEDBACK_THR = (127, 160, 90)


def gray_feedback_cases(black):
    """Saturated colour blocks: gray > black threshold but min(rgb) tiny, so a
    tile fails on the original image and passes once earlier tiles are wiped."""
    def page():
        rng = np.random.default_rng(7)
        rgb = np.full((260, 330, 3), 255, np.uint8)
        for _ in range(60):
            x, y = int(rng.integers(0, 320)), int(rng.integers(0, 250))
            rgb[y:y + int(rng.integers(3, 30)), x:x + int(rng.integers(3, 30))] = \
                [int(rng.integers(200, 256)), int(rng.integers(200, 256)), int(rng.integers(0, 30))]
        return HostImage.from_array(rgb, A.FMT_RGB24, abs_black_threshold=black)
    return [Case("grayfilter", "feedback-%d-%d" % (black, thr), A.FMT_RGB24, page,
                 (gray_params((50, 50), (20, 20), thr),)) for thr in GRAY_FEEDBACK_THR]


def gray_arm_cases():
    """The generic GRAY8 cells kernel (cell height 256 > 255; W > 16384) and
    both sides of the tile kernels' LDS bound 2 * 4 * th * ncx = 32768."""
    out = []
    # ch = gcd(256, 512) = 256; a stroke keeps the first tile, the others go
    def first_tile_kept(size):
        g, rng = cloud_array(*size, 5, strokes=0)
        g[10, 10:20] = 0
        return as_format(g, A.FMT_GRAY8, rng)
    for size in [(300, 200), (1001, 777)]:
        out.append(Case("grayfilter", "ch256-%dx%d" % size, A.FMT_GRAY8,
                        lambda size=size: first_tile_kept(size),
                        (gray_params((512, 512), (256, 256), 127),),
                        arms=("gray.cells_generic", "gray.tiles_lds")))
    out.append(Case("grayfilter", "w16400", A.FMT_GRAY8,
                    lambda: cloud_page(16400, 64, A.FMT_GRAY8, seed=6),
                    (gray_params((50, 50), (20, 20), 127),),
                    arms=("gray.cells_generic", "gray.tiles_generic")))
    # cells of 1 x 1: th = 8, ncx = W; 8 * 8 * 512 = 32768 fits, 8 * 8 * 513 does not
    for w, arm in [(512, "gray.tiles_lds"), (513, "gray.tiles_generic")]:
        for fmt in (A.FMT_GRAY8, A.FMT_RGB24):
            out.append(Case("grayfilter", "lds-edge-%d" % w, fmt,
                            lambda w=w, fmt=fmt: cloud_page(w, 90, fmt, seed=w),
                            (gray_params((8, 8), (3, 5), 127),),
                            arms=(arm,) + (("gray.cells_strips",) if fmt == A.FMT_GRAY8 else
                                           ("gray.cells_generic",))))
    return out


# --------------------------------------------------------------- blurfilter
BLUR_SIZES = [(2480 // 4, 3508 // 4), (1001, 777), (99, 300), (100, 100)]
BLUR_PARAMS = [((100, 100), (50, 50), 0.01), ((40, 30), (15, 20), 0.05),
               ((64, 64), (64, 13), 0.2)]
BLUR_EXTRA_SIZES = [(101, 101)]   # just above one default block
BLUR_WIDE_WIDTHS = [1320, 2000, 3960, 4480, 4520]
BLUR_WIDE_PARAMS = (((40, 30), (15, 20), 0.05), ((40, 40), (40, 10), 0.3))


def blur_params(size, step, intensity):
    return A.BlurfilterParameters(A.RectangleSize(*size), A.Delta(*step), intensity)


def speck_block_array(w, h, seed, density=0.002):
    """White paper, sparse dark specks (what the blurfilter wipes) and one
    40 %-dense block an eighth of the page wide (what it must keep, with the
    blocks around it)."""
    rng = np.random.default_rng(seed)
    g = np.full((h, w), 255, np.uint8)
    m = rng.random((h, w)) < density
    g[m] = rng.integers(0, 120, size=int(m.sum()))
    bw, bh = max(2, w // 8), max(2, h // 8)
    bx, by = (w - bw) * 5 // 8, (h - bh) * 5 // 8
    m = rng.random((bh, bw)) < 0.4
    g[by:by + bh, bx:bx + bw][m] = rng.integers(0, 120, size=int(m.sum()))
    g[h // 2, w // 3] = 0      # a speck whatever the density draws on a small page
    return g, rng


def speck_block_page(w, h, fmt, seed=6, density=0.002):
    g, rng = speck_block_array(w, h, seed, density)
    return as_format(g, fmt, rng)


def blur_page_case(fmt, size, params):
    name = "%dx%d-%dx%d" % (size + params[0])
    noop = None
    if size[0] < params[0][0] or size[1] < params[0][1]:
        noop = "page smaller than one block"
    return Case("blurfilter", name, fmt, lambda: speck_block_page(*size, fmt),
                (blur_params(*params), 229), noop=noop)


def blur_scene_case():  # cuda_filters_test.c:337-383
    def page():
        g = np.full((16, 16), 255, np.uint8)
        for (x, y) in [(1, 5), (2, 5), (1, 6)]:
            g[y, x] = 0
        g[4:8, 8:12] = 0
        return HostImage.from_array(g, A.FMT_GRAY8, abs_black_threshold=64)
    return Case("blurfilter", "scene", A.FMT_GRAY8, page, (blur_params((4, 4), (2, 2), 0.1), 200),
                noop="the reference's scene: its dark pixels lie off the tested block rows' counts, "
                     "the oracle wipes nothing (nor at the reference's intensity 0.5)")


def blur_wide_cases(fmt, width):
    """Rows of 33 .. 112 blocks take the chunked wave resolver (C4's 99), 113
    the generic one."""
    out = []
    for params in BLUR_WIDE_PARAMS:
        bpr = width // params[0][0]
        arm = ("blur.resolve_wave" if bpr <= 32 else
               "blur.resolve_wave_chunked" if bpr <= 112 else "blur.resolve_generic")
        out.append(Case("blurfilter", "wide-%d-%dx%d" % ((width,) + params[0]), fmt,
                        lambda: speck_block_page(width, 300, fmt, seed=7),
                        (blur_params(*params), 229), arms=(arm,)))
    return out


def blur_arm_cases():
    """The generic counts kernel on a gray plane: W > 65536, and a scan height
    above 65535 (which no image of such a page can fill: its one row of counts
    is the first loop's, and no block is ever tested)."""
    return [
        Case("blurfilter", "w65600", A.FMT_GRAY8,
             lambda: speck_block_page(65600, 40, A.FMT_GRAY8, seed=8, density=0.0005),
             (blur_params((40, 20), (40, 10), 0.05), 229),
             arms=("blur.counts_generic", "blur.resolve_generic_hbm")),
        Case("blurfilter", "sh65536", A.FMT_GRAY8,
             lambda: speck_block_page(120, 40, A.FMT_GRAY8, seed=9),
             (blur_params((40, 65536), (40, 10), 0.05), 229),
             noop="scan height above the page: no block is tested",
             arms=("blur.counts_generic",)),
        # the generic resolver with 23 115 counted rectangles (115 blocks a
        # row, 200 block rows): more than LDS holds (the resolver once staged
        # them there whatever their number; beyond the CU's 160 KiB its launch
        # failed and the filter wiped nothing)
        Case("blurfilter", "rows200", A.FMT_GRAY8,
             lambda: speck_block_page(4600, 2000, A.FMT_GRAY8, seed=10),
             (blur_params((40, 10), (40, 5), 0.05), 229),
             work={"changed": 5000}, arms=("blur.resolve_generic_hbm",)),
    ]


# -------------------------------------------------------------- noisefilter
NOISE_PAGE_SIZES = [((300, 200), 1, 400), ((640, 480), 2, 3000), ((129, 257), 3, 800),
                    ((1000, 700), 4, 6000)]
NOISE_INTENSITIES = [4, 2, 6]
NOISE_SALT = [(0.12, 4), (0.3, 4), (0.3, 2), (0.55, 3)]
NOISE_GROUP_CAPS = [(40000, 4), (40000, 2), (6000, 4), (800, 3), (800, 4)]
NOISE_QUIRK_INTENSITIES = [1, 2, 3, 4]


def noise_scene_cases():
    """cuda_filters_test.c:42-90"""
    def blank(w, h, fmt, thr, dots, blocks=()):
        def page():
            shape = {A.FMT_RGB24: (h, w, 3), A.FMT_Y400A: (h, w, 2)}.get(fmt, (h, w))
            a = np.full(shape, 255, np.uint8)
            for (x, y, v) in dots:
                a[y, x] = v
            for (x0, y0, x1, y1, v) in blocks:
                a[y0:y1 + 1, x0:x1 + 1] = v
            return HostImage.from_array(a, fmt, abs_black_threshold=thr)
        return page
    noise = ([(5, 5, 0)], [(15, 10, 17, 12, 0)])
    diag = ([(2 + i, 2 + i, 0) for i in range(4)] +
            [(12 + dx, 12 + dy, 0) for dx, dy in [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)]] +
            [(24, 6, 0), (25, 6, 0)], [])
    return [
        Case("noisefilter", "scene-2", A.FMT_GRAY8, blank(32, 24, A.FMT_GRAY8, 64, *noise), (2, 200)),
        Case("noisefilter", "scene-diag-4", A.FMT_GRAY8, blank(32, 24, A.FMT_GRAY8, 64, *diag), (4, 200)),
        Case("noisefilter", "scene-diag-3", A.FMT_GRAY8, blank(32, 24, A.FMT_GRAY8, 64, *diag), (3, 200)),
        Case("noisefilter", "scene-3", A.FMT_Y400A, blank(20, 16, A.FMT_Y400A, 64, *noise), (3, 180)),
        Case("noisefilter", "scene-rgb", A.FMT_RGB24,
             blank(32, 24, A.FMT_RGB24, 64, [(4, 4, (30, 0, 0)), (5, 4, (28, 0, 0))],
                   [(14, 10, 16, 12, (20, 40, 60))]), (2, 200)),
    ]


def noise_page_case(fmt, size, seed, specks, intensity):
    # dense specks -> many clustered (sequentially resolved) components; specks
    # touch the left/top edge -> the unsigned-loop quirk zone
    return Case("noisefilter", "%dx%d-%d" % (size + (intensity,)), fmt,
                lambda: make_image(*size, fmt, seed=seed, specks=specks, margin=0),
                (intensity, 229))


def noise_salt_case(fmt, density, intensity):
    # so many small components per 64x64 tile that the classify kernel's LDS
    # work lists overflow and it takes its row-loop path
    def page():
        rng = np.random.default_rng(int(density * 100) + intensity)
        g = np.where(rng.random((230, 301)) < density, rng.integers(0, 200, (230, 301)), 255)
        return gray3(g.astype(np.uint8), fmt)
    return Case("noisefilter", "salt-%g-%d" % (density, intensity), fmt, page, (intensity, 229))


def noise_edge_quirk_case():
    # components hugging x < level / y < level-1, where the reference's ring
    # loops skip whole rows (int32 vs uint32 comparison)
    def page():
        g = np.full((40, 50), 255, np.uint8)
        for (x, y) in [(0, 0), (1, 0), (0, 5), (1, 6), (2, 10), (0, 20), (3, 1), (10, 0), (11, 1),
                       (20, 2), (21, 2), (22, 2), (2, 30), (2, 31), (3, 31), (4, 31), (1, 32)]:
            g[y, x] = 0
        return HostImage.from_array(g, A.FMT_GRAY8)
    return Case("noisefilter", "edge-quirk", A.FMT_GRAY8, page, (4, 229))


def noisy_scan(w, h, page, specks, seed, quality=75, border=True, dashes=True):
    """A synthetic page made to look like a poor scan: clustered 1-px specks
    (sequentially resolved components), a ragged dark left border (the
    edge zone; its interior is the no-op triggers k_noise_classify drops), a
    dashed rule in the top zone (one row of several hundred triggers), all
    through a JPEG round trip (compression noise)."""
    from PIL import Image
    from unpaper_hip.pipeline import synth_page_host
    g = synth_page_host(w, h, page).copy()
    rng = np.random.default_rng(seed)
    ys, xs = rng.integers(0, h, specks), rng.integers(0, w, specks)
    g[ys, xs] = rng.integers(0, 120, specks)
    if border:
        edge = 20 + rng.integers(0, 12, h)
        for y in range(h):
            g[y, :edge[y]] = 30
    if dashes:
        g[3, 40::2] = 0
        g[9, 100::3] = 10
    b = io.BytesIO()
    Image.fromarray(g).save(b, "JPEG", quality=quality)
    return np.asarray(Image.open(io.BytesIO(b.getvalue()))).copy()


def noise_group_caps_case(fmt, specks, intensity):
    # more than 4096 sequential triggers (k_noise_group<FMT, 256>'s global
    # layout) at every speck count -- 16.5k with 800 specks, 20k with 6000, 51k
    # with 40000: the JPEG noise around the border and the rules adds the rest;
    # the LDS layout is left to the smaller pages -- all with rows of more than
    # 256 triggers (the dashed rules: the block-wide bucket sort)
    c = Case("noisefilter", "caps-%d-%d" % (specks, intensity), fmt,
             lambda: gray3(noisy_scan(1240, 1754, 3, specks, specks + intensity), fmt),
             (intensity, 229), arms=("noise.group_256", "noise.buckets_rows"))
    c.triggers = (4097, None)
    return c


def noise_quirk_strip_case(intensity):
    # a solid border band with thin spurs reaching into the quirk strip
    # (x < 7, y < 6) at every column 6..9 and row 5..8 of its edge: the no-op
    # trigger test must leave those in the sequence
    def page():
        g = np.full((300, 400), 255, np.uint8)
        g[:, :25] = 0
        g[:40, :] = 0
        for y in range(45, 300, 7):
            g[y, 25:25 + (y % 11)] = 0      # spurs off the band's edge
            g[y + 1, 3] = 255               # notches inside the quirk strip
        g[50:60, 0:2] = 255
        g[2, 100:300:2] = 255
        for i, x in enumerate(range(6, 10)):     # notches and spurs at x = 6..9 ...
            g[70 + 9 * i, x] = 255
            g[40:43 + i, 60 + 20 * i + x] = 0    # ... hanging off the top band
        for i, y in enumerate(range(5, 9)):      # ... and at y = 5..8
            g[y, 120 + 9 * i] = 255
            g[110 + 20 * i + y, 25:28 + i] = 0
        for n in range(1, 6):                    # lone components of 1..5 pixels
            g[150 + 12 * n, 200:200 + n] = 0
            g[150 + 12 * n:150 + 13 * n, 300] = 0
        return HostImage.from_array(g, A.FMT_GRAY8)
    return Case("noisefilter", "quirk-strip-%d" % intensity, A.FMT_GRAY8, page, (intensity, 229))


def salted_array(w, h, seed, salt, edge=0.0, edge_zone=32, clusters=0):
    """White paper with `salt` of its pixels dark, one by one; the first
    edge_zone columns and rows at density `edge` (the noisefilter's edge zone,
    resolved in sequence); `clusters` dark 3 x 3 blobs."""
    rng = np.random.default_rng(seed)
    g = np.full((h, w), 255, np.uint8)
    m = rng.random((h, w)) < salt
    if edge:
        m[:edge_zone] |= rng.random((edge_zone, w)) < edge
        m[:, :edge_zone] |= rng.random((h, edge_zone)) < edge
    g[m] = rng.integers(0, 200, size=int(m.sum()), dtype=np.uint8)
    for _ in range(clusters):
        x, y = int(rng.integers(0, w - 3)), int(rng.integers(0, h - 3))
        g[y:y + 3, x:x + 3] = 40
    return g


# (name, salt, edge density, intensity, triggers: lower and upper bound)
NOISE_BIG = [("lds", 0.0002, 0.02, 4, 4097, 16384),
             ("big", 0.01, 0.2, 4, 16385, None),
             ("allseq", 0.0005, 0.0, 6, 4097, None)]
NOISE_BIG_SIZE = (4000, 4200)    # > 16 Mpixel, H > 4096
NOISE_TALL_SIZE = (300, 4200)


def noise_big_case(fmt, name, salt, edge, intensity, lo, hi):
    """k_noise_group<FMT, 1024> (sheets above 16 Mpixel) with the triggers in
    its LDS layout, beyond it, and every dark pixel in sequence (intensity 6);
    H > 4096: two rows a bucket."""
    w, h = NOISE_BIG_SIZE
    c = Case("noisefilter", "1024-" + name, fmt,
             lambda: gray3(salted_array(w, h, 11, salt, edge, clusters=200), fmt), (intensity, 229),
             arms=("noise.group_1024", "noise.buckets_shifted"))
    c.triggers = (lo, hi)
    return c


# (name, salt, edge density, triggers: lower and upper bound)
NOISE_TALL = [("lds", 0.0005, 0.01, 1, 4096), ("big", 0.01, 0.2, 4097, None)]


def noise_tall_case(fmt, name, salt, edge, lo, hi):
    """k_noise_group<FMT, 256> with two rows a bucket (H > 4096), in its LDS
    layout and beyond it."""
    w, h = NOISE_TALL_SIZE
    c = Case("noisefilter", "256-tall-" + name, fmt,
             lambda: gray3(salted_array(w, h, 12, salt, edge, clusters=50), fmt), (4, 229),
             arms=("noise.group_256", "noise.buckets_shifted"))
    c.triggers = (lo, hi)
    return c


# -------------------------------------------------------------- blackfilter
def black_params(size=(20, 20), step=(5, 5), depth=(500, 500), thr=242, intensity=20,
                 direction=(True, True), exclusions=()):
    p = default_options().blackfilter_parameters
    p.scan_size = A.RectangleSize(*size)
    p.scan_step = A.Delta(*step)
    p.scan_depth.horizontal, p.scan_depth.vertical = depth
    p.abs_threshold = thr
    p.intensity = intensity
    p.scan_direction = A.Direction(*direction)
    p.exclusions_count = len(exclusions)
    for i, e in enumerate(exclusions):
        p.exclusions[i] = A.rect(*e)
    return p


def black_scene_case():  # cuda_filters_test.c:249-290
    def page():
        g = np.full((24, 32), 255, np.uint8)
        g[:, 8:12] = 0
        return HostImage.from_array(g, A.FMT_GRAY8, abs_black_threshold=128)
    return Case("blackfilter", "scene", A.FMT_GRAY8, page,
                (black_params((4, 4), (2, 2), (32, 24), int(255 * np.float32(0.9)), 2),),
                work={"blackfilter_fills": 1})


# (x0, x1, y0, y1): bands a bar of 20 x 500 (the top stripe) finds: down the
# left edge, along the top, at the right edge ending inside the page, and an
# inner column left of the exclusion
BLACK_BANDS = [(0, 40, 0, 700), (0, 600, 0, 25), (560, 600, 0, 520), (100, 130, 0, 700)]
BLACK_BAND_EXCLUSION = (150, 175, 449, 524)


def band_page(w, h, fmt, band, seed, noise=True):
    rng = np.random.default_rng(seed)
    g = make_image(w, h, A.FMT_GRAY8, seed=seed).to_gray()
    x0, x1, y0, y1 = band
    g[y0:y1, x0:x1] = rng.integers(0, 11, size=(y1 - y0, x1 - x0)) if noise else 0
    if fmt == A.FMT_Y400A:
        return HostImage.from_array(np.stack([g, np.full_like(g, 255)], axis=2), fmt)
    if fmt in MONO:
        return HostImage.from_array(g >= 128, fmt)      # 1-bit: white where gray >= 128
    return gray3(g, fmt)


def black_band_case(fmt, band):
    return Case("blackfilter", "band-%d-%d-%d-%d" % band, fmt,
                lambda: band_page(600, 700, fmt, band, seed=8),
                (black_params(exclusions=[BLACK_BAND_EXCLUSION]),),
                work={"blackfilter_fills": 1, "changed": 5000})


BLACK_IRREGULAR_INTENSITIES = [20, 1, 3]
BLACK_IRREGULAR_SIZES = [(300, 400), (123, 77)]


def black_irregular_case(intensity, size):
    """Dark blobs with holes, gaps and stray strokes: the fill order matters.
    The bars (20 x 100 across the top, 100 x 20 down the left) find the band
    down the left edge; the short page, lower than a bar is deep, carries a
    block its left stripe's bars find instead."""
    def page():
        rng = np.random.default_rng(intensity + size[0])
        w, hh = size
        g = np.full((hh, w), 255, np.uint8)
        if hh >= 100:
            g[:, :25] = rng.integers(0, 12, size=(hh, 25))
        else:
            g[12:62, :104] = rng.integers(0, 6, size=(50, 104))
        for _ in range(40):
            y, x = int(rng.integers(0, hh)), int(rng.integers(0, 30))
            g[y:y + int(rng.integers(1, 5)), x:x + int(rng.integers(1, 25))] = rng.integers(0, 200)
        g[rng.random((hh, w)) < 0.02] = 0
        return HostImage.from_array(g, A.FMT_GRAY8)
    return Case("blackfilter", "irregular-%dx%d-%d" % (size + (intensity,)), A.FMT_GRAY8, page,
                (black_params(intensity=intensity, depth=(100, 100)),),
                work={"blackfilter_fills": 1, "changed": 2000})


def speck_page(w, h, density, seed, band=(5, 25)):
    """A dark band for the bars to find, and dark specks a fill line can
    reach through up to intensity-1 light pixels: the pattern of the heavy
    C4 sheets, where one fill percolates through the page's salt specks."""
    rng = np.random.default_rng(seed)
    g = np.full((h, w), 255, np.uint8)
    g[:, band[0]:band[1]] = rng.integers(0, 12, size=(h, band[1] - band[0]))
    m = rng.random((h, w)) < density
    g[m] = rng.integers(0, 60, size=int(m.sum()))
    return g, rng


BLACK_PERCOLATION = [(0.08, 20), (0.2, 6), (0.1, 30)]
BLACK_INTENSITY_EDGES = [0, 63, 64, 65, 1000]
BLACK_MASK_MAX = [0, 30, 254]


def black_percolation_case(fmt, density, intensity):
    # thousands of short frames, most with several matching neighbours: the
    # replay's resume-past-the-windows rule and its stack run every path
    def page():
        g, rng = speck_page(400, 300, density, seed=int(density * 1000) + intensity)
        return as_format(g, fmt, rng)
    return Case("blackfilter", "percolation-%g-%d" % (density, intensity), fmt, page,
                (black_params(intensity=intensity, depth=(100, 100)),),
                work={"blackfilter_fills": 1, "flood_fill_max_depth": 20})


def black_intensity_case(intensity):
    # 0: the counter is 0 after the first position whatever it holds (every
    # line empty); 63 / 64 / 65: the window's run test switches from the
    # in-window smear to the cross-window carry; 1000: lines run to the edge
    def page():
        g, rng = speck_page(300, 200, 0.05, seed=intensity)
        return as_format(g, A.FMT_GRAY8, rng)
    return Case("blackfilter", "intensity-%d" % intensity, A.FMT_GRAY8, page,
                (black_params(intensity=intensity, depth=(100, 100)),),
                work={"blackfilter_fills": 1})


def black_long_lines_case(fmt):
    # fill lines over 1024 positions (several round trips a line) and
    # neighbour runs over 512 (several check windows), in both directions
    def page():
        g, rng = speck_page(2600, 1300, 0.01, seed=7, band=(0, 30))
        g[600:606, :] = rng.integers(0, 20, size=(6, 2600))   # a row band across the page
        g[:, 1800:1804] = rng.integers(0, 20, size=(1300, 4))  # a column band down it
        return as_format(g, fmt, rng)
    return Case("blackfilter", "long-lines", fmt, page,
                (black_params(intensity=20, depth=(200, 200)),),
                work={"blackfilter_fills": 1, "changed": 40000}, arms=("black.resolve_long",))


def black_mask_max_case(thr):
    # the image's abs_black_threshold is the fill's match bound (fill.c:85):
    # 0 matches only black, 254 everything but white
    def page():
        g, rng = speck_page(300, 200, 0.05, seed=thr + 1)
        g[rng.random(g.shape) < 0.3] = rng.integers(0, 255)
        if thr == 0:
            g[:, 5:25] = 0      # only black matches: a band the fill can take
        return as_format(g, A.FMT_GRAY8, rng, thr=thr)
    return Case("blackfilter", "mask-max-%d" % thr, A.FMT_GRAY8, page,
                (black_params(intensity=8, depth=(100, 100), thr=200),),
                work={"blackfilter_fills": 1})


def black_two_fills_case(fmt):
    """Two dark blocks in the top stripe, a white gap wider than the fill's
    reach between them: the bars fill twice (blackfilter_fills counts the
    bars found dark; the second block is still dark when its bars come)."""
    def page():
        g, rng = speck_page(400, 300, 0.03, seed=31, band=(0, 24))
        g[:, 200:230] = rng.integers(0, 12, size=(300, 30))
        g[:, 24:60] = 255
        g[:, 160:200] = 255
        g[:, 230:270] = 255
        return as_format(g, fmt, rng)
    return Case("blackfilter", "two-fills", fmt, page,
                (black_params(intensity=8, depth=(100, 100)),),
                work={"blackfilter_fills": 2, "changed": 10000})


BLACK_SHORT_SIZE = (4104, 4096)   # just over 16 << 20 pixels


def black_short_case(fmt):
    """k_black_resolve<FMT, false>: a sheet over 16 Mpixel whose fill
    percolates through salt specks, a row band and a column band across it."""
    def page():
        w, h = BLACK_SHORT_SIZE
        g, rng = speck_page(w, h, 0.05, seed=41)
        g[2000:2006, :] = rng.integers(0, 20, size=(6, w), dtype=np.uint8)
        g[:, 3000:3004] = rng.integers(0, 20, size=(h, 4), dtype=np.uint8)
        return as_format(g, fmt, rng)
    return Case("blackfilter", "short-16M", fmt, page,
                (black_params(intensity=20, depth=(200, 200)),),
                work={"blackfilter_fills": 1, "flood_fill_calls": 100000, "changed": 100000},
                arms=("black.resolve_short",))


def staircase(g, x, y, steps, dx=1):
    """A 1-px staircase from (x, y): 3 px along x (dx: its sign), 3 px down,
    the next step 2 px on in both: two stack frames a step."""
    for _ in range(steps):
        for k in range(3):
            g[y, x + dx * k] = 0
        for k in range(3):
            g[y + k, x + dx * 2] = 0
        x += 2 * dx
        y += 2
    return x, y


def stairs_array(w, h, flights):
    """A 20-px dark band down the left edge and staircases off it:
    flights = [(y0, steps), ...]."""
    g = np.full((h, w), 255, np.uint8)
    g[:, :20] = 0
    for y0, steps in flights:
        staircase(g, 20, y0, steps)
    return g


# (name, size, flights, frames deep at least / at most)
BLACK_STAIRS = [("spill", (1230, 1215), [(5, 600)], 1025, None),
                ("control", (630, 615), [(5, 300)], 600, 1023),
                ("spill-twice", (1230, 2430), [(5, 600), (1215, 600)], 1025, None)]


def black_stairs_case(name, size, flights, lo, hi, fmt=A.FMT_GRAY8):
    """The resolve's DFS stack beyond its 1024 frames in LDS (deeper frames
    live in HBM): a staircase is two frames a step deep."""
    c = Case("blackfilter", "stairs-" + name, fmt,
             lambda: gray3(stairs_array(*size, flights), fmt),
             (black_params(intensity=1, depth=(100, 100)),),
             work={"blackfilter_fills": 1, "flood_fill_max_depth": lo},
             arms=("black.resolve_long",))
    c.max_depth = hi
    return c


def black_stairs_short_case():
    """The same staircase inside a sheet over 16 Mpixel: the short-line
    instantiation spills too."""
    def page():
        w, h = BLACK_SHORT_SIZE
        g = np.full((h, w), 255, np.uint8)
        g[:1215, :1230] = stairs_array(1230, 1215, [(5, 600)])
        g[1215:, :20] = 0
        return HostImage.from_array(g, A.FMT_GRAY8)
    c = Case("blackfilter", "stairs-16M", A.FMT_GRAY8, page,
             (black_params(intensity=1, depth=(100, 100)),),
             work={"blackfilter_fills": 1, "flood_fill_max_depth": 1025},
             arms=("black.resolve_short",))
    c.max_depth = None
    return c


# ---------------------------------------------------------------- axis sums
def mask_params(direction=(True, True), thr=0.1, minimum=100, size=20):
    p = default_options().mask_detection_parameters
    p.scan_direction = A.Direction(*direction)
    p.scan_threshold.horizontal = p.scan_threshold.vertical = thr
    p.minimum_width = p.minimum_height = minimum
    p.scan_size = A.RectangleSize(size, size)
    return p


# (format, size, arm of the row sums)
AXIS_PAGES = [(A.FMT_RGB24, (300, 2100), "axis.rowsum_stride"),
              (A.FMT_Y400A, (300, 2100), "axis.rowsum_stride"),
              (A.FMT_GRAY8, (1200, 300), "axis.rowsum_gray_wave"),
              # the arms of the small pages, for the record of what selects them
              (A.FMT_GRAY8, (400, 300), "axis.rowsum_gray"),
              (A.FMT_RGB24, (400, 300), "axis.rowsum")]


def axis_cases(fmt, size, arm):
    """detect_masks and detect_border over pages taller than k_rowsum's 2048
    blocks (its grid-stride loop) and wide enough for k_rowsum_g to give a row
    a whole wave (33 16-byte vectors: 498 columns)."""
    w, h = size
    def page():
        g = page_array(w, h, seed=17, margin=min(w, h) // 6)
        return as_format(g, fmt, np.random.default_rng(17)) if fmt == A.FMT_Y400A else gray3(g, fmt)
    p = mask_params()
    p.maximum_width, p.maximum_height = w, h
    b = default_options().border_scan_parameters
    b.scan_direction = A.Direction(True, True)
    return [Case("masks", "%dx%d" % size, fmt, page,
                 (p, [A.Point(w // 2, h // 2), A.Point(w // 3, h // 3)]), work={"edges": 2},
                 arms=(arm,)),
            Case("border", "%dx%d" % size, fmt, page, (b, A.rect(0, 0, w - 1, h - 1)),
                 work={"edges": 2}, arms=(arm,))]


# ------------------------------------------------------------- every case
def all_cases():
    out = [gray_scene_case()]
    out += [gray_page_case(f, s, p) for p in GRAY_PARAMS for s in GRAY_SIZES for f in FORMATS]
    for black in GRAY_FEEDBACK_BLACK:
        out += gray_feedback_cases(black)
    out += gray_arm_cases()

    out.append(blur_scene_case())
    out += [blur_page_case(f, s, p) for p in BLUR_PARAMS for s in BLUR_SIZES + BLUR_EXTRA_SIZES
            for f in FORMATS]
    for f in (A.FMT_GRAY8, A.FMT_RGB24):
        for w in BLUR_WIDE_WIDTHS:
            out += blur_wide_cases(f, w)
    out += blur_arm_cases()

    out += noise_scene_cases()
    out += [noise_page_case(f, s, seed, specks, i) for i in NOISE_INTENSITIES
            for (s, seed, specks) in NOISE_PAGE_SIZES for f in FORMATS]
    for f in (A.FMT_GRAY8, A.FMT_RGB24):
        out += [noise_salt_case(f, d, i) for (d, i) in NOISE_SALT]
        out += [noise_group_caps_case(f, s, i) for (s, i) in NOISE_GROUP_CAPS]
        out += [noise_big_case(f, *b) for b in NOISE_BIG]
        out += [noise_tall_case(f, *t) for t in NOISE_TALL]
    out.append(noise_edge_quirk_case())
    out += [noise_quirk_strip_case(i) for i in NOISE_QUIRK_INTENSITIES]

    out.append(black_scene_case())
    out += [black_band_case(f, b) for b in BLACK_BANDS for f in FORMATS]
    out += [black_irregular_case(i, s) for s in BLACK_IRREGULAR_SIZES
            for i in BLACK_IRREGULAR_INTENSITIES]
    out += [black_percolation_case(f, d, i) for (d, i) in BLACK_PERCOLATION for f in BYTE_FORMATS]
    out += [black_intensity_case(i) for i in BLACK_INTENSITY_EDGES]
    out += [black_long_lines_case(f) for f in (A.FMT_GRAY8, A.FMT_RGB24)]
    out += [black_mask_max_case(t) for t in BLACK_MASK_MAX]
    out += [black_two_fills_case(f) for f in BYTE_FORMATS]
    out += [black_short_case(f) for f in BYTE_FORMATS]
    out += [black_stairs_case(*s) for s in BLACK_STAIRS]
    out.append(black_stairs_short_case())

    for a in AXIS_PAGES:
        out += axis_cases(*a)
    return out


# Arms no image the ABI can make selects, and why.
UNREACHABLE_ARMS = {
    "blur.counts_gray": "k_blur_counts_g<false> needs a plane that is not 16-byte aligned; every "
                        "frame and batch plane is allocated aligned with a pitch of a multiple of 256",
}
# Arms only a batch selects; tests/test_pipeline_gpu.py runs them (a GRAY8
# batch with the default blurfilter: test_default_gray_batch and others).
BATCH_ARMS = {
    "blur.counts_bits": ("blurfilter", A.FMT_GRAY8, (620, 877), ((100, 100), (50, 50), 0.01), 229),
}


# ------------------------------------------------------------- whole sheet
GRAY_SHEET_SIZE = (620, 877)
GRAY_SHEET_PAGES = (0, 2, 3)


def gray_sheet_page(page):
    """A synthetic A4 page (75 dpi) whose blank paper is light-gray clouds:
    in a GRAY8 batch the grayfilter wipes them and adds what it wipes to the
    column sums the mask detection after it takes (k_gray_wipe's colsum)."""
    from unpaper_hip.pipeline import synth_page_host
    w, h = GRAY_SHEET_SIZE
    g = synth_page_host(w, h, page).copy()
    clouds, _ = cloud_array(w, h, 50 + page, strokes=0)
    g[g == 255] = clouds[g == 255]
    return HostImage.from_array(g, A.FMT_GRAY8)
