"""GPU parity of the filters and rotation detection (filters.c / deskew.c
peers): HIP == oracle bit for bit.  The small hand-made scenes restate the
reference's own unit tests (tests/cuda_filters_test.c:42-383,
tests/cuda_deskew_test.c:18-40); the synthetic pages exercise the default
parameters, order-dependent cases (clustered specks, edge-zone quirks, wipe
feedback on colour tiles, flood fills) and odd geometries.

The filter cases (pages, parameters, what each is for) live in
tests/filter_cases.py; tests/test_filter_cases.py checks on the CPU that the
oracle changes every page it is not declared a no-op on, and that a case made
for one arm of a launcher (a kernel picked by sheet size or geometry) selects
it.  What that test measured in the oracle for the arm cases:

  case                         arms                                  oracle
  blackfilter short-16M        black.resolve_short                   1 fill, 260 366 flood calls, depth 33,
    4104 x 4096, 3 formats                                           124 639 px changed (GRAY8)
  blackfilter stairs-spill     black.resolve_long, stack in HBM      depth 1205, 26 701 px
  blackfilter stairs-control   black.resolve_long, stack in LDS      depth 605, 13 501 px
  blackfilter stairs-spill-twice  two flights of 600 steps           depth 1220, 53 402 px
  blackfilter stairs-16M       black.resolve_short, stack in HBM     depth 1205, 84 321 px
  blackfilter two-fills        (2 fills a sheet)                     2 fills, 16 200 px
  noisefilter 1024-lds         noise.group_1024, buckets_shifted     5 426 triggers, 8 513 px
  noisefilter 1024-big           4000 x 4200                         198 297 triggers, 181 033 px
  noisefilter 1024-allseq        intensity 6                         10 268 triggers, 8 469 px
  noisefilter 256-tall-lds     noise.group_256, buckets_shifted      1 579 triggers, 2 035 px
  noisefilter 256-tall-big       300 x 4200                          38 450 triggers, 20 367 px
  grayfilter ch256             gray.cells_generic                    8 800 / 712 241 px (300x200 / 1001x777)
  grayfilter w16400            gray.cells_generic                    708 260 px
  grayfilter lds-edge-512/513  gray.tiles_lds / gray.tiles_generic   45 287 / 45 413 px (GRAY8)
  blurfilter w65600            blur.counts_generic, resolve_generic_hbm  594 px
  blurfilter rows200           blur.resolve_generic_hbm (23 115 rects)   11 991 px
  blurfilter sh65536           blur.counts_generic                   declared no-op (no block fits)
  masks / border 300 x 2100    axis.rowsum_stride (RGB24, Y400A)     masks y 25..2065, border (0, 10, 1, 61)
  masks / border 1200 x 300    axis.rowsum_gray_wave                 masks (25, 25, 1170, 270), border (45, 0, 21, 1)

blurfilter rows200 differed from the oracle when it was added (the HIP filter
wiped nothing): k_blur_resolve staged every count in LDS, and past the CU's
160 KiB its launch failed unseen.  It now reads the counts in HBM where they
do not fit (blur.resolve_generic_hbm).
"""
import math

import numpy as np
import pytest

import filter_cases as FC
from filter_cases import both
from unpaper_hip import ctypes_abi as A
from unpaper_hip.hostimage import HostImage
from helpers import BYTE_FORMATS, FORMATS, make_image

pytestmark = pytest.mark.gpu


def ids(cases):
    return [c.id for c in cases]


# ---------------------------------------------------------------- noisefilter
def scene_noise():          # cuda_filters_test.c:42-54
    return "scene-"


def scene_noise_diag():     # cuda_filters_test.c:56-75
    return "scene-diag-"


@pytest.mark.parametrize("scene,fmt,size,thr,intensity,white", [
    (scene_noise, A.FMT_GRAY8, (32, 24), 64, 2, 200),
    (scene_noise_diag, A.FMT_GRAY8, (32, 24), 64, 4, 200),
    (scene_noise_diag, A.FMT_GRAY8, (32, 24), 64, 3, 200),
    (scene_noise, A.FMT_Y400A, (20, 16), 64, 3, 180),
])
def test_noisefilter_reference_scenes(hip, oracle, scene, fmt, size, thr, intensity, white):
    case, = [c for c in FC.noise_scene_cases() if c.name == scene() + str(intensity)]
    h = case.page()
    assert (case.fmt, case.args) == (fmt, (intensity, white))
    assert (h.width, h.height, h.abs_black_threshold) == size + (thr,)
    both(hip, oracle, case)


def test_noisefilter_rgb_scene(hip, oracle):  # cuda_filters_test.c:77-90
    both(hip, oracle, FC.noise_scene_cases()[-1])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size,seed,specks", FC.NOISE_PAGE_SIZES)
@pytest.mark.parametrize("intensity", FC.NOISE_INTENSITIES)
def test_noisefilter_pages(hip, oracle, fmt, size, seed, specks, intensity):
    both(hip, oracle, FC.noise_page_case(fmt, size, seed, specks, intensity))


@pytest.mark.parametrize("fmt", [A.FMT_GRAY8, A.FMT_RGB24])
@pytest.mark.parametrize("density,intensity", FC.NOISE_SALT)
def test_noisefilter_dense_salt(hip, oracle, fmt, density, intensity):
    both(hip, oracle, FC.noise_salt_case(fmt, density, intensity))


def test_noisefilter_edge_quirk(hip, oracle):
    both(hip, oracle, FC.noise_edge_quirk_case())


@pytest.mark.parametrize("fmt", [A.FMT_GRAY8, A.FMT_RGB24])
@pytest.mark.parametrize("specks,intensity", FC.NOISE_GROUP_CAPS)
def test_noisefilter_group_caps(hip, oracle, fmt, specks, intensity):
    both(hip, oracle, FC.noise_group_caps_case(fmt, specks, intensity))


@pytest.mark.parametrize("intensity", FC.NOISE_QUIRK_INTENSITIES)
def test_noisefilter_border_quirk_strip(hip, oracle, intensity):
    both(hip, oracle, FC.noise_quirk_strip_case(intensity))


@pytest.mark.parametrize("fmt", [A.FMT_GRAY8, A.FMT_RGB24])
@pytest.mark.parametrize("big", FC.NOISE_BIG, ids=[b[0] for b in FC.NOISE_BIG])
def test_noisefilter_group_1024(hip, oracle, fmt, big):
    both(hip, oracle, FC.noise_big_case(fmt, *big))


@pytest.mark.parametrize("fmt", [A.FMT_GRAY8, A.FMT_RGB24])
@pytest.mark.parametrize("tall", FC.NOISE_TALL, ids=[t[0] for t in FC.NOISE_TALL])
def test_noisefilter_tall_buckets(hip, oracle, fmt, tall):
    both(hip, oracle, FC.noise_tall_case(fmt, *tall))


# ---------------------------------------------------------------- grayfilter
def test_grayfilter_reference_scene(hip, oracle):  # cuda_filters_test.c:296-331
    both(hip, oracle, FC.gray_scene_case())


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", FC.GRAY_SIZES)
@pytest.mark.parametrize("params", FC.GRAY_PARAMS)
def test_grayfilter_pages(hip, oracle, fmt, size, params):
    both(hip, oracle, FC.gray_page_case(fmt, size, params))


@pytest.mark.parametrize("black", FC.GRAY_FEEDBACK_BLACK)
def test_grayfilter_feedback_rgb(hip, oracle, black):
    for case in FC.gray_feedback_cases(black):
        both(hip, oracle, case)


@pytest.mark.parametrize("case", FC.gray_arm_cases(), ids=ids(FC.gray_arm_cases()))
def test_grayfilter_arms(hip, oracle, case):
    both(hip, oracle, case)


# ---------------------------------------------------------------- blurfilter
def test_blurfilter_reference_scene(hip, oracle):  # cuda_filters_test.c:337-383
    both(hip, oracle, FC.blur_scene_case())


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", FC.BLUR_SIZES)
@pytest.mark.parametrize("params", FC.BLUR_PARAMS)
def test_blurfilter_pages(hip, oracle, fmt, size, params):
    both(hip, oracle, FC.blur_page_case(fmt, size, params))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", FC.BLUR_EXTRA_SIZES)
@pytest.mark.parametrize("params", FC.BLUR_PARAMS)
def test_blurfilter_pages_above_one_block(hip, oracle, fmt, size, params):
    both(hip, oracle, FC.blur_page_case(fmt, size, params))


@pytest.mark.parametrize("fmt", [A.FMT_GRAY8, A.FMT_RGB24])
@pytest.mark.parametrize("width", FC.BLUR_WIDE_WIDTHS)
def test_blurfilter_wide_rows(hip, oracle, fmt, width):
    for case in FC.blur_wide_cases(fmt, width):
        both(hip, oracle, case)


@pytest.mark.parametrize("case", FC.blur_arm_cases(), ids=ids(FC.blur_arm_cases()))
def test_blurfilter_arms(hip, oracle, case):
    both(hip, oracle, case)


# ---------------------------------------------------------------- blackfilter
def test_blackfilter_reference_scene(hip, oracle):  # cuda_filters_test.c:249-290
    both(hip, oracle, FC.black_scene_case())


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("band", FC.BLACK_BANDS)
def test_blackfilter_bands(hip, oracle, fmt, band):
    both(hip, oracle, FC.black_band_case(fmt, band))


@pytest.mark.parametrize("intensity", FC.BLACK_IRREGULAR_INTENSITIES)
@pytest.mark.parametrize("size", FC.BLACK_IRREGULAR_SIZES)
def test_blackfilter_irregular(hip, oracle, intensity, size):
    both(hip, oracle, FC.black_irregular_case(intensity, size))


@pytest.mark.parametrize("fmt", BYTE_FORMATS)
@pytest.mark.parametrize("density,intensity", FC.BLACK_PERCOLATION)  # 383, 687, 3818 frames
def test_blackfilter_percolation(hip, oracle, fmt, density, intensity):
    both(hip, oracle, FC.black_percolation_case(fmt, density, intensity))


@pytest.mark.parametrize("intensity", FC.BLACK_INTENSITY_EDGES)
def test_blackfilter_intensity_edges(hip, oracle, intensity):
    both(hip, oracle, FC.black_intensity_case(intensity))


@pytest.mark.parametrize("fmt", [A.FMT_GRAY8, A.FMT_RGB24])
def test_blackfilter_long_lines(hip, oracle, fmt):
    both(hip, oracle, FC.black_long_lines_case(fmt))


@pytest.mark.parametrize("thr", FC.BLACK_MASK_MAX)
def test_blackfilter_mask_max(hip, oracle, thr):
    both(hip, oracle, FC.black_mask_max_case(thr))


@pytest.mark.parametrize("fmt", BYTE_FORMATS)
def test_blackfilter_two_fills(hip, oracle, fmt):
    both(hip, oracle, FC.black_two_fills_case(fmt))


@pytest.mark.parametrize("fmt", BYTE_FORMATS)
def test_blackfilter_short_lines_sheet(hip, oracle, fmt):
    both(hip, oracle, FC.black_short_case(fmt))


@pytest.mark.parametrize("stairs", FC.BLACK_STAIRS, ids=[s[0] for s in FC.BLACK_STAIRS])
def test_blackfilter_stack_spill(hip, oracle, stairs):
    both(hip, oracle, FC.black_stairs_case(*stairs))


def test_blackfilter_stack_spill_short_lines_sheet(hip, oracle):
    both(hip, oracle, FC.black_stairs_short_case())


# ------------------------------------------------------------------ axis sums
@pytest.mark.parametrize("fmt,size,arm", FC.AXIS_PAGES, ids=[a[2] + "-" + FC.NAMES[a[0]]
                                                             for a in FC.AXIS_PAGES])
def test_axis_sum_arms(hip, oracle, fmt, size, arm):
    for case in FC.axis_cases(fmt, size, arm):
        both(hip, oracle, case)


# ---------------------------------------------------------- rotation detection
def skewed_edge(w, h, radians, fmt=A.FMT_GRAY8):  # cuda_deskew_test.c:18-33
    cx = np.float32(w) * np.float32(0.35)
    cy = np.float32(h) / np.float32(2.0)
    m = np.float32(math.tan(np.float32(radians)))
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    black = x >= cx + m * (y - cy)
    g = np.where(black, 0, 255).astype(np.uint8)
    return HostImage.from_array(g if fmt == A.FMT_GRAY8 else np.repeat(g[:, :, None], 3, 2),
                                fmt, abs_black_threshold=128)


def deskew_params(oracle, rng=5.0, step=0.1, dev=1.0, size=1500, depth=0.5,
                  edges=(True, False, True, False)):
    p = oracle.default_options().deskew_parameters
    p.deskewScanRangeRad = np.float32(np.float32(rng) * math.pi / 180.0)
    p.deskewScanStepRad = np.float32(np.float32(step) * math.pi / 180.0)
    p.deskewScanDeviationRad = np.float32(np.float32(dev) * math.pi / 180.0)
    p.deskewScanSize = size
    p.deskewScanDepth = depth
    p.scan_edges = A.Edges(*edges)
    return p


@pytest.mark.parametrize("edges", [(True, False, False, False), (True, False, True, False),
                                   (False, True, False, True), (True, True, True, True)])
def test_detect_rotation_reference_scene(hip, oracle, edges):  # cuda_deskew_test.c:86-108
    h = skewed_edge(241, 179, 2.0 * math.pi / 180.0)
    p = deskew_params(oracle, dev=10.0, size=400, edges=edges)
    mask = A.rect(0, 0, 240, 178)
    r1 = hip.detect_rotation(hip.upload(h), mask, p)
    r2 = oracle.detect_rotation(h, mask, p)
    assert np.float32(r1).tobytes() == np.float32(r2).tobytes()
    if edges[0] and not edges[2]:
        assert abs(r2) > 1e-4


@pytest.mark.parametrize("fmt", [A.FMT_GRAY8, A.FMT_RGB24])
@pytest.mark.parametrize("deg", [0.0, 0.6, -1.3, 3.7])
@pytest.mark.parametrize("mask", [(60, 0, 739, 599), (0, 0, 799, 599), (-20, 30, 820, 560)])
def test_detect_rotation_pages(hip, oracle, fmt, deg, mask):
    # a text block rotated by `deg` (rendered via the reference deskew itself)
    h = make_image(800, 600, fmt, seed=9, margin=90)
    if deg:
        oracle.deskew(h, A.rect(0, 0, 799, 599), float(np.float32(deg * math.pi / 180)),
                      A.INTERP_LINEAR)
    p = deskew_params(oracle, size=400)
    r1 = hip.detect_rotation(hip.upload(h), A.rect(*mask), p)
    r2 = oracle.detect_rotation(h, A.rect(*mask), p)
    assert np.float32(r1).tobytes() == np.float32(r2).tobytes()


@pytest.mark.parametrize("fmt", [A.FMT_GRAY8, A.FMT_RGB24])
@pytest.mark.parametrize("case", ["wide_margin", "wide_range", "scan_all"])
def test_detect_rotation_fallbacks(hip, oracle, fmt, case):
    """Lines the band path cannot finish: content > 128 steps from the mask
    edge, a 40 degree range whose band does not fit LDS, and scan size -1."""
    margin = 330 if case == "wide_margin" else 90
    h = make_image(1200, 900, fmt, seed=21, margin=margin)
    oracle.deskew(h, A.rect(0, 0, 1199, 899), float(np.float32(1.7 * math.pi / 180)),
                  A.INTERP_LINEAR)
    if case == "wide_range":
        p = deskew_params(oracle, rng=40.0, step=2.0, dev=90.0, size=1500)
    elif case == "scan_all":
        p = deskew_params(oracle, size=-1, dev=10.0)
    else:
        p = deskew_params(oracle, size=1500, dev=10.0)
    mask = A.rect(0, 0, 1199, 899)
    r1 = hip.detect_rotation(hip.upload(h), mask, p)
    r2 = oracle.detect_rotation(h, mask, p)
    assert np.float32(r1).tobytes() == np.float32(r2).tobytes()


@pytest.mark.parametrize("fmt", [A.FMT_GRAY8, A.FMT_RGB24])
@pytest.mark.parametrize("case", ["page", "left_edge", "wide_margin", "wide_range", "scan_all",
                                  "all_edges", "small_step"])
def test_rotation_peaks_every_line(hip, oracle, fmt, case):
    """Every (edge, angle) peak of detect_edge_rotation_peak (deskew.c:48-146),
    not only the chosen angle: the band path (segments of the float
    recurrence, u16 slice sums), the direct walks (content > 128 steps in,
    top/bottom edges, bands too wide, lines through X = 0 with many binade
    segments) against the oracle, element for element."""
    w, h, margin, deg = 1200, 900, 90, 1.7
    mask = (0, 0, w - 1, h - 1)  # left lines start at X in [0, 1): they cross X = 0
    kw = dict(size=1500, dev=10.0)
    if case == "page":
        w, h, deg, mask, kw = 800, 600, 0.6, (60, 0, 739, 599), dict(size=400)
    elif case == "wide_margin":
        margin = 330
    elif case == "wide_range":
        kw = dict(rng=40.0, step=2.0, dev=90.0, size=1500)
    elif case == "scan_all":
        kw = dict(size=-1, dev=10.0)
    elif case == "all_edges":
        kw = dict(size=700, dev=10.0, edges=(True, True, True, True))
    elif case == "small_step":
        kw = dict(rng=2.0, step=0.01, dev=10.0, size=1500)
    img = make_image(w, h, fmt, seed=21, margin=margin)
    oracle.deskew(img, A.rect(0, 0, w - 1, h - 1), float(np.float32(deg * math.pi / 180)),
                  A.INTERP_LINEAR)
    p = deskew_params(oracle, **kw)
    got = hip.detect_rotation_peaks(hip.upload(img), A.rect(*mask), p)
    exp = oracle.rotation_peaks(img, A.rect(*mask), p)
    assert got.shape == exp.shape
    # scan size -1 makes maxBlackness negative (255 * -1 * depth): every line
    # stops at once and every peak is 0 in the reference too
    assert exp.any() or case == "scan_all"
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:20]
