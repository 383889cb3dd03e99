"""The GRAY8 noisefilter's bit-plane passes (k_noise_cand, k_noise_verdict;
csrc/noise_planes.h) against the oracle, bit for bit: the filter on its own at
intensities 2, 3, 4 (parallel verdicts) and 6 (everything sequential), and in
the batch pipeline fed from a 256-pitched device buffer, where the fused
decode hands the dark bit-plane on and the sheets lie a stride apart.

The content aims at what a streaming pass over 32-pixel words in strips of
rows can get wrong: components across word boundaries, at the zone (32) and
eligibility (40) edges, in the last column, row and partial word, clustered
candidates at every density, each hand-placed case at every row phase
40..140."""
import numpy as np
import pytest

from unpaper_hip import ctypes_abi as A
from unpaper_hip.hostimage import HostImage
from unpaper_hip.pipeline import Batch, DeviceBuffer, synth_page_host
from helpers import assert_same

pytestmark = pytest.mark.gpu

SIZES = [(33, 200), (200, 33), (64, 64), (65, 130), (97, 83), (2480, 96), (640, 480)]
INTENSITIES = [2, 3, 4, 6]


def placed(g, y0):
    """The hand-placed cases at row phase y0, drawn into g (dark = 0)."""
    h, w = g.shape

    def put(x, y):
        if 0 <= x < w and 0 <= y < h:
            g[y, x] = 0

    y = y0
    for n in range(1, 5):       # 1-4-pixel runs at x = 30..33 and 62..65, 10 rows apart
        for i, x in enumerate((30, 31, 32, 33, 62, 63, 64, 65)):
            for k in range(n):
                put(x + k, y + 10 * (i & 3))
        y += 40
    for n in (4, 5):            # diagonal chains across x = 63 | 64 and 95 | 96
        for k in range(n):
            put(62 + k, y + k)
            put(97 - k, y + k)
        y += 12
    for k in range(3):          # L shapes of 4 and 5 pixels across a word boundary
        put(62 + k, y)
        put(126 + k, y)
    put(62, y + 1)
    put(126, y + 1)
    put(126, y + 2)
    y += 12
    for x1 in (31, 63):         # a 3x3 block ending at x1 with a tail in the next word
        for r in range(3):
            for c in range(3):
                put(x1 - 2 + c, y + r)
        put(x1 + 1, y + 1)
        put(x1 + 2, y + 1)
    y += 12
    for xa, xb, dy in ((60, 67, 0), (92, 100, 0), (124, 131, 1), (156, 164, 1)):
        put(xa, y)              # pairs at Chebyshev 7 and 8, and one row apart
        put(xb, y + dy)
    y += 12
    for e in (0, 8):            # components on x = 31 | 32 and 39 | 40
        put(31 + e, y)
        put(32 + e, y + 3)
        put(31 + e, y + 6)
        put(32 + e, y + 6)
    y += 12
    last = (w - 1) & ~31
    for k in range(2):          # the last column and the partial last word
        put(w - 1, y + 5 * k)
        put(w - 1 - k, y + 2)
        put(last, y + 5 * k)
        put(last - 1, y + 5 * k + 1)
    for x in range(40, w, 9):   # the last rows
        put(x, h - 1)
        if x % 2:
            put(x + 1, h - 2)
    for yy in range(31, 41, 3):  # rows 31 | 32 and 39 | 40
        put(50 + 10 * (yy - 31), yy)
        put(51 + 10 * (yy - 31), yy + (yy & 1))


def salt(w, h, density, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((h, w)) < density, rng.integers(0, 200, (h, w)), 255).astype(np.uint8)


def run(hip, oracle, g, intensity):
    h = HostImage.from_array(np.ascontiguousarray(g), A.FMT_GRAY8)
    d = hip.upload(h)
    hip.noisefilter(d, intensity, 229)
    oracle.noisefilter(h, intensity, 229)
    assert_same(d.to_host(), h)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("intensity", INTENSITIES)
def test_salt_and_placed(hip, oracle, size, intensity):
    w, h = size
    for density in (0.02, 0.12, 0.55):
        run(hip, oracle, salt(w, h, density, w + intensity), intensity)
    g = salt(w, h, 0.004, h + intensity)
    placed(g, 3)
    run(hip, oracle, g, intensity)


@pytest.mark.parametrize("intensity", INTENSITIES)
def test_placed_at_every_row_phase(hip, oracle, intensity):
    # one tall image holds a copy of the cases every 400 rows, each copy one
    # row further down: phases 40..140 in eight images of 13 copies
    for first in range(40, 141, 13):
        phases = list(range(first, min(first + 13, 141)))
        g = np.full((400 * len(phases) + 64, 200), 255, np.uint8)
        for i, p in enumerate(phases):
            placed(g[400 * i:], p)
        run(hip, oracle, g, intensity)


@pytest.mark.parametrize("intensity", INTENSITIES)
def test_every_third_pixel(hip, oracle, intensity):
    # W * H / 9 candidates, all small, all clustered: none clears in parallel
    g = np.full((480, 640), 255, np.uint8)
    g[::3, ::3] = 0
    run(hip, oracle, g, intensity)


@pytest.mark.parametrize("intensity", [2, 4, 6])
def test_pipeline_fused_plane(hip, oracle, intensity):
    w, h = 417, 530
    opts = oracle.default_options()
    opts.noisefilter_intensity = intensity
    arrays = [synth_page_host(w, h, 3).copy(), synth_page_host(w, h, 0).copy(), salt(w, h, 0.01, 9)]
    placed(arrays[0][h // 2:], 40)
    arrays[1][h // 2:] = np.minimum(arrays[1][h // 2:], salt(w, h - h // 2, 0.03, 5))
    placed(arrays[2], 77)
    pages = [HostImage.from_array(a, A.FMT_GRAY8, abs_black_threshold=170) for a in arrays]
    n, pitch = len(pages), (w + 255) // 256 * 256
    host = np.zeros((n, h, pitch), np.uint8)
    for s, p in enumerate(pages):
        host[s, :, :w] = p.payload()
    buf = DeviceBuffer(host.nbytes)
    b = Batch(opts, n, w, h, A.FMT_GRAY8)
    try:
        assert buf.lib.uphip_memcpy_htod(buf.ptr, host.ctypes.data, host.nbytes) == 0
        b.run_device(n, buf.ptr, pitch, pitch * h)
        b.wait()
        outs = [b.output(s) for s in range(n)]
    finally:
        b.close()
        buf.close()
    for s, p in enumerate(pages):
        sheet, fmt, _ = oracle.process_sheet(opts, [p])
        assert_same(outs[s], oracle.convert_for_save(sheet, fmt), "sheet %d" % s)
