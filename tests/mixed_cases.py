"""Shared by test_mixed_sizes*.py and test_mixed_runner_gpu.py: the size lists
of the fixed-sheet mode (options.sheet_size fully set: pages of any size up to
the batch geometry's are centred in one sheet, cropped where larger), their
pages and their oracle sheets, computed once per process."""
import numpy as np

from helpers import make_image
from unpaper_hip import ctypes_abi as A

SHEET = (620, 877)
# every placement class into 620 x 877 (the last sheet word is 12 px): the
# identity; a pad of 0 / 1 in x and y; odd and even offsets; a crop in x only,
# in y only, in one with a pad in the other; a page narrower than one 16-byte
# chunk; a single row band; crops in both
LIST1 = [(620, 877), (619, 876), (601, 850), (640, 877), (620, 900), (700, 800), (333, 250), (1, 1),
         (621, 13), (587, 877), (653, 911)]
# every byte offset of the source against the target, tx = 16..0 then
# sx = 1..16, y padded and cropped, into a sheet whose width is whole words
SHEET_OFFSETS = (320, 200)
LIST_OFFSETS = [(288 + 2 * k, 180 + (7 * k) % 41) for k in range(33)]
# a last word of 29 px (>= 16: a whole chunk and a partial one)
SHEET_TAIL = (317, 211)
LIST_TAIL = [(301, 190), (317, 211), (333, 230), (318, 13), (5, 211)]
# two pages a sheet
SHEET_DOUBLE = (1240, 877)
LIST_DOUBLE = [((601, 850), (640, 900)), ((620, 877), (333, 250))]
# the other formats, on the copy route
LIST_FORMATS = [(620, 877), (619, 876), (601, 850), (653, 800)]


def max_size(sizes):
    return max(w for w, _ in sizes), max(h for _, h in sizes)


def sheet_options(oracle, sheet, **fields):
    o = oracle.default_options()
    o.sheet_size = A.RectangleSize(*sheet)
    for k, v in fields.items():
        setattr(o, k, v)
    return o


def copy_options(o):
    return type(o).from_buffer_copy(bytes(o))


def pages_of(sizes, fmt=A.FMT_GRAY8, seed0=0):
    return [make_image(w, h, fmt, seed=seed0 + i) for i, (w, h) in enumerate(sizes)]


_expected = {}


def expected(oracle, opts, pages, key):
    """(saved frame, report) of the oracle on one sheet's pages; kept under
    `key` so that the tests sharing a list run the oracle once."""
    if key not in _expected:
        sheet, fmt, rep = oracle.process_sheet(opts, pages)
        _expected[key] = (oracle.convert_for_save(sheet, fmt), rep)
    return _expected[key]


def assert_report(rep, erep):
    assert rep.mask_count == erep.mask_count
    for i in range(min(erep.mask_count, A.MAX_PAGES)):
        assert np.float32(rep.rotation[i]).tobytes() == np.float32(erep.rotation[i]).tobytes(), \
            "rotation %d" % i
