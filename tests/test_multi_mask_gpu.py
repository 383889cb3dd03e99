"""uphip_batch_get_masks against the oracle, on the sheets the batch takes
today (one or two mask-scan points): every mask of the centring stage's
detection and every rotation's bits, beside the saved frame byte for byte.
The two-point case is mask_cases.py's (two points given explicitly, layout
none); test_multi_mask.py shows on the CPU that it is no no-op."""
import numpy as np
import pytest

from helpers import assert_same
from unpaper_hip import ctypes_abi as A
from unpaper_hip.hostimage import HostImage
from unpaper_hip.pipeline import Batch, synth_page_host
import mask_cases as MC

pytestmark = pytest.mark.gpu

TWO = "f-two-none"


def bits(x):
    return np.float32(x).tobytes()


def run_sheets(b, c, order):
    for slot, s in enumerate(order):
        b.set_input(slot, 0, c.page(s))
    b.run(len(order))
    b.wait()
    return [(b.output(slot), b.report(slot), b.masks(slot)) for slot in range(len(order))]


def assert_sheet(got, exp, what):
    out, rep, (count, masks, rots) = got
    eout, erep, en, emasks, erots = exp
    assert_same(out, eout, what)
    assert rep.mask_count == erep.mask_count == count == en, what
    assert [m.tuple() for m in masks] == emasks[:count], what
    for i in range(min(count, A.MAX_PAGES)):
        assert bits(rep.rotation[i]) == bits(erep.rotation[i]), "%s rotation %d" % (what, i)
    # every index, against the deskew stage restated with the oracle's per-op calls
    assert [bits(r) for r in rots] == [bits(r) for r in erots[:count]], what


@pytest.mark.parametrize("interp", MC.INTERPS)
def test_two_points(hip, interp):
    """Two runs of one batch, the second on the sheets in another order and
    fewer of them: each run's answer is its own sheets'."""
    c = MC.CASES[TWO]
    exp = MC.expected(TWO, A.FMT_GRAY8, interp)
    b = Batch(c.options(interp), MC.SHEETS, *c.size, A.FMT_GRAY8)
    try:
        for order in [(0, 1, 2), (2, 0)]:
            got = run_sheets(b, c, order)
            for slot, s in enumerate(order):
                assert_sheet(got[slot], exp[s], "%s order %r slot %d" % (TWO, order, slot))
    finally:
        b.close()


def test_one_point_default_options(hip, oracle):
    """Layout single, the point the layout gives: the mask and the rotation of
    the oracle's report."""
    opts = oracle.default_options()
    pages = [HostImage.from_array(synth_page_host(620, 877, p), A.FMT_GRAY8) for p in (1, 2)]
    b = Batch(opts, len(pages), 620, 877, A.FMT_GRAY8)
    try:
        for s, p in enumerate(pages):
            b.set_input(s, 0, p)
        b.run(len(pages))
        b.wait()
        for s, p in enumerate(pages):
            _, _, erep = oracle.process_sheet(opts, [p])
            count, masks, rots = b.masks(s)
            assert count == erep.mask_count == 1
            assert masks[0].tuple() == erep.masks[0].tuple()
            assert bits(rots[0]) == bits(erep.rotation[0])
    finally:
        b.close()


def test_capacity_and_refusals(hip):
    """A capacity below the count: the count comes back whole, the arrays
    hold the first `capacity`; null arrays are allowed; a sheet outside the
    batch is refused."""
    c = MC.CASES[TWO]
    b = Batch(c.options(), 1, *c.size, A.FMT_GRAY8)
    try:
        full = run_sheets(b, c, (0,))[0][2]
        count, masks, rots = b.masks(0, capacity=1)
        assert count == 2 and len(masks) == 1 and len(rots) == 1
        assert masks[0].tuple() == full[1][0].tuple() and bits(rots[0]) == bits(full[2][0])
        assert b.lib.uphip_batch_get_masks(b.handle, 0, None, None, 0) == 2
        assert b.lib.uphip_batch_get_masks(b.handle, 1, None, None, 0) == -1
        assert b"batch_get_masks" in b.lib.uphip_last_error()
        b.lib.uphip_clear_error()
        assert b.lib.uphip_batch_get_masks(b.handle, 0, None, None, -1) == -1
        b.lib.uphip_clear_error()
    finally:
        b.close()
