"""The multi-mask cases (mask_cases.py) on the CPU: the oracle really deskews
and centres every mask of every case, the cases made to be order-dependent
are, and the deskew stage restated with the per-op calls (every mask's
rotation; the oracle's report keeps two) equals the oracle's own."""
import numpy as np
import pytest

from unpaper_hip import ctypes_abi as A
import mask_cases as MC


@pytest.mark.parametrize("name", list(MC.CASES))
def test_case_is_no_noop(oracle, name):
    """The deskew and the centring change every sheet, and every point gives
    a mask."""
    c = MC.CASES[name]
    for s in range(MC.SHEETS):
        sheet, _, rep = oracle.process_sheet(c.options(), [c.page(s)])
        plain, _, _ = oracle.process_sheet(c.options(disable=A.NO_DESKEW | A.NO_MASK_CENTER), [c.page(s)])
        assert (sheet.payload() != plain.payload()).any(), "%s sheet %d: a no-op" % (name, s)
        assert rep.mask_count == c.npoints
        n, masks, rots = MC.expected(name)[s][2:]
        assert n == c.npoints
        # what a device parity test compares every mask and rotation with
        # agrees with the oracle's own report where that reports
        assert [rep.masks[i].tuple() for i in range(A.MAX_PAGES)] == masks[:A.MAX_PAGES]
        assert [np.float32(r).tobytes() for r in rots[:A.MAX_PAGES]] == \
            [np.float32(rep.rotation[i]).tobytes() for i in range(A.MAX_PAGES)]
        if not (c.disable & A.NO_DESKEW):
            # both reported rotations are visible skews, but for a blank point's
            assert [float(rep.rotation[i]) != 0.0 for i in range(A.MAX_PAGES)] == \
                [c.blocks[i] is not None for i in range(A.MAX_PAGES)]


def rotated_from_undeskewed(oracle, c, s):
    """Every mask detected and rotated from the image before any deskew, each
    rotated mask put into one result: what the deskew stage gives when no mask
    reads what another wrote."""
    opts = c.options()
    plain, _, _ = oracle.process_sheet(c.options(disable=A.NO_DESKEW | A.NO_MASK_CENTER), [c.page(s)])
    n, masks = oracle.detect_masks(plain, opts.mask_detection_parameters,
                                   [A.Point(*p) for p in c.points])
    out = plain.copy()
    for i in range(n):
        r = oracle.detect_rotation(plain, masks[i], opts.deskew_parameters)
        if r != 0.0:
            tmp = plain.copy()
            oracle.deskew(tmp, masks[i], r, opts.interpolate_type)
            oracle.copy_rectangle(tmp, out, masks[i], masks[i].vertex[0])
    return out


def deskewed(oracle, c, s):
    return oracle.process_sheet(c.options(disable=A.NO_MASK_CENTER), [c.page(s)])[0]


@pytest.mark.parametrize("name", list(MC.CASES))
def test_deskew_stage_restated(oracle, name):
    """mask_cases.deskew_stage (where expected()'s masks and rotations come
    from) leaves the sheet the oracle's own deskew stage leaves."""
    c = MC.CASES[name]
    for s in range(MC.SHEETS):
        pre, rots = MC.deskew_stage(oracle, c, s)
        assert not (pre.payload() != deskewed(oracle, c, s).payload()).any(), s
        assert len(rots) == c.npoints


@pytest.mark.parametrize("name", MC.DEPENDENT)
def test_dependent_cases_depend_on_the_order(oracle, name):
    c = MC.CASES[name]
    differ = [bool((rotated_from_undeskewed(oracle, c, s).payload() !=
                    deskewed(oracle, c, s).payload()).any()) for s in range(MC.SHEETS)]
    assert any(differ), differ
    if name == "c-overlap4":
        assert all(differ), differ


def test_get_masks_in_ctypes_mirror():
    """uphip_batch_get_masks is exported, listed and bound with its five
    arguments."""
    import ctypes as C
    from unpaper_hip.device import EXPORTED, load_library
    assert "uphip_batch_get_masks" in EXPORTED
    f = load_library().uphip_batch_get_masks
    assert f.restype is C.c_int32 and len(f.argtypes) == 5
    # no batch: refused, with an error that names the call
    L = load_library()
    assert f(None, 0, None, None, 0) == -1
    assert b"batch_get_masks" in L.uphip_last_error()
    L.uphip_clear_error()


def test_separate_regions_do_not_depend_on_the_order(oracle):
    """The control of the test above: the same comparison finds the 2 x 2
    grid's masks independent."""
    c = MC.CASES["b-grid4"]
    for s in range(MC.SHEETS):
        assert not (rotated_from_undeskewed(oracle, c, s).payload() !=
                    deskewed(oracle, c, s).payload()).any(), s
