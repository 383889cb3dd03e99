"""GPU parity of the gray move kernels (k_move_rect_g16 in its modes,
k_move_chain_g16) with the oracle, over the case table of tests/move_cases.py,
through uphip_move_probe: the launchers the batch's post stage uses, given
their arguments directly.  Everything is byte-exact and count-exact.

A family's test runs all its cases and reports every failing case with the
first wrong byte, its column within its 16-byte vector and the classes the
case was made for, so that a wrong kernel shows as a class of geometry.
"""
import numpy as np
import pytest

import move_cases as MC
from helpers import make_image
from unpaper_hip import ctypes_abi as A
from unpaper_hip.device import UnpaperHipError

pytestmark = pytest.mark.gpu

_PLANES = {}


def planes(oracle, case):
    """(page, centred plane, result) of the oracle, computed once a case."""
    if case.id not in _PLANES:
        _PLANES[case.id] = case.oracle_planes(oracle)
    return _PLANES[case.id]


def run_probe(hip, case, route=None, **active):
    d = hip.upload(case.page())
    try:
        rows = hip.move_probe(d, case.probe(route, **active))
        return d.to_host().payload().copy(), rows
    finally:
        d.close()


def image_diff(got, want):
    bad = np.argwhere(got != want)
    if not len(bad):
        return None
    y, x = bad[0]
    return "%d bytes differ, first at row %d column %d (byte %d of vector %d): %d, not %d" % (
        len(bad), y, x, x % 16, x // 16, got[y, x], want[y, x])


def rows_diff(got, want):
    bad = np.flatnonzero(got != want)
    if not len(bad):
        return None
    y = bad[0]
    return "%d row counts differ, first row %d: %d, not %d" % (len(bad), y, got[y], want[y])


def check(hip, oracle, case, route=None, **active):
    """The probe's image and rows against the oracle's; a list of complaints."""
    route = case.route if route is None else route
    page, centred, result = planes(oracle, case)
    got, rows = run_probe(hip, case, route, **active)
    want = page if route == MC.DRY else centred if route in (MC.PLAIN, MC.COUNT) else result
    out = [image_diff(got, want)]
    if route in MC.COUNTING:
        out.append(rows_diff(rows, case.expected_rows(centred, route)))
    else:
        assert rows is None
    how = MC.ROUTE_NAMES[route] + "".join(" %s=%d" % kv for kv in sorted(active.items()))
    return ["%s [%s]: %s (made for %s)" % (case.id, how, m, ", ".join(case.classes) or "-")
            for m in out if m]


def check_case(hip, oracle, case):
    bad = check(hip, oracle, case)
    # an identity given as active equals the same switched off
    fc, fa = case.forced
    if fc:
        bad += check(hip, oracle, case, center_active=0)
    if fa:
        bad += check(hip, oracle, case, align_active=0)
    if case.route == MC.CHAIN:
        # the same through an intermediate plane: tells a wrong chain from
        # wrong moves
        bad += check(hip, oracle, case, MC.TWO_PASS)
        a, ra = run_probe(hip, case)
        b, rb = run_probe(hip, case, MC.TWO_PASS)
        m = image_diff(a, b)
        if m:
            bad.append("%s: chain against two passes: %s" % (case.id, m))
        counted = case.counted_rows()
        m = rows_diff(ra[counted], rb[counted])
        if m:
            bad.append("%s: chain against two passes: %s" % (case.id, m))
    return bad


@pytest.mark.parametrize("family", MC.FAMILIES)
def test_moves_equal_oracle(hip, oracle, family):
    cases = MC.family_cases(family)
    assert cases
    bad = []
    for case in cases:
        bad += check_case(hip, oracle, case)
    assert not bad, "%d complaints:\n%s" % (len(bad), "\n".join(bad[:40]))


def test_dry_pass_leaves_unreached_rows_at_the_sentinel(hip, oracle):
    """only = 0: nothing is counted, every row stays unwritten; row ranges:
    the rows between them do."""
    seen = 0
    for case in MC.all_cases():
        if case.route != MC.DRY or case.counted_rows().all():
            continue
        _, rows = run_probe(hip, case)
        assert (rows[~case.counted_rows()] == A.MOVE_ROW_UNWRITTEN).all(), case.id
        assert (rows[case.counted_rows()] != A.MOVE_ROW_UNWRITTEN).all(), case.id
        seen += 1
    assert seen >= 4


# ---------------------------------------------------------------- refusals
def _a_case(route, **kw):
    return next(c for c in MC.all_cases() if c.route == route and c.m1.active and
                all(getattr(c, k) == v for k, v in kw.items()))


def _refused(hip, d, p, rows=True):
    """The probe returns -1 with the error set, and leaves the image alone."""
    before = d.to_host().payload().copy()
    out = np.zeros(d.size[1], np.uint32)
    import ctypes as C
    rc = hip.lib.uphip_move_probe(d.img, C.byref(p), out.ctypes.data if rows else None)
    err = hip.lib.uphip_last_error()
    hip.lib.uphip_clear_error()
    assert rc == -1 and err, (rc, err)
    assert (d.to_host().payload() == before).all()
    return err.decode()


@pytest.mark.parametrize("fmt", [A.FMT_RGB24, A.FMT_Y400A])
@pytest.mark.parametrize("route", [MC.COUNT, MC.DRY, MC.MASKED, MC.TWO_PASS, MC.CHAIN])
def test_probe_refuses_other_formats(hip, fmt, route):
    case = _a_case(MC.CHAIN, W=97, H=61)
    d = hip.upload(make_image(97, 61, fmt, seed=3))
    assert "refused" in _refused(hip, d, case.probe(route))
    d.close()


def test_probe_moves_other_formats_plainly(hip, oracle):
    """launch_move_rect takes every byte format: the plain route does too."""
    case = _a_case(MC.PLAIN, W=97, H=61)
    for fmt in (A.FMT_RGB24, A.FMT_Y400A):
        h = make_image(97, 61, fmt, seed=4, background=(case.bg1,) * 3)
        d = hip.upload(h)
        assert hip.move_probe(d, case.probe()) is None
        oracle.center_mask(h, A.Point(*case.center["point"]), A.rect(*case.center["area"]))
        assert (d.to_host().payload() == h.payload()).all()
        d.close()


def test_probe_refuses_bad_arguments(hip):
    case = _a_case(MC.CHAIN, W=97, H=61)
    d = hip.upload(case.page())
    # row ranges without a dry pass, a dry pass with a mask: the launcher's refusals
    p = case.probe(MC.COUNT)
    p.ya0, p.ya1 = 0, 32
    assert "refused" in _refused(hip, d, p)
    p = case.probe(MC.TWO_PASS)
    p.yb0, p.yb1 = 32, 61
    assert "refused" in _refused(hip, d, p)
    p = case.probe(MC.DRY)
    p.mask_count, p.mask = 1, A.rect(5, 5, 60, 40)
    assert "refused" in _refused(hip, d, p)
    # the probe's own
    for change in ({"route": 6}, {"route": -1}, {"mask_count": 2}, {"mask_count": -1},
                   {"ya0": -1, "ya1": 8}, {"yb0": 3, "yb1": 62}, {"rx0": -1}, {"rx1": 97}):
        p = case.probe(MC.CHAIN)
        for k, v in change.items():
            setattr(p, k, v)
        _refused(hip, d, p)
    assert "rows_out" in _refused(hip, d, case.probe(MC.COUNT), rows=False)
    with pytest.raises(UnpaperHipError):
        p = case.probe(MC.COUNT)
        p.rx1 = 97
        hip.move_probe(d, p)
    # and it still works afterwards
    got = d.to_host().payload().copy()
    assert (got == case.page().payload()).all()
    hip.move_probe(d, case.probe())
    assert (d.to_host().payload() != got).any()
    d.close()
