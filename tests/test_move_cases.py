"""CPU check of the move suite's case table (tests/move_cases.py): the parity
tests of test_move_gpu.py compare the gray move kernels with the oracle, which
proves something only where the oracle moves pixels and where the table holds
the geometries at which the kernels' address arithmetic branches.  No GPU is
used: the oracle runs alone, and what a case meets is computed from its
arguments and the numpy restatement's source map, never from a kernel.

  * the restatement equals the oracle on every case (the centred plane and
    the result);
  * no case is a no-op in the oracle, except those declared identities, at
    most one case in ten;
  * every class move_cases.required() lists is met by some case, each case
    meets the classes it claims, and a class nobody meets fails by name;
  * every page holds bytes equal to thr and thr + 1 in its counted columns;
  * the probe's record is laid out as its ctypes mirror says.
"""
import ctypes

import numpy as np
import pytest

import move_cases as MC
from unpaper_hip import ctypes_abi as A
from unpaper_hip.device import load_library

CASES = MC.all_cases()
IDS = [c.id for c in CASES]
_FACTS = {}


def case_facts(case):
    if case.id not in _FACTS:
        _FACTS[case.id] = MC.facts(case)
    return _FACTS[case.id]


def test_case_ids_unique():
    assert len(set(IDS)) == len(IDS)


def test_every_family_and_size_has_cases():
    assert {c.family for c in CASES} == set(MC.FAMILIES)
    assert {(c.W, c.H) for c in CASES} == set(MC.SIZES)


def test_colours_differ_and_are_not_the_padding():
    for c in CASES:
        assert len({c.bg1, c.bg2, c.mcol}) == 3 and 0 not in (c.bg1, c.bg2, c.mcol), c.id


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_oracle(oracle, case):
    page, centred, result = case.oracle_planes(oracle)
    sc, sr = MC.sources(case)
    assert (MC.render(sc, page, case) == centred).all()
    assert (MC.render(sr, page, case) == result).all()
    if case.identity:
        assert (result == page).all(), "declared an identity (%s) but the oracle changes the page" \
            % case.identity
    else:
        assert (result != page).any(), "a no-op: the oracle leaves the page as it is"
    # thr and thr + 1 among the counted columns
    cols = page[:, case.rx[0]:case.rx[1] + 1]
    assert (cols == case.thr).any()
    if case.thr < 255:
        assert (cols == case.thr + 1).any()


def test_declared_identities_are_few():
    ids = [c.id for c in CASES if c.identity]
    assert 10 * len(ids) <= len(CASES), ids
    for c in CASES:
        if c.identity:
            assert len(c.identity) > 10 and "\n" not in c.identity


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_meets_its_classes(case):
    met = case_facts(case)
    missing = [k for k in case.classes if k not in met]
    assert missing == [], (missing, sorted(met))


def test_claimed_classes_are_required_ones():
    known = set(MC.required())
    for c in CASES:
        assert set(c.classes) <= known, (c.id, sorted(set(c.classes) - known))


def test_every_class_is_met():
    met = set()
    for c in CASES:
        met |= case_facts(c)
    required = MC.required()
    assert len(set(required)) == len(required)
    missing = [k for k in required if k not in met]
    assert missing == [], "classes no case meets"


def test_forced_identities_exist():
    """An identity given as active must equal the same with active = 0: the
    table holds one for the centring and one for the align move."""
    forced = [c.forced for c in CASES]
    assert any(f[0] for f in forced) and any(f[1] for f in forced)


def test_breakpoints_fit_the_chain_kernel():
    for c in CASES:
        if c.route == MC.CHAIN:
            mk = MC.normalize(c.mask) if c.mask is not None else None
            assert len(MC.chain_breakpoints(c.W, c.H, c.m1, c.m2, mk)) <= 17, c.id


def test_raw_moves_follow_the_reference_terms():
    """center_raw / align_raw against hand-worked targets (k_center_args,
    k_border_assemble: C division towards zero, an identity switched off, a
    centring whose target leaves the image switched off)."""
    m = MC.center_raw(97, 61, {"area": (10, 12, 50, 45), "point": (34, 25)}, 5)
    assert (m.tx, m.ty, m.active) == (14, 8, 1)          # 41 x 34: 34 - 20, 25 - 17
    m = MC.center_raw(97, 61, {"area": (10, 12, 50, 45), "point": (30, 29)}, 5)
    assert (m.tx, m.ty, m.active) == (10, 12, 0)         # the identity
    m = MC.center_raw(97, 61, {"area": (10, 12, 50, 45), "point": (80, 29)}, 5)
    assert m.active == 0                                 # 60 + 41 > 97
    a = {"inside": (30, 20, 60, 40), "outside": (0, 0, 20, 10), "alignment": (0, 0, 0, 0),
         "margin": (7, 3)}
    m = MC.align_raw(97, 61, a, 5)
    assert (m.tx, m.ty, m.active) == (-5, -5, 1)         # (20 - 31) / 2, (10 - 21) / 2 in C
    a.update(alignment=(0, 0, 1, 1), outside=(0, 0, 96, 60))
    m = MC.align_raw(97, 61, a, 5)
    assert (m.tx, m.ty) == (96 - 31 - 7, 60 - 21 - 3)


def test_probe_record_layout():
    lib = load_library()
    assert lib.uphip_abi_sizeof(b"UphipMoveStep") == ctypes.sizeof(A.MoveStep)
    assert lib.uphip_abi_sizeof(b"UphipMoveProbe") == ctypes.sizeof(A.MoveProbe)
    p = CASES[0].probe()
    assert isinstance(p, A.MoveProbe) and p.route == CASES[0].route


def test_expected_rows_of_a_dry_pass():
    case = next(c for c in CASES if c.route == MC.DRY and c.ranges == (0, 40, 61, 100))
    centred = np.zeros((case.H, case.W), np.uint8)
    rows = case.expected_rows(centred)
    n = case.rx[1] - case.rx[0] + 1
    assert (rows[:40] == n).all() and (rows[61:] == n).all()
    assert (rows[40:61] == A.MOVE_ROW_UNWRITTEN).all()
