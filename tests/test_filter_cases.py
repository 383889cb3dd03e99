"""CPU check of the filter suite's case tables (tests/filter_cases.py): the
parity tests of test_filters_gpu.py compare HIP with the oracle, which proves
something only where the oracle works on the page and where the launcher takes
the kernel the case was made for.  No GPU is used: the oracle runs alone, and
the launchers' choices come from uphip_filter_arms (host only).

  * every case changes at least one pixel in the oracle (or moves a detected
    edge) and meets its own condition on oracle.stats() -- flood depth, fills,
    flood calls -- unless it is declared a no-op with its reason;
  * per filter, over the byte formats, declared no-ops are at most one case in
    ten (the 1-bit grayfilter cases are no-ops by format and not counted);
  * a case made for an arm selects it;
  * the tables together select every arm uphip_filter_arm_names lists, except
    those declared unreachable through the ABI or reached by a batch only;
  * the noisefilter's arm cases hold the number of sequential triggers they
    were made for, counted from csrc/noise_planes.h compiled for the host.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filter_cases as FC
from helpers import BYTE_FORMATS
from unpaper_hip import ctypes_abi as A
from unpaper_hip.device import load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = FC.all_cases()
IDS = [c.id for c in CASES]
_SIZES = {}   # case id -> (width, height, abs_black_threshold), once its page was made


def test_case_ids_unique():
    assert len(set(IDS)) == len(IDS)


def filter_arms(filter, fmt, width, height, params=None, threshold=0, fused=0):
    lib = load_library()
    out = C.create_string_buffer(256)
    n = lib.uphip_filter_arms(filter.encode(), fmt, width, height,
                              C.cast(C.pointer(params), C.c_void_p) if params is not None else None,
                              threshold, fused, out, len(out))
    assert n >= 0, (filter, fmt, width, height)
    names = out.value.decode().split()
    assert len(names) == n
    return names


def case_arms(case):
    if case.id not in _SIZES:
        h = case.page()
        _SIZES[case.id] = (h.width, h.height, h.abs_black_threshold)
    w, h, black = _SIZES[case.id]
    if case.filter == "grayfilter":
        return filter_arms("grayfilter", case.fmt, w, h, case.args[0], black)
    if case.filter == "blurfilter":
        return filter_arms("blurfilter", case.fmt, w, h, case.args[0], case.args[1])
    if case.filter in ("masks", "border"):
        return filter_arms("axis", case.fmt, w, h)
    return filter_arms(case.filter, case.fmt, w, h)


def detected_edges(case, result, width, height):
    """Sides of a detection's result that are not the page's own."""
    if case.filter == "border":
        return sum(1 for v in result.tuple() if v != 0)
    n = 0
    for m in result[1][:result[0]]:
        x0, y0, x1, y1 = m.tuple()
        n += (x0 > 0) + (y0 > 0) + (x1 < width - 1) + (y1 < height - 1)
    return n


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_works_on_case(oracle, case):
    h = case.page()
    _SIZES[case.id] = (h.width, h.height, h.abs_black_threshold)
    mono = case.fmt in FC.MONO
    before = h.to_gray() if mono else h.data.copy()
    oracle.stats_reset()
    result = case.run(oracle, h)
    got = dict(oracle.stats())
    # pixels of a 1-bit page, bytes of the others
    got["changed"] = int(np.count_nonzero((h.to_gray() if mono else h.data) != before))
    if case.filter in ("masks", "border"):
        got["edges"] = detected_edges(case, result, h.width, h.height)
        assert got["changed"] == 0
    if case.noop:
        assert got["changed"] == 0, "declared a no-op (%s) but the oracle changes the page" % case.noop
    for name, least in case.work.items():
        assert got[name] >= least, (name, got[name], least)
    most = getattr(case, "max_depth", None)
    if most is not None:   # a control below a boundary
        assert got["flood_fill_max_depth"] <= most
    arms = case_arms(case)
    for arm in case.arms:
        assert arm in arms, (arm, arms)


@pytest.mark.parametrize("filter", ["grayfilter", "blurfilter", "noisefilter", "blackfilter"])
def test_declared_noops_are_few(filter):
    cases = [c for c in CASES if c.filter == filter and c.fmt in BYTE_FORMATS]
    noops = [c.id for c in cases if c.noop]
    assert len(cases) >= 10
    assert 10 * len(noops) <= len(cases), noops
    for c in CASES:
        if c.noop:
            assert len(c.noop) > 10 and "\n" not in c.noop


def test_mono_grayfilter_cases_kept():
    mono = [c for c in CASES if c.filter == "grayfilter" and c.fmt in FC.MONO]
    assert len(mono) == 2 * len(FC.GRAY_SIZES) * len(FC.GRAY_PARAMS)
    assert all(c.noop for c in mono)


def test_every_arm_has_a_case():
    listed = load_library().uphip_filter_arm_names().decode().split()
    assert len(set(listed)) == len(listed) and listed
    for arm in list(FC.UNREACHABLE_ARMS) + list(FC.BATCH_ARMS):
        assert arm in listed, arm
    # what a case claims: the arm it names, checked against the launcher above
    claimed = {a for c in CASES for a in c.arms}
    # what the tables select, claimed or not
    selected = set()
    for c in CASES:
        selected.update(case_arms(c))
    for arm, (filter, fmt, size, params, thr) in FC.BATCH_ARMS.items():
        assert arm in filter_arms(filter, fmt, *size, FC.blur_params(*params), thr, fused=1)
        assert arm not in selected   # else it needs no batch
    for arm in FC.UNREACHABLE_ARMS:
        assert arm not in selected, arm + " is reachable: give it a case"
    missing = [a for a in listed
               if a not in selected and a not in FC.UNREACHABLE_ARMS and a not in FC.BATCH_ARMS]
    assert missing == [], "arms no case selects"
    assert claimed <= selected <= set(listed)


def test_arms_reject_bad_queries():
    lib = load_library()
    out = C.create_string_buffer(64)
    assert lib.uphip_filter_arms(b"nofilter", A.FMT_GRAY8, 10, 10, None, 0, 0, out, 64) == -1
    assert lib.uphip_filter_arms(b"grayfilter", A.FMT_GRAY8, 10, 10, None, 0, 0, out, 64) == -1
    assert lib.uphip_filter_arms(b"noisefilter", A.FMT_GRAY8, 10, 10, None, 0, 0, out, 4) == -1
    assert lib.uphip_filter_arms(b"noisefilter", A.FMT_GRAY8, 0, 10, None, 0, 0, out, 64) == -1


def test_thresholds_sit_where_the_cases_assume():
    """The arm cases were sized against these boundaries; a moved threshold
    shows here first."""
    g = A.FMT_GRAY8
    assert filter_arms("blackfilter", g, 4096, 4096) == ["black.resolve_long"]
    assert filter_arms("blackfilter", g, 4097, 4096) == ["black.resolve_short"]
    assert filter_arms("noisefilter", g, 4096, 4096) == ["noise.group_256", "noise.buckets_rows"]
    assert filter_arms("noisefilter", g, 4095, 4097) == ["noise.group_256", "noise.buckets_shifted"]
    assert filter_arms("noisefilter", g, 4097, 4096) == ["noise.group_1024", "noise.buckets_rows"]
    p = FC.gray_params((50, 50), (20, 20), 127)
    assert "gray.cells_strips" in filter_arms("grayfilter", g, 16384, 60, p, 170)
    assert "gray.cells_generic" in filter_arms("grayfilter", g, 16385, 60, p, 170)
    assert "gray.cells_generic" in filter_arms("grayfilter", A.FMT_RGB24, 300, 60, p, 170)
    assert "gray.cells_strips" in filter_arms("grayfilter", g, 300, 600,
                                              FC.gray_params((510, 510), (255, 255), 127), 170)
    b = FC.blur_params((40, 20), (40, 10), 0.05)
    assert "blur.counts_gray_v16" in filter_arms("blurfilter", g, 65536, 40, b, 229)
    assert "blur.counts_generic" in filter_arms("blurfilter", g, 65537, 40, b, 229)
    assert "blur.counts_generic" in filter_arms("blurfilter", A.FMT_Y400A, 300, 40, b, 229)
    assert "blur.counts_bits" in filter_arms("blurfilter", g, 300, 40, b, 229, fused=1)
    assert "blur.counts_bits" not in filter_arms("blurfilter", g, 300, 40, b, 255, fused=1)
    assert filter_arms("axis", A.FMT_RGB24, 300, 2048) == ["axis.colsum", "axis.rowsum"]
    assert filter_arms("axis", A.FMT_RGB24, 300, 2049) == ["axis.colsum", "axis.rowsum_stride"]
    # (W + 30) / 16 vectors a row: 33 and more take a whole wave
    assert filter_arms("axis", g, 498, 30) == ["axis.colsum_gray", "axis.rowsum_gray_wave"]
    assert filter_arms("axis", g, 497, 30) == ["axis.colsum_gray", "axis.rowsum_gray"]
    # 1-bit frames are filtered through a GRAY8 proxy
    assert filter_arms("axis", A.FMT_MONOWHITE, 400, 30) == filter_arms("axis", g, 400, 30)


# ------------------------------------------------------ noisefilter triggers
@pytest.fixture(scope="module")
def seq_count(tmp_path_factory):
    """tests/c/noise_seq_count.cpp: the seq and clear sets of
    csrc/noise_planes.h for a gray page, counted on the host."""
    d = tmp_path_factory.mktemp("noise_seq_count")
    exe = str(d / "noise_seq_count")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall",
                           "-I" + os.path.join(ROOT, "unpaper-gpu_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "noise_seq_count.cpp"), "-o", exe])

    def count(gray, white, intensity):
        path = str(d / "page.bin")
        with open(path, "wb") as f:
            f.write(b"%d %d %d %d\n" % (gray.shape[1], gray.shape[0], white, intensity))
            f.write(np.ascontiguousarray(gray).tobytes())
        seq, clear = subprocess.check_output([exe, path], timeout=120).split()
        return int(seq), int(clear)
    return count


TRIGGER_CASES = [c for c in CASES if hasattr(c, "triggers")]


@pytest.mark.parametrize("case", TRIGGER_CASES, ids=[c.id for c in TRIGGER_CASES])
def test_noise_arm_cases_hold_their_triggers(seq_count, case):
    """k_noise_group keeps 16 triggers a thread in LDS: 4096 at 256 threads,
    16384 at 1024; more go through its global layout.  The count is the seq
    set of noise_planes.h, which k_noise_cand / k_noise_verdict queue for
    GRAY8.  The RGB24 cases carry three equal channels: k_noise_classify's
    trigger plane (max(rgb) < white) and dark plane (min(rgb) < white) are then
    this plane, its zone rule (dark, in the zone, not an l3 pixel at x >= 8,
    y >= 7) is the header's, and its verdict outside the zone is the one
    np_verdict restates."""
    h = case.page()
    rgb = h.to_rgb()
    assert (rgb[:, :, 0] == rgb[:, :, 1]).all() and (rgb[:, :, 0] == rgb[:, :, 2]).all()
    intensity, white = case.args
    seq, clear = seq_count(rgb[:, :, 0], white, intensity)
    lo, hi = case.triggers
    assert seq >= lo, (seq, lo)
    if hi is not None:
        assert seq <= hi, (seq, hi)
    if intensity <= 4:
        assert clear > 0    # the parallel clears have work too


# --------------------------------------------------------------- whole sheet
@pytest.mark.parametrize("page", FC.GRAY_SHEET_PAGES)
def test_gray_sheet_needs_its_grayfilter(oracle, page):
    """test_pipeline_gpu.py::test_gray_batch_grayfilter_wipes proves the
    batch's grayfilter (and the column sums it hands to the mask detection)
    only if the oracle's sheet differs without the grayfilter."""
    outs = []
    for disable in (0, A.NO_GRAYFILTER):
        opts = oracle.default_options()
        opts.disable = disable
        sheet, fmt, _ = oracle.process_sheet(opts, [FC.gray_sheet_page(page)])
        outs.append(oracle.convert_for_save(sheet, fmt).payload().copy())
    assert outs[0].shape == outs[1].shape
    assert np.count_nonzero(outs[0] != outs[1]) > 10000
