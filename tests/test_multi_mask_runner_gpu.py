"""The runner with more than two mask-scan points: a-row3's three sheets as a
PGM list in, a PGM sink out, the files byte-equal to the oracle's saved
frames.  The runner creates batches, so it takes what they take."""
import os

import numpy as np
import pytest

from unpaper_hip import ctypes_abi as A
from unpaper_hip.pipeline import Runner, pnm_read, pnm_write, sink_pnm, source_pnm
import mask_cases as MC

pytestmark = pytest.mark.gpu


def test_row3_through_the_runner(hip, tmp_path):
    name = "a-row3"
    c, exp = MC.CASES[name], MC.expected(name)
    paths = []
    for s in range(MC.SHEETS):
        p = str(tmp_path / ("in_%d.pgm" % s))
        pnm_write(p, c.page(s))
        paths.append(p)
    r = Runner(c.options(), 2, *c.size, A.FMT_GRAY8, devices=(0,), streams=2, host_threads=2)
    try:
        failed, err = r.run_host(MC.SHEETS, source_pnm(paths), sink_pnm(str(tmp_path / "out_%02d.pgm")))
    finally:
        r.close()
    assert not failed, err
    for s in range(MC.SHEETS):
        out, want = str(tmp_path / ("out_%02d.pgm" % s)), str(tmp_path / ("want_%d.pgm" % s))
        got = pnm_read(out)
        assert (got.width, got.height, got.format) == (exp[s][0].width, exp[s][0].height, A.FMT_GRAY8)
        assert np.array_equal(got.payload(), exp[s][0].payload()), "sheet %d" % s
        pnm_write(want, exp[s][0])
        with open(out, "rb") as f, open(want, "rb") as g:
            assert f.read() == g.read(), "sheet %d: the files differ" % s
