"""The word-level logic of the GRAY8 noisefilter's bit-plane passes
(csrc/noise_planes.h: l3 / candidate / zone words from neighbouring words in
strips of rows, the restricted flood, the verdict over a plane accessor, which
k_noise_cand and k_noise_verdict share) against a per-pixel brute force of the
definitions on the CPU (tests/c/noise_planes_check.cpp).

Sizes 1x1, 31x50, 32x41, 33x200, 65x130, 97x83, 129x257 and 2480x96 (78 words
a row, the last of 16 bits); random salt at densities 0.02, 0.12 and 0.55,
every third pixel in both directions, and hand-placed components across word
boundaries, at the zone and eligibility edges and in the last column, row and
word, at every phase of a strip.  Every word's l3, candidate, zone and small
bits and the seq / clear sets for intensities 2, 3, 4 and 6 must equal the
definitions'.  The header is compiled for the host with plain g++, once as it
is and once under the address and undefined-behaviour sanitizers (a
stand-alone program)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unpaper-gpu_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_planes_match_brute_force(tmp_path, flags):
    exe = str(tmp_path / "noise_planes_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + CSRC] + flags +
                          [os.path.join(ROOT, "tests", "c", "noise_planes_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: "), r.stdout
