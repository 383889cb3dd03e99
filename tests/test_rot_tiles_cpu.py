"""The tile geometry of the GRAY8 bicubic rotation (csrc/rot_tiles.h: the
per-sheet constants, every tile's source window and class, which a small
kernel writes once per launch and the rotation's tiles only read) against a
brute force over pixels on the CPU (tests/c/rot_tiles_check.cpp).

Sizes 128x48, 127x47, 129x49 and 400x560; masks inside the image, touching
each edge, partly outside it and inverted; angles +-0.3, +-2.0, +-2.6, +-2.8
and +-4.9 degrees.  For every tile each in-mask pixel's 4 x 4 taps, from the
row loop's own coordinate expressions, must lie inside the tile's window, and
every flag (outside, partial, staged, interior, posc, full) must equal its
definition.  The header is compiled for the host with plain g++, contraction
off like the device build."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unpaper-gpu_amd", "csrc")


def test_tile_records_match_brute_force(tmp_path):
    exe = str(tmp_path / "rot_tiles_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "c", "rot_tiles_check.cpp"), "-o", exe,
                           "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: "), r.stdout
