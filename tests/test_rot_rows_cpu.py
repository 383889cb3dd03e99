"""How the GRAY8 bicubic rotation deals the rows of a 128 x 48 tile to its
eight waves (csrc/rot_tiles.h rot_wave_row), checked on the CPU
(tests/c/rot_rows_check.cpp): (wave, k) -> tile row is a bijection onto
0 .. kRFH - 1, strictly increasing in k for every wave (the kernel ends a
wave's column sums at its first row below the image), and no band of n
consecutive rows gives a wave more than ceil(n / 8) of them (the balance the
round-robin deal is there for).  The header is compiled for the host with
plain g++, as in test_rot_tiles_cpu.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unpaper-gpu_amd", "csrc")


def test_wave_rows_are_a_bijection_increasing_and_balanced(tmp_path):
    exe = str(tmp_path / "rot_rows_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "c", "rot_rows_check.cpp"), "-o", exe,
                           "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: 48 rows, 8 waves, 6 rows a wave"), r.stdout
