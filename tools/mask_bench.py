#!/usr/bin/env python3
"""Measurements of the batch with more than two mask-scan points:
the one-launch mask scan (k_mask_sums_points) against the looped route
(memset + one reduction per point and axis: the kernels a batch of one or two
points uses), in one build, on one batch.

Workloads, --sheets sheets of GRAY8 A4 (2480 x 3508) each, filters off:

  mixed6    mask_cases.py's d-mixed6 scaled by 4: six points, six skewed text
            blocks, two of them pushed together.
  limit100  g-limit's 10 x 10 grid of points scaled to the sheet, a skewed
            text block in every cell (the case itself has the deskew off and
            blobs; here every mask rotates, so that the deskew's cost at 100
            points shows).

Per workload the routes alternate --rounds times (route 0, route 1, route 0,
...); a round is --reps runs of the batch after one warm-up run, timed by the
batch's stage events (uphip_batch_kernel_times).  One JSON line per workload:
per route the mean, least and largest `masks_deskew + masks_center` time of a
batch over the rounds, the mean of every stage, and whether the two routes'
sheets are the same bytes.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unpaper-gpu_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from unpaper_hip import ctypes_abi as A  # noqa: E402
from unpaper_hip.device import Backend  # noqa: E402
from unpaper_hip.hostimage import HostImage  # noqa: E402
from unpaper_hip.pipeline import Batch  # noqa: E402
from unpaper_hip.workloads import A4_H, A4_W  # noqa: E402
import mask_cases as MC  # noqa: E402

SCAN = ("masks_deskew", "masks_center")


def scan_options(L, points, cell, scan, minimum):
    o = A.Options()
    L.uphip_options_init(C.byref(o))
    o.layout = A.LAYOUT_NONE
    o.disable = MC.FILTERS
    o.point_count = len(points)
    for i, (x, y) in enumerate(points):
        o.points[i] = A.Point(x, y)
    mp = o.mask_detection_parameters
    mp.scan_direction = A.Direction(True, True)
    mp.scan_size = A.RectangleSize(scan[0], scan[0])
    mp.scan_step = A.Delta(scan[1], scan[1])
    mp.scan_depth.horizontal, mp.scan_depth.vertical = cell[1], cell[0]
    mp.minimum_width = mp.minimum_height = minimum
    mp.maximum_width, mp.maximum_height = cell
    return o


def mixed6(L):
    c = MC.CASES["d-mixed6"]
    assert (c.size[0] * 4, c.size[1] * 4) == (A4_W, A4_H)
    pages = [np.repeat(np.repeat(c.gray(s)[0], 4, 0), 4, 1) for s in range(MC.SHEETS)]
    o = scan_options(L, [(4 * x, 4 * y) for x, y in c.points], (4 * c.cell[0], 4 * c.cell[1]),
                     (4 * c.scan[0], 4 * c.scan[1]), 200)
    return o, pages


def limit100(L):
    cw, ch = A4_W // 10, A4_H // 10
    pts = [(cw * col + cw // 2, ch * row + ch // 2) for row in range(10) for col in range(10)]
    pages = []
    for s in range(MC.SHEETS):
        rng = np.random.default_rng(900 + s)
        g = np.full((A4_H, A4_W), 255, np.uint8)
        for i, (x, y) in enumerate(pts):
            deg = MC.BASE_DEGS[(i + s) % len(MC.BASE_DEGS)] * (1 if (i + s) % 2 == 0 else -1)
            MC.draw_block(g, x + int(rng.integers(-12, 13)), y + int(rng.integers(-12, 13)),
                          cw * 5 // 8, ch * 5 // 8, deg, rng)
        pages.append(g)
    return scan_options(L, pts, (cw * 9 // 10, ch * 9 // 10), (24, 6), 50), pages


WORKLOADS = {"mixed6": mixed6, "limit100": limit100}


def measure(L, name, args):
    o, pages = WORKLOADS[name](L)
    n = args.sheets
    b = Batch(o, n, A4_W, A4_H, A.FMT_GRAY8, timing=True)
    try:
        def load():
            for s in range(n):
                b.set_input(s, 0, HostImage.from_array(pages[s % len(pages)], A.FMT_GRAY8))

        def round_of(route):
            b.set_mask_scan_route(route)
            load()
            b.run(n)  # warm-up
            b.wait()
            b.stage_times()
            for _ in range(args.reps):
                b.run(n)
            b.wait()
            return {k: v / args.reps for k, v in b.stage_times()}
        rounds = {0: [], 1: []}
        sha = {}
        for r in range(args.rounds):
            for route in (0, 1):
                rounds[route].append(round_of(route))
                if r == 0:
                    h = hashlib.sha256()
                    for s in range(min(n, 2 * len(pages))):
                        h.update(b.output(s).payload().tobytes())
                        h.update(repr([m.tuple() for m in b.masks(s)[1]]).encode())
                    sha[route] = h.hexdigest()
        out = dict(workload=name, points=int(o.point_count), sheets=n, reps=args.reps, rounds=args.rounds,
                   device_bytes=b.device_bytes(), same_sheets=sha[0] == sha[1])
        for route, label in ((0, "one_launch"), (1, "looped")):
            scan = [sum(t.get(k, 0.0) for k in SCAN) for t in rounds[route]]
            stages = {k: round(float(np.mean([t.get(k, 0.0) for t in rounds[route]])), 4)
                      for k in rounds[route][0]}
            out[label] = dict(scan_ms_mean=round(float(np.mean(scan)), 4), scan_ms_min=round(min(scan), 4),
                              scan_ms_max=round(max(scan), 4), stage_ms_per_batch=stages,
                              total_ms=round(sum(stages.values()), 3))
        return out
    finally:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=list(WORKLOADS))
    ap.add_argument("--sheets", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    L = Backend().lib
    bad = False
    for name in args.workloads:
        out = measure(L, name, args)
        bad = bad or not out["same_sheets"]
        print(json.dumps(out), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
