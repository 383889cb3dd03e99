#!/usr/bin/env python3
"""Measurements of the fixed-sheet mode: pages of their own sizes
centred in one sheet, and the fused fit decode (k_decode_gray_fit).

Device-resident: the bench's synthetic GRAY8 pages are generated in a device
buffer, one batch of --sheets sheets runs --reps times after a warm-up run,
stage times come from uphip_batch_kernel_times.  Parts:

  fit      2400 x 3400 pages into sheet_size 2480 x 3508.  A build with the
           fit decode takes route 2, one without it the copy route (fill,
           k_copy, the filters' own plane passes): run both builds
           (UNPAPER_HIP_LIB) and compare.
  copy     the same on the copy route of this build (rows 8 bytes off the
           16-byte alignment the fused decodes ask for).
  uniform  A4 pages, no sheet_size: the default line's batch (route 1).
  mixed    sizes cycling through A4 -5 % .. +5 % in both dimensions, odd
           offsets included, into sheet_size A4.
  mixed-copy  the same on the copy route.

--skip-band leaves out the synthetic pages with the dark band at the left edge
(every fourth): in a padded sheet the band no longer touches the sheet's edge.

Every part prints one JSON line: the decode route, pages a second, the stage
times a batch, the sum of decode + blackfilter + noisefilter + blurfilter, the
decode's bytes and their share of --hbm-gbs, and a SHA-256 over every output
sheet.  --dump FILE writes the hashes of the parts run, --check FILE compares
them with another run's (another build's, or the copy route's: fit and copy,
mixed and mixed-copy must agree).
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unpaper-gpu_amd", "python"))

from unpaper_hip import ctypes_abi as A  # noqa: E402
from unpaper_hip.device import Backend  # noqa: E402
from unpaper_hip.pipeline import Batch, DeviceBuffer  # noqa: E402
from unpaper_hip.workloads import A4_H, A4_W  # noqa: E402

FUSED = ("decode", "blackfilter", "noisefilter", "blurfilter")
# A4 -5 % .. +5 %: pads and crops in either dimension, odd and even offsets
MIXED = [(A4_W, A4_H), (2356, 3333), (2604, 3683), (2479, 3507), (2481, 3509), (2400, 3600), (2590, 3400),
         (2357, 3508), (2480, 3341), (2603, 3682), (2433, 3471)]


def run_part(L, name, args):
    o = A.Options()
    L.uphip_options_init(C.byref(o))
    n = args.sheets
    if name in ("fit", "copy"):
        sizes = [(2400, 3400)] * n
        o.sheet_size = A.RectangleSize(A4_W, A4_H)
    elif name == "uniform":
        sizes = [(A4_W, A4_H)] * n
    else:
        sizes = [MIXED[i % len(MIXED)] for i in range(n)]
        o.sheet_size = A.RectangleSize(A4_W, A4_H)
    gw, gh = max(w for w, _ in sizes), max(h for _, h in sizes)
    pitch = (gw + 255) // 256 * 256 + (8 if name.endswith("copy") else 0)
    stride = pitch * gh
    buf = DeviceBuffer(stride * n + 256)
    b = Batch(o, n, gw, gh, A.FMT_GRAY8, timing=True)
    try:
        for i, (w, h) in enumerate(sizes):
            page = 4 * (i // 3) + i % 3 if args.skip_band else i
            if L.uphip_synth_pages(buf.ptr + i * stride, pitch, stride, w, h, page, 1) != 0:
                raise RuntimeError("synth_pages failed")
            if (w, h) != (gw, gh):
                b.set_page_size(i, 0, w, h)
        b.run_device(n, buf.ptr, pitch, stride)  # warm-up
        b.wait()
        b.stage_times()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            b.run_device(n, buf.ptr, pitch, stride)
        b.wait()
        dt = time.perf_counter() - t0
        stages = {k: round(v / args.reps, 4) for k, v in b.stage_times()}
        route = b.decode_route() if hasattr(L, "uphip_batch_decode_route") else None
        sha = hashlib.sha256()
        for s in range(n):
            sha.update(b.output(s).payload().tobytes())
        sw, sh = b.out_width, b.out_height
        # the fused decodes read the placed page once and write the sheet and
        # three bit-planes of it
        placed = sum(min(w, sw) * min(h, sh) for w, h in sizes)
        moved = placed + n * (sw * sh + 3 * ((sw + 31) // 32) * 4 * sh)
        out = dict(part=name, skip_band=args.skip_band, lib=os.environ.get("UNPAPER_HIP_LIB", "lib"), route=route,
                   sheets=n, reps=args.reps, pages_per_s=round(n * args.reps / dt, 1), stage_ms_per_batch=stages,
                   fused_ms_per_batch=round(sum(stages.get(k, 0.0) for k in FUSED), 4), sha256=sha.hexdigest())
        if route in (1, 2):
            out["decode_MB_per_batch"] = round(moved / 1e6, 1)
            out["decode_hbm_fraction"] = round(moved / (stages["decode"] * 1e-3) / (args.hbm_gbs * 1e9), 3)
        return out
    finally:
        b.close()
        buf.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["fit"])
    ap.add_argument("--sheets", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM peak the decode's rate is set against")
    ap.add_argument("--skip-band", action="store_true")
    ap.add_argument("--dump")
    ap.add_argument("--check")
    args = ap.parse_args()
    L = Backend().lib
    want = json.load(open(args.check)) if args.check else {}
    same = {"copy": "fit", "mixed-copy": "mixed"}  # parts whose sheets must be the same
    hashes, bad = {}, []
    for name in args.parts:
        out = run_part(L, name, args)
        hashes[name] = out["sha256"]
        for other in (name, same.get(name), {v: k for k, v in same.items()}.get(name)):
            ref = want.get(other) or (hashes.get(other) if other != name else None)
            if ref:
                out["verified_against_" + other] = ref == out["sha256"]
                if ref != out["sha256"]:
                    bad.append(name)
        print(json.dumps(out), flush=True)
    if args.dump:
        with open(args.dump, "w") as f:
            json.dump(hashes, f)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
