#!/usr/bin/env python3
"""Measurements of the TIFF source.

The bench's synthetic A4 GRAY8 pages, written once as one multi-page LZW TIFF
with libtiff's default strips (PIL) and as PGM files, in tmpfs.

  files    pages a second through the runner into a memory sink, alternating,
           --runs runs each after one warm-up round: uphip_source_tiff with
           UPHIP_TIFF_DEVICE_DECODE, the same file on the host route, and the
           PGM files through uphip_source_pnm.  Every sheet of every run is
           compared with the first PGM run's.
  kernels  one warm-up pass and --reps passes of one 64-page chunk on the
           device route: the run to put under
           `rocprofv3 --kernel-trace --stats -- python tools/tiff_bench.py kernels`.
  trace    the k_tiff_* rows of that run's kernel trace CSV (--csv): launches,
           median and min..max duration of each kernel, the warm-up pass left
           out.

Prints one JSON line per part.
"""
import argparse
import csv
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unpaper-gpu_amd", "python"))

import numpy as np  # noqa: E402

from unpaper_hip import ctypes_abi as A  # noqa: E402
from unpaper_hip.device import Backend, UnpaperHipError  # noqa: E402
from unpaper_hip.hostimage import HostImage  # noqa: E402
from unpaper_hip.pipeline import (Runner, TiffDocument, pnm_write, sink_memory, source_pnm,  # noqa: E402
                                  source_tiff, synth_page_host)
from unpaper_hip.workloads import A4_H, A4_W  # noqa: E402

W, H = A4_W, A4_H


def write_inputs(tmpdir, npages, pgm):
    from PIL import Image
    pages = [synth_page_host(W, H, i) for i in range(npages)]
    ims = [Image.fromarray(p, "L") for p in pages]
    tif = os.path.join(tmpdir, "pages.tif")
    ims[0].save(tif, format="TIFF", compression="tiff_lzw", save_all=True, append_images=ims[1:])
    paths = []
    if pgm:
        for i, p in enumerate(pages):
            paths.append(os.path.join(tmpdir, "p%04d.pgm" % i))
            pnm_write(paths[-1], HostImage.from_array(p, A.FMT_GRAY8))
    d = TiffDocument(tif)
    try:
        info = {"tiff_MB": round(os.path.getsize(tif) / 1e6, 1), "pages": d.page_count,
                "on_device": all(d.on_device(p) for p in range(d.page_count))}
    finally:
        d.close()
    with Image.open(tif) as im:
        info["strips_a_page"] = len(im.tag_v2[273])
        info["rows_per_strip"] = im.tag_v2[278]
    return tif, paths, info


def options(L):
    import ctypes as C
    o = A.Options()
    L.uphip_options_init(C.byref(o))
    return o


def files_part(L, args, tmpdir):
    tif, pgm, info = write_inputs(tmpdir, args.pages, True)
    n = args.pages
    r = Runner(options(L), args.batch, W, H, A.FMT_GRAY8, devices=(0,), streams=args.streams,
               host_threads=args.threads)
    out = dict(part="files", sheets_per_batch=args.batch, streams=args.streams, host_threads=args.threads, **info)
    try:
        ref = np.zeros((n, r.out_height, r.out_linesize), np.uint8)
        got = np.zeros_like(ref)
        sources = (("tiff_device", lambda: source_tiff(tif, A.TIFF_DEVICE_DECODE)),
                   ("tiff_host", lambda: source_tiff(tif, A.TIFF_HOST_DECODE)),
                   ("pgm", lambda: source_pnm(pgm)))

        def run(make, dst):
            snk = sink_memory(dst.ctypes.data, r.out_linesize, r.out_linesize * r.out_height, n, keep=dst)
            src = make()
            t0 = time.perf_counter()
            failed, err = r.run_host(n, src, snk)
            t = time.perf_counter() - t0
            if failed:
                raise UnpaperHipError("%d failed: %s" % (failed, err))
            st = r.stats()
            src.close()
            snk.close()
            return n / t, st.load_s

        run(sources[2][1], ref)  # the reference sheets (and the warm-up of the runner)
        rates = {k: [] for k, _ in sources}
        loads = {k: [] for k, _ in sources}
        equal = True
        for rep in range(args.runs + 1):
            for name, make in sources:
                got[:] = 0
                rate, load = run(make, got)
                equal &= bool(np.array_equal(got, ref))
                if rep:  # round 0 warms every source up
                    rates[name].append(rate)
                    loads[name].append(load)
        for name, _ in sources:
            v = rates[name]
            out[name] = {"pages_per_s": {"median": round(statistics.median(v), 1), "min": round(min(v), 1),
                                         "max": round(max(v), 1)},
                         "load_s_median": round(statistics.median(loads[name]), 3)}
        out["all_sheets_equal_pgm_run"] = equal
    finally:
        r.close()
    return out


def kernels_part(L, args, tmpdir):
    tif, _, info = write_inputs(tmpdir, 64, False)
    r = Runner(options(L), 64, W, H, A.FMT_GRAY8, devices=(0,), streams=1, host_threads=args.threads)
    try:
        out = np.zeros((64, r.out_height, r.out_linesize), np.uint8)
        for _ in range(args.reps + 1):
            snk = sink_memory(out.ctypes.data, r.out_linesize, r.out_linesize * r.out_height, 64, keep=out)
            failed, err = r.run_host(64, source_tiff(tif, A.TIFF_DEVICE_DECODE), snk)
            if failed:
                raise UnpaperHipError("%d failed: %s" % (failed, err))
    finally:
        r.close()
    return dict(part="kernels", reps=args.reps, **info)


def trace_part(path):
    rows = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name", "")
            if "k_tiff_" not in name:
                continue
            key = "k_tiff_strips" if "k_tiff_strips" in name else "k_tiff_rows"
            rows.setdefault(key, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    out = {"part": "trace"}
    for key, v in rows.items():
        ms = [(e - s) / 1e6 for s, e in sorted(v)][1:]  # the first launch is the warm-up pass
        out[key] = {"launches": len(ms), "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
                    "max_ms": round(max(ms), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["files"])
    ap.add_argument("--pages", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS") or 16))
    ap.add_argument("--csv")
    args = ap.parse_args()
    if "trace" in args.parts:
        print(json.dumps(trace_part(args.csv)), flush=True)
    if not set(args.parts) & {"files", "kernels"}:
        return
    L = Backend().lib
    tmpdir = tempfile.mkdtemp(prefix="uphip_tiff_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        if "kernels" in args.parts:
            print(json.dumps(kernels_part(L, args, tmpdir)), flush=True)
        if "files" in args.parts:
            print(json.dumps(files_part(L, args, tmpdir)), flush=True)
    finally:
        shutil.rmtree(tmpdir, ignore_errors=True)


if __name__ == "__main__":
    main()
