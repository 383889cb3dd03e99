#!/usr/bin/env python3
"""Measurements of the TIFF output branch, against PNG, the
measured neighbour (tools/png_bench.py, whose helpers this uses).

  device   64 synthetic A4 GRAY8 sheets of the bench workload after the default
           pipeline: the TIFF encode (Deflate strips) and, in the same run, the
           PNG encode of the same sheets; HIP events on the batch stream around
           each encode, alternating repetitions after warm-up; bytes a page of
           both (what Predictor 2 alone and a table per strip cost against
           PNG's filter choice per row and one table a page).
  files    pages fed from host RAM through the runner into tmpfs:
           sink_tiff_multipage against sink_png and sink_pnm.
  kernels  warm-up and three TIFF encodes only: the run to put under
           `rocprofv3 --kernel-trace --stats -- python tools/tiff_enc_bench.py kernels`.

Prints one JSON line per part.
"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import png_bench as B  # noqa: E402
from unpaper_hip import ctypes_abi as A  # noqa: E402
from unpaper_hip.device import Backend, UnpaperHipError  # noqa: E402
from unpaper_hip.pipeline import (Batch, Runner, sink_png, sink_pnm, sink_tiff_multipage,  # noqa: E402
                                  source_memory, tiff_encode_host)

W, H = B.W, B.H


def device_part(L, n, reps, kernels_only):
    buf, pitch = B.synth(L, n)
    gray = Batch(B.options(L), n, W, H, A.FMT_GRAY8)
    try:
        gray.run_device(n, buf.ptr, pitch, pitch * H)
        gray.wait()
        st = L.uphip_batch_stream(gray.handle)
        for _ in range(3):  # warm-up: the first encode allocates
            gray.encode_tiff()
            gray.wait()
        if kernels_only:
            return {"part": "kernels", "pages": n}
        for _ in range(3):
            gray.encode_png()
            gray.wait()
        t = {"tiff": [], "png": []}
        for _ in range(reps):
            t["tiff"].append(B.timed(gray, st, gray.encode_tiff))
            t["png"].append(B.timed(gray, st, gray.encode_png))
        gray.encode_tiff()
        pages = gray.tiff_pages(n)
        gray.encode_png()
        png = [len(s) for s in gray.png_files(n)]
        sizes = [len(p) for p in pages]
        same = 0
        for s in range(min(4, n)):
            sheet = gray.output(s)
            twin = tiff_encode_host(sheet.data, W, A.FMT_GRAY8)
            same += twin[8:8 + len(pages[s])] == pages[s]
        dev = C.c_int64()
        L.uphip_batch_device_bytes(gray.handle, C.byref(dev))
        return {"part": "device", "pages": n, "reps": reps, "tiff": B.stats(t["tiff"]), "png": B.stats(t["png"]),
                "tiff_series_ms": [round(v, 3) for v in t["tiff"]], "png_series_ms": [round(v, 3) for v in t["png"]],
                "tiff_bytes_a_page": {"mean": int(statistics.mean(sizes)), "min": min(sizes), "max": max(sizes)},
                "png_bytes_a_page": {"mean": int(statistics.mean(png)), "min": min(png), "max": max(png)},
                "tiff_over_png_bytes": round(sum(sizes) / sum(png), 4), "raw": W * H,
                "equal_host_twin": "%d of %d" % (same, min(4, n)), "batch_device_bytes": dev.value}
    finally:
        gray.close()
        buf.close()


def files_part(L, npages, batch, streams, threads):
    host_in = np.empty((npages, H, W), np.uint8)
    for i in range(npages):
        L.uphip_synth_page_host(host_in[i].ctypes.data, W, W, H, i)
    r = Runner(B.options(L), batch, W, H, A.FMT_GRAY8, devices=(0,), streams=streams, host_threads=threads)
    tmpdir = tempfile.mkdtemp(prefix="uphip_tiff_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"part": "files", "pages": npages, "sheets_per_batch": batch, "streams": streams, "host_threads": threads}
    try:
        src = source_memory(host_in.ctypes.data, W, W * H, npages, keep=host_in)
        doc = os.path.join(tmpdir, "doc.tif")
        for name, make in (("pnm", lambda: sink_pnm(os.path.join(tmpdir, "o_%04lld.pgm"), 64)),
                           ("png", lambda: sink_png(os.path.join(tmpdir, "o_%04lld.png"), 64, 300)),
                           ("tiff_multipage", lambda: sink_tiff_multipage(doc, 300))):
            for rep in range(2):  # one untimed warm-up pass
                snk = make()
                t0 = time.perf_counter()
                failed, err = r.run_host(npages, src, snk)
                if name == "tiff_multipage":
                    snk.finish()
                t = time.perf_counter() - t0
                snk.close()
                if failed:
                    raise UnpaperHipError("%s run: %d failed: %s" % (name, failed, err))
            stt = r.stats()
            size = os.path.getsize(doc) / npages if name == "tiff_multipage" else \
                os.path.getsize(os.path.join(tmpdir, "o_0000." + {"pnm": "pgm", "png": "png"}[name]))
            out[name] = {"pages_per_s": round(npages / t, 1), "load_s": round(stt.load_s, 3),
                         "store_s": round(stt.store_s, 3), "kB_a_page": round(size / 1e3)}
        from PIL import Image
        # o_0000.pgm holds the last page whose number is a multiple of the wrap
        last = (npages - 1) // 64 * 64
        with Image.open(doc) as im:
            out["tiff_frames"] = im.n_frames
            im.seek(last)
            back = np.asarray(im)
        ref = np.fromfile(os.path.join(tmpdir, "o_0000.pgm"), np.uint8)[-W * H:].reshape(H, W)
        out["tiff_page%d_equals_pgm" % last] = bool(np.array_equal(back, ref))
    finally:
        r.close()
        shutil.rmtree(tmpdir, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["device", "files"])
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS") or 16))
    args = ap.parse_args()
    L = Backend().lib
    if "kernels" in args.parts:
        print(json.dumps(device_part(L, args.pages, 0, True)), flush=True)
    if "device" in args.parts:
        print(json.dumps(device_part(L, args.pages, args.reps, False)), flush=True)
    if "files" in args.parts:
        print(json.dumps(files_part(L, args.files, args.batch, args.streams, args.threads)), flush=True)


if __name__ == "__main__":
    main()
