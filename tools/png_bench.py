#!/usr/bin/env python3
"""Measurements of the lossless PNG output branch.

  device      64 synthetic A4 GRAY8 sheets of the bench workload after the
              default pipeline: the PNG encode and, in the same run, the JPEG
              q85 encode of the same sheets and the Group 4 encode of the same
              pages with MONOWHITE output; HIP events on the batch stream
              around each encode, alternating repetitions after warm-up.
  files       pages fed from host RAM through the runner into tmpfs files:
              sink_png against sink_pnm and sink_jp2.
  compression bytes a page against PIL at compress_level 1 and 6 on the same
              pixels: the bench sheets, a tests/helpers.page_array A4 page and
              any PNG files named with --image.
  kernels     warm-up and three PNG encodes only: the run to put under
              `rocprofv3 --kernel-trace --stats -- python tools/png_bench.py kernels`.

Prints one JSON line per part.
"""
import argparse
import ctypes as C
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unpaper-gpu_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from unpaper_hip import ctypes_abi as A  # noqa: E402
from unpaper_hip.device import Backend, UnpaperHipError  # noqa: E402
from unpaper_hip.pipeline import (Batch, DeviceBuffer, Runner, png_encode_host, png_wrap, sink_jp2,  # noqa: E402
                                  sink_png, sink_pnm, source_memory)
from unpaper_hip.workloads import A4_H, A4_W  # noqa: E402

W, H = A4_W, A4_H


def options(L, out_fmt=None):
    o = A.Options()
    L.uphip_options_init(C.byref(o))
    if out_fmt is not None:
        o.output_pixel_format = out_fmt
    return o


def synth(L, n):
    pitch = (W + 255) // 256 * 256
    buf = DeviceBuffer(pitch * H * n)
    if L.uphip_synth_pages(buf.ptr, pitch, pitch * H, W, H, 0, n) != 0:
        raise UnpaperHipError("synth_pages failed")
    return buf, pitch


_hip = None


def hip_runtime():
    """The HIP runtime the library runs on, for events on the batch's stream."""
    global _hip
    if _hip is None:
        try:
            _hip = C.CDLL("libamdhip64.so")
        except OSError:
            _hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
        _hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        _hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        _hip.hipEventSynchronize.argtypes = [C.c_void_p]
        _hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        _hip.hipEventDestroy.argtypes = [C.c_void_p]
    return _hip


def timed(batch, stream, fn):
    """Milliseconds between two events recorded on `stream` around fn()."""
    hip = hip_runtime()
    a, b, ms = C.c_void_p(), C.c_void_p(), C.c_float()
    if hip.hipEventCreate(C.byref(a)) or hip.hipEventCreate(C.byref(b)):
        raise UnpaperHipError("hipEventCreate failed")
    try:
        if hip.hipEventRecord(a, stream):
            raise UnpaperHipError("hipEventRecord failed")
        fn()
        if hip.hipEventRecord(b, stream) or hip.hipEventSynchronize(b):
            raise UnpaperHipError("hipEventRecord failed")
        batch.wait()
        if hip.hipEventElapsedTime(C.byref(ms), a, b):
            raise UnpaperHipError("hipEventElapsedTime failed")
        return ms.value
    finally:
        hip.hipEventDestroy(a)
        hip.hipEventDestroy(b)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def device_part(L, n, reps, kernels_only):
    buf, pitch = synth(L, n)
    gray = Batch(options(L), n, W, H, A.FMT_GRAY8)
    mono = None if kernels_only else Batch(options(L, A.FMT_MONOWHITE), n, W, H, A.FMT_GRAY8)
    try:
        for b in (gray, mono):
            if b is not None:
                b.run_device(n, buf.ptr, pitch, pitch * H)
                b.wait()
        sg = L.uphip_batch_stream(gray.handle)
        for _ in range(3):  # warm-up: the first encode allocates
            gray.encode_png()
            gray.wait()
        if kernels_only:
            return {"part": "kernels", "pages": n}
        sm = L.uphip_batch_stream(mono.handle)
        for _ in range(2):
            gray.encode_jpeg(85, 0)
            gray.wait()
            mono.encode_g4()
            mono.wait()
        t = {"png": [], "jpeg": [], "g4": []}
        for _ in range(reps):
            t["png"].append(timed(gray, sg, gray.encode_png))
            t["jpeg"].append(timed(gray, sg, lambda: gray.encode_jpeg(85, 0)))
            t["g4"].append(timed(mono, sm, mono.encode_g4))
        gray.encode_png()
        streams = gray.png_files(n)
        sizes = [len(s) for s in streams]
        # the first four pages equal the host twin
        same = 0
        for s in range(min(4, n)):
            sheet = gray.output(s)
            same += png_wrap(streams[s], W, H, A.FMT_GRAY8) == png_encode_host(sheet.data, W, A.FMT_GRAY8)
        dev = C.c_int64()
        L.uphip_batch_device_bytes(gray.handle, C.byref(dev))
        out = {"part": "device", "pages": n, "reps": reps, "png": stats(t["png"]), "jpeg_q85": stats(t["jpeg"]),
               "g4": stats(t["g4"]), "png_bytes_a_page": {"mean": int(statistics.mean(sizes)), "min": min(sizes),
                                                          "max": max(sizes), "raw": W * H},
               "equal_host_twin": "%d of %d" % (same, min(4, n)), "batch_device_bytes": dev.value}
        sheets = [gray.output(s).data[:, :W].copy() for s in range(min(4, n))]
        return out, sheets, sizes[:len(sheets)]
    finally:
        gray.close()
        if mono is not None:
            mono.close()
        buf.close()


def files_part(L, npages, batch, streams, threads):
    host_in = np.empty((npages, H, W), np.uint8)
    for i in range(npages):
        L.uphip_synth_page_host(host_in[i].ctypes.data, W, W, H, i)
    r = Runner(options(L), batch, W, H, A.FMT_GRAY8, devices=(0,), streams=streams, host_threads=threads)
    tmpdir = tempfile.mkdtemp(prefix="uphip_png_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"part": "files", "pages": npages, "sheets_per_batch": batch, "streams": streams, "host_threads": threads}
    try:
        src = source_memory(host_in.ctypes.data, W, W * H, npages, keep=host_in)
        for name, make in (("pnm", lambda: sink_pnm(os.path.join(tmpdir, "o_%04lld.pgm"), 64)),
                           ("png", lambda: sink_png(os.path.join(tmpdir, "o_%04lld.png"), 64, 300)),
                           ("jp2", lambda: sink_jp2(os.path.join(tmpdir, "o_%04lld.jp2"), 64))):
            snk = make()
            for rep in range(2):  # one untimed warm-up pass
                t0 = time.perf_counter()
                failed, err = r.run_host(npages, src, snk)
                t = time.perf_counter() - t0
                if failed:
                    raise UnpaperHipError("%s run: %d failed: %s" % (name, failed, err))
            st = r.stats()
            ext = {"pnm": "pgm", "png": "png", "jp2": "jp2"}[name]
            out[name] = {"pages_per_s": round(npages / t, 1), "load_s": round(st.load_s, 3),
                         "store_s": round(st.store_s, 3),
                         "kB_a_page": round(os.path.getsize(os.path.join(tmpdir, "o_0000." + ext)) / 1e3)}
            snk.close()
        from PIL import Image
        back = np.asarray(Image.open(os.path.join(tmpdir, "o_0000.png")))
        ref = np.fromfile(os.path.join(tmpdir, "o_0000.pgm"), np.uint8)[-W * H:].reshape(H, W)
        out["png_equals_pgm"] = bool(np.array_equal(back, ref))
    finally:
        r.close()
        shutil.rmtree(tmpdir, ignore_errors=True)
    return out


def pil_size(arr, level):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "PNG", compress_level=level)
    return len(b.getvalue())


def compression_part(sheets, sizes, images):
    from helpers import page_array
    rows = []

    def add(name, arr, fmt, ours=None):
        flat = np.ascontiguousarray(arr.reshape(arr.shape[0], -1))
        ours = ours if ours is not None else len(png_encode_host(flat, arr.shape[1], fmt))
        l1, l6 = pil_size(arr, 1), pil_size(arr, 6)
        rows.append({"image": name, "raw": int(arr.size), "ours": ours, "pil_level1": l1, "pil_level6": l6,
                     "ours_over_level1": round(ours / l1, 3), "ours_over_level6": round(ours / l6, 3)})
    for i, (s, n) in enumerate(zip(sheets, sizes)):
        add("bench sheet %d" % i, s, A.FMT_GRAY8, ours=n + 57)  # the stream plus the file's chunks
    add("page_array A4 gray", page_array(1240, 1754, seed=1), A.FMT_GRAY8)
    add("page_array A4 colour", page_array(1240, 1754, seed=1, color=True), A.FMT_RGB24)
    for path in images:
        from PIL import Image
        im = Image.open(path)
        im = im.convert("RGB" if im.mode not in ("L",) else "L")
        a = np.asarray(im)
        add(os.path.basename(path), a, A.FMT_GRAY8 if a.ndim == 2 else A.FMT_RGB24)
    return {"part": "compression", "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["device", "files", "compression"])
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS") or 16))
    ap.add_argument("--image", action="append", default=[])
    args = ap.parse_args()
    sheets, sizes = [], []
    L = None
    if set(args.parts) & {"device", "files", "kernels"}:
        L = Backend().lib
    if "kernels" in args.parts:
        print(json.dumps(device_part(L, args.pages, 0, True)), flush=True)
    if "device" in args.parts:
        out, sheets, sizes = device_part(L, args.pages, args.reps, False)
        print(json.dumps(out), flush=True)
    if "files" in args.parts:
        print(json.dumps(files_part(L, args.files, args.batch, args.streams, args.threads)), flush=True)
    if "compression" in args.parts:
        print(json.dumps(compression_part(sheets, sizes, args.image)), flush=True)


if __name__ == "__main__":
    main()
