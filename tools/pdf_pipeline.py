#!/usr/bin/env python3
"""PDF in -> cleaned PDF out on the GPU: the peer of the reference's
pdf_pipeline_batch_process (pdf/pdf_pipeline_batch.h; `unpaper in.pdf
out.pdf`), on the runner's PDF source and sink.

    python tools/pdf_pipeline.py in.pdf out.pdf [--pdf-quality fast|high]
        [--pdf-dpi N] [--jpeg-quality Q] [--input-pages 1|2] [--output-pages 1|2]
        [--sheet-size WxH] [--mask-scan-point X,Y ...]

Every input page is decoded where its codec runs (JPEG / JPEG 2000 on the
device, JBIG2 / CCITT / Flate on the load pool), the sheets go through the
default pipeline, and each output page is encoded on the device (JPEG, or
lossless JPEG 2000 with --pdf-quality high) into one PDF with the input's
metadata.  With --sheet-size WxH (the reference's --sheet-size, in pixels)
the pages may be of any sizes: the runner is sized for the largest
(uphip_source_max_geometry) and every page is centred in a W x H sheet,
cropped where larger.  Without it the pages must share the first page's image
geometry; a page that does not is left out of the output, as the reference's
page accumulator leaves out failed pages.
--mask-scan-point X,Y (the reference's option, repeatable up to
UPHIP_MAX_POINTS times) gives the points the mask detection starts from, in
sheet pixels, in place of the layout's: one mask is detected, deskewed and
centred per point, in the order given.
--pdf-dpi 0 (the default here) takes the page images as they are; a dpi
applies the reference's size check (an image off the page size would need
a rasteriser and fails).
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unpaper-gpu_amd", "python"))

from unpaper_hip import ctypes_abi as A  # noqa: E402
from unpaper_hip import pdf as P  # noqa: E402
from unpaper_hip.device import load_library  # noqa: E402
from unpaper_hip.pipeline import (Runner, sink_pdf, source_max_geometry, source_page_count,  # noqa: E402
                                  source_pdf)


def point_arg(text):
    try:
        x, y = (int(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError("expected X,Y, got %r" % text)
    return x, y


def apply_mask_scan_points(opts, points):
    """The options' mask-scan points from --mask-scan-point's list."""
    if len(points) > A.MAX_POINTS:
        raise ValueError("--mask-scan-point: at most %d points (got %d)" % (A.MAX_POINTS, len(points)))
    opts.point_count = len(points)
    for i, (x, y) in enumerate(points):
        opts.points[i] = A.Point(x, y)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--pdf-quality", choices=("fast", "high"), default="fast")
    ap.add_argument("--pdf-dpi", type=int, default=0)
    ap.add_argument("--jpeg-quality", type=int, default=0, help="0 = 85 (PDF_OUTPUT_JPEG_QUALITY)")
    ap.add_argument("--input-pages", type=int, default=1, choices=(1, 2))
    ap.add_argument("--output-pages", type=int, default=1, choices=(1, 2))
    ap.add_argument("--sheet-size", metavar="WxH", help="one sheet size in pixels: admits pages of any sizes")
    ap.add_argument("--mask-scan-point", metavar="X,Y", type=point_arg, action="append", default=[],
                    help="a point the mask detection starts from (repeatable)")
    ap.add_argument("--sheets-per-batch", type=int, default=16)
    ap.add_argument("--streams", type=int, default=8)
    return ap.parse_args(argv)


def main():
    args = parse_args()

    L = load_library()
    doc = P.PdfDocument.open(args.input)
    w, h, fmt = doc.page_probe(0, args.pdf_dpi)
    meta = doc.metadata()
    opts = A.Options()
    L.uphip_options_init(C.byref(opts))
    opts.input_count = args.input_pages
    opts.output_count = args.output_pages
    apply_mask_scan_points(opts, args.mask_scan_point)
    src = source_pdf(args.input, args.pdf_dpi)
    if args.sheet_size:
        sw, sh = (int(v) for v in args.sheet_size.lower().split("x"))
        opts.sheet_size = A.RectangleSize(sw, sh)
        w, h, fmt = source_max_geometry(src)
    npages = source_page_count(src)
    jobs = npages // args.input_pages
    snk = sink_pdf(args.output, meta, args.pdf_dpi if args.pdf_dpi else 0, args.jpeg_quality,
                   1 if args.pdf_quality == "high" else 0)
    r = Runner(opts, args.sheets_per_batch, w, h, fmt, devices=(0,), streams=args.streams)
    try:
        t0 = time.perf_counter()
        failed, err = r.run_host(jobs, src, snk)
        snk.finish()
        dt = time.perf_counter() - t0
    finally:
        r.close()
    out = P.PdfDocument.open(args.output)
    print("%s: %d pages in, %d sheets, %d pages out, %d failed%s, %.2f s (%.1f sheets/s)"
          % (args.output, npages, jobs, out.page_count, failed, (" (" + err + ")") if failed else "",
             dt, jobs / dt if dt > 0 else 0.0))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
