"""Batch sheet pipeline (uphip_batch_*): the device peer of process_sheet
(sheet_process.c:134) run by lib/batch_worker.c for every job, here for a whole
batch of sheets per launch sequence."""
import ctypes as C

import numpy as np

from . import ctypes_abi as A
from .device import UnpaperHipError, _check, load_library
from .hostimage import HostImage


def synth_page_host(width, height, page):
    """Deterministic synthetic GRAY8 page, host copy."""
    L = load_library()
    arr = np.empty((height, width), np.uint8)
    L.uphip_synth_page_host(arr.ctypes.data, width, width, height, page)
    return arr


def synth_sheet_rgb_host(width, height, sheet):
    """C4 synthetic RGB24 double-page sheet (synth.h synth_rgb_channel), host copy."""
    L = load_library()
    arr = np.empty((height, width, 3), np.uint8)
    L.uphip_synth_sheet_rgb_host(arr.ctypes.data, width * 3, width, height, sheet)
    return arr


class DeviceBuffer:
    """Raw HBM allocation (bench inputs)."""

    def __init__(self, nbytes):
        self.lib = load_library()
        self.ptr = self.lib.uphip_device_alloc(nbytes)
        _check(self.lib)
        if not self.ptr:
            raise UnpaperHipError("device_alloc failed")
        self.nbytes = nbytes

    def close(self):
        if self.ptr:
            self.lib.uphip_device_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    def __init__(self, options, capacity, page_width, page_height, page_format, timing=False):
        self.lib = L = load_library()
        self.options = options
        self.geometry = A.BatchGeometry(capacity, page_width, page_height, page_format)
        self.capacity = capacity
        self.handle = L.uphip_batch_create(C.byref(options), C.byref(self.geometry))
        _check(L)
        if not self.handle:
            raise UnpaperHipError("batch_create failed")
        w, h, f, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        L.uphip_batch_output_info(self.handle, C.byref(w), C.byref(h), C.byref(f), C.byref(n))
        if timing:
            self.set_timing(True)
        self.out_width, self.out_height, self.out_format = w.value, h.value, f.value

    def set_page_size(self, sheet, page_index, width, height):
        """The page in this input slot is width x height, at most the batch's
        page size; (0, 0) puts it back (uphip_batch_set_page_size: needs a
        fully set sheet_size and no pre_rotate)."""
        slot = sheet * self.options.input_count + page_index
        rc = self.lib.uphip_batch_set_page_size(self.handle, slot, width, height)
        _check(self.lib)
        if rc != 0:
            raise UnpaperHipError("batch_set_page_size failed")
        self._sized = True

    def decode_route(self):
        """The decode of the last run: 0 fill + copy, 1 k_decode_gray,
        2 k_decode_gray_fit; -1 before any run."""
        return self.lib.uphip_batch_decode_route(self.handle)

    def set_input(self, sheet, page_index, h: HostImage):
        """Upload a page; one smaller than the batch's page size sets the
        slot's size first (a later full-size page sets it back)."""
        slot = sheet * self.options.input_count + page_index
        full = (h.width, h.height) == (self.geometry.page_width, self.geometry.page_height)
        if not full:
            self.set_page_size(sheet, page_index, h.width, h.height)
        elif getattr(self, "_sized", False):
            self.set_page_size(sheet, page_index, 0, 0)
        arr = np.ascontiguousarray(h.data)
        # the copy is asynchronous on the batch stream: the source must live
        # until the stream has passed it (released by wait())
        self._inputs = getattr(self, "_inputs", {})
        self._inputs[slot] = arr
        if self.lib.uphip_batch_set_input(self.handle, slot, arr.ctypes.data, arr.shape[1]) != 0:
            _check(self.lib)

    def run(self, count):
        rc = self.lib.uphip_batch_run(self.handle, count)
        _check(self.lib)
        if rc != 0:
            raise UnpaperHipError("batch_run failed")

    def run_device(self, count, pages_ptr, pitch, page_stride):
        rc = self.lib.uphip_batch_run_device(self.handle, count, pages_ptr, pitch, page_stride)
        _check(self.lib)
        if rc != 0:
            raise UnpaperHipError("batch_run_device failed")

    def wait(self):
        rc = self.lib.uphip_batch_wait(self.handle)
        self._inputs = {}
        _check(self.lib)
        if rc != 0:
            raise UnpaperHipError("batch_wait failed")

    def output(self, sheet, background=(255, 255, 255), threshold=170) -> HostImage:
        out = HostImage(self.out_width, self.out_height, self.out_format, background=background,
                        abs_black_threshold=threshold)
        if self.lib.uphip_batch_get_output(self.handle, sheet, out.data.ctypes.data,
                                           out.linesize) != 0:
            _check(self.lib)
            raise UnpaperHipError("batch_get_output failed")
        return out

    def encode_jpeg(self, quality=0, sampling=0):
        """Queue the GPU JPEG output branch on the last run's pages
        (uphip_batch_encode_jpeg_async)."""
        if self.lib.uphip_batch_encode_jpeg_async(self.handle, quality, sampling) != 0:
            _check(self.lib)
            raise UnpaperHipError("batch_encode_jpeg failed")

    def jpeg_files(self, pages):
        """The encoded files of the last encode_jpeg (None for a page the
        batch's buffers could not hold: uphip_batch_jpeg_page + jpeg_encode)."""
        L = self.lib
        self.wait()
        sizes = (C.c_int64 * pages)()
        total = L.uphip_batch_jpeg_sizes(self.handle, sizes, pages)
        _check(L)
        buf = np.zeros(max(total, 1), np.uint8)
        if total > 0 and L.uphip_batch_jpeg_download_async(self.handle, buf.ctypes.data, total) != 0:
            _check(L)
        self.wait()
        out, off = [], 0
        for i in range(pages):
            n = sizes[i]
            if n > 0:
                out.append(buf[off:off + n].tobytes())
                off += n
            else:
                out.append(None)
        return out

    def jpeg_page(self, page):
        """(device pointer, pitch, width, height, format) of output page `page`."""
        src, pitch = C.c_void_p(), C.c_int64()
        w, h, f = C.c_int32(), C.c_int32(), C.c_int32()
        if self.lib.uphip_batch_jpeg_page(self.handle, page, C.byref(src), C.byref(pitch),
                                          C.byref(w), C.byref(h), C.byref(f)) != 0:
            _check(self.lib)
        return src.value, pitch.value, w.value, h.value, f.value

    def encode_g4(self):
        """Queue the bilevel output branch on the last run's pages: CCITT
        Group 4 streams (uphip_batch_encode_g4_async; MONOWHITE output only)."""
        if self.lib.uphip_batch_encode_g4_async(self.handle) != 0:
            _check(self.lib)
            raise UnpaperHipError("batch_encode_g4 failed")

    def g4_files(self, pages):
        """The streams of the last encode_g4 (None for a page larger than its
        share of the encode buffer: g4_encode from output_ptr)."""
        L = self.lib
        self.wait()
        sizes = (C.c_int64 * pages)()
        total = L.uphip_batch_g4_sizes(self.handle, sizes, pages)
        _check(L)
        buf = np.zeros(max(total, 1), np.uint8)
        if total > 0 and L.uphip_batch_g4_download_async(self.handle, buf.ctypes.data, total) != 0:
            _check(L)
        self.wait()
        out, off = [], 0
        for i in range(pages):
            n = sizes[i]
            if n > 0:
                out.append(buf[off:off + n].tobytes())
                off += n
            else:
                out.append(None)
        return out

    def encode_png(self):
        """Queue the lossless output branch on the last run's pages: the zlib
        streams of PNG IDAT chunks (uphip_batch_encode_png_async; any output
        format)."""
        if self.lib.uphip_batch_encode_png_async(self.handle) != 0:
            _check(self.lib)
            raise UnpaperHipError("batch_encode_png failed")

    def png_files(self, pages):
        """The zlib streams of the last encode_png, one per output page
        (png_wrap makes a file of one, PdfWriter.add_page_flate a PDF page)."""
        L = self.lib
        self.wait()
        sizes = (C.c_int64 * pages)()
        total = L.uphip_batch_png_sizes(self.handle, sizes, pages)
        _check(L)
        if total <= 0:
            raise UnpaperHipError("batch_png_sizes failed")
        buf = np.zeros(total, np.uint8)
        if L.uphip_batch_png_download_async(self.handle, buf.ctypes.data, total) != 0:
            _check(L)
            raise UnpaperHipError("batch_png_download failed")
        self.wait()
        out, off = [], 0
        for i in range(pages):
            out.append(buf[off:off + sizes[i]].tobytes())
            off += sizes[i]
        return out

    def encode_tiff(self):
        """Queue the TIFF output branch on the last run's pages: each page's
        Deflate strips (uphip_batch_encode_tiff_async; GRAY8 and RGB24
        output)."""
        if self.lib.uphip_batch_encode_tiff_async(self.handle) != 0:
            _check(self.lib)
            raise UnpaperHipError("batch_encode_tiff failed")

    def tiff_pages(self, pages):
        """The packed pages of the last encode_tiff, one per output page
        (TiffWriter.add_page_deflate takes each)."""
        L = self.lib
        self.wait()
        sizes = (C.c_int64 * pages)()
        total = L.uphip_batch_tiff_sizes(self.handle, sizes, pages)
        _check(L)
        if total <= 0:
            raise UnpaperHipError("batch_tiff_sizes failed")
        buf = np.zeros(total, np.uint8)
        if L.uphip_batch_tiff_download_async(self.handle, buf.ctypes.data, total) != 0:
            _check(L)
            raise UnpaperHipError("batch_tiff_download failed")
        self.wait()
        out, off = [], 0
        for i in range(pages):
            out.append(buf[off:off + sizes[i]].tobytes())
            off += sizes[i]
        return out

    def output_ptr(self, sheet):
        """(device pointer, pitch) of output sheet `sheet` (waits for the run)."""
        pitch = C.c_int64()
        p = self.lib.uphip_batch_output_ptr(self.handle, sheet, C.byref(pitch))
        if not p:
            _check(self.lib)
            raise UnpaperHipError("batch_output_ptr failed")
        return p, pitch.value

    def report(self, sheet):
        r = A.SheetReport()
        self.lib.uphip_batch_get_report(self.handle, sheet, C.byref(r))
        return r

    def masks(self, sheet, capacity=A.MAX_POINTS):
        """(mask_count, masks, rotations) of a sheet: the masks of the last
        detection and the rotation the deskew found for each
        (uphip_batch_get_masks)."""
        m = (A.Rectangle * max(capacity, 1))()
        r = (C.c_float * max(capacity, 1))()
        n = self.lib.uphip_batch_get_masks(self.handle, sheet, m, r, capacity)
        if n < 0:
            _check(self.lib)
            raise UnpaperHipError("batch_get_masks failed")
        k = min(n, capacity)
        return n, [m[i] for i in range(k)], [r[i] for i in range(k)]

    def set_mask_scan_route(self, route):
        """How a batch of more than two mask-scan points sums its scan bars
        from the next run on: 0 every point in one launch (the default), 1 per
        point and axis, the looped twin (uphip_batch_set_mask_scan_route)."""
        if self.lib.uphip_batch_set_mask_scan_route(self.handle, route) != 0:
            _check(self.lib)
            raise UnpaperHipError("batch_set_mask_scan_route failed")

    def device_bytes(self):
        """Device memory the batch holds (uphip_batch_device_bytes)."""
        v = C.c_int64()
        if self.lib.uphip_batch_device_bytes(self.handle, C.byref(v)) != 0:
            _check(self.lib)
            raise UnpaperHipError("batch_device_bytes failed")
        return v.value

    def set_timing(self, enable=True):
        """Record per-stage HIP events on every run (uphip_batch_set_timing)."""
        self.lib.uphip_batch_set_timing(self.handle, 1 if enable else 0)

    def stage_times(self):
        names = (C.c_char_p * 64)()
        ms = (C.c_float * 64)()
        n = self.lib.uphip_batch_kernel_times(self.handle, names, ms, 64)
        return [(names[i].decode(), ms[i]) for i in range(max(n, 0))]

    def close(self):
        if self.handle:
            self.lib.uphip_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostBuffer:
    """Pinned host memory (uphip_host_alloc) viewed as a numpy uint8 array."""

    def __init__(self, nbytes):
        self.lib = load_library()
        self.ptr = self.lib.uphip_host_alloc(nbytes)
        _check(self.lib)
        if not self.ptr:
            raise UnpaperHipError("host_alloc failed")
        self.nbytes = nbytes
        self.array = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(self.ptr))

    def close(self):
        if self.ptr:
            self.array = None
            self.lib.uphip_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Runner:
    """Multi-device runner (uphip_runner_*): the peer of lib/batch_worker.c's
    batch_process_parallel with one host thread and `streams` batches of
    `sheets` sheets per device; sources/sinks are the decode/encode queues.
    sheets=0 / streams=0: the runner sizes them from the geometry and the
    device's free memory (uphip_runner_layout reports the choice)."""

    def __init__(self, options, sheets, page_width, page_height, page_format, devices=(0,),
                 streams=4, host_threads=0, timing=False):
        self.lib = L = load_library()
        self.options = options
        self.geometry = A.BatchGeometry(sheets, page_width, page_height, page_format)
        self._devs = (C.c_int32 * len(devices))(*devices)
        self.config = A.RunnerConfig(len(devices), self._devs, streams, host_threads,
                                     1 if timing else 0)
        self.ndevices = len(devices)
        self.streams = streams
        self.handle = L.uphip_runner_create(C.byref(options), C.byref(self.geometry),
                                            C.byref(self.config))
        _check(L)
        if not self.handle:
            raise UnpaperHipError("runner_create failed")
        w, h, f, ls = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        L.uphip_runner_output_info(self.handle, C.byref(w), C.byref(h), C.byref(f), C.byref(ls))
        self.out_width, self.out_height, self.out_format = w.value, h.value, f.value
        self.out_linesize = ls.value
        k, cap, bb = C.c_int32(), C.c_int32(), C.c_int64()
        L.uphip_runner_layout(self.handle, C.byref(k), C.byref(cap), C.byref(bb))
        self.streams, self.batch_bytes = k.value, bb.value
        self.geometry.capacity = cap.value

    def batch(self, device_index, slot):
        """The Batch object behind one stream (borrowed; not closed here)."""
        h = self.lib.uphip_runner_batch(self.handle, device_index, slot)
        if not h:
            raise UnpaperHipError("no such batch")
        b = Batch.__new__(Batch)
        b.lib, b.options, b.capacity, b.handle = self.lib, self.options, self.geometry.capacity, h
        b.geometry = self.geometry
        b.out_width, b.out_height, b.out_format = self.out_width, self.out_height, self.out_format
        b.close = lambda: None
        return b

    def slot_chunk(self, device_index, slot):
        """(first job, sheet count) of the chunk batch `slot` ran last (its
        outputs are resident), or None when it has run none."""
        n = C.c_int32(0)
        first = self.lib.uphip_runner_slot_chunk(self.handle, device_index, slot, C.byref(n))
        return None if first < 0 else (first, n.value)

    def run_device(self, shards, passes=1):
        """shards: one (device_ptr, pitch, page_stride, count) per device.
        Returns (failed jobs, the library's error message or None)."""
        arr = (A.DevicePages * self.ndevices)(*[A.DevicePages(*s) for s in shards])
        failed = self.lib.uphip_runner_run_device(self.handle, arr, passes)
        err = self.lib.uphip_last_error()
        self.lib.uphip_clear_error()
        return failed, (err.decode() if err else None)

    def run_host(self, njobs, source, sink):
        failed = self.lib.uphip_runner_run_host(self.handle, njobs, source.handle, sink.handle)
        err = self.lib.uphip_last_error()
        self.lib.uphip_clear_error()
        return failed, (err.decode() if err else None)

    def stats(self):
        s = A.RunnerStats()
        self.lib.uphip_runner_get_stats(self.handle, C.byref(s))
        return s

    def placement(self, device_index):
        """(NUMA node or -1, CPUs bound to or 0, load/store pool threads)."""
        node, ncpu, pool = C.c_int32(), C.c_int32(), C.c_int32()
        if self.lib.uphip_runner_placement(self.handle, device_index, C.byref(node),
                                           C.byref(ncpu), C.byref(pool)) != 0:
            _check(self.lib)
        return node.value, ncpu.value, pool.value

    def close(self):
        if self.handle:
            self.lib.uphip_runner_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Handle:
    def __init__(self, handle, destroy, keep=()):
        self.handle = handle
        self._destroy = destroy
        self._keep = keep          # buffers / callbacks the C side points into

    def close(self):
        if self.handle:
            self._destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def source_memory(ptr, linesize, page_stride, npages, keep=None):
    L = load_library()
    h = L.uphip_source_memory(ptr, linesize, page_stride, npages)
    _check(L)
    return _Handle(h, L.uphip_source_destroy, (keep,))


def source_pnm(paths):
    L = load_library()
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    h = L.uphip_source_pnm(arr, len(paths))
    _check(L)
    return _Handle(h, L.uphip_source_destroy, (arr,))


def source_max_geometry(src):
    """(width, height, format): the largest width and height and the common
    format over the pages of a PNM-list, TIFF or PDF source
    (uphip_source_max_geometry): the geometry of a Runner whose options have
    a fully set sheet_size."""
    L = load_library()
    info = A.PnmInfo()
    rc = L.uphip_source_max_geometry(src.handle, C.byref(info))
    _check(L)
    if rc != 0:
        raise UnpaperHipError("source_max_geometry failed")
    return info.width, info.height, info.format


def source_pdf(path, dpi=0):
    """Page i of a PDF as input page i (uphip_source_pdf; dpi 0 = the page
    images as they are, dpi > 0 = the reference's size check)."""
    L = load_library()
    h = L.uphip_source_pdf(path.encode(), dpi)
    _check(L)
    if not h:
        raise UnpaperHipError("source_pdf failed")
    return _Handle(h, L.uphip_source_destroy)


def source_tiff(path, flags=0):
    """IFD i of a TIFF as input page i (uphip_source_tiff; flags:
    ctypes_abi.TIFF_DEVICE_DECODE sends the pages that qualify through the
    device decode, TIFF_HOST_DECODE or 0 every page to the load tasks)."""
    L = load_library()
    h = L.uphip_source_tiff(path.encode(), flags)
    _check(L)
    if not h:
        raise UnpaperHipError("source_tiff failed")
    return _Handle(h, L.uphip_source_destroy)


class TiffDocument:
    """A TIFF file, one page per IFD (uphip_tiff_open)."""

    def __init__(self, path):
        self.lib = L = load_library()
        self.handle = L.uphip_tiff_open(path.encode())
        if not self.handle:
            _check(L)
            raise UnpaperHipError("tiff_open failed")

    @property
    def page_count(self):
        return self.lib.uphip_tiff_page_count(self.handle)

    def probe(self, page):
        """(width, height, format, (x dpi, y dpi))"""
        info, dpi = A.PnmInfo(), (C.c_float * 2)()
        if self.lib.uphip_tiff_page_probe(self.handle, page, C.byref(info), dpi) != 0:
            _check(self.lib)
        return info.width, info.height, info.format, (dpi[0], dpi[1])

    def on_device(self, page):
        r = self.lib.uphip_tiff_page_on_device(self.handle, page)
        if r < 0:
            _check(self.lib)
        return r == 1

    def read_page(self, page) -> HostImage:
        w, h, fmt, _ = self.probe(page)
        img = HostImage(w, h, fmt)
        if self.lib.uphip_tiff_read_page(self.handle, page, img.data.ctypes.data, img.linesize,
                                         None) != 0:
            _check(self.lib)
        return img

    def close(self):
        if self.handle:
            self.lib.uphip_tiff_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tiff_decode(data: bytes, page, device_ptr, pitch):
    """Page `page` of a TIFF file image decoded on the device into device_ptr
    (uphip_tiff_decode); returns (width, height, format)."""
    L = load_library()
    info = A.PnmInfo(0, 0, 0)
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    if L.uphip_tiff_decode(buf, len(data), page, device_ptr, pitch, C.byref(info)) != 0:
        _check(L)
        raise UnpaperHipError("tiff_decode failed")
    return info.width, info.height, info.format


def source_page_count(src):
    L = load_library()
    n = L.uphip_source_page_count(src.handle)
    _check(L)
    return n


def source_callback(fn):
    """fn(job, page, dst_ptr, linesize) -> 0 on success (called from C threads)."""
    L = load_library()
    cb = A.LoadFn(lambda user, job, page, dst, ls: fn(job, page, dst, ls))
    h = L.uphip_source_callback(cb, None)
    _check(L)
    return _Handle(h, L.uphip_source_destroy, (cb,))


def sink_memory(ptr, linesize, sheet_stride, nsheets, keep=None):
    L = load_library()
    h = L.uphip_sink_memory(ptr, linesize, sheet_stride, nsheets)
    _check(L)
    return _Handle(h, L.uphip_sink_destroy, (keep,))


def sink_pnm(pattern, wrap=0):
    L = load_library()
    h = L.uphip_sink_pnm(pattern.encode(), wrap)
    _check(L)
    return _Handle(h, L.uphip_sink_destroy)


def sink_jpeg(pattern, wrap=0, quality=0, sampling=0):
    """JPEG files encoded on the device (uphip_sink_jpeg; quality 0 = 85,
    sampling 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0 for RGB24 sheets)."""
    L = load_library()
    h = L.uphip_sink_jpeg(pattern.encode(), wrap, quality, sampling)
    _check(L)
    return _Handle(h, L.uphip_sink_destroy)


def jpeg_encode(device_ptr, pitch, width, height, fmt, quality=0, sampling=0):
    """uphip_jpeg_encode: one device image -> JPEG file bytes."""
    L = load_library()
    n = L.uphip_jpeg_encode(device_ptr, pitch, width, height, fmt, quality, sampling, None, 0)
    _check(L)
    if n <= 0:
        raise UnpaperHipError("jpeg_encode failed")
    buf = np.zeros(n, np.uint8)
    m = L.uphip_jpeg_encode(device_ptr, pitch, width, height, fmt, quality, sampling,
                            buf.ctypes.data, n)
    _check(L)
    if m != n:
        raise UnpaperHipError("jpeg_encode: size changed between calls")
    return buf.tobytes()


def sink_jp2(pattern, wrap=0):
    """Lossless JPEG 2000 files (uphip_sink_jp2: transforms on the device,
    code-blocks on the store tasks)."""
    L = load_library()
    h = L.uphip_sink_jp2(pattern.encode(), wrap)
    _check(L)
    return _Handle(h, L.uphip_sink_destroy)


def jp2_encode(device_ptr, pitch, width, height, fmt):
    """uphip_jp2_encode: one device image -> lossless JP2 file bytes."""
    L = load_library()
    cap = width * height * (1 if fmt == 0 else 3) // 2 + 65536
    buf = np.zeros(cap, np.uint8)
    n = L.uphip_jp2_encode(device_ptr, pitch, width, height, fmt, buf.ctypes.data, cap)
    _check(L)
    if n > cap:
        buf = np.zeros(n, np.uint8)
        n = L.uphip_jp2_encode(device_ptr, pitch, width, height, fmt, buf.ctypes.data, n)
        _check(L)
    if n <= 0:
        raise UnpaperHipError("jp2_encode failed")
    return buf[:n].tobytes()


class _PdfSink(_Handle):
    def finish(self):
        """Completes the PDF (uphip_sink_finish)."""
        L = load_library()
        if self.handle and L.uphip_sink_finish(self.handle) != 0:
            _check(L)
            raise UnpaperHipError("sink_finish failed")


def sink_pdf(path, meta=None, dpi=0, quality=0, mode=0):
    """All output pages into one PDF (uphip_sink_pdf): mode 0 = JPEG pages
    (fast), 1 = lossless JPEG 2000 pages (high); dpi 0 = 300.  Call
    finish() after the run."""
    from .pdf import _meta_struct
    L = load_library()
    m, keep = _meta_struct(meta)
    h = L.uphip_sink_pdf(path.encode(), C.byref(m) if m is not None else None, dpi, quality, mode)
    _check(L)
    if not h:
        raise UnpaperHipError("sink_pdf failed")
    return _PdfSink(h, L.uphip_sink_destroy, (m, keep))


def sink_tiff_g4(pattern, wrap=0, dpi=0):
    """One CCITT Group 4 TIFF per output page, coded on the device
    (uphip_sink_tiff_g4; bilevel output only; dpi 0 = 300)."""
    L = load_library()
    h = L.uphip_sink_tiff_g4(pattern.encode(), wrap, dpi)
    _check(L)
    if not h:
        raise UnpaperHipError("sink_tiff_g4 failed")
    return _Handle(h, L.uphip_sink_destroy)


def sink_pdf_bilevel(path, meta=None, dpi=0):
    """All output pages into one PDF of CCITT Group 4 images
    (uphip_sink_pdf_bilevel; bilevel output only; dpi 0 = 300).  Call
    finish() after the run."""
    from .pdf import _meta_struct
    L = load_library()
    m, keep = _meta_struct(meta)
    h = L.uphip_sink_pdf_bilevel(path.encode(), C.byref(m) if m is not None else None, dpi)
    _check(L)
    if not h:
        raise UnpaperHipError("sink_pdf_bilevel failed")
    return _PdfSink(h, L.uphip_sink_destroy, (m, keep))


def sink_png(pattern, wrap=0, dpi=0):
    """One lossless PNG per output page, coded on the device (uphip_sink_png;
    any output format; dpi > 0 writes a pHYs chunk)."""
    L = load_library()
    h = L.uphip_sink_png(pattern.encode(), wrap, dpi)
    _check(L)
    if not h:
        raise UnpaperHipError("sink_png failed")
    return _Handle(h, L.uphip_sink_destroy)


def sink_pdf_lossless(path, meta=None, dpi=0):
    """All output pages into one PDF of lossless /FlateDecode images coded on
    the device (uphip_sink_pdf_lossless; not Y400A; dpi 0 = 300).  Call
    finish() after the run."""
    from .pdf import _meta_struct
    L = load_library()
    m, keep = _meta_struct(meta)
    h = L.uphip_sink_pdf_lossless(path.encode(), C.byref(m) if m is not None else None, dpi)
    _check(L)
    if not h:
        raise UnpaperHipError("sink_pdf_lossless failed")
    return _PdfSink(h, L.uphip_sink_destroy, (m, keep))


def sink_tiff(pattern, wrap=0, dpi=0):
    """One TIFF per output page, coded on the device (uphip_sink_tiff): Group
    4 for MONOWHITE output, Deflate strips for GRAY8 and RGB24; dpi 0 = 300."""
    L = load_library()
    h = L.uphip_sink_tiff(pattern.encode(), wrap, dpi)
    _check(L)
    if not h:
        raise UnpaperHipError("sink_tiff failed")
    return _Handle(h, L.uphip_sink_destroy)


def sink_tiff_multipage(path, dpi=0):
    """All output pages into one TIFF (uphip_sink_tiff_multipage; codec as
    sink_tiff).  Call finish() after the run."""
    L = load_library()
    h = L.uphip_sink_tiff_multipage(path.encode(), dpi)
    _check(L)
    if not h:
        raise UnpaperHipError("sink_tiff_multipage failed")
    return _PdfSink(h, L.uphip_sink_destroy)


def tiff_encode(device_ptr, pitch, width, height, fmt, offset=0, dpi=0):
    """uphip_tiff_encode: rows in device memory -> a one-page TIFF file
    (Deflate strips; Group 4 for MONOWHITE, whose `offset` is the bit of a
    row that holds pixel 0)."""
    return _png(load_library().uphip_tiff_encode, device_ptr, pitch, offset, width, height, fmt, dpi)


def tiff_encode_host(rows, width, fmt, offset=0, dpi=0):
    """uphip_tiff_encode_host: a 2-D uint8 array of rows (no device); the
    same bytes as tiff_encode."""
    rows = np.ascontiguousarray(rows, np.uint8)
    return _png(load_library().uphip_tiff_encode_host, rows.ctypes.data, rows.shape[1], offset, width,
                rows.shape[0], fmt, dpi)


def tiff_encode_pages(device_ptr, pitch, page_stride, npages, width, height, fmt, fold=0, device_out=None,
                      device_capacity=0):
    """uphip_tiff_encode_pages: byte-format pages in device memory -> their
    packed pages (StripByteCounts, then the strips), a list of bytes;
    device_out: device memory the encoder packs them into."""
    L = load_library()
    sizes = (C.c_int64 * npages)()
    n = L.uphip_tiff_encode_pages(device_ptr, pitch, page_stride, npages, width, height, fmt, fold, sizes,
                                  None, 0, device_out, device_capacity)
    _check(L)
    if n <= 0:
        raise UnpaperHipError("tiff_encode_pages failed")
    buf = np.zeros(n, np.uint8)
    if L.uphip_tiff_encode_pages(device_ptr, pitch, page_stride, npages, width, height, fmt, fold, sizes,
                                 buf.ctypes.data, n, device_out, device_capacity) != n:
        _check(L)
        raise UnpaperHipError("tiff_encode_pages failed")
    out, off = [], 0
    for i in range(npages):
        out.append(buf[off:off + sizes[i]].tobytes())
        off += sizes[i]
    return out


class TiffWriter:
    """uphip_tiff_writer_*: one TIFF of many pages.  add_page_* take the
    page's place in the file as `index` (-1: after the highest so far)."""

    def __init__(self, path, dpi=0):
        self.lib = load_library()
        self.handle = self.lib.uphip_tiff_writer_open(path.encode(), dpi)
        _check(self.lib)
        if not self.handle:
            raise UnpaperHipError("tiff_writer_open failed")

    def add_page_deflate(self, page: bytes, width, height, fmt, index=-1, dpi=0):
        if self.lib.uphip_tiff_writer_add_page_deflate(self.handle, index, page, len(page), width, height,
                                                       fmt, dpi) != 0:
            _check(self.lib)
            raise UnpaperHipError("tiff_writer_add_page_deflate failed")

    def add_page_g4(self, stream: bytes, width, height, index=-1, dpi=0):
        if self.lib.uphip_tiff_writer_add_page_g4(self.handle, index, stream, len(stream), width, height,
                                                  dpi) != 0:
            _check(self.lib)
            raise UnpaperHipError("tiff_writer_add_page_g4 failed")

    def finish(self):
        if self.lib.uphip_tiff_writer_finish(self.handle) != 0:
            _check(self.lib)
            raise UnpaperHipError("tiff_writer_finish failed")

    def close(self):
        if self.handle:
            self.lib.uphip_tiff_writer_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _png(fn, ptr, pitch, offset, width, height, fmt, dpi):
    L = load_library()
    n = fn(ptr, pitch, offset, width, height, fmt, dpi, None, 0)
    _check(L)
    if n <= 0:
        raise UnpaperHipError("png encode failed")
    buf = np.zeros(n, np.uint8)
    m = fn(ptr, pitch, offset, width, height, fmt, dpi, buf.ctypes.data, n)
    _check(L)
    if m != n:
        raise UnpaperHipError("png encode: size changed between calls")
    return buf.tobytes()


def png_encode(device_ptr, pitch, width, height, fmt, offset=0, dpi=0):
    """uphip_png_encode: rows in device memory -> a lossless PNG file (`offset`:
    the bit of a row that holds pixel 0, bilevel formats only)."""
    return _png(load_library().uphip_png_encode, device_ptr, pitch, offset, width, height, fmt, dpi)


def png_encode_host(rows, width, fmt, offset=0, dpi=0):
    """uphip_png_encode_host: a 2-D uint8 array of rows (no device); the same
    bytes as png_encode."""
    rows = np.ascontiguousarray(rows, np.uint8)
    return _png(load_library().uphip_png_encode_host, rows.ctypes.data, rows.shape[1], offset, width,
                rows.shape[0], fmt, dpi)


def png_wrap(stream: bytes, width, height, fmt, dpi=0):
    """uphip_png_wrap: a zlib stream of the encoder as a PNG file."""
    L = load_library()
    n = L.uphip_png_wrap(stream, len(stream), width, height, fmt, dpi, None, 0)
    _check(L)
    if n <= 0:
        raise UnpaperHipError("png_wrap failed")
    buf = np.zeros(n, np.uint8)
    if L.uphip_png_wrap(stream, len(stream), width, height, fmt, dpi, buf.ctypes.data, n) != n:
        _check(L)
        raise UnpaperHipError("png_wrap failed")
    return buf.tobytes()


def _g4(fn, ptr, pitch, bit_offset, width, height):
    L = load_library()
    n = fn(ptr, pitch, bit_offset, width, height, None, 0)
    _check(L)
    if n <= 0:
        raise UnpaperHipError("g4 encode failed")
    buf = np.zeros(n, np.uint8)
    m = fn(ptr, pitch, bit_offset, width, height, buf.ctypes.data, n)
    _check(L)
    if m != n:
        raise UnpaperHipError("g4 encode: size changed between calls")
    return buf.tobytes()


def g4_encode(device_ptr, pitch, width, height, bit_offset=0):
    """uphip_g4_encode: packed 1-bit rows in device memory (1 = black, pixel
    0 at bit `bit_offset` of a row) -> CCITT Group 4 stream."""
    return _g4(load_library().uphip_g4_encode, device_ptr, pitch, bit_offset, width, height)


def g4_encode_host(rows, width, bit_offset=0):
    """uphip_g4_encode_host: a 2-D uint8 array of packed rows (no device)."""
    rows = np.ascontiguousarray(rows, np.uint8)
    return _g4(load_library().uphip_g4_encode_host, rows.ctypes.data, rows.shape[1], bit_offset, width,
               rows.shape[0])


def tiff_g4_write(path, stream: bytes, width, height, dpi=0):
    """uphip_tiff_g4_write: a Group 4 stream as a one-strip TIFF file."""
    L = load_library()
    if L.uphip_tiff_g4_write(path.encode(), stream, len(stream), width, height, dpi) != 0:
        _check(L)
        raise UnpaperHipError("tiff_g4_write failed")


def sink_discard():
    L = load_library()
    return _Handle(L.uphip_sink_discard(), L.uphip_sink_destroy)


def pnm_write(path, h: HostImage):
    L = load_library()
    arr = np.ascontiguousarray(h.data)
    if L.uphip_pnm_write(path.encode(), arr.ctypes.data, arr.shape[1], h.width, h.height,
                         h.format) != 0:
        _check(L)


def pnm_read(path) -> HostImage:
    L = load_library()
    info = A.PnmInfo()
    if L.uphip_pnm_probe(path.encode(), C.byref(info)) != 0:
        _check(L)
    img = HostImage(info.width, info.height, info.format)
    if L.uphip_pnm_read(path.encode(), img.data.ctypes.data, img.linesize, C.byref(info)) != 0:
        _check(L)
    return img


def image_read(path) -> HostImage:
    """loadImage's peer (file.c:29-131): PNG or PNM, picked by signature."""
    L = load_library()
    info = A.PnmInfo()
    if L.uphip_image_probe(path.encode(), C.byref(info)) != 0:
        _check(L)
    img = HostImage(info.width, info.height, info.format)
    if L.uphip_image_read(path.encode(), img.data.ctypes.data, img.linesize, C.byref(info)) != 0:
        _check(L)
    return img
