"""GPU tests of the TIFF device decode (csrc/kernels_tiff.hip: a lane per
strip over the decoder of csrc/tiff_strip.h, a wave per row) and of TIFF pages
in the runner.  Every comparison is exact: uphip_tiff_decode equals the host
twin (uphip_tiff_read_page) equals PIL; runner sheets equal the sheets of the
same pages fed as PGM."""

import numpy as np
import pytest
from PIL import Image

import tiff_cases as T
from unpaper_hip import ctypes_abi as A
from unpaper_hip.device import UnpaperHipError
from unpaper_hip.hostimage import HostImage
from unpaper_hip.pipeline import (DeviceBuffer, Runner, TiffDocument, image_read, pnm_read, pnm_write,
                                  sink_memory, sink_pnm, sink_tiff_g4, source_page_count, source_pnm,
                                  source_tiff, synth_page_host, tiff_decode)

pytestmark = pytest.mark.gpu

SMALL = (620, 877)  # the runner tests' small page (tests/test_runner_gpu.py)
# the 9-bit codes Clear, 'A', 300: 300 is above the next free code (258)
LZW_BAD_CODE = bytes([0x80, 0x10, 0x65, 0x80])


def _fill2_packbits(path):
    """1-bit 701x90, PackBits, MinIsWhite, FillOrder 2, nine strips."""
    w, h, rps = 701, 90, 10
    bits = (T.noise(h * w, 12).reshape(h, w) > 150).astype(np.uint8)
    rows = np.packbits(bits, axis=1)
    strips = [T.BITREV[np.frombuffer(T.packbits_literal(rows[i:i + rps]), np.uint8)].tobytes()
              for i in range(0, h, rps)]
    with open(path, "wb") as f:
        f.write(T.build(w, h, strips, rps, {258: (3, [1]), 259: (3, [32773]), 262: (3, [0]), 266: (3, [2]),
                                            277: (3, [1])}))


CASES = {
    "L-333x50-rps3": lambda p: T.save(p, T.page("L", 333, 50), "tiff_lzw", rps=3),
    "L-2481x130-rps26": lambda p: T.save(p, T.page("L", 2481, 130), "tiff_lzw", rps=26),
    "L-65-strips": lambda p: T.save(p, T.page("L", 97, 65), "tiff_lzw", rps=1),
    "RGB-500x40-rps1-pred2": lambda p: T.save(p, T.page("RGB", 500, 40), "tiff_lzw", rps=1, predictor=2),
    "LA-pred2": lambda p: T.save(p, T.page("LA", 333, 50), "tiff_lzw", rps=3, predictor=2),
    "P": lambda p: T.save(p, T.page("P", 333, 50), "tiff_lzw", rps=7),
    "L-miniswhite-packbits": lambda p: T.save(p, T.page("L", 333, 50), "packbits", rps=3, tags={262: 0}),
    "1-fill2-packbits": _fill2_packbits,
    "lzw-mid-strip-clear": lambda p: T.save(p, Image.fromarray(T.noise(60000, 5).reshape(200, 300), "L"),
                                            "tiff_lzw", rps=200),
    "lzw-all-white": lambda p: T.save(p, Image.new("L", (2481, 26), 255), "tiff_lzw", rps=26),
}


def _decode_guarded(hip, data, fmt, w, h, page=0):
    """uphip_tiff_decode into rows 37 bytes wider than the page, a row of
    sentinel above and below: (rows, whole buffer, pitch, row bytes)."""
    rb = T.row_bytes(fmt, w)
    pitch = rb + 37
    host = np.full((h + 2, pitch), 0xA5, np.uint8)
    buf = DeviceBuffer(host.nbytes)
    try:
        assert hip.lib.uphip_memcpy_htod(buf.ptr, host.ctypes.data, host.nbytes) == 0
        err = None
        try:
            assert tiff_decode(data, page, buf.ptr + pitch, pitch) == (w, h, fmt)
        except UnpaperHipError as e:
            err = str(e)
        assert hip.lib.uphip_memcpy_dtoh(host.ctypes.data, buf.ptr, host.nbytes) == 0
    finally:
        buf.close()
    assert (host[0] == 0xA5).all() and (host[-1] == 0xA5).all() and (host[1:-1, rb:] == 0xA5).all()
    return host[1:-1], err


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_decode_equals_host_equals_pil(hip, tmp_path, name):
    path = str(tmp_path / "case.tif")
    CASES[name](path)
    fmt, w, h, want = T.expected(path)
    d = TiffDocument(path)
    try:
        assert np.array_equal(T.pixels(fmt, w, d.read_page(0).data), want), "host twin"
    finally:
        d.close()
    rows, err = _decode_guarded(hip, open(path, "rb").read(), fmt, w, h)
    assert err is None
    assert np.array_equal(T.pixels(fmt, w, rows), want), "device"


def _corrupt_file(tmp_path, name):
    """Three pages of 333x50 in 17 strips, the middle one with a strip that
    cannot decode; every case is deterministic and the host twin refuses it
    too.  Returns (path, the pages' expected rows)."""
    comp = "packbits" if name == "run-past-end" else "tiff_lzw"
    path = str(tmp_path / (name + ".tif"))
    T.save(path, T.page("L", 333, 50, 1), comp, rps=3, more=[T.page("L", 333, 50, 2), T.page("L", 333, 50, 3)])
    want = [T.expected(path, p)[3] for p in range(3)]
    off, cnt, _ = T.strips(path, 1)
    raw = bytearray(open(path, "rb").read())
    if name == "truncated":          # strip 5 cut in half
        T.patch_array(raw, 1, 279, 5, cnt[5] // 2)
    elif name == "bad-code":         # strip 11 starts Clear, 'A', 300
        raw[off[11]:off[11] + 4] = LZW_BAD_CODE
    else:                            # strip 7: eight runs of 128 into three rows of 333
        assert cnt[7] >= 16
        raw[off[7]:off[7] + 16] = bytes([0x81, 7]) * 8
    with open(path, "wb") as f:
        f.write(bytes(raw))
    return path, want


CORRUPT = [("truncated", "end too early"), ("bad-code", "cannot occur"), ("run-past-end", "passes the strip")]


@pytest.mark.parametrize("name,word", CORRUPT)
def test_corrupt_strip_sets_the_status(hip, tmp_path, name, word):
    path, want = _corrupt_file(tmp_path, name)
    d = TiffDocument(path)
    try:
        assert d.probe(1)[:3] == (333, 50, A.FMT_GRAY8) and d.on_device(1)
        with pytest.raises(UnpaperHipError, match=word):
            d.read_page(1)
    finally:
        d.close()
    data = open(path, "rb").read()
    _, err = _decode_guarded(hip, data, A.FMT_GRAY8, 333, 50, page=1)
    assert err is not None and word in err
    rows, err = _decode_guarded(hip, data, A.FMT_GRAY8, 333, 50, page=2)
    assert err is None and np.array_equal(rows[:, :333], want[2])


def test_device_decode_refuses_other_pages(hip, tmp_path):
    path = T.save(str(tmp_path / "z.tif"), T.page("L", 64, 16), "tiff_adobe_deflate")
    _, err = _decode_guarded(hip, open(path, "rb").read(), A.FMT_GRAY8, 64, 16)
    assert err is not None and "Compression 8" in err


# ---- the runner -------------------------------------------------------------------

def _pages(n, first=200):
    w, h = SMALL
    return [synth_page_host(w, h, first + i) for i in range(n)]


def _run(opts, n, src, fmt=A.FMT_GRAY8, sheets=3):
    w, h = SMALL
    r = Runner(opts, sheets, w, h, fmt, devices=(0,), streams=2, host_threads=3)
    try:
        out = np.zeros((n, r.out_height, r.out_linesize), np.uint8)
        snk = sink_memory(out.ctypes.data, r.out_linesize, r.out_linesize * r.out_height, n, keep=out)
        failed, err = r.run_host(n, src, snk)
        # the sheets' bytes only: what lies between a row's end and the linesize is not output
        return failed, err, out[:, :, :T.row_bytes(r.out_format, r.out_width)], r.stats().jobs_failed
    finally:
        r.close()


def _write_pgms(tmp_path, pages):
    paths = []
    for i, a in enumerate(pages):
        paths.append(str(tmp_path / ("p%d.pgm" % i)))
        pnm_write(paths[-1], HostImage.from_array(a, A.FMT_GRAY8))
    return paths


def test_runner_mixed_sources(hip, oracle, tmp_path):
    """PGM, LZW TIFF and Deflate TIFF pages in one source_pnm list give the
    sheets of the all-PGM run."""
    n = 7
    opts = oracle.default_options()
    pages = _pages(n)
    pgm = _write_pgms(tmp_path, pages)
    mixed = list(pgm)
    for i, a in enumerate(pages):
        if i % 3 == 0:
            continue
        mixed[i] = str(tmp_path / ("p%d.tif" % i))
        T.save(mixed[i], Image.fromarray(a, "L"), "tiff_lzw" if i % 3 == 1 else "tiff_adobe_deflate",
               predictor=2 if i == 1 else None)
    failed, err, want, _ = _run(opts, n, source_pnm(pgm))
    assert failed == 0, err
    failed, err, got, _ = _run(opts, n, source_pnm(mixed))
    assert failed == 0, err
    assert want.any() and np.array_equal(got, want)


def _five_page_file(tmp_path, pages):
    path = str(tmp_path / "doc.tif")
    ims = [Image.fromarray(a, "L") for a in pages]
    T.save(path, ims[0], "tiff_lzw", more=ims[1:])
    return path


def test_runner_source_tiff_both_routes(hip, oracle, tmp_path):
    n = 5
    opts = oracle.default_options()
    pages = _pages(n, 300)
    failed, err, want, _ = _run(opts, n, source_pnm(_write_pgms(tmp_path, pages)))
    assert failed == 0, err
    path = _five_page_file(tmp_path, pages)
    d = TiffDocument(path)
    try:
        assert d.page_count == n and all(d.on_device(p) for p in range(n))  # the device route takes them all
    finally:
        d.close()
    for flags in (0, A.TIFF_HOST_DECODE, A.TIFF_DEVICE_DECODE):
        src = source_tiff(path, flags)
        assert source_page_count(src) == n
        failed, err, got, _ = _run(opts, n, src)
        assert failed == 0, err
        assert np.array_equal(got, want), "flags %d" % flags


def test_runner_corrupt_middle_page_fails_alone(hip, oracle, tmp_path):
    """Page 2 of five with a strip that holds an impossible LZW code: its job
    fails on the device, the four others (two of them in its chunk, decoded by
    the same launch) give their sheets."""
    n = 5
    opts = oracle.default_options()
    pages = _pages(n, 300)
    failed, err, want, _ = _run(opts, n, source_pnm(_write_pgms(tmp_path, pages)))
    assert failed == 0, err
    path = _five_page_file(tmp_path, pages)
    off, cnt, _ = T.strips(path, 2)
    raw = bytearray(open(path, "rb").read())
    raw[off[3]:off[3] + 4] = LZW_BAD_CODE
    with open(path, "wb") as f:
        f.write(bytes(raw))
    failed, err, got, nfailed = _run(opts, n, source_tiff(path, A.TIFF_DEVICE_DECODE))
    assert failed == 1 and nfailed == 1 and "TIFF strip (device decode)" in err
    for i in (0, 1, 3, 4):
        assert np.array_equal(got[i], want[i]), i
    assert not got[2].any()
    # the host route refuses the same page
    failed, err, got, nfailed = _run(opts, n, source_tiff(path, A.TIFF_HOST_DECODE))
    assert failed == 1 and nfailed == 1
    for i in (0, 1, 3, 4):
        assert np.array_equal(got[i], want[i]), i


@pytest.mark.parametrize("name,word", CORRUPT)
def test_runner_good_pages_beside_a_corrupt_one(hip, oracle, tmp_path, name, word):
    """[good, corrupt, good] as one chunk on the device route, so one launch
    decodes all three: the corrupt page fails alone."""
    path, want = _corrupt_file(tmp_path, name)
    w, h = 333, 50
    opts = oracle.default_options()
    opts.disable = A.NO_PROCESSING
    r = Runner(opts, 3, w, h, A.FMT_GRAY8, devices=(0,), streams=1, host_threads=2)
    try:
        out = np.zeros((3, r.out_height, r.out_linesize), np.uint8)
        snk = sink_memory(out.ctypes.data, r.out_linesize, r.out_linesize * r.out_height, 3, keep=out)
        failed, err = r.run_host(3, source_tiff(path, A.TIFF_DEVICE_DECODE), snk)
    finally:
        r.close()
    assert failed == 1 and "TIFF strip (device decode)" in err
    for i in (0, 2):
        assert np.array_equal(out[i][:, :w], want[i]), i
    assert not out[1].any()


def test_runner_reads_back_its_g4_tiffs(hip, oracle, tmp_path):
    """A bilevel run into uphip_sink_tiff_g4 and uphip_sink_pnm; the TIFFs fed
    back through uphip_source_pnm are the PBM pages."""
    w, h = SMALL
    n = 3
    opts = oracle.default_options()
    opts.disable = A.NO_PROCESSING
    opts.output_pixel_format = A.FMT_MONOWHITE
    pgm = _write_pgms(tmp_path, _pages(n, 400))
    for sink in (sink_pnm(str(tmp_path / "o%d.pbm")), sink_tiff_g4(str(tmp_path / "o%d.tif"), dpi=200)):
        r = Runner(opts, 2, w, h, A.FMT_GRAY8, devices=(0,), streams=2, host_threads=2)
        try:
            failed, err = r.run_host(n, source_pnm(pgm), sink)
            assert failed == 0, err
        finally:
            r.close()
    tifs = [str(tmp_path / ("o%d.tif" % i)) for i in range(n)]
    pbms = [str(tmp_path / ("o%d.pbm" % i)) for i in range(n)]
    for t, p in zip(tifs, pbms):
        a, b = image_read(t), pnm_read(p)
        assert (a.width, a.height, a.format) == (b.width, b.height, b.format) == (w, h, A.FMT_MONOWHITE)
        assert np.array_equal(a.payload(), b.payload())
    back = oracle.default_options()
    back.disable = A.NO_PROCESSING
    failed, err, want, _ = _run(back, n, source_pnm(pbms), fmt=A.FMT_MONOWHITE)
    assert failed == 0, err
    failed, err, got, _ = _run(back, n, source_pnm(tifs), fmt=A.FMT_MONOWHITE)
    assert failed == 0, err
    assert want.any() and np.array_equal(got, want)
