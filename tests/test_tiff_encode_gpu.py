"""GPU tests of TIFF output: the device Deflate encoder
(csrc/kernels_tiff_enc.hip) against its host twin over the same core, the
batch encode and the runner's TIFF sinks.  Every comparison is exact.  The
host twin itself is checked against PIL, the project's TIFF reader and a hand
decode by test_tiff_encode.py."""
import ctypes as C
import os

import numpy as np
import pytest

import tiff_enc_cases as K
from helpers import page_array
from unpaper_hip import ctypes_abi as A
from unpaper_hip.hostimage import HostImage
from unpaper_hip.pipeline import (Batch, DeviceBuffer, Runner, TiffDocument, pnm_read, pnm_write, sink_pnm,
                                  sink_tiff, sink_tiff_g4, sink_tiff_multipage, source_pnm, source_tiff,
                                  tiff_encode, tiff_encode_host, tiff_encode_pages)

pytestmark = pytest.mark.gpu


def _upload(rows):
    rows = np.ascontiguousarray(rows, np.uint8)
    buf = DeviceBuffer(rows.nbytes)
    assert buf.lib.uphip_memcpy_htod(buf.ptr, rows.ctypes.data, rows.nbytes) == 0
    return buf


def _blob(data):
    """The packed page inside a one-page Deflate file."""
    t = K.ifds(data)[0][0]
    return data[8: t[273][1][-1] + t[279][1][-1]]


@pytest.mark.parametrize("case", K.CASES, ids=K.CASE_IDS)
def test_device_encoder_equals_host(hip, case):
    name, fmt, width, rows = case
    want = tiff_encode_host(rows, width, fmt, dpi=200)
    buf = _upload(rows)
    try:
        assert tiff_encode(buf.ptr, rows.shape[1], width, rows.shape[0], fmt, dpi=200) == want
    finally:
        buf.close()


@pytest.mark.parametrize("name", ["gray_257_short_last", "rgb_85_equal_rows", "ya_87_equal_rows"])
def test_device_encoder_pitch_and_alignment(hip, name):
    """The image inside rows of an odd pitch with garbage in the padding, 3
    bytes into the buffer: rows start at every alignment of a dword."""
    _, fmt, width, rows = K.CASES[K.CASE_IDS.index(name)]
    want = tiff_encode_host(rows, width, fmt)
    big = K.embed(rows, 13, 7)
    flat = np.concatenate([np.full(3, 0xA5, np.uint8), big.ravel(), np.full(8, 0xA5, np.uint8)])
    buf = _upload(flat)
    try:
        assert tiff_encode(buf.ptr + 3, big.shape[1], width, rows.shape[0], fmt) == want
    finally:
        buf.close()


def test_output_buffer_sentinels(hip):
    """The file lands in a buffer of exactly its size; the bytes around it stay."""
    L = hip.lib
    _, fmt, width, rows = K.CASES[K.CASE_IDS.index("gray_stored_between_flat")]
    want = tiff_encode_host(rows, width, fmt)
    buf = _upload(rows)
    try:
        out = np.full(len(want) + 128, 0x5A, np.uint8)
        n = L.uphip_tiff_encode(buf.ptr, rows.shape[1], 0, width, rows.shape[0], fmt, 0, out.ctypes.data + 64,
                                len(want))
        assert n == len(want) and out[64:64 + n].tobytes() == want
        assert (out[:64] == 0x5A).all() and (out[64 + n:] == 0x5A).all()
        # one byte short: refused, nothing written
        out[:] = 0x5A
        assert L.uphip_tiff_encode(buf.ptr, rows.shape[1], 0, width, rows.shape[0], fmt, 0, out.ctypes.data + 64,
                                   len(want) - 1) == -1
        assert b"buffer" in L.uphip_last_error()
        L.uphip_clear_error()
        assert (out == 0x5A).all()
    finally:
        buf.close()


def test_device_output_guard_bands(hip):
    """The encoder packs two pages into device memory the test lends, between
    bands of 0x5A.  Page 0 has a noise strip between text strips (stored and
    coded streams side by side), the last strips are 3 rows, and the packed
    total ends off a dword, so the last stream's final word is a shared one.
    The encoder may touch the lent bytes only: the packed pages, then zeros up
    to the documented bound; both bands stay."""
    L = hip.lib
    w, rps = 255, 257
    h = 2 * rps + 3
    assert K.rows_per_strip(w, h) == rps
    for seed in range(20, 40):  # a total off a dword (the host twin says which input has one)
        rng = np.random.default_rng(seed)
        pages = np.stack([K._text(rng, h, w) for _ in range(2)])
        pages[0, rps:2 * rps] = rng.integers(0, 256, (rps, w), dtype=np.uint8)
        want = b"".join(_blob(tiff_encode_host(pages[i], w, A.FMT_GRAY8)) for i in range(2))
        if len(want) % 4:
            break
    assert len(want) % 4
    bound = 4 * 3 + 2 * K.stored_size(rps * w) + K.stored_size(3 * w)
    need = (2 * bound + 3) // 4 * 4 + 4
    band = 256
    src = _upload(pages)
    dst = _upload(np.full(need + 2 * band, 0x5A, np.uint8))
    try:
        got = tiff_encode_pages(src.ptr, w, w * h, 2, w, h, A.FMT_GRAY8, device_out=dst.ptr + band,
                                device_capacity=need)
        back = np.zeros(need + 2 * band, np.uint8)
        assert L.uphip_memcpy_dtoh(back.ctypes.data, dst.ptr, back.nbytes) == 0
        for cap, ptr in ((need - 1, dst.ptr + band), (need, dst.ptr + band + 1)):
            assert L.uphip_tiff_encode_pages(src.ptr, w, w * h, 2, w, h, A.FMT_GRAY8, 0, None, None, 0, ptr, cap) == -1
            assert b"lent output" in L.uphip_last_error()
            L.uphip_clear_error()
    finally:
        src.close()
        dst.close()
    assert b"".join(got) == want
    assert (back[:band] == 0x5A).all(), "bytes before the device output"
    assert back[band:band + len(want)].tobytes() == want
    assert not back[band + len(want):band + need].any(), "bytes after the packed pages, inside the bound"
    assert (back[band + need:] == 0x5A).all(), "bytes after the device output"


def test_device_encoder_argument_errors(hip):
    L = hip.lib
    buf = DeviceBuffer(1 << 18)
    try:
        # a row too wide for the block's LDS is refused before any launch
        assert L.uphip_tiff_encode(buf.ptr, 200000, 0, 200000, 1, A.FMT_GRAY8, 0, None, 0) == -1
        assert b"k_tiff_predict" in L.uphip_last_error()
        L.uphip_clear_error()
        assert L.uphip_tiff_encode(buf.ptr, 2, 0, 16, 4, A.FMT_MONOBLACK, 0, None, 0) == -1
        assert b"MONOBLACK" in L.uphip_last_error()
        L.uphip_clear_error()
        for args in ((None, 16, 0, 16, 4, A.FMT_GRAY8), (buf.ptr, 16, 0, 0, 4, A.FMT_GRAY8),
                     (buf.ptr, 16, 0, 16, 0, A.FMT_GRAY8), (buf.ptr, 16, 0, 16, 4, 12),
                     (buf.ptr, 16, 2, 8, 4, A.FMT_GRAY8), (buf.ptr, 2, 1, 16, 4, A.FMT_MONOWHITE)):
            assert L.uphip_tiff_encode(*args, 0, None, 0) == -1, args
            assert L.uphip_last_error()
            L.uphip_clear_error()
    finally:
        buf.close()


def test_monowhite_is_the_group4_file(hip):
    rng = np.random.default_rng(3)
    w, h = 203, 57
    bits = rng.random((h, w + 5)) < 0.1
    rows = np.packbits(bits, axis=1)
    buf = _upload(rows)
    try:
        got = tiff_encode(buf.ptr, rows.shape[1], w, h, A.FMT_MONOWHITE, offset=5, dpi=150)
    finally:
        buf.close()
    assert got == tiff_encode_host(rows, w, A.FMT_MONOWHITE, offset=5, dpi=150)


def test_streams_fold_onto_the_grid(hip):
    """Two pages of four strips with the launcher's limit at 3 streams: blocks
    take streams y, y + 3, y + 6.  Page 1's strip 2 is noise, so a stored
    stream is among the folded ones.  The pages equal the unfolded encode and
    the host twin."""
    L = hip.lib
    rng = np.random.default_rng(11)
    w, h = 256, 4 * 256 - 10
    pages = np.stack([K._text(rng, h, w) for _ in range(2)])
    pages[1, 512:768] = rng.integers(0, 256, (256, w), dtype=np.uint8)
    assert K.rows_per_strip(w, h) == 256
    buf = _upload(pages)
    try:
        folded = tiff_encode_pages(buf.ptr, w, w * h, 2, w, h, A.FMT_GRAY8, fold=3)
        plain = tiff_encode_pages(buf.ptr, w, w * h, 2, w, h, A.FMT_GRAY8)
        one = tiff_encode_pages(buf.ptr, w, w * h, 2, w, h, A.FMT_GRAY8, fold=1)
        for bad in (-1, 65536):
            assert L.uphip_tiff_encode_pages(buf.ptr, w, w * h, 2, w, h, A.FMT_GRAY8, bad, None, None, 0, None, 0) == -1
            assert b"k_tiff_hist" in L.uphip_last_error()
            L.uphip_clear_error()
    finally:
        buf.close()
    want = [_blob(tiff_encode_host(pages[i], w, A.FMT_GRAY8)) for i in range(2)]
    assert folded == want and plain == want and one == want


def _pages(n, w, h, seed, fmt):
    return [HostImage.from_array(page_array(w, h, seed + i, specks=30, color=fmt == A.FMT_RGB24), fmt)
            for i in range(n)]


def _plain_options(oracle, output_count, out_fmt):
    """The pages as they are (thresholded for MONOWHITE output)."""
    opts = oracle.default_options()
    opts.disable = A.NO_PROCESSING
    if out_fmt == A.FMT_MONOWHITE:
        opts.output_pixel_format = A.FMT_MONOWHITE
    if output_count == 2:
        opts.layout = A.LAYOUT_DOUBLE
        opts.output_count = 2
    return opts


@pytest.mark.parametrize("out_fmt", [A.FMT_GRAY8, A.FMT_RGB24], ids=["gray", "rgb"])
@pytest.mark.parametrize("output_count", [1, 2])
def test_batch_encode_equals_host(hip, oracle, output_count, out_fmt):
    """Three 1240 x 1754 sheets (pages 620 wide in the double layout: page 1
    starts in the middle of a row).  Sheet 1 is overwritten with random bytes
    on the device after the run, so every strip of its pages leaves stored.
    Every page equals the host twin on the sheet's own pixels."""
    w, h, n = 1240, 1754, 3
    pw = w // output_count
    ch = K.CHANNELS[out_fmt]
    b = Batch(_plain_options(oracle, output_count, out_fmt), n, w, h, out_fmt)
    try:
        assert (b.out_width, b.out_height, b.out_format) == (w, h, out_fmt)
        for s, p in enumerate(_pages(n, w, h, 40, out_fmt)):
            b.set_input(s, 0, p)
        b.run(n)
        b.wait()
        before = C.c_int64()
        assert b.lib.uphip_batch_device_bytes(b.handle, C.byref(before)) == 0
        ptr, pitch = b.output_ptr(1)
        noise = np.random.default_rng(8).integers(0, 256, (h, pitch), dtype=np.uint8)
        assert b.lib.uphip_memcpy_htod(ptr, noise.ctypes.data, noise.nbytes) == 0
        b.encode_tiff()
        blobs = b.tiff_pages(n * output_count)
        after = C.c_int64()
        assert b.lib.uphip_batch_device_bytes(b.handle, C.byref(after)) == 0
        # the encode buffers are counted: at least the predicted bytes and the pages' bound
        assert after.value - before.value >= 2 * n * w * ch * h
        sheets = [b.output(s) for s in range(n)]
        for i, blob in enumerate(blobs):
            s, j = divmod(i, output_count)
            want = tiff_encode_host(sheets[s].data[:, j * pw * ch:], pw, out_fmt)
            assert blob == _blob(want), "page %d" % i
            _, strips = K.hand_decode(want, K.ifds(want)[0][0])
            assert all(st[2] == (s == 1) for st in strips), "page %d" % i
        assert len(set(blobs)) == len(blobs)
        # a second encode on the same buffers gives the same pages
        b.encode_tiff()
        assert b.tiff_pages(n * output_count) == blobs
    finally:
        b.close()


def test_batch_encode_refuses_bilevel(hip, oracle):
    w, h = 130, 96
    b = Batch(_plain_options(oracle, 1, A.FMT_MONOWHITE), 1, w, h, A.FMT_GRAY8)
    try:
        b.set_input(0, 0, _pages(1, w, h, 1, A.FMT_GRAY8)[0])
        b.run(1)
        b.wait()
        with pytest.raises(Exception, match="uphip_batch_encode_g4_async"):
            b.encode_tiff()
    finally:
        b.close()


def _write_inputs(tmp_path, pages, missing=()):
    paths = []
    for i, p in enumerate(pages):
        q = str(tmp_path / ("in_%03d.pnm" % i))
        if i not in missing:
            pnm_write(q, p)
        paths.append(q)
    return paths


def _run(opts, source, n, w, h, sink, fmt):
    r = Runner(opts, 2, w, h, fmt, devices=(0,), streams=2, host_threads=2)
    try:
        return r.run_host(n, source, sink)
    finally:
        r.close()


@pytest.mark.parametrize("output_count,out_fmt", [(1, A.FMT_GRAY8), (2, A.FMT_GRAY8), (1, A.FMT_RGB24)],
                         ids=["gray1", "gray2", "rgb1"])
def test_runner_tiff_sinks_equal_pnm(hip, oracle, tmp_path, output_count, out_fmt):
    """Six jobs (three chunks of two sheets on two streams), the file of job
    3 missing, through sink_pnm, sink_tiff and sink_tiff_multipage: every page
    present decodes in PIL and in the project's reader to exactly the PNM
    page, in order; the missing job's pages are left out and the rest
    renumbered.  The multi-page file fed back through uphip_source_tiff into a
    run whose stages are all off returns the same pages."""
    from PIL import Image
    w, h, n, bad = 406, 400, 6, 3  # 400 rows of 406 (1218) bytes: three (two) strips a page
    oc = output_count
    pw = w // oc
    ch = K.CHANNELS[out_fmt]
    opts = _plain_options(oracle, oc, out_fmt)
    paths = _write_inputs(tmp_path, _pages(n, w, h, 60, out_fmt), missing=(bad,))
    runs = [sink_pnm(str(tmp_path / "p%03d.pnm")), sink_tiff(str(tmp_path / "q%03d.tif"), dpi=150),
            sink_tiff_multipage(str(tmp_path / "doc.tif"), dpi=150)]
    for sink in runs:
        failed, err = _run(opts, source_pnm(paths), n, w, h, sink, out_fmt)
        assert failed == 1 and "could not be loaded" in err
    runs[2].finish()
    present = [i for i in range(n * oc) if i // oc != bad]
    want = {}
    for i in present:
        pnm = pnm_read(str(tmp_path / ("p%03d.pnm" % i)))
        assert (pnm.width, pnm.height, pnm.format) == (pw, h, out_fmt)
        want[i] = pnm.data[:, :pw * ch].copy()
    assert len({v.tobytes() for v in want.values()}) == len(present)  # the order check means something
    for i in range(n * oc):
        assert os.path.exists(str(tmp_path / ("q%03d.tif" % i))) == (i in present)
    # one file per page: the host twin's file for the page's pixels
    for i in present:
        with open(str(tmp_path / ("q%03d.tif" % i)), "rb") as f:
            assert f.read() == tiff_encode_host(want[i], pw, out_fmt, dpi=150), "file %d" % i
    # the multi-page file through PIL
    mode = {A.FMT_GRAY8: "L", A.FMT_RGB24: "RGB"}[out_fmt]
    with Image.open(str(tmp_path / "doc.tif")) as im:
        assert im.n_frames == len(present)
        for k, i in enumerate(present):
            im.seek(k)
            assert im.size == (pw, h) and im.mode == mode
            assert abs(float(im.info["dpi"][0]) - 150) < 0.05
            assert np.array_equal(np.array(im).reshape(h, -1), want[i]), "PIL page %d" % i
    # through the project's reader, and by hand
    with open(str(tmp_path / "doc.tif"), "rb") as f:
        data = f.read()
    tags, _ = K.ifds(data)
    assert [t[297][1] for t in tags] == [[k, len(present)] for k in range(len(present))]
    d = TiffDocument(str(tmp_path / "doc.tif"))
    try:
        assert d.page_count == len(present)
        for k, i in enumerate(present):
            assert d.probe(k)[:3] == (pw, h, out_fmt)
            assert np.array_equal(d.read_page(k).data[:, :pw * ch], want[i]), "page %d" % i
            assert np.array_equal(K.hand_decode(data, tags[k])[0], want[i]), "page %d" % i
    finally:
        d.close()
    # round trip: the file as the source of a run that changes nothing
    back = _plain_options(oracle, 1, out_fmt)
    failed, err = _run(back, source_tiff(str(tmp_path / "doc.tif")), len(present), pw, h,
                       sink_pnm(str(tmp_path / "r%03d.pnm")), out_fmt)
    assert failed == 0, err
    for k, i in enumerate(present):
        pnm = pnm_read(str(tmp_path / ("r%03d.pnm" % k)))
        assert (pnm.width, pnm.height, pnm.format) == (pw, h, out_fmt)
        assert np.array_equal(pnm.data[:, :pw * ch], want[i]), "round trip page %d" % i


def test_runner_bilevel_pages_are_group4(hip, oracle, tmp_path):
    """A MONOWHITE run: sink_tiff writes the files of sink_tiff_g4, and the
    multi-page file's pages hold the same Group 4 streams, one strip each."""
    w, h, n, oc = 406, 131, 5, 2
    pw = w // oc
    opts = _plain_options(oracle, oc, A.FMT_MONOWHITE)
    paths = _write_inputs(tmp_path, _pages(n, w, h, 80, A.FMT_GRAY8))
    runs = [sink_tiff_g4(str(tmp_path / "g%03d.tif"), dpi=200), sink_tiff(str(tmp_path / "q%03d.tif"), dpi=200),
            sink_tiff_multipage(str(tmp_path / "doc.tif"), dpi=200)]
    for sink in runs:
        failed, err = _run(opts, source_pnm(paths), n, w, h, sink, A.FMT_GRAY8)
        assert failed == 0, err
    runs[2].finish()
    with open(str(tmp_path / "doc.tif"), "rb") as f:
        data = f.read()
    tags, _ = K.ifds(data)
    assert len(tags) == n * oc
    seen = set()
    for i in range(n * oc):
        with open(str(tmp_path / ("g%03d.tif" % i)), "rb") as f:
            g = f.read()
        with open(str(tmp_path / ("q%03d.tif" % i)), "rb") as f:
            assert f.read() == g, "file %d" % i
        st = K.ifds(g)[0][0]
        stream = g[st[273][1][0]: st[273][1][0] + st[279][1][0]]
        seen.add(stream)
        t = tags[i]
        assert t[259][1] == [4] and t[256][1] == [pw] and t[257][1] == [h] and t[278][1] == [h]
        assert t[297][1] == [i, n * oc] and t[282][1] == [(200, 1)]
        assert data[t[273][1][0]: t[273][1][0] + t[279][1][0]] == stream, "page %d" % i
    assert len(seen) == n * oc


def test_runner_monoblack_request_leaves_as_group4(hip, oracle, tmp_path):
    """A batch asked for MONOBLACK saves MONOWHITE sheets (saveImage's
    mapping), so the TIFF sink's pages are Group 4; a sink destroyed
    unfinished leaves no file."""
    w, h = 203, 131
    opts = oracle.default_options()
    opts.disable = A.NO_PROCESSING
    opts.output_pixel_format = A.FMT_MONOBLACK
    paths = _write_inputs(tmp_path, _pages(2, w, h, 60, A.FMT_GRAY8))
    sink = sink_tiff_multipage(str(tmp_path / "doc.tif"))
    failed, err = _run(opts, source_pnm(paths), 2, w, h, sink, A.FMT_GRAY8)
    assert failed == 0, err
    sink.finish()
    with open(str(tmp_path / "doc.tif"), "rb") as f:
        tags, _ = K.ifds(f.read())
    assert [t[259][1] for t in tags] == [[4], [4]]
    gone = sink_tiff_multipage(str(tmp_path / "gone.tif"))
    failed, err = _run(opts, source_pnm(paths), 2, w, h, gone, A.FMT_GRAY8)
    assert failed == 0, err
    gone.close()
    assert sorted(os.listdir(str(tmp_path))) == ["doc.tif", "in_000.pnm", "in_001.pnm"]
