"""CPU tests of TIFF output: the Deflate encoder's host twin
(uphip_tiff_encode_host, csrc/tiff_enc_core.h) and the container writer
(uphip_tiff_writer_*).  Every file is decoded three ways: by PIL (libtiff), by
the project's own TIFF reader, and by hand (the IFD parsed, every strip
inflated on its own with zlib, the predictor undone in numpy)."""
import os
import subprocess

import numpy as np
import pytest

from unpaper_hip import ctypes_abi as A
from unpaper_hip import pipeline as P
from unpaper_hip.device import load_library

import tiff_enc_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read_pages(path):
    """Every page through uphip_tiff_read_page."""
    d = P.TiffDocument(str(path))
    try:
        return [d.read_page(i) for i in range(d.page_count)], [d.probe(i) for i in range(d.page_count)]
    finally:
        d.close()


@pytest.mark.parametrize("case", K.CASES, ids=K.CASE_IDS)
def test_decodes_three_ways(case, tmp_path):
    name, fmt, width, rows = case
    height, rb = rows.shape
    data = P.tiff_encode_host(rows, width, fmt, dpi=200)
    pages, offs = K.ifds(data)
    assert len(pages) == 1
    t = pages[0]
    # the strip rule
    rps = K.rows_per_strip(rb, height)
    assert t[278][1] == [rps]
    assert len(t[273][1]) == (height + rps - 1) // rps
    # the tags
    assert t[256][1] == [width] and t[257][1] == [height]
    assert t[277][1] == [K.CHANNELS[fmt]]
    assert t[262][1] == [2 if fmt == A.FMT_RGB24 else 1]
    assert (t.get(338, (0, None))[1] == [2]) == (fmt == A.FMT_Y400A)
    assert t[282][1] == [(200, 1)] and t[283][1] == [(200, 1)] and t[296][1] == [2]
    assert 254 not in t and 297 not in t  # a file of one page
    # StripByteCounts is the head of the page's data, the strips follow in order
    counts = t[279][1]
    at = 8 + 4 * len(counts)
    for o, c in zip(t[273][1], counts):
        assert o == at
        at += c
    assert offs[0] == (at + 1) // 2 * 2
    # by hand
    got, _ = K.hand_decode(data, t)
    assert np.array_equal(got, rows)
    # PIL
    pil = K.pil_pages(data)
    assert len(pil) == 1 and np.array_equal(pil[0], rows)
    # the project's reader
    path = tmp_path / "a.tif"
    path.write_bytes(data)
    imgs, probes = read_pages(path)
    assert probes[0][:3] == (width, height, fmt) and probes[0][3] == (200.0, 200.0)
    assert np.array_equal(imgs[0].data[:, :rb], rows)


def test_stored_and_coded_strips_share_a_page():
    _, fmt, width, rows = K.CASES[K.CASE_IDS.index("gray_stored_between_flat")]
    data = P.tiff_encode_host(rows, width, fmt)
    _, strips = K.hand_decode(data, K.ifds(data)[0][0])
    assert [s[2] for s in strips] == [False, True, False]
    assert strips[1][1] == K.stored_size(65536)
    assert strips[0][1] < 1000 and strips[2][1] < 1000


def test_strip_shorter_than_a_segment():
    _, fmt, width, rows = K.CASES[K.CASE_IDS.index("gray_strip_below_segment")]
    assert rows.shape[1] * (rows.shape[0] % K.rows_per_strip(*rows.shape[::-1])) < K.SEG
    assert K.rows_per_strip(1, 1) == 1  # 1x1: a strip of one byte


@pytest.mark.parametrize("name", ["gray_257_short_last", "rgb_85_equal_rows", "ya_87_equal_rows"])
def test_pitch_does_not_matter(name):
    """Rows in a wider pitch with garbage in the padding."""
    _, fmt, width, rows = K.CASES[K.CASE_IDS.index(name)]
    want = P.tiff_encode_host(rows, width, fmt)
    assert P.tiff_encode_host(K.embed(rows, 13, 5), width, fmt) == want


def _mono(w, h, seed):
    rng = np.random.default_rng(seed)
    bits = rng.random((h, w)) < 0.1
    bits[:, : w // 3] = False
    return np.packbits(bits, axis=1)


def test_monowhite_is_the_group4_file(tmp_path):
    w, h = 203, 57
    rows = _mono(w, h, 3)
    data = P.tiff_encode_host(rows, w, A.FMT_MONOWHITE, dpi=150)
    path = tmp_path / "g4.tif"
    P.tiff_g4_write(str(path), P.g4_encode_host(rows, w), w, h, dpi=150)
    assert data == path.read_bytes()
    # a page that starts inside a byte
    off = 5
    wide = np.packbits(np.concatenate([np.ones((h, off), bool), np.unpackbits(rows, axis=1)[:, :w]], axis=1), axis=1)
    assert P.tiff_encode_host(wide, w, A.FMT_MONOWHITE, offset=off, dpi=150) == data
    pil = K.pil_pages(data)
    assert np.array_equal(np.unpackbits(pil[0], axis=1)[:, :w], 1 - np.unpackbits(rows, axis=1)[:, :w])


def test_monoblack_is_refused():
    rows = _mono(16, 4, 1)
    with pytest.raises(P.UnpaperHipError, match="MONOBLACK"):
        P.tiff_encode_host(rows, 16, A.FMT_MONOBLACK)


def test_encode_argument_errors():
    L = load_library()
    one = np.zeros((4, 16), np.uint8)
    p = one.ctypes.data
    out = np.zeros(8, np.uint8)
    for args in ((None, 16, 0, 16, 4, A.FMT_GRAY8, 0, None, 0), (p, 16, 0, 0, 4, A.FMT_GRAY8, 0, None, 0),
                 (p, 16, 0, 16, 0, A.FMT_GRAY8, 0, None, 0), (p, 16, 0, 16, 4, 12, 0, None, 0),
                 (p, 16, 2, 8, 4, A.FMT_GRAY8, 0, None, 0), (p, 15, 0, 16, 4, A.FMT_GRAY8, 0, None, 0),
                 (p, 16, 0, 6, 4, A.FMT_RGB24, 0, None, 0), (p, 16, 0, 16, 4, A.FMT_GRAY8, -1, None, 0),
                 (p, 1, 1, 16, 4, A.FMT_MONOWHITE, 0, None, 0),
                 (p, 16, 0, 16, 4, A.FMT_GRAY8, 0, out.ctypes.data, 8)):
        assert L.uphip_tiff_encode_host(*args) == -1, args
        assert L.uphip_last_error()
        L.uphip_clear_error()


# ---- the writer -------------------------------------------------------------

def _blob(data):
    """The packed page inside a one-page Deflate file: from the header's end
    to the last strip's end."""
    t = K.ifds(data)[0][0]
    return data[8: t[273][1][-1] + t[279][1][-1]]


def _gray_pages(n, w, h, seed):
    rng = np.random.default_rng(seed)
    return [K._text(rng, h, w) for _ in range(n)]


def test_one_page_writer_equals_encode(tmp_path):
    rows = _gray_pages(1, 300, 500, 1)[0]
    data = P.tiff_encode_host(rows, 300, A.FMT_GRAY8, dpi=100)
    path = tmp_path / "one.tif"
    w = P.TiffWriter(str(path), dpi=100)
    w.add_page_deflate(_blob(data), 300, 500, A.FMT_GRAY8)
    assert not path.exists()
    w.finish()
    w.close()
    assert path.read_bytes() == data
    assert os.listdir(str(tmp_path)) == ["one.tif"]


def test_shuffled_pages_come_out_in_index_order(tmp_path):
    n, w, h = 7, 301, 250  # 217 rows a strip: two strips a page
    pages = _gray_pages(n, w, h, 2)
    blobs = [_blob(P.tiff_encode_host(p, w, A.FMT_GRAY8)) for p in pages]
    path = tmp_path / "doc.tif"
    wr = P.TiffWriter(str(path))
    for i in (4, 0, 6, 2, 5, 1, 3):
        wr.add_page_deflate(blobs[i], w, h, A.FMT_GRAY8, index=i)
    wr.finish()
    wr.close()
    data = path.read_bytes()
    tags, offs = K.ifds(data)
    assert len(tags) == n
    assert offs == sorted(offs) and offs[0] > max(t[273][1][-1] for t in tags)  # the IFDs follow the data
    for i, t in enumerate(tags):
        assert t[254][1] == [2] and t[297][1] == [i, n]
        assert t[282][1] == [(300, 1)]
        assert t[279][0] == 4 and len(t[279][1]) == 2
        got, _ = K.hand_decode(data, t)
        assert np.array_equal(got, pages[i]), i
    pil = K.pil_pages(data)
    imgs, _ = read_pages(path)
    assert len(pil) == len(imgs) == n
    for i in range(n):
        assert np.array_equal(pil[i], pages[i]) and np.array_equal(imgs[i].data[:, :w], pages[i]), i


def test_missing_page_is_left_out_and_renumbered(tmp_path):
    w, h = 120, 90
    pages = _gray_pages(4, w, h, 3)
    path = tmp_path / "doc.tif"
    wr = P.TiffWriter(str(path), dpi=72)
    for i in (3, 0, 2):  # page 1 failed
        wr.add_page_deflate(_blob(P.tiff_encode_host(pages[i], w, A.FMT_GRAY8)), w, h, A.FMT_GRAY8, index=i)
    wr.finish()
    wr.close()
    data = path.read_bytes()
    tags, _ = K.ifds(data)
    assert [t[297][1] for t in tags] == [[0, 3], [1, 3], [2, 3]]
    assert all(t[282][1] == [(72, 1)] for t in tags)
    pil = K.pil_pages(data)
    for k, i in enumerate((0, 2, 3)):
        assert np.array_equal(pil[k], pages[i])
        assert np.array_equal(K.hand_decode(data, tags[k])[0], pages[i])


def test_mixed_group4_and_deflate_pages(tmp_path):
    w, h = 203, 57
    mono = _mono(w, h, 9)
    g4 = P.g4_encode_host(mono, w)
    rng = np.random.default_rng(4)
    rgb = K._text(rng, h, w * 3)
    ya = K._text(rng, h, w * 2)
    path = tmp_path / "mixed.tif"
    wr = P.TiffWriter(str(path))
    wr.add_page_deflate(_blob(P.tiff_encode_host(rgb, w, A.FMT_RGB24)), w, h, A.FMT_RGB24)
    wr.add_page_g4(g4, w, h, dpi=200)
    wr.add_page_deflate(_blob(P.tiff_encode_host(ya, w, A.FMT_Y400A)), w, h, A.FMT_Y400A)
    wr.finish()
    wr.close()
    data = path.read_bytes()
    tags, _ = K.ifds(data)
    assert [t[259][1][0] for t in tags] == [8, 4, 8]
    # the Group 4 page has the tags of uphip_tiff_g4_write and its stream as the only strip
    single = tmp_path / "g4.tif"
    P.tiff_g4_write(str(single), g4, w, h, dpi=200)
    st = K.ifds(single.read_bytes())[0][0]
    t = tags[1]
    assert sorted(set(t) - {254, 297}) == sorted(st)
    for tag in st:
        if tag not in (273, 282, 283):
            assert t[tag] == st[tag], tag
    assert t[282][1] == [(200, 1)]
    assert data[t[273][1][0]: t[273][1][0] + t[279][1][0]] == g4
    assert t[273][1][0] % 2 == 0
    imgs, probes = read_pages(path)
    assert [p[2] for p in probes] == [A.FMT_RGB24, A.FMT_MONOWHITE, A.FMT_Y400A]
    assert np.array_equal(imgs[0].data[:, :w * 3], rgb)
    assert np.array_equal(imgs[1].data[:, :mono.shape[1]], mono)
    assert np.array_equal(imgs[2].data[:, :w * 2], ya)
    pil = K.pil_pages(data)
    assert np.array_equal(pil[0], rgb) and np.array_equal(pil[2], ya)
    assert np.array_equal(np.unpackbits(pil[1], axis=1)[:, :w], 1 - np.unpackbits(mono, axis=1)[:, :w])


def test_unfinished_writer_leaves_no_file(tmp_path):
    rows = _gray_pages(1, 64, 64, 5)[0]
    path = tmp_path / "gone.tif"
    wr = P.TiffWriter(str(path))
    wr.add_page_deflate(_blob(P.tiff_encode_host(rows, 64, A.FMT_GRAY8)), 64, 64, A.FMT_GRAY8)
    wr.close()
    assert os.listdir(str(tmp_path)) == []
    # a writer without pages cannot finish, and leaves nothing either
    wr = P.TiffWriter(str(path))
    with pytest.raises(P.UnpaperHipError, match="no pages"):
        wr.finish()
    wr.close()
    assert os.listdir(str(tmp_path)) == []


def test_writer_argument_errors(tmp_path):
    L = load_library()
    rows = _gray_pages(1, 64, 700, 6)[0]
    blob = _blob(P.tiff_encode_host(rows, 64, A.FMT_GRAY8))
    assert L.uphip_tiff_writer_open(None, 0) is None and L.uphip_last_error()
    L.uphip_clear_error()
    assert L.uphip_tiff_writer_open(str(tmp_path / "no" / "dir.tif").encode(), 0) is None and L.uphip_last_error()
    L.uphip_clear_error()
    assert L.uphip_tiff_writer_open(str(tmp_path / "a.tif").encode(), 5000) is None and L.uphip_last_error()
    L.uphip_clear_error()
    wr = P.TiffWriter(str(tmp_path / "a.tif"))
    bad = [(blob, 64, 700, A.FMT_MONOWHITE), (blob, 64, 700, 12), (blob, 0, 700, A.FMT_GRAY8),
           (blob, 64, 1100, A.FMT_GRAY8),      # two strips, the blob counts one
           (blob[:-1], 64, 700, A.FMT_GRAY8),  # the counts do not add up
           (blob[:3], 64, 700, A.FMT_GRAY8), (b"", 64, 700, A.FMT_GRAY8)]
    for b, w, h, fmt in bad:
        with pytest.raises(P.UnpaperHipError):
            wr.add_page_deflate(b, w, h, fmt)
    with pytest.raises(P.UnpaperHipError):
        wr.add_page_g4(b"", 64, 64)
    with pytest.raises(P.UnpaperHipError):
        wr.add_page_g4(b"\x00\x10\x01", 0, 64)
    wr.add_page_deflate(blob, 64, 700, A.FMT_GRAY8, index=2)
    with pytest.raises(P.UnpaperHipError, match="added before"):
        wr.add_page_deflate(blob, 64, 700, A.FMT_GRAY8, index=2)
    wr.finish()
    with pytest.raises(P.UnpaperHipError):
        wr.finish()
    with pytest.raises(P.UnpaperHipError):
        wr.add_page_deflate(blob, 64, 700, A.FMT_GRAY8)
    wr.close()
    assert L.uphip_tiff_writer_finish(None) == -1
    L.uphip_clear_error()
    assert len(K.ifds((tmp_path / "a.tif").read_bytes())[0]) == 1


# ---- the host twin and the writer under ASan / UBSan -------------------------

def test_host_twin_and_writer_under_sanitizers():
    """tests/c/tiff_enc_main.cpp: a stand-alone program that runs the host twin
    over its own list of the cases above, writes a multi-page file and reads
    it back through the project's TIFF reader (make sanitize_tiff_enc builds
    and runs it)."""
    r = subprocess.run(["make", "-s", "sanitize_tiff_enc"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "tiff_enc_main: ok" in r.stdout
