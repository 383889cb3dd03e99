"""The bilevel test bitmaps of the Group 4 encoder (tests/golden/g4): built
from integer arithmetic alone, so the fixture writer and the tests make the
same bits on every machine.  A bitmap is a (h, w) uint8 array of 0 / 1,
1 = black."""
import hashlib
import json
import os

import numpy as np

GOLDEN_G4 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g4")
# bitmaps whose packed rows are larger than this are not committed: the tests
# rebuild them from CASES and check the manifest's hash
NPY_LIMIT = 64 << 10


def _mix(z):
    """splitmix64 finaliser on a uint64 array (wraps like the C code)."""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def noise(h, w, per_million, seed):
    """Independent pixels, black with probability per_million / 1e6."""
    with np.errstate(over="ignore"):
        idx = np.arange(h * w, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x100000001B3)
        v = _mix(_mix(idx)) % np.uint64(1000000)
    return (v < np.uint64(per_million)).astype(np.uint8).reshape(h, w)


def alternating(h, w):
    """Every other pixel black, the same in every row."""
    return np.tile((np.arange(w) & 1).astype(np.uint8), (h, 1))


def checker(h, w):
    """Every other pixel black, inverted from row to row: no code is shorter
    than three bits a pixel (the largest expansion)."""
    y, x = np.mgrid[0:h, 0:w]
    return ((x + y) & 1).astype(np.uint8)


def moving_edge(k, h=12, w=80):
    """Black right of an edge that moves by k pixels a row (|k| <= 3 is
    vertical mode, 4 horizontal mode)."""
    a = np.zeros((h, w), np.uint8)
    x0 = 8 if k >= 0 else w - 8
    for y in range(h):
        a[y, max(0, min(w, x0 + k * y)):] = 1
    return a


def blobs(h=24, w=96):
    """Rectangles that end in the row above a white stretch (pass mode), some
    touching the left and right borders."""
    a = np.zeros((h, w), np.uint8)
    a[2:6, 10:20] = 1
    a[2:9, 30:33] = 1
    a[4:7, 0:5] = 1
    a[5:12, w - 6:w] = 1
    a[10:11, 40:70] = 1
    a[11:15, 50:60] = 1
    a[16:20, 0:w] = 1
    a[17:19, 20:50] = 0
    a[21:23, 1:2] = 1
    return a


def single_pixel(h, w, y, x):
    a = np.zeros((h, w), np.uint8)
    a[y, x] = 1
    return a


def _cases():
    c = [
        ("rand_5x7", lambda: noise(5, 7, 500000, 1)),
        ("rand_40x100", lambda: noise(40, 100, 500000, 2)),
        ("rand_33x2700", lambda: noise(33, 2700, 20000, 3)),
        ("white_20x64", lambda: np.zeros((20, 64), np.uint8)),
        ("black_20x65", lambda: np.ones((20, 65), np.uint8)),
        ("rand_64x333", lambda: noise(64, 333, 300000, 4)),
        ("rand_16x5300", lambda: noise(16, 5300, 1000, 5)),
        ("rand_600x2480", lambda: noise(600, 2480, 10000, 6)),
        ("one_2x5300", lambda: single_pixel(2, 5300, 1, 5290)),
        ("alternating_9x67", lambda: alternating(9, 67)),
        ("checker_9x67", lambda: checker(9, 67)),
        ("blobs_24x96", blobs),
    ]
    for w in (1, 8, 31, 32, 33):
        c.append(("width_%d" % w, lambda w=w: noise(11, w, 400000, 10 + w)))
    for h in (1, 2, 65, 130):
        c.append(("height_%d" % h, lambda h=h: noise(h, 70, 150000, 50 + h)))
    for k in range(-4, 5):
        c.append(("edge_%s%d" % ("m" if k < 0 else "p", abs(k)), lambda k=k: moving_edge(k)))
    return c


CASES = _cases()
NAMES = [n for n, _ in CASES]


def bitmap(name):
    return dict(CASES)[name]()


def pack(bits):
    """Packed rows, MSB first, padding bits zero."""
    return np.packbits(bits, axis=1)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def manifest():
    with open(os.path.join(GOLDEN_G4, "index.json")) as f:
        return json.load(f)


def load(name):
    """(bitmap, expected T.6 stream) of a committed case."""
    m = manifest()[name]
    p = os.path.join(GOLDEN_G4, name + ".npy")
    if os.path.isfile(p):
        bits = np.unpackbits(np.load(p), axis=1)[:, :m["width"]]
    else:
        bits = bitmap(name)
    assert bits.shape == (m["height"], m["width"]) and sha(pack(bits)) == m["sha256"], name
    with open(os.path.join(GOLDEN_G4, name + ".g4"), "rb") as f:
        return bits, f.read()
