"""Writes the Group 4 fixtures: for every case of tests/g4_cases.py the T.6
stream libtiff produces (<name>.g4), the packed bitmap (<name>.npy, when
small) and index.json (geometry, bitmap hash).

PIL saves a mode "1" image as Photometric 1 (min-is-black) and libtiff codes
the file's 1-bits as the "black" runs of T.6, so a bitmap's 1 (black) goes
in as PIL's 255.  RowsPerStrip = height gives one strip: its bytes are the
stream.  Needs PIL with libtiff; run from anywhere:
    python tests/golden/g4/make_g4_fixtures.py
"""
import io
import json
import os
import sys

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import g4_cases  # noqa: E402


def libtiff_g4(bits):
    h, w = bits.shape
    im = Image.fromarray((bits * 255).astype(np.uint8), "L").convert("1", dither=Image.Dither.NONE)
    buf = io.BytesIO()
    im.save(buf, format="TIFF", compression="group4", tiffinfo={278: h})
    buf.seek(0)
    t = Image.open(buf)
    tags = t.tag_v2
    assert tags[259] == 4 and tags[262] == 1 and tags[278] == h, dict(tags)
    offs, counts = tags[273], tags[279]
    assert len(offs) == 1 and len(counts) == 1
    return buf.getvalue()[offs[0]:offs[0] + counts[0]]


def main():
    assert features.check("libtiff"), "PIL without libtiff cannot write Group 4"
    index = {}
    for name, make in g4_cases.CASES:
        bits = make()
        packed = g4_cases.pack(bits)
        stream = libtiff_g4(bits)
        with open(os.path.join(HERE, name + ".g4"), "wb") as f:
            f.write(stream)
        if packed.nbytes <= g4_cases.NPY_LIMIT:
            np.save(os.path.join(HERE, name + ".npy"), packed)
        index[name] = {"height": int(bits.shape[0]), "width": int(bits.shape[1]),
                       "sha256": g4_cases.sha(packed), "stream_bytes": len(stream)}
        print("%-20s %4d x %4d  %6d bytes" % (name, bits.shape[0], bits.shape[1], len(stream)))
    with open(os.path.join(HERE, "index.json"), "w") as f:
        json.dump(index, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
