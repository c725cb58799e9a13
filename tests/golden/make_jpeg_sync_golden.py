"""Writes tests/golden/jpeg_sync: the four .jpg fixtures of tests/jpeg_sync_cases.SYNC_CASES -- PIL files without DRI, one restart
interval each, long enough that at 8-byte segments they span more than two windows of the synchronisation -- and expected.npz,
PIL's (libjpeg-turbo's) pixels of each as uint8 [h, w, 3].  Needs PIL; the tests that use the fixtures do not.

    python -m tests.golden.make_jpeg_sync_golden
"""
import io
import os

import numpy as np
from PIL import Image

from tests import jpeg_decode_cases as dc
from tests import jpeg_sync_cases as sc


def main():
    os.makedirs(sc.GOLDEN, exist_ok=True)
    files = {}
    for name, kind, h, w, c, seed, opts in sc.SYNC_CASES:
        buf = io.BytesIO()
        Image.fromarray(sc.make(kind, h, w, c, seed)).save(buf, "JPEG", **opts)
        files[name] = buf.getvalue()
        assert dc.walk(files[name])["restart"] == 0 and len(files[name]) > 2 * sc.WINDOW * 8
    for name, blob in files.items():
        with open(os.path.join(sc.GOLDEN, name + ".jpg"), "wb") as f:
            f.write(blob)
    np.savez_compressed(os.path.join(sc.GOLDEN, "expected.npz"), **{name: dc.pil_pixels(blob) for name, blob in files.items()})
    total = sum(len(b) for b in files.values()) + os.path.getsize(os.path.join(sc.GOLDEN, "expected.npz"))
    print({n: len(b) for n, b in files.items()}, f"{total} bytes in all")


if __name__ == "__main__":
    main()
