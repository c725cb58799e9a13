"""Writes tests/golden/jpeg_decode: the .jpg fixtures of tests/jpeg_decode_cases.py and expected.npz, PIL's (libjpeg-turbo's) pixels of
every one of them as uint8 [h, w, 3].  Needs PIL; the tests that use the fixtures do not.

    python -m tests.golden.make_jpeg_decode_golden

The files: PIL's own at every sampling, size and restart layout of jpeg_decode_cases.PIL_CASES; files of the project's encoder
(OWN_CASES); hand-edited framings (EDIT_CASES: a frame without its DHT segments -- expected.npz holds the pixels of the unedited
file for it, whose tables are the Annex K.3 ones --, FF fill bytes in front of markers); and five files jpeg_gpu.parse must refuse
(REFUSED), the last three made by patching headers: nothing ever decodes them."""
import io
import os

import numpy as np
from PIL import Image

from tests import jpeg_cases as jc
from tests import jpeg_decode_cases as dc


def pil_file(case):
    _, kind, h, w, c, seed, opts = case
    buf = io.BytesIO()
    Image.fromarray(jc.make(kind, h, w, c, seed)).save(buf, "JPEG", **opts)
    return buf.getvalue()


def refused():
    img = Image.fromarray(jc.make("mixed", 16, 16, 3, 1))
    out = {}
    buf = io.BytesIO()
    img.save(buf, "JPEG", progressive=True)
    out["refuse-progressive"] = buf.getvalue()
    buf = io.BytesIO()
    img.convert("CMYK").save(buf, "JPEG")
    out["refuse-cmyk"] = buf.getvalue()
    buf = io.BytesIO()
    img.save(buf, "JPEG", subsampling=0)
    base = buf.getvalue()
    sof = next(lo for m, lo, _ in dc.segments(base) if m == 0xC0)
    out["refuse-411"] = base[:sof + 7] + b"\x41" + base[sof + 8:]                       # luma sampling 4 x 1
    out["refuse-12bit"] = base[:sof] + b"\x0c" + base[sof + 1:]                         # sample precision 12
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"                       # APP14, transform 0: RGB
    out["refuse-rgb-adobe"] = base[:2] + adobe + base[2:]
    return out


def main():
    os.makedirs(dc.GOLDEN, exist_ok=True)
    files = {c[0]: pil_file(c) for c in dc.PIL_CASES}
    files.update({c[0]: dc.own_file(c) for c in dc.OWN_CASES})
    pixels = {name: dc.pil_pixels(blob) for name, blob in files.items()}
    for name, src, how in dc.EDIT_CASES:
        files[name] = dc.edit(files[src], how)
        pixels[name] = pixels[src] if how == "strip-dht" else dc.pil_pixels(files[name])
        assert np.array_equal(pixels[name], pixels[src])
    assert list(files) == dc.NAMES
    files.update(refused())
    for name, blob in files.items():
        with open(os.path.join(dc.GOLDEN, name + ".jpg"), "wb") as f:
            f.write(blob)
    np.savez_compressed(os.path.join(dc.GOLDEN, "expected.npz"), **pixels)
    total = sum(len(b) for b in files.values()) + os.path.getsize(os.path.join(dc.GOLDEN, "expected.npz"))
    print(f"{len(files)} files, largest {max(len(b) for b in files.values())} bytes, {total} bytes in all")


if __name__ == "__main__":
    main()
