"""PNG test encoder and cases for the GPU row unfilter (csrc/png_unfilter.hip, streamflow_amd/png_gpu.py): this repository's own code,
written from the PNG specification (section 9, "Filtering") in vectorised numpy -- the FORWARD filters, so nothing here shares code
with the decoders it feeds (flow_io.read_png on the host, sf_png_unfilter on the GPU).  tests/test_png_cases_cpu.py pins it to
flow_io.read_png and, where installed, to PIL.

encode(img, filter_types, path, depth): a non-interlaced PNG whose row y is filtered with filter_types[y]; also returns the filtered
scanline block [h, 1 + w * bpp] (filter-type byte first), which is exactly what flow_io.png_scanlines returns for the file and what
sf_png_unfilter takes, so kernels can be fed without a file."""
import os
import re
import struct
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CTYPE = {1: 0, 2: 4, 3: 2, 4: 6}


def header_constant(name):
    hdr = open(os.path.join(REPO, "include", "streamflow_hip.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, hdr).group(1))


def raw_rows(img, depth):
    """[h, w(, c)] uint8 / uint16 -> (the bytes of the rows as a PNG stores them [h, w * bpp] (16-bit samples big-endian), channels)."""
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[:, :, None]
    assert a.dtype == (np.uint16 if depth == 16 else np.uint8) and a.ndim == 3 and a.shape[2] in _CTYPE, (a.dtype, a.shape, depth)
    h = a.shape[0]
    return np.ascontiguousarray(a.astype(">u2" if depth == 16 else np.uint8)).reshape(h, -1).view(np.uint8).reshape(h, -1), a.shape[2]


def filter_rows(rows, bpp, filter_types):
    """Forward filters of the PNG specification 9.2 on reconstructed rows [h, stride]: row y with type filter_types[y] (0 None,
    1 Sub, 2 Up, 3 Average, 4 Paeth; a = the byte bpp to the left, b = above, c = above left, zero outside the image)."""
    h, stride = rows.shape
    ft = np.asarray(filter_types, np.int64).reshape(h)
    assert ((ft >= 0) & (ft <= 4)).all()
    cur = rows.astype(np.int32)
    b = np.zeros_like(cur)
    b[1:] = cur[:-1]
    a = np.zeros_like(cur)
    a[:, bpp:] = cur[:, :-bpp] if stride > bpp else 0
    c = np.zeros_like(cur)
    c[:, bpp:] = b[:, :-bpp] if stride > bpp else 0
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    pred = np.select([ft[:, None] == 1, ft[:, None] == 2, ft[:, None] == 3, ft[:, None] == 4], [a, b, (a + b) >> 1, paeth], 0)
    return ((cur - pred) & 255).astype(np.uint8)


def write_block(path, block, w, depth, channels):
    """A filtered scanline block [h, 1 + w * bpp] as a PNG file."""
    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, block.shape[0], depth, _CTYPE[channels], 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(np.ascontiguousarray(block).tobytes(), 1)) + chunk(b"IEND", b""))


def encode(img, filter_types, path=None, depth=8):
    """-> the filtered scanline block uint8 [h, 1 + w * bpp]; with `path`, also written as a PNG file."""
    rows, channels = raw_rows(img, depth)
    bpp = channels * depth // 8
    block = np.concatenate([np.asarray(filter_types, np.uint8).reshape(-1, 1), filter_rows(rows, bpp, filter_types)], axis=1)
    if path is not None:
        write_block(path, block, rows.shape[1] // bpp, depth, channels)
    return block


def image(h, w, channels, depth, seed, kind="random"):
    """Uniform random samples, or (kind "binary") only 0 and all-ones bytes: the latter catches an Average computed on 8 bits
    ((255 + 255) >> 1 must be 255) and a Paeth with the wrong tie order (a, b, c equal or at the extremes tie constantly)."""
    rng = np.random.default_rng(seed)
    dt = np.uint16 if depth == 16 else np.uint8
    if kind == "binary":
        a = (rng.integers(0, 2, size=(h, w, channels)) * (65535 if depth == 16 else 255)).astype(dt)
    else:
        a = rng.integers(0, 65536 if depth == 16 else 256, size=(h, w, channels)).astype(dt)
    return a


def filter_types(how, h, seed=0):
    """how: 0 .. 4 (every row that type) or "mixed" (drawn per row)."""
    if how == "mixed":
        return np.random.default_rng(1000 + seed).integers(0, 5, size=h).astype(np.uint8)
    return np.full(h, int(how), np.uint8)


# (h, w, channels, depth, how the filter types are chosen, seed): every format, every single type (row 0 included) and mixtures
CASES = [(7, 5, 1, 8, "mixed", 1), (6, 9, 2, 8, "mixed", 2), (37, 53, 3, 8, "mixed", 3), (9, 6, 4, 8, "mixed", 4),
         (5, 7, 1, 16, "mixed", 5), (8, 3, 2, 16, "mixed", 6), (11, 13, 3, 16, "mixed", 7), (6, 5, 4, 16, "mixed", 8),
         (1, 1, 3, 8, 4, 9), (3, 1, 1, 8, "mixed", 10), (1, 17, 4, 16, 3, 11)] + \
        [(12, 10, 3, 8, t, 20 + t) for t in range(5)] + [(9, 4, 3, 16, t, 30 + t) for t in range(5)]


def case_id(c):
    return "-".join(str(x) for x in c)
