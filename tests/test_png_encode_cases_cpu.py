"""CPU: tests/png_encode_cases.py's encode_ref -- the restatement sf_png_encode (csrc/png_encode.hip) must equal byte for byte -- pinned
from outside: zlib inflates its streams to scanlines that an independent filter implementation (tests/png_cases.filter_rows, given
the stream's own filter-type bytes) reproduces, the filter types equal a brute-force choice, flow_io.png_file around a stream reads
back through flow_io.read_png and PIL, the stream sizes stay within the stated margins of zlib's, and the bound of
sf_png_encode_bound holds.  kitti16_ref equals flow_io.kitti_encode."""
import os
import zlib

import numpy as np
import pytest

from tests import png_cases as pc
from tests import png_encode_cases as ec


def file_rows(img, bpp, swap16):
    mem = img.reshape(img.shape[0], -1)
    return mem.reshape(mem.shape[0], -1, 2)[:, :, ::-1].reshape(mem.shape) if swap16 else mem


def brute_force_types(rows, bpp):
    """Per row and byte in plain Python integers: the type with the smallest sum of min(v, 256 - v), the first on ties."""
    types = []
    for y in range(rows.shape[0]):
        cur = [int(v) for v in rows[y]]
        up = [int(v) for v in rows[y - 1]] if y else [0] * len(cur)
        sums = [0] * 5
        for x, v in enumerate(cur):
            a = cur[x - bpp] if x >= bpp else 0
            b = up[x]
            c = up[x - bpp] if x >= bpp else 0
            p = a + b - c
            pa, pb, pc_ = abs(p - a), abs(p - b), abs(p - c)
            paeth = a if pa <= pb and pa <= pc_ else (b if pb <= pc_ else c)
            for t, pred in enumerate((0, a, b, (a + b) // 2, paeth)):
                f = (v - pred) % 256
                sums[t] += min(f, 256 - f)
        types.append(sums.index(min(sums)))
    return types


def test_header_constant_and_bound_formula():
    assert ec.header_band_rows() == ec.BAND_ROWS
    assert ec.HEADER_BITS_MAX == 1887 and ec.bound(436, 1024, 3) == (2 + -(-(14 * 1896 + 9 * 436 * 3073) // 8) + 4 + 3) // 4 * 4


@pytest.mark.parametrize("case", ec.CASES, ids=ec.case_id)
def test_reference_stream_inflates_to_independently_filtered_scanlines(case, tmp_path):
    from streamflow_amd import flow_io
    kind, h, w, bpp, swap16, seed = case
    img = ec.make(kind, h, w, bpp, seed)
    stream = ec.encode_ref(img, bool(swap16))
    assert stream[:2] == b"\x78\x01" and len(stream) <= ec.bound(h, w, bpp)
    scan = np.frombuffer(zlib.decompress(stream), np.uint8).reshape(h, 1 + w * bpp)      # zlib also checks the Adler-32
    rows = file_rows(img, bpp, swap16)
    assert scan[:, 0].tolist() == brute_force_types(rows, bpp)
    assert np.array_equal(scan[:, 1:], pc.filter_rows(rows, bpp, scan[:, 0]))
    # as a file: the 16-bit formats are the swap16 cases, everything else is 8-bit; bpp 6 / 8 without swap16 are 8-bit only as bytes
    depth = 16 if swap16 else 8
    channels = bpp * 8 // depth
    if channels <= 4:
        path = str(tmp_path / "a.png")
        with open(path, "wb") as f:
            f.write(flow_io.png_file(stream, h, w, depth, channels))
        want = img.reshape(h, w, bpp).view(np.uint16).reshape(h, w, channels) if swap16 else img
        got = flow_io.read_png(path)
        assert got.dtype == want.dtype and np.array_equal(got.reshape(want.shape), want)
        if not (depth == 16 and channels != 1):                             # PIL has no 16-bit multi-channel mode
            Image = pytest.importorskip("PIL.Image")
            with Image.open(path) as im:
                im.load()
                assert np.array_equal(np.asarray(im).reshape(want.shape).astype(want.dtype), want)


def test_every_filter_type_wins_and_ties_go_to_the_lowest_type():
    rng = np.random.default_rng(3)
    w, bpp = 40, 3
    noise = rng.integers(0, 256, size=(1, w * bpp), dtype=np.uint8)
    ramp = ((np.arange(w * bpp) // bpp) * 37 % 256).astype(np.uint8)[None]              # steps between pixels: Sub leaves one value
    rows = np.concatenate([
        rng.integers(0, 2, size=(1, w * bpp), dtype=np.uint8),                          # 0: tiny values, nothing to predict from
        ramp,                                                                           # 1: Sub
        ramp,                                                                           # 2: Up (the row above repeated)
        noise,                                                                          # (some row to average with)
        ((noise.astype(np.int32) + np.roll(noise, bpp)) // 2 % 256).astype(np.uint8),   # 3: mostly Average of left and above
        noise]).astype(np.uint8)
    rows[4, :bpp] = noise[0, :bpp] // 2
    y, x = np.mgrid[0:6, 0:w * bpp]
    plane = (7 * (x // bpp) + 13 * y + rng.integers(0, 2, size=y.shape)).astype(np.uint8)          # 4: a plane, Paeth's case
    rows = np.concatenate([rows, plane])
    scan = ec.scanlines(rows, bpp, False)
    types = scan[:, 0].tolist()
    assert types == brute_force_types(rows, bpp)
    assert set(types) == {0, 1, 2, 3, 4}, types
    # exact ties, the lowest of the tied cheapest types must win: a zero image ties all five types in every row
    zeros = np.zeros((3, 12), np.uint8)
    assert ec.scanlines(zeros, 3, False)[:, 0].tolist() == [0, 0, 0] == brute_force_types(zeros, 3)
    const = np.full((2, 12), 9, np.uint8)                                   # row 0: Sub wins; row 1: Up = Paeth = 0 cost -> Up
    assert ec.scanlines(const, 3, False)[:, 0].tolist() == [1, 2] == brute_force_types(const, 3)
    one = np.full((1, 3), 200, np.uint8)                                    # one pixel, no neighbours: all five tie
    assert ec.scanlines(one, 3, False)[:, 0].tolist() == [0] == brute_force_types(one, 3)


def test_length_limit_case_needs_the_limit():
    band = ec.fibonacci_band(23)
    scan = ec.scanlines(band.reshape(32, -1), 1, False)
    assert (scan[:, 0] == 0).all()                                          # so the histogram is the constructed one
    lit, cl, deepest, fallback = ec.band_tables(np.bincount(scan.reshape(-1), minlength=256))
    assert deepest == 16 and max(lit) == 15 and max(cl) <= 7
    assert sum(2.0 ** -l for l in lit if l) == 1.0 and sum(2.0 ** -l for l in cl if l) == 1.0


def test_tables_are_complete_prefix_codes_for_odd_histograms():
    rng = np.random.default_rng(11)
    hists = [np.zeros(256, np.int64) for _ in range(3)]
    hists[0][7] = 5                                                          # one byte value: two 1-bit codes
    hists[1][:] = 1                                                          # everything once
    hists[2][:] = rng.integers(0, 3, size=256) * rng.integers(1, 2000, size=256)
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    hists.append(np.array(fib[:30] + [0] * 226, np.int64))                   # 30 deep before the limit
    for h in hists:
        lit, cl, _, _ = ec.band_tables(h)
        assert max(lit) <= 15 and max(cl) <= 7 and cl[16] == cl[17] == cl[18] == 0
        assert sum(2.0 ** -l for l in lit if l) == 1.0 and sum(2.0 ** -l for l in cl if l) == 1.0
        assert all((l > 0) == (f > 0) for l, f in zip(lit, list(h) + [1]))
        codes = ec.canonical_codes(lit)
        assert len({(c, l) for c, l in zip(codes, lit) if l}) == sum(1 for l in lit if l)
    assert ec.band_tables(hists[0])[0][7] == 1 and ec.band_tables(hists[0])[0][256] == 1


@pytest.fixture(scope="module")
def smooth_images():
    from streamflow_amd import flow_io
    f = ec.smooth_field(436, 1024, 7)
    return {"rgb8": ec.wheel_rgb(f), "kitti16": flow_io.kitti_encode(f.transpose(1, 2, 0))}


@pytest.mark.parametrize("name", ["rgb8", "kitti16"])
def test_stream_size_against_zlib_and_write_png(smooth_images, name, tmp_path):
    from streamflow_amd import flow_io
    img = smooth_images[name]
    mem, bpp, swap16 = ec.memory_bytes(img)
    scan = ec.scanlines(mem, bpp, swap16)
    stream = ec.deflate_ref(scan)
    assert zlib.decompress(stream) == scan.tobytes()
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    huff_only = len(co.compress(scan.tobytes()) + co.flush())
    path = str(tmp_path / "host.png")
    flow_io.write_png(path, img)
    idat = os.path.getsize(path) - (8 + 25 + 12 + 12)                        # signature, IHDR, IDAT's and IEND's framing
    print(f"{name}: reference {len(stream)} B, zlib Z_HUFFMAN_ONLY {huff_only} B ({len(stream) / huff_only:.4f}), write_png IDAT {idat} B "
          f"({len(stream) / idat:.3f})")
    assert len(stream) <= 1.01 * huff_only
    assert len(stream) < idat
    with open(path, "wb") as f:
        f.write(flow_io.png_file(stream, img.shape[0], img.shape[1], 8 * img.dtype.itemsize, 3))
    assert np.array_equal(flow_io.read_png(path), img)


def test_bound_holds_on_noise_and_the_length_limit_case():
    rng = np.random.default_rng(5)
    for h, w, bpp in ((65, 100, 3), (1, 1, 1), (33, 7, 8), (32, 1025, 1), (40, 4097, 1)):
        img = rng.integers(0, 256, size=(h, w, bpp), dtype=np.uint8)
        assert len(ec.encode_ref(img, False)) <= ec.bound(h, w, bpp), (h, w, bpp)
    assert len(ec.encode_ref(ec.fibonacci_band(23), False)) <= ec.bound(32, 150, 1)
    # the fixed table is what bounds a block: a histogram built against the length limit must not cost more than 9 bits a byte
    fib = [1, 1]
    while len(fib) < 34:
        fib.append(fib[-1] + fib[-2])
    hist = np.array(fib[2:34] + [0] * 224, np.int64)
    lit, _, _, _ = ec.band_tables(hist)
    assert sum(int(f) * l for f, l in zip(list(hist) + [1], lit)) <= 9 * int(hist.sum()) + 9


def test_kitti16_ref_equals_kitti_encode():
    from streamflow_amd import flow_io
    rng = np.random.default_rng(9)
    flow = (rng.standard_normal((2, 37, 53)) * 60).astype(np.float32)
    flow[0, 0, :4] = [0.0, -0.0, 511.98, -511.99]
    assert np.array_equal(ec.kitti16_ref(flow), flow_io.kitti_encode(flow.transpose(1, 2, 0)))
    assert ec.kitti16_ref(np.array([[[np.nan, -600.0, 600.0, np.inf]], [[0, 0, 0, -np.inf]]], np.float32))[0, :, :2].tolist() == \
        [[0, 32768], [0, 32768], [65535, 32768], [65535, 0]]
