"""CPU: the PNG test encoder (tests/png_cases.py) against two independent decoders; flow_io.png_scanlines (the host half of the GPU
PNG decode) and read_png through it; sf_png_unfilter's argument checks through the C ABI (they run before any launch, so dummy
pointers are never dereferenced); the loud failures of png_gpu without a GPU."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from tests import png_cases as pc


@pytest.fixture(scope="module")
def lib():
    from streamflow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def _expected(img):
    return img[:, :, 0] if img.shape[2] == 1 else img                    # read_png squeezes a single channel


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_encoder_round_trip_through_two_decoders(tmp_path, case):
    """read_png (and PIL, where installed) of an encoded file is the image, for every case: the encoder -- and with it the GPU
    tests' inputs -- is a valid PNG filter implementation, whichever filter types the rows carry."""
    from streamflow_amd import flow_io
    h, w, c, depth, how, seed = case
    img = pc.image(h, w, c, depth, seed)
    path = str(tmp_path / "case.png")
    block = pc.encode(img, pc.filter_types(how, h, seed), path, depth)
    assert block.shape == (h, 1 + w * c * depth // 8) and block.dtype == np.uint8
    got = flow_io.read_png(path)
    assert got.dtype == img.dtype and np.array_equal(got, _expected(img))
    raw, hh, ww, dd, cc = flow_io.png_scanlines(path)
    assert (hh, ww, dd, cc) == (h, w, depth, c) and raw.dtype == np.uint8 and np.array_equal(raw, block.reshape(-1))


@pytest.mark.parametrize("case", [c for c in pc.CASES if not (c[3] == 16 and c[2] != 1)], ids=pc.case_id)
def test_encoder_round_trip_through_pil(tmp_path, case):
    """PIL decodes 8-bit files of every colour type and 16-bit grey to arrays (it reduces 16-bit colour to 8 bits, so those cases
    rest on read_png and on the 8-bit cases, which share the encoder's code path with bpp = 6 / 8 replaced by 3 / 4)."""
    Image = pytest.importorskip("PIL.Image")
    h, w, c, depth, how, seed = case
    img = pc.image(h, w, c, depth, seed)
    path = str(tmp_path / "case.png")
    pc.encode(img, pc.filter_types(how, h, seed), path, depth)
    with Image.open(path) as im:
        got = np.asarray(im)
    assert np.array_equal(got.astype(img.dtype).reshape(h, w, c), img)


def test_binary_image_round_trip(tmp_path):
    from streamflow_amd import flow_io
    for c, depth in ((1, 8), (3, 8), (4, 16)):
        for how in (3, 4, "mixed"):
            img = pc.image(19, 23, c, depth, 5, kind="binary")
            pc.encode(img, pc.filter_types(how, 19, 2), str(tmp_path / "b.png"), depth)
            assert np.array_equal(flow_io.read_png(str(tmp_path / "b.png")), _expected(img))


def test_read_png_results_are_unchanged(tmp_path):
    """read_png through png_scanlines on files of tests/test_flow_io_cpu.py's kind (write_png: 8- and 16-bit; grey, grey + alpha,
    RGB, RGBA) returns bytewise the array that was written -- what it returned before the split -- with a single channel squeezed."""
    from streamflow_amd import flow_io
    rng = np.random.default_rng(0)
    for dt, top in ((np.uint8, 256), (np.uint16, 65536)):
        for c in (1, 2, 3, 4):
            img = rng.integers(0, top, size=(13, 17, c)).astype(dt)
            path = str(tmp_path / f"{np.dtype(dt).name}_{c}.png")
            flow_io.write_png(path, img if c > 1 else img[:, :, 0])
            got = flow_io.read_png(path)
            assert got.dtype == dt and got.shape == ((13, 17) if c == 1 else (13, 17, c)) and np.array_equal(got, _expected(img))
            raw, h, w, depth, cc = flow_io.png_scanlines(path)
            assert (h, w, depth, cc) == (13, 17, 8 * np.dtype(dt).itemsize, c) and raw.size == h * (1 + w * c * depth // 8)
            assert not raw[::1 + w * c * depth // 8].any()                # write_png writes filter type 0


def _chunks(path):
    data = open(path, "rb").read()
    pos, out = 8, []
    while pos < len(data):
        n = struct.unpack(">I", data[pos:pos + 4])[0]
        out.append((data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]))
        pos += 12 + n
    return out


def _write_chunks(path, chunks):
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        for tag, body in chunks:
            f.write(struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF))


def test_png_scanlines_rejects_what_read_png_rejected(tmp_path):
    from streamflow_amd import flow_io
    img = pc.image(6, 5, 3, 8, 1)
    good = str(tmp_path / "good.png")
    block = pc.encode(img, pc.filter_types("mixed", 6, 1), good, 8)
    bad = str(tmp_path / "bad.png")
    # a filter byte of 5: the existing error, now raised before any row is unfiltered (and so before any upload)
    blk = block.copy()
    blk[3, 0] = 5
    pc.write_block(bad, blk, 5, 8, 3)
    for fn in (flow_io.png_scanlines, flow_io.read_png):
        with pytest.raises(IOError, match="bad filter type 5"):
            fn(bad)
    # interlaced
    chunks = _chunks(good)
    hdr = bytearray(chunks[0][1])
    hdr[12] = 1
    _write_chunks(bad, [(b"IHDR", bytes(hdr))] + chunks[1:])
    for fn in (flow_io.png_scanlines, flow_io.read_png):
        with pytest.raises(IOError, match="unsupported PNG"):
            fn(bad)
    # a wrong CRC
    data = bytearray(open(good, "rb").read())
    data[-20] ^= 0x55                                                    # inside the IDAT body
    open(bad, "wb").write(bytes(data))
    for fn in (flow_io.png_scanlines, flow_io.read_png):
        with pytest.raises(IOError, match="CRC mismatch"):
            fn(bad)
    # truncated file, truncated image data, not a PNG
    open(bad, "wb").write(open(good, "rb").read()[:-25])
    for fn in (flow_io.png_scanlines, flow_io.read_png):
        with pytest.raises(IOError, match="truncated PNG chunk"):
            fn(bad)
    pc.write_block(bad, block[:-1], 5, 8, 3)
    _write_chunks(bad, [_chunks(good)[0]] + _chunks(bad)[1:])             # the header of 6 rows over the data of 5
    for fn in (flow_io.png_scanlines, flow_io.read_png):
        with pytest.raises(IOError, match="truncated image data"):
            fn(bad)
    open(bad, "wb").write(b"not a png at all")
    with pytest.raises(IOError, match="not a PNG"):
        flow_io.png_scanlines(bad)


def test_c_level_rejection(lib):
    """Every SF_ERR_BAD_ARG / SF_ERR_UNSUPPORTED condition of sf_png_unfilter, with sf_last_error() naming the argument."""
    R, MAXB = pc.header_constant("SF_PNG_BAND_ROWS"), pc.header_constant("SF_PNG_MAX_ROW_BYTES")
    assert R >= 2 and MAXB >= 1920 * 8
    S, O = 0x10000, 0x20000                                              # never dereferenced

    def call(scan=S, sstride=None, n=1, h=4, w=5, bpp=3, out=O, ostride=None, rstride=None, swap16=0):
        rstride = w * bpp if rstride is None else rstride
        sstride = h * (1 + w * bpp) if sstride is None else sstride
        ostride = (h - 1) * rstride + w * bpp if ostride is None else ostride
        return lib.sf_png_unfilter(scan, sstride, n, h, w, bpp, out, ostride, rstride, swap16, None), lib.sf_last_error()

    bad = [(dict(scan=None), b"null"), (dict(out=None), b"null"), (dict(n=0), b"n_images"), (dict(n=65536), b"n_images"),
           (dict(h=0), b"h = 0"), (dict(w=0), b"w = 0"), (dict(h=-3), b"h = -3")]
    bad += [(dict(bpp=b), b"bpp = %d" % b) for b in (0, 5, 7, 9, 16, -1)]
    bad += [(dict(bpp=3, swap16=1), b"swap16"), (dict(bpp=1, swap16=1), b"swap16")]
    bad += [(dict(sstride=4 * 16 - 1), b"scan_image_stride"), (dict(sstride=0), b"scan_image_stride"),
            (dict(rstride=14), b"out_row_stride"), (dict(rstride=20, ostride=3 * 20 + 14), b"out_image_stride"),
            (dict(ostride=0), b"out_image_stride"),
            (dict(h=1 << 20, w=2047, bpp=1), b"2^31"), (dict(h=(1 << 31) // 16 + 1, w=5, bpp=3), b"2^31")]
    for kw, word in bad:
        status, msg = call(**kw)
        assert status == -1 and b"sf_png_unfilter" in msg and word in msg, (kw, status, msg)
    for kw in (dict(w=MAXB + 1, bpp=1), dict(w=MAXB // 8 + 1, bpp=8), dict(w=MAXB // 3 + 1, bpp=3)):
        status, msg = call(**kw)
        assert status == -2 and b"SF_PNG_MAX_ROW_BYTES" in msg and b"w * bpp" in msg, (kw, status, msg)
    # (the widest rows and the largest block that pass the checks fail only at the launch: there is no device here, or the dummy
    #  pointers would be used -- so the accepting side is tested on the GPU, tests/test_gpu_png_unfilter.py)


def test_wrapper_and_decode_batch_fail_loudly(tmp_path, monkeypatch):
    from streamflow_amd import ops, png_gpu, video
    for i, (h, w) in enumerate(((6, 5), (6, 5), (6, 7))):
        pc.encode(pc.image(h, w, 3, 8, i), pc.filter_types("mixed", h, i), str(tmp_path / f"{i}.png"), 8)
    pc.encode(pc.image(6, 5, 1, 8, 9), pc.filter_types("mixed", 6, 9), str(tmp_path / "grey.png"), 8)
    paths = [str(tmp_path / f"{i}.png") for i in range(3)]
    with pytest.raises(ValueError, match="2.png"):                       # mixed sizes: before the GPU is looked at
        png_gpu.decode_batch(paths, "cuda")
    with pytest.raises(ValueError, match="grey.png"):                    # mixed formats
        png_gpu.decode_batch(paths[:2] + [str(tmp_path / "grey.png")], "cuda")
    with pytest.raises(ValueError, match="2.png"):
        png_gpu.decode_frames(paths, "cuda")
    with pytest.raises(ValueError, match="no files"):
        png_gpu.decode_batch([], "cuda")
    assert 1 <= png_gpu.pool_threads() <= 8 and png_gpu.pool_threads(3) == 3
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        png_gpu.decode_batch(paths[:2], "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.png_unfilter(torch.zeros(1, 6 * 16, dtype=torch.uint8), 6, 5, 3)
    # FrameDir(decode="gpu") without a GPU: the usual loud error, never the host decoder behind the caller's back
    os.remove(paths[2])
    os.remove(str(tmp_path / "grey.png"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    fd = video.FrameDir(str(tmp_path), decode="gpu")
    assert len(fd) == 2 and fd[0].shape == (6, 5, 3)                     # a single frame still decodes on the host
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fd.device_batch(0, 2, torch.device("cuda"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        video.predict_video(lambda x: [x[:, 0, :2]], fd, T=2)
    assert not hasattr(video.FrameDir(str(tmp_path)), "device_batch")    # the default stays the host path
    with pytest.raises(ValueError, match="decode"):
        video.FrameDir(str(tmp_path), decode="auto")
