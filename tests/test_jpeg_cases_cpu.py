"""Pins tests/jpeg_cases.py's encode_ref -- the restatement the GPU encoder must equal byte for byte (tests/test_gpu_jpeg_encode.py) --
on the CPU: against an independent Huffman decoder of the segment, a float64 DCT, PIL's libjpeg (decoding our files, encoding the
same images at the same tables, its quantisation and Huffman tables), and the host-side writers (jpeg_gpu.quant_tables / jpeg_file,
avi.MjpegWriter) against a RIFF walker (tests/avi_walk.py).  No player is installed here: whether the AVI plays rests on the walker's
field checks and on PIL decoding every frame."""
import struct

import numpy as np
import pytest

from streamflow_amd import avi, jpeg_gpu
from tests import jpeg_cases as jc
from tests.avi_walk import walk


def _segments(blob):
    """[(marker, payload)] of a JPEG file's marker segments up to and including SOS."""
    assert blob[:2] == b"\xff\xd8"
    out, i = [], 2
    while True:
        assert blob[i] == 0xFF, i
        size = struct.unpack_from(">H", blob, i + 2)[0]
        out.append((blob[i + 1], blob[i + 4:i + 2 + size]))
        i += 2 + size
        if out[-1][0] == 0xDA:
            return out


@pytest.fixture(scope="module")
def encoded():
    """{case: (image, tables, levels, segment)}: every case encoded once."""
    out = {}
    for case in jc.CASES:
        kind, h, w, c, quality, seed = case
        img, q = jc.make(kind, h, w, c, seed), jc.tables(quality)
        lv = jc.levels(img, q)
        out[case] = (img, q, lv, jc.entropy(lv))
    return out


def test_the_tables_the_header_states():
    assert np.array_equal(np.rint(2 ** 13 * np.sqrt(2) * jc.dct_basis()).astype(np.int64), jc.DCT_TABLE)
    assert np.array_equal(jc.ZZ, np.array(jpeg_gpu.ZIGZAG)) and sorted(jc.ZZ) == list(range(64))
    specs = [jc.DC_LUMA, jc.AC_LUMA, jc.DC_CHROMA, jc.AC_CHROMA]
    for (tc, bits, vals), spec in zip(jpeg_gpu.HUFFMAN_TABLES, specs):
        assert (list(bits), list(vals)) == (spec[0], spec[1]), hex(tc)
        assert sum(spec[0]) == len(spec[1]) == len(set(spec[1]))
    assert jc.dct_bound() <= jc.DCT_B < jc.dct_bound() + 1e-3
    assert jc.bound(2160, 3840, 3) < 2 ** 31 and jc.bound(jc.header_constant("SF_JPEG_MAX_DIM"), jc.header_constant("SF_JPEG_MAX_DIM"), 3) < 2 ** 31


@pytest.mark.parametrize("case", jc.CASES, ids=jc.case_id)
def test_decode_scan_returns_the_levels(encoded, case):
    """An independent decoder reads back exactly the restatement's quantised levels; the segment keeps the bound; no marker bytes but
    the RSTm between intervals."""
    img, q, lv, seg = encoded[case]
    _, h, w, c = case[:4]
    assert np.array_equal(jc.decode_scan(seg, h, w, c), lv)
    assert len(seg) <= jc.bound(h, w, c)
    assert np.abs(lv[..., 0]).max() <= 1024 and np.abs(lv[..., 1:]).max(initial=0) <= 1023


def test_the_cases_hold_what_they_are_there_for(encoded):
    by_kind = {}
    for case, (img, q, lv, seg) in encoded.items():
        by_kind.setdefault((case[0], case[4]), []).append((case, lv, seg))
    for case, lv, seg in by_kind[("noise", 100)]:
        assert seg.count(b"\xff\x00") >= 5, case                                   # stuffed bytes
    for case, lv, seg in by_kind[("basis77", "only63")]:
        assert (lv[:, :, 0, 63] != 0).all() and not lv[:, :, 0, :63].any() and not lv[:, :, 1:].any(), case     # 62-zero runs, no EOB
    assert max(np.abs(lv[..., 1:]).max() for _, lv, _ in by_kind[("checker", 100)]) >= 512      # AC category 10
    for case, lv, seg in by_kind[("blocks", 100)]:
        assert np.abs(np.diff(lv[:, :, 0, 0], axis=1)).max() >= 1024, case         # DC difference category 11
    for case, lv, seg in by_kind[("const", 75)] + by_kind[("const", 100)]:
        assert not lv[..., 1:].any(), case
    assert jc.encode_ref(jc.make("const", 16, 8, 1, 128), jc.tables(90)) == b"\x2b\xff\xd0\x2b"  # 00 1010 + 11: one-byte intervals
    rst = jc.encode_ref(jc.make("mixed", 73, 9, 1, 2), jc.tables(90))
    assert [rst[i + 1] for i in range(len(rst) - 1) if rst[i] == 0xFF and rst[i + 1] != 0] == [0xD0 + k % 8 for k in range(9)]


def test_the_integer_dct_is_within_the_derived_bound(encoded):
    """B = jc.DCT_B = 0.3126 coefficient units is the WORST-CASE distance of the integer DCT (G / 2^18) from the exact coefficient,
    derived from the table width and the shifts alone (jc.dct_bound: rows 8 x 128 x 2^-14 + 2^-5 = 0.09375, columns 4 x 0.09375 +
    8 x 2^-14 x (512 + 0.09375) = 0.62505, halved because two passes of the sqrt 2-scaled table give twice the coefficient).  Every
    coefficient of every case obeys it, and every quantised level obeys |q level - exact| <= q / 2 + B.  Also on the corners of the
    sample cube that maximise single coefficients (sign patterns of the basis functions)."""
    a = jc.dct_basis()
    extra = [np.where(np.outer(a[v], a[u]) >= 0, 127, -128)[None, None, None] for v in range(8) for u in range(8)]
    extra += [-e - 1 for e in extra]
    worst = 0.0
    for img, q, lv, _ in encoded.values():
        s = jc.blocks(img)
        exact = np.einsum("vy,...yx,ux->...vu", a, s.astype(np.float64), a)
        err = np.abs(jc.dct_int(s) / 2.0 ** 18 - exact).max()
        worst = max(worst, err)
        qc = np.stack([np.asarray(q, np.float64).reshape(2, 64)[0 if c == 0 else 1] for c in range(s.shape[2])])
        natural = exact.reshape(exact.shape[:3] + (64,))[..., jc.ZZ]
        assert (np.abs(qc[:, jc.ZZ] * lv - natural) <= qc[:, jc.ZZ] / 2 + jc.DCT_B).all()
    for s in extra:
        exact = np.einsum("vy,...yx,ux->...vu", a, s.astype(np.float64), a)
        worst = max(worst, np.abs(jc.dct_int(s) / 2.0 ** 18 - exact).max())
        assert np.abs(exact.reshape(-1)[1:]).max() <= 1020 + 1e-6
    print(f"largest DCT error {worst:.4f} of B = {jc.DCT_B}")
    assert worst <= jc.DCT_B


def test_pil_decodes_every_file_as_well_as_its_own(encoded):
    """Every case's jpeg_file opens in PIL with the right size and mode and decodes, and its PSNR against the source is at least the
    PSNR of libjpeg's own file of the same image (qtables= the same tables, subsampling=0, optimize=False) minus jc.PSNR_MARGIN_DB =
    0.164 dB: the restatement's worst deficit over CASES measured here, 0.114 dB (on the 9 x 7 colour case; the median case is
    bit-identical to libjpeg's decode, and several are above it), plus 0.05 dB for the colour-conversion and DCT rounding differences
    between two correct encoders."""
    pytest.importorskip("PIL.Image")
    worst = -99.0
    for case, (img, q, lv, seg) in encoded.items():
        _, h, w, c = case[:4]
        im = jc.pil_decode(jpeg_gpu.jpeg_file(seg, h, w, c, q))
        assert im.size == (w, h) and im.mode == ("RGB" if c == 3 else "L"), case
        ours = jc.psnr(img, np.asarray(im))
        theirs = jc.psnr(img, np.asarray(jc.pil_decode(jc.pil_file(img, q))))
        worst = max(worst, theirs - ours)
        assert ours >= theirs - jc.PSNR_MARGIN_DB, (case, ours, theirs)
    print(f"worst PSNR deficit against libjpeg {worst:.4f} dB (recorded: {jc.PSNR_DEFICIT_DB})")
    assert worst <= jc.PSNR_DEFICIT_DB


def test_quant_tables_are_the_ones_pil_writes():
    """jpeg_gpu.quant_tables(q) equals the DQT tables of a PIL file saved at quality=q (read from the file's DQT segments, which are in
    zigzag order) for EVERY quality 1 .. 100, not only the required 25 .. 100."""
    pytest.importorskip("PIL.Image")
    import io
    from PIL import Image
    for quality in range(1, 101):
        buf = io.BytesIO()
        Image.new("RGB", (8, 8)).save(buf, "JPEG", quality=quality)
        dqt = [p for m, p in _segments(buf.getvalue()) if m == 0xDB]
        tables = {p[0]: list(p[1:65]) for p in dqt}
        mine = jpeg_gpu.quant_tables(quality)
        for t in (0, 1):
            assert tables[t] == [int(mine[t, z]) for z in jc.ZZ], (quality, t)
    for bad in (0, 101, -3):
        with pytest.raises(ValueError):
            jpeg_gpu.quant_tables(bad)


def test_header_segments_against_pil():
    """The four DHT segments equal the ones PIL writes with optimize=False, byte for byte; DQT and SOF0 too, and the file differs from
    PIL's header only by its DRI segment."""
    pytest.importorskip("PIL.Image")
    img, q = jc.make("wheel", 24, 40, 3, 5), jpeg_gpu.quant_tables(75)
    theirs = _segments(jc.pil_file(img, q))
    ours = _segments(jpeg_gpu.jpeg_file(jc.encode_ref(img, q), 24, 40, 3, q))
    dht = [p for m, p in ours if m == 0xC4]
    assert len(dht) == 4 and dht == [p for m, p in theirs if m == 0xC4]
    assert [b"\xff\xc4" + struct.pack(">H", len(p) + 2) + p for p in dht] == jpeg_gpu.dht_segments(3)
    assert [s for s in ours if s[0] != 0xDD] == theirs
    assert [p for m, p in ours if m == 0xDD] == [struct.pack(">H", 5)]
    grey = _segments(jpeg_gpu.jpeg_file(jc.encode_ref(img[:, :, 0], q), 24, 40, 1, q))
    assert [s for s in grey if s[0] != 0xDD] == _segments(jc.pil_file(img[:, :, 0], q))
    for bad in (dict(h=0), dict(w=65536), dict(channels=2)):
        with pytest.raises(ValueError):
            jpeg_gpu.jpeg_file(b"", **dict(dict(h=8, w=8, channels=1, qtables=q), **bad))
    with pytest.raises(ValueError):
        jpeg_gpu.jpeg_file(b"", 8, 8, 1, np.zeros((2, 64)))


@pytest.mark.parametrize("fps,rate,scale", [(8, 8, 1), (30, 30, 1), (23.976, 2997, 125), (30000 / 1001, 30000, 1001)])
def test_mjpeg_writer_passes_the_riff_walker(tmp_path, fps, rate, scale):
    """Every size field and the even padding, avih / strh frame counts and rate / scale, each idx1 entry against its 00dc chunk
    (tests/avi_walk.py), and every frame's bytes come back and (with PIL) decode."""
    q = jpeg_gpu.quant_tables(90)
    images = [jc.make("wheel", 24, 40, 3, s) for s in range(5)]
    frames = [jpeg_gpu.jpeg_file(jc.encode_ref(im, q), 24, 40, 3, q) for im in images]
    frames[1] += b"\x00" * (1 - len(frames[1]) % 2)                          # one odd and one even length at least
    frames[2] += b"\x00" * (len(frames[2]) % 2)
    assert len(frames[1]) % 2 == 1 and len(frames[2]) % 2 == 0
    path = str(tmp_path / "v.avi")
    with avi.MjpegWriter(path, 40, 24, fps) as v:
        for f in frames:
            v.add(f)
    info = walk(open(path, "rb").read())
    assert (info["width"], info["height"], info["rate"], info["scale"]) == (40, 24, rate, scale)
    assert info["frames"] == frames
    try:
        from PIL import Image  # noqa: F401
    except ImportError:
        return
    for im, f in zip(images, info["frames"]):
        got = jc.pil_decode(f)
        assert got.size == (40, 24) and jc.psnr(im, np.asarray(got)) > 30


def test_mjpeg_writer_refusals(tmp_path, monkeypatch):
    q = jpeg_gpu.quant_tables(50)
    frame = jpeg_gpu.jpeg_file(jc.encode_ref(jc.make("const", 8, 16, 1, 9), q), 8, 16, 1, q)
    other = jpeg_gpu.jpeg_file(jc.encode_ref(jc.make("const", 16, 8, 1, 9), q), 16, 8, 1, q)
    for bad in (dict(width=0), dict(height=70000), dict(fps=0), dict(fps=-1), dict(fps=1e-9)):
        with pytest.raises(ValueError):
            avi.MjpegWriter(**dict(dict(path=str(tmp_path / "bad.avi"), width=16, height=8, fps=8), **bad))
    v = avi.MjpegWriter(str(tmp_path / "v.avi"), 16, 8, 8)
    v.add(frame)
    for bad in (other, b"", b"not a jpeg", frame[:10]):
        with pytest.raises(ValueError):
            v.add(bad)
    monkeypatch.setattr(avi, "MAX_FILE_BYTES", v.pos + 8 + len(frame) + len(frame) % 2 + 8 + 32 - 1)       # one byte short of a second frame
    with pytest.raises(ValueError):
        v.add(frame)
    monkeypatch.setattr(avi, "MAX_FILE_BYTES", v.pos + 8 + len(frame) + len(frame) % 2 + 8 + 32)
    v.add(frame)
    v.close()
    v.close()
    with pytest.raises(ValueError):
        v.add(frame)
    data = open(str(tmp_path / "v.avi"), "rb").read()
    assert len(data) == avi.MAX_FILE_BYTES and walk(data)["frames"] == [frame, frame]
    empty = str(tmp_path / "empty.avi")
    avi.MjpegWriter(empty, 16, 8, 8).close()
    assert walk(open(empty, "rb").read())["frames"] == []


def test_command_line_needs_out_or_video(capsys):
    from streamflow_amd import demo
    with pytest.raises(SystemExit) as e:
        demo.main(["--frames", "frames", "--ckpt", "ckpt.pth"])
    assert e.value.code == 2 and "--out (or --video)" in capsys.readouterr().err


def test_no_gpu_no_fallback(tmp_path):
    """CPU tensors are refused with a RuntimeError, with or without a GPU in the machine; without one vis_flow_video raises too."""
    import torch
    from streamflow_amd import demo, ops
    images = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ops.jpeg_encode(images, jpeg_gpu.quant_tables(90))
    with pytest.raises(RuntimeError):
        jpeg_gpu.encode_batch(images)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            demo.vis_flow_video([torch.zeros(2, 8, 8)], str(tmp_path / "unused.avi"))
