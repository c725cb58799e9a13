"""CPU: the fixtures and the restatement the GPU JPEG decoder is held to (tests/jpeg_decode_cases.py), and the host half of the
decoder.  decode_ref equals PIL's libjpeg-turbo bit for bit on every fixture (where PIL is installed) and the pixels recorded in
expected.npz (always); jpeg_gpu.parse agrees with decode_ref's own marker walk and refuses what the decoder does not take; the
coefficient bounds of SF_JPEG_COEF_RANGE keep the integer inverse DCT inside 32 bits by a worst-case argument; avi.MjpegReader reads
what avi.MjpegWriter wrote, and files other writers make; video.open_frames picks the right source."""
import os
import struct

import numpy as np
import pytest

from tests import jpeg_cases as jc
from tests import jpeg_decode_cases as dc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_directory_matches_the_case_list():
    files = sorted(f for f in os.listdir(dc.GOLDEN))
    assert files == sorted([n + ".jpg" for n in dc.NAMES + list(dc.REFUSED)] + ["expected.npz"])
    sizes = {f: os.path.getsize(os.path.join(dc.GOLDEN, f)) for f in files}
    assert max(v for f, v in sizes.items() if f.endswith(".jpg")) <= 4096 and sum(sizes.values()) < 200 * 1024
    assert sorted(dc.expected()) == sorted(dc.NAMES)
    for case in dc.OWN_CASES:                                               # the project's own encoder gives these bytes anywhere
        assert dc.own_file(case) == dc.load(case[0])
    for name, src, how in dc.EDIT_CASES:
        assert dc.edit(dc.load(src), how) == dc.load(name)
    assert b"\xff\xc4" not in dc.load("444-16x17-nodht")[:200] and b"\xff\xff\xda" in dc.load("420-33x33-rst3-fill")


@pytest.mark.parametrize("name", dc.NAMES)
def test_decode_ref_equals_the_recorded_pixels(name):
    want = dc.expected()[name]
    got = dc.decode_ref(dc.load(name))
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)


def test_decode_ref_equals_pil_on_every_case():
    pytest.importorskip("PIL.Image")
    for name in dc.NAMES:
        src = dict((n, s) for n, s, how in dc.EDIT_CASES if how == "strip-dht").get(name, name)   # PIL's pixels of the file with its DHT
        assert np.array_equal(dc.decode_ref(dc.load(name)), dc.pil_pixels(dc.load(src))), name
    try:                                                                    # libjpeg-turbo supplies the Annex K.3 tables itself
        assert np.array_equal(dc.pil_pixels(dc.load("444-16x17-nodht")), dc.expected()["444-16x17-nodht"])
    except OSError:
        pass


def test_the_cases_cover_what_they_are_there_for():
    infos = {n: dc.walk(dc.load(n)) for n in dc.NAMES}
    assert {(i["nc"], i["hs"], i["vs"]) for i in infos.values()} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert {1, 7, 8, 9, 16, 17, 33} <= {i["h"] for i in infos.values()} & {i["w"] for i in infos.values()}
    assert len(infos["444-73x9-rows"]["intervals"]) == 10 and len(infos["444-8x2736"]["intervals"]) == 1
    assert infos["420-33x33-rst1"]["restart"] == 1 and infos["420-33x33-rst3"]["restart"] == 3 and infos["420-33x33"]["restart"] == 0
    assert any(b"\xff\x00" in dc.load(n) for n in dc.NAMES if "noise" in n)
    longest = max(max(k + 1 for k, c in enumerate(spec[0]) if c) for i in infos.values() for spec in i["ac"])
    assert longest == 16
    std = infos["444-16x17"]["ac"][0]
    assert any(i["ac"][0] != std for n, i in infos.items() if n.endswith("-opt"))          # optimize=True wrote tables of its own
    info, coef = dc.coefficients(dc.load("own-basis77-only63-8x8-grey"))
    assert np.count_nonzero(coef[0][0, 0]) == 1 and coef[0][0, 0, 63] != 0                   # three ZRLs, coefficient 63, no EOB
    # clamping: the checker and block images decode to samples at both ends of the range
    assert dc.decode_ref(dc.load("grey-16x24-q100-checker")).min() == 0 and dc.decode_ref(dc.load("grey-16x24-q100-checker")).max() == 255


@pytest.mark.parametrize("name", dc.NAMES)
def test_parse_agrees_with_the_reference_walk(name):
    from streamflow_amd import jpeg_gpu
    blob = dc.load(name)
    info, p = dc.walk(blob), jpeg_gpu.parse(blob, name)
    assert (p.h, p.w, p.components, p.hs, p.vs) == (info["h"], info["w"], info["nc"], info["hs"], info["vs"])
    assert len(p.table_set) == dc.TABLE_SET_BYTES == jpeg_gpu.TABLE_SET_BYTES and jpeg_gpu.DESC_WORDS == dc.DESC_WORDS
    for c in range(info["nc"]):
        rec = p.table_set[c * 608:(c + 1) * 608]
        assert list(rec[:64]) == [int(v) for v in info["quant"][c]]
        for k, spec in enumerate((info["dc"][c], info["ac"][c])):
            got = rec[64 + 272 * k:64 + 272 * (k + 1)]
            assert list(got[:16]) == list(spec[0]) and list(got[16:16 + len(spec[1])]) == list(spec[1])
    assert [(off, off + n) for off, n, _, _ in p.intervals] == info["intervals"]
    mcus = -(-info["w"] // (8 * info["hs"])) * -(-info["h"] // (8 * info["vs"]))
    per = info["restart"] or mcus
    assert [(first, n) for _, _, first, n in p.intervals] == [(k, min(per, mcus - k)) for k in range(0, mcus, per)]


def test_parse_refusals_and_broken_framing(tmp_path):
    from streamflow_amd import jpeg_gpu
    for name in dc.REFUSED:
        with pytest.raises(jpeg_gpu.UnsupportedJpeg):
            jpeg_gpu.parse(dc.load(name), name)
    blob = dc.load("444-16x33-rows")
    sof = next(lo for m, lo, _ in dc.segments(blob) if m == 0xC0)
    with pytest.raises(jpeg_gpu.UnsupportedJpeg, match="height 0"):         # the height a DNL marker would set
        jpeg_gpu.parse(blob[:sof + 1] + b"\x00\x00" + blob[sof + 3:], "patched")
    ids = bytearray(blob)
    sos = next(lo for m, lo, _ in dc.segments(blob) if m == 0xDA)
    for i, ch in enumerate(b"RGB"):
        ids[sof + 6 + 3 * i], ids[sos + 1 + 2 * i] = ch, ch
    with pytest.raises(jpeg_gpu.UnsupportedJpeg, match="RGB"):
        jpeg_gpu.parse(bytes(ids), "rgb ids")
    dnl = blob[:-2] + b"\xff\xdc\x00\x04\x00\x10\xff\xd9"
    with pytest.raises(jpeg_gpu.UnsupportedJpeg, match="DNL"):
        jpeg_gpu.parse(dnl, "dnl")
    # broken framing is a ValueError that names the file, and no UnsupportedJpeg
    body = blob.index(b"\xff\xd0")
    wrong = blob[:body + 1] + b"\xd3" + blob[body + 2:]
    for bad, what in ((b"\x89PNG" + blob, "no SOI"), (blob[:60], "ends"), (wrong, "RST"), (blob[:body] + blob[body + 2:], "restart markers"),
                      (blob[:-2], "EOI")):
        with pytest.raises(ValueError, match="frame 7") as e:
            jpeg_gpu.parse(bad, "frame 7")
        assert not isinstance(e.value, jpeg_gpu.UnsupportedJpeg), what
    # tolerated: a comment, an unknown APPn segment, bytes behind EOI
    noisy = blob[:2] + b"\xff\xfe\x00\x05abc" + b"\xff\xe7\x00\x04\x01\x02" + blob[2:] + b"\x00trailing\xff\xd8"
    assert jpeg_gpu.parse(noisy).intervals[0][1] == jpeg_gpu.parse(blob).intervals[0][1]
    assert jpeg_gpu.parse(noisy)[:6] == jpeg_gpu.parse(blob)[:6]


def test_pack_deduplicates_table_sets_and_lays_out_descriptors():
    from streamflow_amd import jpeg_gpu
    call = dc.Call(dc.MUTATED)
    assert call.tables.shape == (2, dc.TABLE_SET_BYTES)                      # the two non-optimised files share their tables
    assert call.desc.shape == (1 + 9 + 3, dc.DESC_WORDS) and call.desc.dtype == np.int64
    assert [len(call.rows(i)) for i in range(3)] == [1, 9, 3]
    for r in call.desc:
        off, n, image = int(r[0]), int(r[1]), int(r[2])
        blob = dc.load(dc.MUTATED[image])
        p = jpeg_gpu.parse(blob)
        k = [iv[2] for iv in p.intervals].index(int(r[3]))
        assert call.data[off:off + n].tobytes() == blob[p.intervals[k][0]:p.intervals[k][0] + p.intervals[k][1]]
    with pytest.raises(RuntimeError):
        jpeg_gpu.decode_batch([dc.load(n) for n in dc.MUTATED], "cpu")
    with pytest.raises(ValueError):
        jpeg_gpu.decode_batch([], "cpu")


def test_coefficient_bounds_keep_the_inverse_dct_inside_32_bits():
    """X = 2048 per coefficient and 18432 per block (SF_JPEG_COEF_RANGE) by the worst-case argument of idct_bounds; the
    per-coefficient bound alone would not do; and the bounds admit every block an 8-bit image can produce."""
    hdr = open(os.path.join(REPO, "include", "streamflow_hip.h")).read()
    core = open(os.path.join(REPO, "streamflow_amd", "csrc", "jpeg_decode_core.h")).read()
    assert f"kCoefMax = {dc.COEF_MAX}, kBlockSumMax = {dc.BLOCK_SUM_MAX}" in core and "beyond 2048" in hdr and "beyond 18432" in hdr
    assert dc.COEF_MAX >= 2048
    p1, p2 = dc.idct_bounds(dc.COEF_MAX, dc.BLOCK_SUM_MAX)
    assert p1 < 2 ** 31 and p2 < 2 ** 31, (p1 / 2 ** 31, p2 / 2 ** 31)
    assert p2 <= 0.88 * 2 ** 31                                             # the figure the header quotes
    assert dc.idct_bounds(dc.COEF_MAX, 64 * dc.COEF_MAX)[1] >= 2 ** 31      # without the block bound the argument fails ...
    worst = np.full(64, dc.COEF_MAX, np.int64)                              # ... and so does the arithmetic: all 64 at +2048
    f = worst.reshape(8, 8)
    cols = (np.stack(dc.islow_1d([f[v, :] for v in range(8)]), axis=-2) + 1024) >> 11
    assert int(np.abs(np.stack(dc.islow_1d([cols[:, u] for u in range(8)]), axis=-1)).max()) >= 2 ** 31
    # what 8-bit samples can reach: the exact DCT has |F| <= 1024 and sum |F| <= 8192, dequantised values at most double them
    basis = jc.dct_basis()
    assert float(np.abs(np.einsum("vy,ux->vuyx", basis, basis)).sum(axis=(2, 3)).max()) * 128 <= 1024 + 1e-9
    assert 2 * 1024 <= dc.COEF_MAX and 2 * 8 * 8 * 128 + 2048 <= dc.BLOCK_SUM_MAX
    rng = np.random.default_rng(5)
    for s in (rng.integers(0, 2, (200, 8, 8)) * 255 - 128, np.sign(np.einsum("vy,ux->vuyx", basis, basis)).reshape(64, 8, 8) * 127.5 - 0.5):
        F = np.einsum("vy,nyx,ux->nvu", basis, s.astype(np.float64), basis)
        assert np.abs(F).max() <= 1024 and np.abs(F).reshape(len(F), -1).sum(axis=1).max() <= 8192 + 1e-6


def _write_avi(path, frames, fps=12.5):
    from streamflow_amd import avi
    w, h = avi.jpeg_size(frames[0])
    with avi.MjpegWriter(str(path), w, h, fps) as v:
        for f in frames:
            v.add(f)
    return open(path, "rb").read()


def test_mjpeg_reader_reads_what_the_writer_wrote(tmp_path):
    from streamflow_amd import avi
    frames = [dc.load(n) for n in dc.MUTATED]
    data = _write_avi(tmp_path / "a.avi", frames)
    with avi.MjpegReader(str(tmp_path / "a.avi")) as r:
        assert len(r) == 3 and r.hw == (33, 33) and r.fps == 12.5
        assert [r.frame_bytes(i) for i in range(3)] == frames
        assert hasattr(r, "device_batch") and hasattr(r, "__getitem__")
    # without idx1: the reader walks movi
    idx = data.rindex(b"idx1")
    cut = data[:idx]
    cut = cut[:4] + struct.pack("<I", len(cut) - 8) + cut[8:]
    (tmp_path / "noidx.avi").write_bytes(cut)
    with avi.MjpegReader(str(tmp_path / "noidx.avi")) as r:
        assert [r.frame_bytes(i) for i in range(len(r))] == frames
    # frames inside 'rec ' lists, '00db' tags, an audio chunk between them, and an empty chunk that repeats frame 1
    movi = data.index(b"movi")

    def chunk(tag, payload):
        return tag + struct.pack("<I", len(payload)) + payload + b"\x00" * (len(payload) & 1)

    recs = b"".join(chunk(b"LIST", b"rec " + chunk(b"01wb", b"\x00" * 6) + chunk(b"00db" if k else b"00dc", f)) for k, f in enumerate(frames[:2]))
    body = b"movi" + recs + chunk(b"00dc", b"") + chunk(b"00dc", frames[2])
    head = data[:movi - 4] + struct.pack("<I", len(body))
    rebuilt = head + body
    rebuilt = rebuilt[:4] + struct.pack("<I", len(rebuilt) - 8) + rebuilt[8:]
    (tmp_path / "rec.avi").write_bytes(rebuilt)
    with avi.MjpegReader(str(tmp_path / "rec.avi")) as r:
        assert [r.frame_bytes(i) for i in range(len(r))] == [frames[0], frames[1], frames[1], frames[2]]
    # idx1 with an empty chunk, offsets from the start of the file
    body = b"movi" + chunk(b"00dc", frames[0]) + chunk(b"00dc", b"") + chunk(b"00dc", frames[1])
    start = len(head) - 0                                                   # the 'movi' tag follows the list's size field
    offs, at = [], start + 4
    for size in (len(frames[0]), 0, len(frames[1])):
        offs.append((at, size))
        at += 8 + size + (size & 1)
    index = chunk(b"idx1", b"".join(struct.pack("<4sIII", b"00dc", 0x10, off, size) for off, size in offs))
    rebuilt = head[:-4] + struct.pack("<I", len(body)) + body + index
    rebuilt = rebuilt[:4] + struct.pack("<I", len(rebuilt) - 8) + rebuilt[8:]
    (tmp_path / "abs.avi").write_bytes(rebuilt)
    with avi.MjpegReader(str(tmp_path / "abs.avi")) as r:
        assert [r.frame_bytes(i) for i in range(len(r))] == [frames[0], frames[0], frames[1]]


def test_mjpeg_reader_refuses_what_it_cannot_read(tmp_path):
    from streamflow_amd import avi
    data = _write_avi(tmp_path / "a.avi", [dc.load(n) for n in dc.MUTATED])
    bad = {"png": b"\x89PNG\r\n\x1a\n" + bytes(64), "wave": data[:8] + b"WAVE" + data[12:], "short": data[:10],
           "h264": data.replace(b"MJPG", b"H264"), "avix": data + b"RIFF" + struct.pack("<I", 4) + b"AVIX"}
    for name, blob in bad.items():
        p = tmp_path / (name + ".avi")
        p.write_bytes(blob)
        with pytest.raises(ValueError, match=name + ".avi"):
            avi.MjpegReader(str(p))
    lower = tmp_path / "lower.avi"
    lower.write_bytes(data.replace(b"MJPG", b"mjpg"))
    assert len(avi.MjpegReader(str(lower))) == 3


def test_open_frames_dispatches_on_what_the_path_holds(tmp_path):
    from streamflow_amd import avi, flow_io, video
    img = jc.make("mixed", 33, 33, 3, 1)
    for d in ("png", "jpg", "jpeg", "mixed", "empty"):
        (tmp_path / d).mkdir()
    for i in range(3):
        flow_io.write_png(str(tmp_path / "png" / f"{i:03d}.png"), img)
        flow_io.write_png(str(tmp_path / "mixed" / f"{i:03d}.png"), img)
        (tmp_path / "jpg" / f"{i:03d}.jpg").write_bytes(dc.load(dc.MUTATED[i]))
        (tmp_path / "jpeg" / f"{2 - i:03d}.jpeg").write_bytes(dc.load(dc.MUTATED[i]))
    (tmp_path / "mixed" / "003.jpg").write_bytes(dc.load(dc.MUTATED[0]))
    src = video.open_frames(str(tmp_path / "png"))
    assert isinstance(src, video.FrameDir) and not hasattr(src, "device_batch") and len(src) == 3 and src.hw == (33, 33)
    assert hasattr(video.open_frames(str(tmp_path / "png"), "gpu"), "device_batch")
    for d in ("jpg", "jpeg"):
        src = video.open_frames(str(tmp_path / d))
        assert isinstance(src, video.JpegDir) and len(src) == 3 and src.hw == (33, 33) and hasattr(src, "device_batch")
        assert [os.path.basename(p) for p in src.paths] == sorted(os.listdir(tmp_path / d))
    _write_avi(tmp_path / "v.avi", [dc.load(n) for n in dc.MUTATED])
    src = video.open_frames(str(tmp_path / "v.avi"))
    assert isinstance(src, avi.MjpegReader) and len(src) == 3 and src.hw == (33, 33)
    with pytest.raises(ValueError, match="one kind"):
        video.open_frames(str(tmp_path / "mixed"))
    with pytest.raises(FileNotFoundError):
        video.open_frames(str(tmp_path / "empty"))
    with pytest.raises(FileNotFoundError):
        video.open_frames(str(tmp_path / "nothing-here"))
    (tmp_path / "jpg" / "009.jpg").write_bytes(dc.load("444-16x17"))
    with pytest.raises(ValueError, match="009.jpg"):
        video.JpegDir(str(tmp_path / "jpg"))
    # predict_video's source takes both as lazy sequences with a size, without decoding anything
    s = video._Source(video.open_frames(str(tmp_path / "v.avi")))
    assert (s.n, s.hw) == (3, (33, 33))


def test_the_entry_points_are_declared_and_registered():
    from streamflow_amd import _lib, build, ops
    hdr = open(os.path.join(REPO, "include", "streamflow_hip.h")).read()
    for name in ("sf_jpeg_decode", "sf_jpeg_decode_ws_bytes"):
        assert name in _lib.SIGNATURES and name + "(" in hdr
    assert len(_lib.SIGNATURES["sf_jpeg_decode"][1]) == 20 and callable(ops.jpeg_decode)
    assert "jpeg_decode.hip" in build.SOURCES and any(h.endswith("jpeg_decode_core.h") for h in build.HEADERS)
    assert all(k in build.HOT_KERNELS for k in ("jpeg_entropy_kernel", "jpeg_status_kernel", "jpeg_idct_kernel", "jpeg_colour_kernel"))
    from streamflow_amd import jpeg_gpu
    words = [w for w in ("OK", "BAD_CODE", "BAD_RUN", "BAD_CATEGORY", "TRUNCATED", "NOT_CONSUMED", "BAD_DESC", "COEF_RANGE", "BAD_TABLE",
                         "BAD_MARKER")]
    for k, w in enumerate(words):
        assert f"SF_JPEG_{w} = {k}" in hdr and getattr(dc, w) == k
    assert len(jpeg_gpu.DECODE_STATUS) == len(words)
    assert f"#define SF_JPEG_TABLE_SET_BYTES {dc.TABLE_SET_BYTES}" in hdr and f"#define SF_JPEG_DESC_WORDS {dc.DESC_WORDS}" in hdr
