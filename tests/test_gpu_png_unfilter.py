"""PNG row unfiltering on the GPU: sf_png_unfilter (csrc/png_unfilter.hip) through the C ABI, ops.png_unfilter, png_gpu.decode_batch,
video.FrameDir(decode="gpu") and the dataset loops with png_decode="gpu", against tests/png_cases.py's encoder (pinned to two
decoders by tests/test_png_cases_cpu.py) and flow_io.read_png.

Criterion: every comparison is BITWISE.  The arithmetic is on integers mod 256, so there is no tolerance to choose.  Inputs and
outputs sit between guard bands (tests/guarded.GuardedBytes) that must come back intact; `out` has a row stride and an image stride
larger than the extent, and the bytes between rows and images must be unchanged.  The shapes are derived from SF_PNG_BAND_ROWS (R)
and SF_PNG_MAX_ROW_BYTES as the header states them: the smallest at which the band hand-over, a wave's edge and the LDS row can go
wrong."""
import os

import numpy as np
import pytest
import torch

from tests import png_cases as pc
from tests import video_cases as vc
from tests.guarded import GuardedBytes

pytestmark = pytest.mark.gpu

R = pc.header_constant("SF_PNG_BAND_ROWS")
MAXB = pc.header_constant("SF_PNG_MAX_ROW_BYTES")
FILL = 0x7F
# (channels, depth): bpp 1, 2, 3, 4, 6, 8
FORMATS = [(1, 8), (2, 8), (3, 8), (4, 8), (3, 16), (4, 16)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def swapped(rows):
    """The bytes of every 16-bit sample exchanged."""
    return np.ascontiguousarray(rows.reshape(rows.shape[0], -1, 2)[:, :, ::-1]).reshape(rows.shape)


def unfilter(dev, blocks, w, bpp, swap16=False, shift=0):
    """sf_png_unfilter through the C ABI on the scanline blocks [h, 1 + w * bpp] of n images -> uint8 [n, h, w * bpp].  The scan
    buffer starts `shift` bytes off the allocation's alignment and leaves 7 bytes between images; out has 5 bytes between rows and
    3 more between images.  Asserts on the way: status, guard bands, the bytes outside the view, every byte inside written."""
    from streamflow_amd import _lib
    n, h = len(blocks), blocks[0].shape[0]
    line, row = 1 + w * bpp, w * bpp
    sstride, rstride = h * line + 7, row + 5
    ostride = h * rstride + 3
    scan = GuardedBytes(dev, (n - 1) * sstride + h * line, fill=0xEE, shift=shift)
    host = np.full(scan.size, 0xEE, np.uint8)
    for i, b in enumerate(blocks):
        assert b.shape == (h, line) and b.dtype == np.uint8
        host[i * sstride:i * sstride + h * line] = b.reshape(-1)
    scan.view().copy_(torch.from_numpy(host))
    out = GuardedBytes(dev, (n - 1) * ostride + (h - 1) * rstride + row, fill=FILL, shift=(shift * 3) % 4)
    status = _lib.load().sf_png_unfilter(scan.ptr, sstride, n, h, w, bpp, out.ptr, ostride, rstride, 1 if swap16 else 0,
                                         torch.cuda.current_stream().cuda_stream)
    assert status == 0, _lib.load().sf_last_error()
    torch.cuda.synchronize()
    assert scan.guards_unchanged() and out.guards_unchanged()
    assert np.array_equal(scan.view().cpu().numpy(), host)
    flat = out.view().cpu().numpy()
    idx = (np.arange(n)[:, None, None] * ostride + np.arange(h)[None, :, None] * rstride + np.arange(row)[None, None, :])
    inside = np.zeros(flat.size, bool)
    inside[idx.reshape(-1)] = True
    assert (flat[~inside] == FILL).all(), "bytes between rows / images were written"
    return flat[idx]


def check(dev, images, types, depth, swap16=False, shift=0):
    """Encode each image with its filter types, unfilter the batch on the GPU, compare with the images' own bytes."""
    blocks, rows = [], []
    for img, ft in zip(images, types):
        blocks.append(pc.encode(img, ft, None, depth))
        rows.append(pc.raw_rows(img, depth)[0])
    c = images[0].shape[2]
    got = unfilter(dev, blocks, images[0].shape[1], c * depth // 8, swap16, shift)
    want = np.stack([swapped(r) if swap16 else r for r in rows])
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} bytes differ, first at (image, row, byte) {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    return got


@pytest.mark.parametrize("h", sorted({1, 2, 63, 64, 65, R - 1, R, R + 1, 2 * R + 1}))
def test_rows_at_wave_and_band_edges(dev, h):
    """A wave's edge (63, 64, 65 rows), the carried row (R - 1, R, R + 1) and a last band of one row (2 R + 1), each with rows of 1,
    2, 5 and 17 pixels (shorter than, equal to and longer than the diagonal's lead), 8-bit RGB and grey, filter types per row."""
    for w in (1, 2, 5, 17):
        for c in (3, 1):
            check(dev, [pc.image(h, w, c, 8, 7 * h + w + c)], [pc.filter_types("mixed", h, h + w)], 8, shift=w % 4)


@pytest.mark.parametrize("hw", [(2, 4099), (3, MAXB // 8)], ids=lambda x: f"{x[0]}x{x[1]}")
def test_long_rows_at_bpp_8(dev, hw):
    """A long row, and the widest one the LDS row buffer takes (w * bpp = SF_PNG_MAX_ROW_BYTES), 16-bit RGBA."""
    h, w = hw
    assert w * 8 <= MAXB
    check(dev, [pc.image(h, w, 4, 16, w)], [pc.filter_types("mixed", h, w) if h == 2 else np.array([4, 3, 4], np.uint8)], 16)
    if w * 8 == MAXB:                                                   # one pixel more is refused, not truncated
        from streamflow_amd import _lib
        assert _lib.load().sf_png_unfilter(4096, 3 * (1 + MAXB + 8), 1, 3, w + 1, 8, 8192, 3 * (MAXB + 8), MAXB + 8, 0, None) == -2


@pytest.mark.parametrize("fmt", FORMATS, ids=lambda f: f"c{f[0]}d{f[1]}")
def test_every_bpp_with_and_without_swap16(dev, tmp_path, fmt):
    """bpp 1, 2, 3, 4, 6, 8 over R + 3 rows (two bands) of 19 pixels; with swap16 where bpp is even.  For the 16-bit formats the
    swap16 output viewed as uint16 is flow_io.read_png's array of the same file."""
    from streamflow_amd import flow_io
    c, depth = fmt
    h, w, bpp = R + 3, 19, c * depth // 8
    img, ft = pc.image(h, w, c, depth, 40 + bpp), pc.filter_types("mixed", h, bpp)
    check(dev, [img], [ft], depth, shift=1)
    if bpp % 2 == 0:
        got = check(dev, [img], [ft], depth, swap16=True, shift=3)
        if depth == 16:
            path = str(tmp_path / "f.png")
            pc.encode(img, ft, path, depth)
            assert np.array_equal(np.ascontiguousarray(got[0]).view(np.uint16).reshape(h, w, c), flow_io.read_png(path))
    else:
        from streamflow_amd import _lib
        assert _lib.load().sf_png_unfilter(4096, h * (1 + w * bpp), 1, h, w, bpp, 8192, h * w * bpp, w * bpp, 1, None) == -1


@pytest.mark.parametrize("kind", ["random", "binary"])
def test_filter_types(dev, kind):
    """All rows of one type for each of the five types (that type on row 0 too, where b = c = 0), types drawn per row, and a band's
    first row of each type directly under a row of each type (25 images of R + 1 rows, one call); uniform random bytes and an image
    of only 0 and 255 (an Average on 8 bits, a Paeth with the wrong tie order)."""
    h, w = R + 1, 9
    for c, depth in ((3, 8), (1, 8), (3, 16)):
        images = [pc.image(h, w, c, depth, 60 + t, kind) for t in range(6)]
        types = [pc.filter_types(t, h) for t in range(5)] + [pc.filter_types("mixed", h, 3)]
        check(dev, images, types, depth)
    images, types = [], []
    for above in range(5):
        for first in range(5):
            ft = pc.filter_types("mixed", h, 5 * above + first)
            ft[R - 1], ft[R] = above, first
            types.append(ft)
            images.append(pc.image(h, w, 3, 8, 100 + 5 * above + first, kind))
    check(dev, images, types, 8, shift=2)


def test_filter_byte_above_4_is_type_0(dev, tmp_path):
    """A filter byte of 7 in one row: the host result with that row taken as type 0 (the header's rule; png_scanlines rejects such
    files, so the expected bytes come from the same block with the byte set to 0)."""
    from streamflow_amd import flow_io
    h, w = 12, 7
    block = pc.encode(pc.image(h, w, 3, 8, 5), pc.filter_types("mixed", h, 5), None, 8)
    block[4, 0], block[0, 0] = 7, 200
    legal = block.copy()
    legal[4, 0] = legal[0, 0] = 0
    path = str(tmp_path / "legal.png")
    pc.write_block(path, legal, w, 8, 3)
    got = unfilter(dev, [block], w, 3)
    assert np.array_equal(got[0].reshape(h, w, 3), flow_io.read_png(path))


@pytest.mark.parametrize("n", [1, 3, 33])
def test_several_images_per_call(dev, n):
    """n images, each with its own data and filter sequence, image strides larger than an image: image i of the batch call equals
    the single-image call."""
    h, w = R + 2, 11
    images = [pc.image(h, w, 3, 8, 200 + i) for i in range(n)]
    types = [pc.filter_types("mixed", h, 300 + i) for i in range(n)]
    got = check(dev, images, types, 8, shift=n % 4)
    for i in sorted({0, n // 2, n - 1}):
        assert np.array_equal(check(dev, [images[i]], [types[i]], 8)[0], got[i])


def test_repeatable_and_wrapper(dev):
    """The same call twice into two buffers gives equal bytes; ops.png_unfilter with and without `out` (a strided view) agrees."""
    from streamflow_amd import ops
    h, w, c, depth = R + 5, 23, 4, 16
    img, ft = pc.image(h, w, c, depth, 9), pc.filter_types("mixed", h, 9)
    block = pc.encode(img, ft, None, depth)
    first, second = unfilter(dev, [block], w, 8, True), unfilter(dev, [block], w, 8, True)
    assert np.array_equal(first, second)
    scan = torch.from_numpy(np.stack([block.reshape(-1)] * 2)).to(dev)
    got = ops.png_unfilter(scan, h, w, 8, swap16=True)
    assert got.shape == (2, h, w * 8) and got.dtype == torch.uint8 and np.array_equal(got[1].cpu().numpy(), first[0])
    assert np.array_equal(got.view(torch.uint16).view(2, h, w, c)[0].cpu().numpy(), img)
    big = torch.full((2, h + 1, w * 8 + 3), FILL, dtype=torch.uint8, device=dev)
    res = ops.png_unfilter(scan, h, w, 8, out=big[:, :h, :w * 8], swap16=True)
    assert res.data_ptr() == big.data_ptr() and torch.equal(big[:, :h, :w * 8], got)
    assert bool((big[:, h] == FILL).all()) and bool((big[:, :, w * 8:] == FILL).all())
    with pytest.raises(RuntimeError, match="scan must be uint8"):
        ops.png_unfilter(scan[:, :-1], h, w, 8)
    with pytest.raises(RuntimeError, match="swap16"):
        ops.png_unfilter(torch.zeros(1, 2 * 4, dtype=torch.uint8, device=dev), 2, 1, 3, swap16=True)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.png_unfilter(scan, h, w, 8, out=torch.empty(2, h, w * 8, dtype=torch.int8, device=dev))


# ---- through the layers ---------------------------------------------------------------------------------------------------------
def _write_frames(folder, n, h, w, c, depth, seed):
    os.makedirs(folder, exist_ok=True)
    paths = []
    for i in range(n):
        paths.append(os.path.join(str(folder), "frame_%04d.png" % i))
        pc.encode(pc.image(h, w, c, depth, seed + i), pc.filter_types("mixed", h, seed + i), paths[-1], depth)
    return paths


def test_decode_batch_equals_read_png(dev, tmp_path):
    from streamflow_amd import flow_io, png_gpu
    paths = _write_frames(tmp_path / "rgb", 5, 37, 53, 3, 8, 1)
    got = png_gpu.decode_batch(paths, dev)
    assert got.device == dev and got.dtype == torch.uint8 and got.shape == (5, 37, 53, 3)
    assert np.array_equal(got.cpu().numpy(), np.stack([flow_io.read_png(p) for p in paths]))
    assert torch.equal(png_gpu.decode_batch(paths, dev, threads=1), got)
    # one 16-bit KITTI-style file: the uint16 samples in host order
    (kitti,) = _write_frames(tmp_path / "kitti", 1, 29, 41, 3, 16, 7)
    smp = png_gpu.decode_batch([kitti], dev)
    assert smp.dtype == torch.uint16 and smp.shape == (1, 29, 41, 3)
    assert torch.equal(smp[0].cpu().view(torch.int16), torch.from_numpy(flow_io.read_png(kitti)).view(torch.int16))
    # grey keeps its channel: no squeeze
    (grey,) = _write_frames(tmp_path / "grey", 1, 9, 8, 1, 8, 3)
    g = png_gpu.decode_batch([grey], dev)
    assert g.shape == (1, 9, 8, 1) and np.array_equal(g[0, :, :, 0].cpu().numpy(), flow_io.read_png(grey))


@pytest.mark.parametrize("fmt", [(1, 8), (4, 8), (2, 8), (3, 16)], ids=lambda f: f"c{f[0]}d{f[1]}")
def test_frame_dir_gpu_decode_through_predict_video(dev, tmp_path, fmt):
    """Grey and RGBA files (and grey + alpha, 16-bit RGB): FrameDir(decode="gpu") through predict_video with a stub model gives
    flows bitwise equal to FrameDir(decode="host"): grey becomes three channels and alpha is dropped as datasets.read_frame does."""
    from streamflow_amd import datasets, png_gpu, video
    c, depth = fmt
    paths = _write_frames(tmp_path / "frames", 7, 36, 50, c, depth, 11 * c + depth)
    host, gpu = video.FrameDir(str(tmp_path / "frames")), video.FrameDir(str(tmp_path / "frames"), decode="gpu")
    batch = gpu.device_batch(2, 6, dev)
    assert batch.dtype == torch.uint8 and batch.shape == (4, 36, 50, 3)
    assert np.array_equal(batch.cpu().numpy(), np.stack([datasets.read_frame(p) for p in paths[2:6]]))
    assert np.array_equal(gpu[3], host[3])
    want = video.predict_video(vc.stub_model, host, T=3, clips_per_step=2, device=dev)
    got = video.predict_video(vc.stub_model, gpu, T=3, clips_per_step=2, device=dev)
    assert got.shape == (6, 2, 36, 50) and torch.equal(got, want)
    # a directory that mixes formats: still read_frame's bytes
    pc.encode(pc.image(36, 50, 3, 8, 99), pc.filter_types("mixed", 36, 99), paths[4], 8)
    assert np.array_equal(png_gpu.decode_frames(paths, dev).cpu().numpy(), np.stack([datasets.read_frame(p) for p in paths]))


# ---- dataset loops --------------------------------------------------------------------------------------------------------------
class _Stub:
    """vc.stub_model behind both call conventions (as tests/test_gpu_evaluate_batched.py's)."""
    def __call__(self, images, iters=None, test_mode=False):
        if isinstance(images, (list, tuple)):
            images = vc.normalise(torch.stack(list(images), dim=1))
        return vc.stub_model(images)


def _record_rows(monkeypatch):
    """Every accumulator ops.flow_score_batch is given, in call order (the tensors are read after the report)."""
    from streamflow_amd import ops
    seen, real = [], ops.flow_score_batch

    def recording(preds, gts, acc, *a, **kw):
        seen.append(acc)
        return real(preds, gts, acc, *a, **kw)

    monkeypatch.setattr(ops, "flow_score_batch", recording)
    return seen


def test_sintel_report_gpu_decode_equals_host_decode(dev, tmp_path, monkeypatch):
    """The stub Sintel tree of the batched tests (two scenes of 5 and 9 frames, 44 x 60) with frames written by png_cases.encode
    with mixed filters: png_decode="gpu" returns exactly the report of png_decode="host", every accumulator row equal."""
    from streamflow_amd import evaluate, flow_io
    rng = np.random.default_rng(11)
    H, W = 44, 60
    for s, (scene, n) in enumerate((("alley_1", 5), ("market_2", 9))):
        frames = vc.random_frames(20 + s, n, H, W).numpy()
        for dstype in ("clean", "final"):
            os.makedirs(tmp_path / "training" / dstype / scene)
            for i in range(n):
                pc.encode(frames[i], pc.filter_types("mixed", H, 31 * s + i), str(tmp_path / "training" / dstype / scene / f"frame_{i + 1:04d}.png"))
        os.makedirs(tmp_path / "training" / "flow" / scene)
        for i in range(n - 1):
            flow_io.write_flo(str(tmp_path / "training" / "flow" / scene / f"frame_{i + 1:04d}.flo"),
                              rng.normal(0, 2, size=(H, W, 2)).astype(np.float32))
    seen = _record_rows(monkeypatch)
    reports, rows = {}, {}
    for mode in ("host", "gpu"):
        del seen[:]
        reports[mode] = evaluate.sintel_report(_Stub(), iters=3, root=str(tmp_path), nframes=4, device=dev, clips_per_step=8,
                                               png_decode=mode)
        rows[mode] = torch.cat([a.cpu() for a in seen])
    assert reports["gpu"] == reports["host"] and reports["gpu"]["clean"]["pairs"] == 12
    assert rows["gpu"].shape == rows["host"].shape == (2 * 12, rows["gpu"].shape[1]) and torch.equal(rows["gpu"], rows["host"])
    assert evaluate.validate_sintel_mf(_Stub(), iters=3, root=str(tmp_path), nframes=4, device=dev, clips_per_step=8,
                                       png_decode="gpu") == {k: v["epe"] for k, v in reports["host"].items()}
    with pytest.raises(ValueError, match="png_decode"):
        evaluate.sintel_report(_Stub(), root=str(tmp_path), nframes=4, device=dev, clips_per_step=8, png_decode="device")


def test_kitti_batched_gpu_decode_equals_host_decode(dev, tmp_path, monkeypatch):
    """Four sequences, two of 42 x 60 and two of 42 x 52 (a size change flushes the batch), frames and 16-bit flow_occ files written
    with mixed filters: the batched validate_kitti_mf with png_decode="gpu" returns exactly what png_decode="host" returns."""
    from streamflow_amd import evaluate, flow_io
    rng = np.random.default_rng(4)
    H, T = 42, 3
    os.makedirs(tmp_path / "training" / "image_2")
    os.makedirs(tmp_path / "training" / "flow_occ")
    for s, W in enumerate((60, 60, 52, 52)):
        frames = vc.random_frames(50 + s, T, H, W).numpy()
        for k, i in enumerate(range(12 - T, 12)):
            pc.encode(frames[k], pc.filter_types("mixed", H, 7 * s + k), str(tmp_path / "training" / "image_2" / ("%06d_%02d.png" % (s, i))))
        enc = flow_io.kitti_encode(rng.normal(0, 1.5, size=(H, W, 2)).astype(np.float32))
        enc[..., 2] = rng.random((H, W)) < 0.4
        pc.encode(enc, pc.filter_types("mixed", H, 90 + s), str(tmp_path / "training" / "flow_occ" / ("%06d_10.png" % s)), 16)
    seen = _record_rows(monkeypatch)
    results, rows = {}, {}
    for mode in ("host", "gpu"):
        del seen[:]
        results[mode] = evaluate.validate_kitti_mf(_Stub(), iters=3, multi_root=str(tmp_path), nframes=T, device=dev, clips_per_step=8,
                                                   png_decode=mode)
        rows[mode] = torch.cat([a.cpu() for a in seen])
    assert results["gpu"] == results["host"] and set(results["gpu"]) == {"kitti_epe", "kitti_f1"}
    assert rows["gpu"].shape[0] == 4 and torch.equal(rows["gpu"], rows["host"])
    assert 0 < results["gpu"]["kitti_f1"] < 100
