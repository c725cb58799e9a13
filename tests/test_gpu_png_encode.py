"""PNG encoding on the GPU: sf_png_encode and sf_flow_to_kitti16 (csrc/png_encode.hip) through the C ABI, ops.png_encode,
png_gpu.encode_batch and the writers with png_encode="gpu", against tests/png_encode_cases.py's encode_ref (pinned to zlib,
flow_io.read_png and PIL by tests/test_png_encode_cases_cpu.py).

Criterion: every comparison is BITWISE -- the format is integer arithmetic, so there is no tolerance to choose.  Stream lengths and
stream bytes must equal encode_ref's; output slots are prefilled with 0xA5 between guard bands, the bytes behind a stream up to
sf_png_encode_bound are unspecified, everything behind the bound and between slots must come back intact.  Shapes: band edges
(h = 1, 31, 32, 33, 65 for SF_PNG_ENC_BAND_ROWS = 32) against row lengths around a wave (64), a workgroup pass (256, 1024) and odd
ones, every bpp, swap16, the single-symbol block, the length-limit case and noise (tests/png_encode_cases.CASES)."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import png_encode_cases as ec
from tests.guarded import GuardedBytes

pytestmark = pytest.mark.gpu
FILL = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def lib():
    from streamflow_amd import _lib
    return _lib.load()


def encode(dev, images, swap16, row_gap=0, image_gap=0, slot_gap=0, shift=0):
    """sf_png_encode through the C ABI on memory-byte images uint8 [h, w, bpp] -> (streams, the flat output bytes, slot stride).
    The input rows are row_gap bytes apart, the images image_gap more, the input starts `shift` bytes off the allocation's alignment;
    slots are the bound + slot_gap apart.  Asserts on the way: status, guard bands, input unchanged, nothing written behind the
    bound of a slot."""
    n, (h, w, bpp) = len(images), images[0].shape
    row = w * bpp
    rstride = row + row_gap
    istride = h * rstride + image_gap
    src = GuardedBytes(dev, (n - 1) * istride + (h - 1) * rstride + row, fill=0xEE, shift=shift)
    host = np.full(src.size, 0xEE, np.uint8)
    for i, img in enumerate(images):
        assert img.shape == (h, w, bpp) and img.dtype == np.uint8
        for y in range(h):
            host[i * istride + y * rstride:][:row] = img[y].reshape(-1)
    src.view().copy_(torch.from_numpy(host))
    bound, ws_bytes = lib().sf_png_encode_bound(h, w, bpp), lib().sf_png_encode_ws_bytes(n, h, w, bpp)
    assert bound == ec.bound(h, w, bpp) and ws_bytes > 0
    ostride = bound + slot_gap
    out = GuardedBytes(dev, (n - 1) * ostride + bound, fill=FILL)
    ws = GuardedBytes(dev, ws_bytes, fill=0x3C, shift=shift)
    lengths = torch.full((n + 2,), -7, dtype=torch.int64, device=dev)
    status = lib().sf_png_encode(src.ptr, istride, rstride, n, h, w, bpp, 1 if swap16 else 0, out.ptr, ostride, lengths[1:].data_ptr(),
                                 ws.ptr, ws_bytes, torch.cuda.current_stream().cuda_stream)
    assert status == 0, lib().sf_last_error()
    torch.cuda.synchronize()
    assert src.guards_unchanged() and out.guards_unchanged() and ws.guards_unchanged()
    assert np.array_equal(src.view().cpu().numpy(), host)
    got = lengths.cpu().numpy()
    assert got[0] == -7 and got[-1] == -7
    flat = out.view().cpu().numpy()
    streams = []
    for i in range(n):
        assert 6 < got[1 + i] <= bound, got
        streams.append(flat[i * ostride:i * ostride + got[1 + i]].tobytes())
        assert (flat[i * ostride + bound:(i + 1) * ostride] == FILL).all(), "bytes between the slots were written"
    return streams, flat, ostride


def check(dev, images, swap16, **kw):
    streams, _, _ = encode(dev, images, swap16, **kw)
    for i, (img, got) in enumerate(zip(images, streams)):
        want = ec.encode_ref(img, bool(swap16))
        assert len(got) == len(want), (i, len(got), len(want))
        if got != want:
            a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
            first = int(np.argmax(a != b))
            raise AssertionError(f"image {i}: {int((a != b).sum())} of {len(want)} bytes differ, first at {first}: {a[first]:#x} != {b[first]:#x}")
    return streams


@pytest.mark.parametrize("case", ec.CASES, ids=ec.case_id)
def test_stream_equals_the_reference(dev, case):
    kind, h, w, bpp, swap16, seed = case
    check(dev, [ec.make(kind, h, w, bpp, seed)], swap16)


def test_batch_of_three_with_strides_larger_than_dense(dev):
    """Three different images (smooth, noise, zeros) in one call, dense and with gaps between rows, images and slots, the input off
    the allocation's alignment; and the same call twice gives the same bytes."""
    h, w, bpp = 37, 45, 3
    images = [ec.make("smooth", h, w, bpp, 31), ec.make("noise", h, w, bpp, 32), ec.make("zeros", h, w, bpp, 33)]
    dense = check(dev, images, 0)
    gaps = check(dev, images, 0, row_gap=5, image_gap=11, slot_gap=12, shift=3)
    assert dense == gaps
    images16 = [ec.make("smooth", 33, 20, 6, 34), ec.make("noise", 33, 20, 6, 35), ec.make("smooth", 33, 20, 6, 36)]
    first = check(dev, images16, 1, row_gap=2, image_gap=6, slot_gap=4)
    again = check(dev, images16, 1, row_gap=2, image_gap=6, slot_gap=4)
    assert first == again


def test_refusals_write_nothing(dev):
    """Every refusal of the header's list returns its code before any launch: the output, the lengths and the workspace keep their
    fill."""
    h, w, bpp, n = 5, 7, 4, 2
    bound, ws_bytes = lib().sf_png_encode_bound(h, w, bpp), lib().sf_png_encode_ws_bytes(n, h, w, bpp)
    src = torch.zeros(n * h * w * bpp, dtype=torch.uint8, device=dev)
    out = GuardedBytes(dev, n * bound, fill=FILL)
    ws = GuardedBytes(dev, ws_bytes, fill=0x3C)
    lengths = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    row, image = w * bpp, h * w * bpp
    good = dict(img=src.data_ptr(), istride=image, rstride=row, n=n, h=h, w=w, bpp=bpp, swap16=0, out=out.ptr, ostride=bound,
                lengths=lengths.data_ptr(), ws=ws.ptr, ws_bytes=ws_bytes)
    big = ec.header_constant("SF_PNG_MAX_ROW_BYTES")
    bad = [(-1, dict(img=None)), (-1, dict(out=None)), (-1, dict(lengths=None)), (-1, dict(ws=None)), (-1, dict(n=0)), (-1, dict(n=65536)),
           (-1, dict(h=0)), (-1, dict(w=0)), (-1, dict(bpp=5)), (-1, dict(bpp=7)), (-1, dict(bpp=3, swap16=1)),
           (-1, dict(rstride=row - 1)), (-1, dict(istride=image - 1)), (-1, dict(ostride=bound - 4)), (-1, dict(ws_bytes=ws_bytes - 1)),
           (-1, dict(lengths=lengths.data_ptr() + 4)), (-1, dict(out=out.ptr + 2)), (-1, dict(ostride=bound + 2)),
           (-1, dict(h=1 << 20, w=1 << 9, ostride=1 << 40, ws_bytes=1 << 40)),                 # h (1 + w bpp) >= 2^31
           (-2, dict(h=1, w=big // 4 + 1, rstride=big + 4, istride=big + 4, ostride=1 << 30, ws_bytes=1 << 30))]
    for code, change in bad:
        a = dict(good, **change)
        status = lib().sf_png_encode(a["img"], a["istride"], a["rstride"], a["n"], a["h"], a["w"], a["bpp"], a["swap16"], a["out"],
                                     a["ostride"], a["lengths"], a["ws"], a["ws_bytes"], torch.cuda.current_stream().cuda_stream)
        assert status == code, (change, status, lib().sf_last_error())
    torch.cuda.synchronize()
    assert (out.view() == FILL).all() and (ws.view() == 0x3C).all() and (lengths == -7).all()
    assert out.guards_unchanged() and ws.guards_unchanged()
    assert lib().sf_png_encode_bound(0, 1, 1) == -1 and lib().sf_png_encode_bound(1, 1, 5) == -1
    assert lib().sf_png_encode_ws_bytes(0, 1, 1, 1) == -1 and lib().sf_png_encode_ws_bytes(1, 1 << 20, 1 << 9, 4) == -1
    flow = torch.zeros(2 * 4 * 4, device=dev)
    codes = torch.full((4 * 4 * 3,), 7, dtype=torch.int16, device=dev)
    for args in ((None, codes.data_ptr(), 1, 4, 4), (flow.data_ptr(), None, 1, 4, 4), (flow.data_ptr(), codes.data_ptr(), 0, 4, 4),
                 (flow.data_ptr(), codes.data_ptr(), 1, 0, 4), (flow.data_ptr(), codes.data_ptr(), 1, 1 << 15, 1 << 15),
                 (flow.data_ptr(), codes.data_ptr() + 1, 1, 4, 4)):
        assert lib().sf_flow_to_kitti16(*args, torch.cuda.current_stream().cuda_stream) == -1, args
    torch.cuda.synchronize()
    assert (codes == 7).all()


def test_flow_to_kitti16_equals_kitti_encode(dev):
    from streamflow_amd import flow_io, ops
    rng = np.random.default_rng(12)
    n, h, w = 3, 37, 301                                                     # more than one workgroup per field, an odd tail
    flows = (rng.standard_normal((n, 2, h, w)) * 80).astype(np.float32)
    flows[0, 0, 0, :6] = [0.0, -0.0, 511.98, -511.99, 1e-3, -1e-3]
    flows[1, :, 1, :3] = rng.standard_normal((2, 3)).astype(np.float32) * 1e-5          # products that round in the sum
    got = ops.flow_to_kitti16(torch.from_numpy(flows).to(dev))
    assert got.dtype == torch.uint16 and tuple(got.shape) == (n, h, w, 3)
    got = got.cpu().numpy()
    for i in range(n):
        assert np.array_equal(got[i], flow_io.kitti_encode(flows[i].transpose(1, 2, 0))), i
    edge = np.zeros((1, 2, 1, 6), np.float32)
    edge[0, 0, 0] = [np.nan, -600.0, 600.0, np.inf, -np.inf, 511.99]
    got = ops.flow_to_kitti16(torch.from_numpy(edge).to(dev)).cpu().numpy()
    assert np.array_equal(got[0], ec.kitti16_ref(edge[0])) and got[0, 0, :, 0].tolist() == [0, 0, 65535, 65535, 0, 65535]


def test_ops_png_encode_on_views(dev):
    """ops.png_encode: uint8 and uint16 tensors, a batch that is a strided view (a crop of a larger tensor)."""
    from streamflow_amd import ops
    rng = np.random.default_rng(13)
    big = torch.from_numpy(rng.integers(0, 256, size=(2, 40, 50, 3), dtype=np.uint8)).to(dev)
    view = big[:, 3:38, 4:47]
    streams, lengths = ops.png_encode(view)
    assert streams.dtype == torch.uint8 and lengths.dtype == torch.int64 and tuple(streams.shape) == (2, ec.bound(35, 43, 3))
    for i in range(2):
        assert streams[i, :int(lengths[i])].cpu().numpy().tobytes() == ec.encode_ref(view[i].cpu().numpy())
    codes = torch.from_numpy(rng.integers(0, 65536, size=(1, 33, 21, 3)).astype(np.uint16)).to(dev)
    streams, lengths = ops.png_encode(codes)
    assert streams[0, :int(lengths[0])].cpu().numpy().tobytes() == ec.encode_ref(codes[0].cpu().numpy())
    with pytest.raises(RuntimeError):
        ops.png_encode(big.cpu())
    with pytest.raises(RuntimeError):
        ops.png_encode(big.permute(0, 2, 1, 3))


def test_encode_batch_files_read_back(dev, tmp_path):
    from streamflow_amd import flow_io, ops, png_gpu
    f = torch.from_numpy(np.stack([ec.smooth_field(70, 90, s) for s in (1, 2, 3)])).to(dev)
    images = ops.flow_to_image(f)
    paths = [str(tmp_path / f"c{i}.png") for i in range(3)]
    sizes = png_gpu.encode_batch(images, paths, threads=2)
    for i, p in enumerate(paths):
        assert os.path.getsize(p) == sizes[i]
        assert np.array_equal(flow_io.read_png(p), images[i].cpu().numpy())
    codes = ops.flow_to_kitti16(f)
    paths = [str(tmp_path / f"k{i}.png") for i in range(3)]
    png_gpu.encode_batch(codes, paths)
    for i, p in enumerate(paths):
        got = flow_io.read_png(p)
        assert got.dtype == np.uint16 and np.array_equal(got, codes[i].cpu().numpy())
    grey = images[:1, :, :, :1].contiguous()
    png_gpu.encode_batch(grey, [str(tmp_path / "g.png")])
    assert np.array_equal(flow_io.read_png(str(tmp_path / "g.png")), grey[0, :, :, 0].cpu().numpy())
    with pytest.raises(ValueError):
        png_gpu.encode_batch(images, paths[:2])
    with pytest.raises(RuntimeError):
        png_gpu.encode_batch(images.cpu(), paths)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_writers_give_the_host_runs_pixels(dev, tmp_path):
    """vis_flow, the Sintel clip writer and create_kitti_submission_mf with png_encode="gpu" on a 64x96 clip: the same file names, and
    every file decodes to the pixels of the png_encode="host" run (the file bytes differ: other filters, other deflate).  The model
    is a stub (a smooth field from the frames' means): the test is about the writers."""
    from streamflow_amd import demo, flow_io, submit
    H, W, T = 64, 96, 3
    rng = np.random.default_rng(14)
    os.makedirs(tmp_path / "testing" / "image_2")
    for i in range(12 - T, 12):
        flow_io.write_png(str(tmp_path / "testing" / "image_2" / ("000000_%02d.png" % i)), rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8))

    def model(images, iters, test_mode):
        h, w = images[0].shape[-2:]
        y, x = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
        return [torch.stack([(k + 2) * torch.sin(x / 17 + im.mean() / 255), (k + 1) * 1.5 * torch.cos(y / 13) - x / 40])[None]
                for k, im in enumerate(images[:-1])]

    runs = {}
    for mode in ("host", "gpu"):
        out, vis = tmp_path / mode / "out", tmp_path / mode / "vis"
        submit.create_kitti_submission_mf(Namespace(multi_root=str(tmp_path)), model, 1, output_path=str(out), nframes=T, vis_path=str(vis),
                                          device=dev, png_encode=mode)
        fields = [f[0] for f in model([torch.zeros(1, 3, H, W, device=dev)] * T, 1, True)]
        paths = demo.vis_flow(fields, str(tmp_path / mode / "seq"), png_encode=mode)
        assert [os.path.basename(p) for p in paths] == ["frame_0000.png", "frame_0001.png"]
        submit._write_sintel_clip(fields, [4, 5, 6], str(tmp_path / mode / "sintel"), "clean", "alley_9", True, png_encode=mode)
        runs[mode] = {p: flow_io.read_png(str(tmp_path / mode / p)) for p in _files(tmp_path / mode) if p.endswith(".png")}
        runs[mode + "_bytes"] = {p: open(str(tmp_path / mode / p), "rb").read() for p in _files(tmp_path / mode)}
    assert sorted(runs["host"]) == sorted(runs["gpu"]) and len(runs["host"]) == 6
    assert sorted(runs["host_bytes"]) == sorted(runs["gpu_bytes"])
    for p, want in runs["host"].items():
        assert runs["gpu"][p].dtype == want.dtype and np.array_equal(runs["gpu"][p], want), p
        assert runs["gpu_bytes"][p] != runs["host_bytes"][p], p
    for p in runs["host_bytes"]:
        if p.endswith(".flo"):
            assert runs["gpu_bytes"][p] == runs["host_bytes"][p], p
    assert runs["host"]["out/000000_10.png"].dtype == np.uint16
    with pytest.raises(ValueError):
        demo.vis_flow(fields, str(tmp_path / "bad"), png_encode="device")
