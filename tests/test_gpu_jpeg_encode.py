"""JPEG encoding on the GPU: sf_jpeg_encode (csrc/jpeg_encode.hip) through the C ABI, ops.jpeg_encode, jpeg_gpu.encode_batch and
demo.vis_flow_video, against tests/jpeg_cases.py's encode_ref (pinned to an independent Huffman decoder, a float64 DCT and PIL's
libjpeg by tests/test_jpeg_cases_cpu.py).

Criterion: every comparison is BITWISE -- the format is integer arithmetic, so there is no tolerance to choose.  Segment lengths and
bytes must equal encode_ref's; output slots are prefilled with 0xA5 between guard bands and everything behind a segment, between
slots and in the guard bands of input, output and workspace must come back intact.  Shapes (tests/jpeg_cases.CASES): block edges
(h, w in 1, 7, 8, 9, 17), 10 intervals (the RST counter wraps), 255 / 258 / 1026 blocks per interval (a workgroup pass is 256
blocks-of-a-component, so both channel counts cross a pass boundary), constant images, noise with stuffed bytes, the (7, 7) basis
pattern (62-zero runs, no EOB), checkerboards and black / white blocks (AC category 10, DC difference category 11), colour wheels."""
import numpy as np
import pytest
import torch

from tests import jpeg_cases as jc
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


def encode(dev, images, qtables, row_gap=0, image_gap=0, slot_gap=0, shift=0):
    """sf_jpeg_encode through the C ABI on images uint8 [h, w, 3] / [h, w] -> the segments.  The input rows are row_gap bytes apart,
    the images image_gap more, the input starts `shift` bytes off the allocation's alignment; slots are the bound + slot_gap apart.
    Asserts on the way: status, guard bands, input unchanged, nothing written behind a segment or between the slots."""
    n, (h, w), c = len(images), images[0].shape[:2], 3 if images[0].ndim == 3 else 1
    row = w * c
    rstride = row + row_gap
    istride = h * rstride + image_gap
    src = GuardedBytes(dev, (n - 1) * istride + (h - 1) * rstride + row, fill=0xEE, shift=shift)
    host = np.full(src.size, 0xEE, np.uint8)
    for i, img in enumerate(images):
        assert img.shape[:2] == (h, w) and img.dtype == np.uint8
        for y in range(h):
            host[i * istride + y * rstride:][:row] = img[y].reshape(-1)
    src.view().copy_(torch.from_numpy(host))
    bound, ws_bytes = lib().sf_jpeg_encode_bound(h, w, c), lib().sf_jpeg_encode_ws_bytes(n, h, w, c)
    assert bound == jc.bound(h, w, c) and ws_bytes > 0
    ostride = bound + slot_gap
    out = GuardedBytes(dev, (n - 1) * ostride + bound, fill=FILL)
    ws = GuardedBytes(dev, ws_bytes, fill=0x3C, shift=shift)
    lengths = torch.full((n + 2,), -7, dtype=torch.int64, device=dev)
    q = np.ascontiguousarray(qtables, np.uint16)
    status = lib().sf_jpeg_encode(src.ptr, istride, rstride, n, h, w, c, q.ctypes.data, out.ptr, ostride, lengths[1:].data_ptr(),
                                  ws.ptr, ws_bytes, torch.cuda.current_stream().cuda_stream)
    assert status == 0, lib().sf_last_error()
    torch.cuda.synchronize()
    assert src.guards_unchanged() and out.guards_unchanged() and ws.guards_unchanged()
    assert np.array_equal(src.view().cpu().numpy(), host)
    got = lengths.cpu().numpy()
    assert got[0] == -7 and got[-1] == -7
    flat = out.view().cpu().numpy()
    segments = []
    for i in range(n):
        assert 2 <= got[1 + i] <= bound, got
        segments.append(flat[i * ostride:i * ostride + got[1 + i]].tobytes())
        assert (flat[i * ostride + got[1 + i]:(i + 1) * ostride] == FILL).all(), "bytes behind the segment or between the slots were written"
    return segments


def check(dev, images, qtables, **kw):
    segments = encode(dev, images, qtables, **kw)
    for i, (img, got) in enumerate(zip(images, segments)):
        want = jc.encode_ref(img, qtables)
        assert len(got) == len(want), (i, len(got), len(want))
        if got != want:
            a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
            first = int(np.argmax(a != b))
            raise AssertionError(f"image {i}: {int((a != b).sum())} of {len(want)} bytes differ, first at {first}: {a[first]:#x} != {b[first]:#x}")
    return segments


@pytest.mark.parametrize("case", jc.CASES, ids=jc.case_id)
def test_segment_equals_the_reference(dev, case):
    kind, h, w, c, quality, seed = case
    segments = check(dev, [jc.make(kind, h, w, c, seed)], jc.tables(quality))
    if kind == "noise" and quality == 100:
        assert b"\xff\x00" in segments[0], "the case is there for its stuffed bytes"


def test_batch_of_three_with_strides_larger_than_dense(dev):
    """Three different images (wheel, noise, constant) in one call, dense and with gaps between rows, images and slots, the input off
    the allocation's alignment; and the same call twice gives the same bytes."""
    for c, q in ((3, jc.tables(90)), (1, jc.tables(100))):
        h, w = 37, 45
        images = [jc.make("wheel", h, w, c, 31), jc.make("noise", h, w, c, 32), jc.make("const", h, w, c, 33)]
        dense = check(dev, images, q)
        gaps = check(dev, images, q, row_gap=5, image_gap=11, slot_gap=12, shift=3)
        again = check(dev, images, q, row_gap=5, image_gap=11, slot_gap=12, shift=3)
        assert dense == gaps == again


def test_refusals_write_nothing(dev):
    """Every refusal of the header's list returns its code before any launch: the output, the lengths and the workspace keep their
    fill."""
    h, w, c, n = 5, 7, 3, 2
    bound, ws_bytes = lib().sf_jpeg_encode_bound(h, w, c), lib().sf_jpeg_encode_ws_bytes(n, h, w, c)
    src = torch.zeros(n * h * w * c, dtype=torch.uint8, device=dev)
    out = GuardedBytes(dev, n * bound, fill=FILL)
    ws = GuardedBytes(dev, ws_bytes, fill=0x3C)
    lengths = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    q = np.ascontiguousarray(jc.tables(75), np.uint16)
    zero, big = q.copy(), q.copy()
    zero[1, 63], big[0, 0] = 0, 256
    row, image = w * c, h * w * c
    good = dict(img=src.data_ptr(), istride=image, rstride=row, n=n, h=h, w=w, c=c, q=q.ctypes.data, out=out.ptr, ostride=bound,
                lengths=lengths.data_ptr(), ws=ws.ptr, ws_bytes=ws_bytes)
    top = jc.header_constant("SF_JPEG_MAX_DIM")
    assert top >= 3840
    bad = [(-1, dict(img=None)), (-1, dict(q=None)), (-1, dict(out=None)), (-1, dict(lengths=None)), (-1, dict(ws=None)),
           (-1, dict(n=0)), (-1, dict(n=65536)), (-1, dict(h=0)), (-1, dict(w=0)), (-1, dict(c=2)), (-1, dict(c=4)), (-1, dict(c=0)),
           (-1, dict(q=zero.ctypes.data)), (-1, dict(q=big.ctypes.data)),
           (-1, dict(rstride=row - 1)), (-1, dict(istride=image - 1)), (-1, dict(ostride=bound - 4)), (-1, dict(ws_bytes=ws_bytes - 1)),
           (-1, dict(lengths=lengths.data_ptr() + 4)), (-1, dict(out=out.ptr + 2)), (-1, dict(ostride=bound + 2)),
           (-2, dict(h=1, w=top + 1, c=1, rstride=top + 1, istride=top + 1, ostride=1 << 30, ws_bytes=1 << 30)),
           (-2, dict(h=top + 1, w=1, c=1, rstride=1, istride=top + 1, ostride=1 << 30, ws_bytes=1 << 30))]
    for code, change in bad:
        a = dict(good, **change)
        status = lib().sf_jpeg_encode(a["img"], a["istride"], a["rstride"], a["n"], a["h"], a["w"], a["c"], a["q"], a["out"], a["ostride"],
                                      a["lengths"], a["ws"], a["ws_bytes"], torch.cuda.current_stream().cuda_stream)
        assert status == code, (change, status, lib().sf_last_error())
    torch.cuda.synchronize()
    assert (out.view() == FILL).all() and (ws.view() == 0x3C).all() and (lengths == -7).all()
    assert out.guards_unchanged() and ws.guards_unchanged()
    assert lib().sf_jpeg_encode_bound(0, 1, 1) == -1 and lib().sf_jpeg_encode_bound(1, 1, 2) == -1
    assert lib().sf_jpeg_encode_bound(top + 1, 8, 3) == -1 and lib().sf_jpeg_encode_bound(2160, 3840, 3) == jc.bound(2160, 3840, 3)
    assert lib().sf_jpeg_encode_ws_bytes(0, 1, 1, 1) == -1 and lib().sf_jpeg_encode_ws_bytes(1, 8, top + 1, 3) == -1


def test_ops_jpeg_encode_and_encode_batch(dev, tmp_path):
    """ops.jpeg_encode on a 64 x 96 batch and on a strided view; jpeg_gpu.encode_batch's files are jpeg_file around encode_ref."""
    from streamflow_amd import jpeg_gpu, ops
    host = np.stack([jc.make("wheel", 64, 96, 3, s) for s in (1, 2, 3)])
    images = torch.from_numpy(host).to(dev)
    q = jpeg_gpu.quant_tables(90)
    segments, lengths = ops.jpeg_encode(images, q)
    assert segments.dtype == torch.uint8 and lengths.dtype == torch.int64 and tuple(segments.shape) == (3, jc.bound(64, 96, 3))
    want = [jc.encode_ref(host[i], q) for i in range(3)]
    for i in range(3):
        assert segments[i, :int(lengths[i])].cpu().numpy().tobytes() == want[i]
    view = images[:2, 3:60, 4:91]
    segments, lengths = ops.jpeg_encode(view, q)
    for i in range(2):
        assert segments[i, :int(lengths[i])].cpu().numpy().tobytes() == jc.encode_ref(host[i, 3:60, 4:91], q)
    grey = images[:, :, :, 1].contiguous()
    segments, lengths = ops.jpeg_encode(grey, q)
    assert segments[2, :int(lengths[2])].cpu().numpy().tobytes() == jc.encode_ref(host[2, :, :, 1], q)
    with pytest.raises(RuntimeError):
        ops.jpeg_encode(images.cpu(), q)
    with pytest.raises(RuntimeError):
        ops.jpeg_encode(images.permute(0, 2, 1, 3), q)
    with pytest.raises(RuntimeError):
        ops.jpeg_encode(images, np.zeros((2, 64), np.uint16))
    paths = [str(tmp_path / f"c{i}.jpg") for i in range(3)]
    blobs = jpeg_gpu.encode_batch(images, paths, quality=90, threads=2)
    for i, p in enumerate(paths):
        assert blobs[i] == jpeg_gpu.jpeg_file(want[i], 64, 96, 3, q) and open(p, "rb").read() == blobs[i]
    assert jpeg_gpu.encode_batch(grey[:1], quality=50)[0] == jpeg_gpu.jpeg_file(jc.encode_ref(host[0, :, :, 1], jpeg_gpu.quant_tables(50)), 64, 96, 1,
                                                                                  jpeg_gpu.quant_tables(50))
    with pytest.raises(ValueError):
        jpeg_gpu.encode_batch(images, paths[:2])
    with pytest.raises(ValueError):
        jpeg_gpu.encode_batch(images, quality=0)
    with pytest.raises(RuntimeError):
        jpeg_gpu.encode_batch(images.cpu())


def test_vis_flow_video_frames_are_encode_batch_of_the_colour_images(dev, tmp_path):
    """demo.vis_flow_video on a three-field 64 x 96 clip: the AVI passes the RIFF walker, its frames are jpeg_gpu.encode_batch of
    _colour_batches' images, and (where PIL is there) decode to within the CPU test's margin of libjpeg's own files of those images."""
    from streamflow_amd import demo, jpeg_gpu
    from tests.avi_walk import walk
    H, W = 64, 96
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    fields = [torch.stack([(k + 2) * torch.sin(x / 17 + k), (k + 1) * 1.5 * torch.cos(y / 13) - x / 40]) for k in range(3)]
    path = demo.vis_flow_video(fields, str(tmp_path / "flow.avi"), fps=8, quality=90)
    assert path == str(tmp_path / "flow.avi")
    info = walk(open(path, "rb").read())
    assert (info["width"], info["height"], info["rate"], info["scale"], len(info["frames"])) == (W, H, 8, 1, 3)
    (idx, images), = demo._colour_batches(fields)
    assert idx == [0, 1, 2]
    assert info["frames"] == jpeg_gpu.encode_batch(images, quality=90)
    with pytest.raises(ValueError):
        demo.vis_flow_video(fields + [fields[0][:, :56]], str(tmp_path / "bad.avi"))
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        return
    host, q = images.cpu().numpy(), jpeg_gpu.quant_tables(90)
    for i, blob in enumerate(info["frames"]):
        im = jc.pil_decode(blob)
        assert im.size == (W, H) and im.mode == "RGB"
        ours, theirs = jc.psnr(host[i], np.asarray(im)), jc.psnr(host[i], np.asarray(jc.pil_decode(jc.pil_file(host[i], q))))
        assert ours >= theirs - jc.PSNR_MARGIN_DB, (i, ours, theirs)


def test_command_line_video_of_a_frame_directory(dev, tmp_path):
    """demo.main with --video and no --out over six 124 x 188 PNG frames, one clip per model call (so two batches are appended to one
    writer): the AVI passes the RIFF walker, holds the five pairs' frames in order at 12.5 fps = 25 / 2, they are
    jpeg_gpu.encode_batch of the colour images of what predict_video returns, and (with PIL) each decodes at the frame size."""
    from streamflow_amd import demo, flow_io, jpeg_gpu, synthetic as syn, video
    from streamflow_amd.model import StreamFlowT4
    from tests import video_cases as vc
    from tests.avi_walk import walk
    H, W, n, iters = 124, 188, 6, 3
    frames = vc.random_frames(5, n, H, W).numpy()
    (tmp_path / "frames").mkdir()
    for i, f in enumerate(frames):
        flow_io.write_png(str(tmp_path / "frames" / ("%04d.png" % i)), f)
    sd = dict(syn.make_params(51, 4))
    sd.update({"fnet." + k: v for k, v in syn.make_twins_params(52).items()})
    sd.update({"cnet." + k: v for k, v in syn.make_twins_params(53).items()})
    ckpt = str(tmp_path / "ckpt.pth")
    torch.save({"model": {"module." + k: v for k, v in sd.items()}}, ckpt)
    path = str(tmp_path / "out.avi")
    assert demo.main(["--frames", str(tmp_path / "frames"), "--ckpt", ckpt, "--video", path, "--fps", "12.5", "--jpeg-quality", "80",
                      "--iters", str(iters), "--clips-per-step", "1"]) == 0
    assert sorted(p.name for p in tmp_path.iterdir()) == ["ckpt.pth", "frames", "out.avi"]
    info = walk(open(path, "rb").read())
    assert (info["width"], info["height"], info["rate"], info["scale"], len(info["frames"])) == (W, H, 25, 2, n - 1)
    model = StreamFlowT4(ckpt).to(dev).eval()
    want = video.predict_video(model, video.FrameDir(str(tmp_path / "frames")), T=4, iters=iters, clips_per_step=1)
    (idx, images), = demo._colour_batches(list(want))
    assert info["frames"] == jpeg_gpu.encode_batch(images, quality=80)
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        return
    for blob in info["frames"]:
        im = jc.pil_decode(blob)
        assert im.size == (W, H) and im.mode == "RGB"
