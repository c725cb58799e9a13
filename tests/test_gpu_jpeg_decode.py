"""JPEG decoding on the GPU: sf_jpeg_decode (csrc/jpeg_decode.hip) through the C ABI, ops.jpeg_decode, jpeg_gpu.decode_batch,
avi.MjpegReader and video.JpegDir under predict_video, against tests/jpeg_decode_cases.py's decode_ref (pinned to PIL's
libjpeg-turbo and to the recorded pixels by tests/test_jpeg_decode_cases_cpu.py).

Criterion: every comparison is BITWISE -- the format is integer arithmetic, so there is no tolerance to choose.  The output sits
between guard bands, prefilled with 0xA5, with gaps between rows and images that must keep the fill; the workspace and the status
words sit between guard bands too.  Shapes (tests/jpeg_decode_cases.NAMES, files of a few hundred bytes): h and w in 1, 7, 8, 9, 16, 17,
33 and the widths 3 and 4 where libjpeg replicates chroma samples, 4:4:4 / 4:2:2 / 4:2:0 / grey, typical and optimised Huffman
tables, restart intervals of 1 and 3 MCUs and of an MCU row, ten intervals (the RST counter wraps), one interval of 342 MCUs,
quality 1 and quality 100 on noise / checker / block images (16-bit codes, clamping, stuffed FF bytes), files of the project's own
encoder (ZRL runs, no EOB), a frame without DHT and one with FF fill bytes.  Malformed streams go to the device only after the
sanitized host program (csrc/host/jpeg_decode_host_main.cpp, the same decoder core) has run the same call clean."""
import numpy as np
import pytest
import torch

from tests import jpeg_decode_cases as dc
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


def decode(dev, call, out_channels=3, row_gap=0, image_gap=0, shift=0):
    """sf_jpeg_decode through the C ABI -> (pixels uint8 [n, h, w, out_channels], status int32 [n]).  Rows are row_gap bytes apart,
    images image_gap more; the data starts `shift` bytes off its allocation's alignment.  Asserts on the way: the return code, the
    guard bands of out, ws and status, the inputs unchanged, the gaps of the output untouched."""
    n, h, w = call.n, call.h, call.w
    row = w * out_channels
    rstride = row + row_gap
    istride = h * rstride + image_gap
    data = GuardedBytes(dev, max(len(call.data), 1), fill=0xEE, shift=shift)
    data.view()[:len(call.data)].copy_(torch.from_numpy(call.data))
    desc = torch.from_numpy(np.ascontiguousarray(call.desc, np.int64)).to(dev)
    tables = torch.from_numpy(np.ascontiguousarray(call.tables, np.uint8)).to(dev)
    ws_bytes = lib().sf_jpeg_decode_ws_bytes(n, h, w, call.nc, call.hs, call.vs)
    assert ws_bytes > 0
    out = GuardedBytes(dev, (n - 1) * istride + (h - 1) * rstride + row, fill=FILL)
    ws = GuardedBytes(dev, ws_bytes, fill=0x3C)
    status = GuardedBytes(dev, 4 * n, fill=0x77)
    rc = lib().sf_jpeg_decode(data.ptr, len(call.data), desc.data_ptr(), len(call.desc), tables.data_ptr(), len(call.tables), n, h, w,
                              call.nc, call.hs, call.vs, out.ptr, istride, rstride, out_channels, status.ptr, ws.ptr, ws_bytes,
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib().sf_last_error()
    torch.cuda.synchronize()
    assert data.guards_unchanged() and out.guards_unchanged() and ws.guards_unchanged() and status.guards_unchanged()
    assert np.array_equal(data.view()[:len(call.data)].cpu().numpy(), call.data)
    assert np.array_equal(desc.cpu().numpy(), call.desc) and np.array_equal(tables.cpu().numpy(), call.tables)
    flat = out.view().cpu().numpy()
    inside = np.zeros(flat.size, bool)
    pixels = np.empty((n, h, w, out_channels), np.uint8)
    for i in range(n):
        for y in range(h):
            at = i * istride + y * rstride
            pixels[i, y] = flat[at:at + row].reshape(w, out_channels)
            inside[at:at + row] = True
    assert (flat[~inside] == FILL).all(), "bytes between rows or images were written"
    return pixels, status.view().cpu().numpy().view(np.int32).copy()


@pytest.mark.parametrize("name", dc.NAMES)
def test_pixels_equal_the_reference(dev, name):
    pixels, status = decode(dev, dc.Call([name]))
    assert status[0] == 0
    want = dc.decode_ref(dc.load(name))
    if not np.array_equal(pixels[0], want):
        diff = pixels[0].astype(int) - want
        raise AssertionError(f"{name}: {np.count_nonzero(diff)} of {diff.size} samples differ, largest by {np.abs(diff).max()}, first at "
                             f"{tuple(int(v) for v in np.argwhere(diff)[0])}")
    assert np.array_equal(want, dc.expected()[name])


def test_batches_mix_table_sets_and_restart_layouts_with_padded_strides(dev):
    """Three files of one geometry in one call -- no DRI, DRI 1 and DRI 3 with optimised tables: 13 intervals, two table sets --
    dense and with gaps between rows and images and the data off its alignment; the same call twice gives the same bytes.  And a
    batch in which every file has its own restart layout in rows (444, 73 x 9) next to one without."""
    call = dc.Call(dc.MUTATED)
    want = np.stack([dc.decode_ref(dc.load(n)) for n in dc.MUTATED])
    dense, status = decode(dev, call)
    assert not status.any() and np.array_equal(dense, want)
    gaps, status = decode(dev, call, row_gap=5, image_gap=11, shift=3)
    again, _ = decode(dev, call, row_gap=5, image_gap=11, shift=3)
    assert not status.any() and np.array_equal(gaps, want) and np.array_equal(again, want)
    for names in (("444-16x17", "444-16x17-nodht", "444-16x17-q100-noise"), ("420-33x33-rst3", "420-33x33-rst3-fill", "420-33x33-rst1"),
                  ("grey-16x24-q100-noise", "grey-16x24-q100-checker")):
        pixels, status = decode(dev, dc.Call(names), row_gap=1, image_gap=2)
        assert not status.any()
        for i, n in enumerate(names):
            assert np.array_equal(pixels[i], dc.decode_ref(dc.load(n))), n


def test_grey_files_with_one_and_three_output_channels(dev):
    for name in ("grey-33x33", "grey-1x1", "grey-33x17-rst1", "own-basis77-only63-8x8-grey"):
        want = dc.decode_ref(dc.load(name))
        one, status = decode(dev, dc.Call([name]), out_channels=1, row_gap=3)
        three, _ = decode(dev, dc.Call([name]), out_channels=3)
        assert status[0] == 0 and np.array_equal(one[0, :, :, 0], want[:, :, 0]) and np.array_equal(three[0], want)
        assert np.array_equal(three[0, :, :, 0], three[0, :, :, 1]) and np.array_equal(three[0, :, :, 0], three[0, :, :, 2])


def test_refusals_write_nothing(dev):
    """Every refusal of the header's list returns its code before anything is enqueued: out, status and ws keep their fill."""
    call = dc.Call(dc.MUTATED)
    n, h, w = call.n, call.h, call.w
    data = torch.from_numpy(call.data).to(dev)
    desc = torch.from_numpy(call.desc).to(dev)
    tables = torch.from_numpy(call.tables).to(dev)
    ws_bytes = lib().sf_jpeg_decode_ws_bytes(n, h, w, 3, 2, 2)
    out = GuardedBytes(dev, n * h * w * 3, fill=FILL)
    ws = GuardedBytes(dev, ws_bytes, fill=0x3C)
    status = GuardedBytes(dev, 4 * n, fill=0x77)
    good = dict(data=data.data_ptr(), data_bytes=len(call.data), desc=desc.data_ptr(), n_int=len(call.desc), tables=tables.data_ptr(),
                n_sets=len(call.tables), n=n, h=h, w=w, c=3, hs=2, vs=2, out=out.ptr, istride=h * w * 3, rstride=w * 3, oc=3,
                status=status.ptr, ws=ws.ptr, ws_bytes=ws_bytes)
    top = dc.jc.header_constant("SF_JPEG_MAX_DIM")
    bad = [(-1, dict(data=None)), (-1, dict(desc=None)), (-1, dict(tables=None)), (-1, dict(out=None)), (-1, dict(status=None)),
           (-1, dict(ws=None)), (-1, dict(data_bytes=-1)), (-1, dict(n_int=0)), (-1, dict(n_int=(1 << 26) + 1)), (-1, dict(n_sets=0)),
           (-1, dict(n_sets=65536)), (-1, dict(n=0)), (-1, dict(n=65536)), (-1, dict(h=0)), (-1, dict(w=0)), (-1, dict(c=2)), (-1, dict(c=4)),
           (-1, dict(hs=1, vs=2)), (-1, dict(hs=4, vs=1)), (-1, dict(hs=2, vs=4)), (-1, dict(hs=0, vs=1)), (-1, dict(c=1, hs=2, vs=2)),
           (-1, dict(oc=2)), (-1, dict(oc=1)), (-1, dict(oc=0)), (-1, dict(rstride=w * 3 - 1)), (-1, dict(istride=h * w * 3 - 1)),
           (-1, dict(desc=desc.data_ptr() + 4)), (-1, dict(status=status.ptr + 2)), (-1, dict(ws=ws.ptr + 8, ws_bytes=ws_bytes - 8)),
           (-1, dict(ws_bytes=ws_bytes - 1)),
           (-2, dict(h=1, w=top + 1, rstride=3 * (top + 1), istride=3 * (top + 1), ws_bytes=1 << 30)),
           (-2, dict(h=top + 1, w=1, rstride=3, istride=3 * (top + 1), ws_bytes=1 << 30))]
    for code, change in bad:
        a = dict(good, **change)
        rc = lib().sf_jpeg_decode(a["data"], a["data_bytes"], a["desc"], a["n_int"], a["tables"], a["n_sets"], a["n"], a["h"], a["w"], a["c"],
                                  a["hs"], a["vs"], a["out"], a["istride"], a["rstride"], a["oc"], a["status"], a["ws"], a["ws_bytes"],
                                  torch.cuda.current_stream().cuda_stream)
        assert rc == code, (change, rc, lib().sf_last_error())
    torch.cuda.synchronize()
    assert (out.view() == FILL).all() and (ws.view() == 0x3C).all() and (status.view() == 0x77).all()
    assert out.guards_unchanged() and ws.guards_unchanged() and status.guards_unchanged()
    assert lib().sf_jpeg_decode_ws_bytes(0, 8, 8, 3, 1, 1) == -1 and lib().sf_jpeg_decode_ws_bytes(1, 8, top + 1, 3, 1, 1) == -1
    assert lib().sf_jpeg_decode_ws_bytes(1, 8, 8, 1, 2, 1) == -1 and lib().sf_jpeg_decode_ws_bytes(1, 8, 8, 3, 1, 2) == -1
    assert lib().sf_jpeg_decode_ws_bytes(24, 436, 1024, 3, 2, 2) > 24 * 436 * 1024 * 3


def test_malformed_streams_fail_alone(dev, tmp_path):
    """The deterministic mutations of jpeg_decode_cases.mutations(): each call first runs clean through the sanitized host program;
    then on the device the statuses equal the host's, the undamaged images of the batch are bitwise right and every guard band is
    intact (decode() asserts that)."""
    muts = dc.mutations()
    exe = dc.host_program(tmp_path)
    host = dc.run_host(exe, [c for _, c in muts], tmp_path, "mutations")       # asserts a clean exit without a sanitizer report
    want = [dc.decode_ref(dc.load(n)) for n in dc.MUTATED]
    failed = 0
    for (label, call), (hstatus, _, _) in zip(muts, host):
        pixels, status = decode(dev, call, row_gap=2, image_gap=7)
        assert np.array_equal(status, hstatus), (label, status, hstatus)
        for i in np.flatnonzero(status == 0):
            if i != 1:                                                      # image 1 is the damaged one: a flipped bit may still decode
                assert np.array_equal(pixels[i], want[i]), (label, i)
        assert status[0] == 0 or label == "image-negative"
        failed += int(status[1] != 0)
    assert failed >= len(muts) - 8                                          # only a flipped bit may go unnoticed


def test_ops_decode_batch_and_the_round_trip(dev, tmp_path):
    """ops.jpeg_decode on a packed batch; jpeg_gpu.decode_batch on bytes and on paths; encode_batch then decode_batch gives
    decode_ref of the same bytes; files of another geometry, broken files and files the device refuses raise ValueError by name."""
    from streamflow_amd import jpeg_gpu, ops
    call = dc.Call(dc.MUTATED)
    want = np.stack([dc.decode_ref(dc.load(n)) for n in dc.MUTATED])
    out, status = ops.jpeg_decode(torch.from_numpy(call.data).to(dev), torch.from_numpy(call.desc).to(dev), torch.from_numpy(call.tables).to(dev),
                                  3, 33, 33, 3, 2, 2)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (3, 33, 33, 3) and status.dtype == torch.int32 and not status.any()
    assert np.array_equal(out.cpu().numpy(), want)
    with pytest.raises(RuntimeError):
        ops.jpeg_decode(torch.from_numpy(call.data), torch.from_numpy(call.desc).to(dev), torch.from_numpy(call.tables).to(dev), 3, 33, 33, 3, 2, 2)
    with pytest.raises(RuntimeError):
        ops.jpeg_decode(torch.from_numpy(call.data).to(dev), torch.from_numpy(call.desc).to(dev), torch.from_numpy(call.tables).to(dev), 3, 33, 33, 3, 1, 2)
    blobs = [dc.load(n) for n in dc.MUTATED]
    got = jpeg_gpu.decode_batch(blobs, dev, threads=2)
    assert got.device == dev and np.array_equal(got.cpu().numpy(), want)
    paths = []
    for n, b in zip(dc.MUTATED, blobs):
        paths.append(str(tmp_path / (n + ".jpg")))
        with open(paths[-1], "wb") as f:
            f.write(b)
    assert np.array_equal(jpeg_gpu.decode_batch(paths, dev).cpu().numpy(), want)
    grey = jpeg_gpu.decode_batch([dc.load("grey-33x33")], dev)
    assert tuple(grey.shape) == (1, 33, 33, 3) and np.array_equal(grey[0].cpu().numpy(), dc.decode_ref(dc.load("grey-33x33")))
    # round trip through the project's own encoder: 64 x 96 wheels, an interval per MCU row
    images = torch.from_numpy(np.stack([dc.jc.make("wheel", 64, 96, 3, s) for s in (1, 2, 3)])).to(dev)
    files = jpeg_gpu.encode_batch(images, quality=90)
    back = jpeg_gpu.decode_batch(files, dev).cpu().numpy()
    for i, blob in enumerate(files):
        assert np.array_equal(back[i], dc.decode_ref(blob)), i
    assert dc.jc.psnr(back, images.cpu().numpy()) > 35
    with pytest.raises(ValueError, match="image 1"):
        jpeg_gpu.decode_batch([blobs[0], dc.load("444-16x17")], dev)
    with pytest.raises(jpeg_gpu.UnsupportedJpeg, match="refuse-progressive"):
        jpeg_gpu.decode_batch([blobs[0], dc.load("refuse-progressive")], dev, names=["a", "refuse-progressive"])
    off, length = jpeg_gpu.parse(blobs[1]).intervals[3][:2]                 # the framing stays whole: interval 3 becomes zero bits, which
    broken = blobs[1][:off] + bytes(length) + blobs[1][off + length:]       # the host program has refused (mutation "all-zero-bits")
    with pytest.raises(ValueError, match="the broken one.*status") as e:
        jpeg_gpu.decode_batch([blobs[1], broken], dev, names=["good", "the broken one"])
    assert not isinstance(e.value, jpeg_gpu.UnsupportedJpeg)


def test_predict_video_reads_an_mjpeg_file_and_a_jpeg_directory(dev, tmp_path):
    """Five 132 x 196 wheels encoded on the GPU and written as an AVI and as a directory of .jpg files: predict_video on the
    MjpegReader and on the JpegDir (two clips per model call: the batches' frame ranges overlap) equals predict_video on the stacked
    decoded tensor bit for bit; indexing a source gives the decoded host frame.  The tiny synthetic-weight model of the video tests."""
    from streamflow_amd import avi, jpeg_gpu, synthetic as syn, video
    from streamflow_amd.model import SKFlow_MF8, default_args
    H, W, T, n, iters = 132, 196, 3, 5, 3
    images = torch.from_numpy(np.stack([dc.jc.make("wheel", H, W, 3, 10 + s) for s in range(n)])).to(dev)
    (tmp_path / "frames").mkdir()
    files = jpeg_gpu.encode_batch(images, [str(tmp_path / "frames" / f"{i:04d}.jpg") for i in range(n)], quality=85)
    with avi.MjpegWriter(str(tmp_path / "in.avi"), W, H, 25) as v:
        for blob in files:
            v.add(blob)
    stacked = jpeg_gpu.decode_batch(files, dev)
    assert tuple(stacked.shape) == (n, H, W, 3) and np.array_equal(stacked[2].cpu().numpy(), dc.decode_ref(files[2]))
    model = SKFlow_MF8(default_args(T=T, Encoder="PatchEncoder")).to(dev)
    model.load_state_dict(dict(syn.make_params(41, T)), strict=True)
    want = video.predict_video(model, stacked, T=T, iters=iters, clips_per_step=2)
    assert want.shape == (n - 1, 2, H, W) and torch.isfinite(want).all()
    reader = video.open_frames(str(tmp_path / "in.avi"))
    assert isinstance(reader, avi.MjpegReader) and (len(reader), reader.hw, reader.fps) == (n, (H, W), 25.0)
    assert torch.equal(video.predict_video(model, reader, T=T, iters=iters, clips_per_step=2), want)
    frames = video.open_frames(str(tmp_path / "frames"))
    assert isinstance(frames, video.JpegDir)
    assert torch.equal(video.predict_video(model, frames, T=T, iters=iters, clips_per_step=2), want)
    assert np.array_equal(reader[3], stacked[3].cpu().numpy()) and np.array_equal(frames[-1], stacked[n - 1].cpu().numpy())
    reader.close()
