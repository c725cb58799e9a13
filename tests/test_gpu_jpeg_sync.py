"""JPEG decoding on the GPU with long restart intervals split into segments: sf_jpeg_decode_split (csrc/jpeg_decode.hip, the walks of
csrc/jpeg_sync_core.h) through the C ABI, ops.jpeg_decode, jpeg_gpu.decode_batch(split=...) and avi.MjpegReader(split=...) under
predict_video, against tests/jpeg_decode_cases.py's decode_ref and against sf_jpeg_decode itself.

Criterion: every comparison is BITWISE -- the format is integer arithmetic, so there is no tolerance to choose.  The data, the
output, the workspace and the status words sit between guard bands; gaps between rows and images must keep their fill.  Shapes:
the 70 files of tests/golden/jpeg_decode (a few hundred bytes to 1.8 KB) and the four of tests/golden/jpeg_sync (5 to 13 KB, no
DRI), every interval split, at segments of 8, 16 and 128 bytes: one segment and dozens, more segments than two windows of 256 hold
(the window hand-over), the slow synchronisation of quality 100 on noise, symbols and blocks that straddle segments, stuffed FF
bytes at segment ends.  Malformed streams go to the device only after the sanitized host program
(csrc/host/jpeg_sync_host_main.cpp, the same functions) has run the same call clean."""
import numpy as np
import pytest
import torch

from tests import jpeg_decode_cases as dc
from tests import jpeg_sync_cases as sc
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


def decode(dev, call, split=True, out_channels=3, row_gap=0, image_gap=0, shift=0):
    """sf_jpeg_decode_split (split = False: sf_jpeg_decode) through the C ABI -> (pixels uint8 [n, h, w, out_channels], status int32
    [n]).  Asserts on the way: the return code, the guard bands of data, out, ws and status, the inputs unchanged, the gaps of the
    output untouched."""
    n, h, w = call.n, call.h, call.w
    row = w * out_channels
    rstride = row + row_gap
    istride = h * rstride + image_gap
    data = GuardedBytes(dev, max(len(call.data), 1), fill=0xEE, shift=shift)
    data.view()[:len(call.data)].copy_(torch.from_numpy(call.data))
    desc = torch.from_numpy(np.ascontiguousarray(call.desc, np.int64)).to(dev)
    tables = torch.from_numpy(np.ascontiguousarray(call.tables, np.uint8)).to(dev)
    geom = (n, h, w, call.nc, call.hs, call.vs)
    ws_bytes = lib().sf_jpeg_decode_split_ws_bytes(*geom, len(call.data), len(call.desc), call.segment_bytes) if split else \
        lib().sf_jpeg_decode_ws_bytes(*geom)
    assert ws_bytes > 0
    out = GuardedBytes(dev, (n - 1) * istride + (h - 1) * rstride + row, fill=FILL)
    ws = GuardedBytes(dev, ws_bytes, fill=0x3C)
    status = GuardedBytes(dev, 4 * n, fill=0x77)
    head = (data.ptr, len(call.data), desc.data_ptr(), len(call.desc), tables.data_ptr(), len(call.tables), *geom, out.ptr, istride, rstride,
            out_channels, status.ptr)
    tail = (ws.ptr, ws_bytes, torch.cuda.current_stream().cuda_stream)
    rc = lib().sf_jpeg_decode_split(*head, call.segment_bytes, call.split_min_bytes, *tail) if split else lib().sf_jpeg_decode(*head, *tail)
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


@pytest.mark.parametrize("name", sc.NAMES)
def test_every_interval_split_gives_the_reference_pixels(dev, name):
    want = dc.decode_ref(sc.load(name))
    assert np.array_equal(want, sc.expected()[name])
    for S in sc.SEGMENT_BYTES:
        pixels, status = decode(dev, sc.Call([name], S, 0))
        assert status[0] == 0, (S, status)
        if not np.array_equal(pixels[0], want):
            diff = pixels[0].astype(int) - want
            raise AssertionError(f"{name} at {S}-byte segments: {np.count_nonzero(diff)} of {diff.size} samples differ, largest by "
                                 f"{np.abs(diff).max()}, first at {tuple(int(v) for v in np.argwhere(diff)[0])}")


def test_a_batch_mixes_both_routes_and_the_threshold_above_the_data_is_the_wave_route(dev):
    """dc.MUTATED (no DRI, DRI 1, DRI 3) with a threshold between its interval sizes: the long intervals split, the others take the
    wave; with padded strides and the data off its alignment; the same call twice gives the same bytes; split_min_bytes above
    data_bytes is sf_jpeg_decode."""
    want = np.stack([dc.decode_ref(dc.load(n)) for n in dc.MUTATED])
    call = sc.Call(dc.MUTATED, 16, 0)
    sizes = sorted({int(v) for v in call.desc[:, 1]})
    call.split_min_bytes = sizes[len(sizes) // 2]
    assert sizes[0] < call.split_min_bytes <= sizes[-1]
    wave, wstatus = decode(dev, call, split=False)
    assert not wstatus.any() and np.array_equal(wave, want)
    for S in sc.SEGMENT_BYTES:
        call.segment_bytes = S
        dense, status = decode(dev, call)
        assert not status.any() and np.array_equal(dense, want), S
    gaps, status = decode(dev, call, row_gap=5, image_gap=11, shift=3)
    again, _ = decode(dev, call, row_gap=5, image_gap=11, shift=3)
    assert not status.any() and np.array_equal(gaps, want) and np.array_equal(again, want)
    call.split_min_bytes = len(call.data) + 1
    same, status = decode(dev, call, row_gap=1, shift=1)
    assert not status.any() and np.array_equal(same, want)
    everything = sc.Call(dc.MUTATED, 8, 0)
    pixels, status = decode(dev, everything, row_gap=2, image_gap=3, shift=5)
    assert not status.any() and np.array_equal(pixels, want)
    for name in ("grey-33x33", "sync-grey-96x128-q90"):                     # a grey file's one output channel
        one, status = decode(dev, sc.Call([name], 16, 0), out_channels=1, row_gap=3)
        assert status[0] == 0 and np.array_equal(one[0, :, :, 0], dc.decode_ref(sc.load(name))[:, :, 0])


def test_refusals_write_nothing(dev):
    """sf_jpeg_decode's refusals and the three new ones return their code before anything is enqueued."""
    call = sc.Call(dc.MUTATED, 64, 0)
    n, h, w = call.n, call.h, call.w
    data = torch.from_numpy(call.data).to(dev)
    desc = torch.from_numpy(call.desc).to(dev)
    tables = torch.from_numpy(call.tables).to(dev)
    ws_bytes = lib().sf_jpeg_decode_split_ws_bytes(n, h, w, 3, 2, 2, len(call.data), len(call.desc), 64)
    assert ws_bytes > lib().sf_jpeg_decode_ws_bytes(n, h, w, 3, 2, 2) + len(call.data)
    out = GuardedBytes(dev, n * h * w * 3, fill=FILL)
    ws = GuardedBytes(dev, ws_bytes, fill=0x3C)
    status = GuardedBytes(dev, 4 * n, fill=0x77)
    good = dict(data=data.data_ptr(), data_bytes=len(call.data), desc=desc.data_ptr(), n_int=len(call.desc), tables=tables.data_ptr(),
                n_sets=len(call.tables), n=n, h=h, w=w, c=3, hs=2, vs=2, out=out.ptr, istride=h * w * 3, rstride=w * 3, oc=3,
                status=status.ptr, seg=64, smin=0, ws=ws.ptr, ws_bytes=ws_bytes)
    top = dc.jc.header_constant("SF_JPEG_MAX_DIM")
    bad = [(-1, dict(data=None)), (-1, dict(desc=None)), (-1, dict(tables=None)), (-1, dict(out=None)), (-1, dict(status=None)),
           (-1, dict(ws=None)), (-1, dict(data_bytes=-1)), (-1, dict(n_int=0)), (-1, dict(n_int=(1 << 26) + 1)), (-1, dict(n_sets=0)),
           (-1, dict(n_sets=65536)), (-1, dict(n=0)), (-1, dict(n=65536)), (-1, dict(h=0)), (-1, dict(w=0)), (-1, dict(c=2)), (-1, dict(c=4)),
           (-1, dict(hs=1, vs=2)), (-1, dict(hs=4, vs=1)), (-1, dict(hs=2, vs=4)), (-1, dict(hs=0, vs=1)), (-1, dict(c=1, hs=2, vs=2)),
           (-1, dict(oc=2)), (-1, dict(oc=1)), (-1, dict(oc=0)), (-1, dict(rstride=w * 3 - 1)), (-1, dict(istride=h * w * 3 - 1)),
           (-1, dict(desc=desc.data_ptr() + 4)), (-1, dict(status=status.ptr + 2)), (-1, dict(ws=ws.ptr + 8, ws_bytes=ws_bytes - 8)),
           (-1, dict(ws_bytes=ws_bytes - 1)),
           (-1, dict(seg=0)), (-1, dict(seg=4)), (-1, dict(seg=96)), (-1, dict(seg=8192)), (-1, dict(seg=-128)), (-1, dict(smin=-1)),
           (-2, dict(h=1, w=top + 1, rstride=3 * (top + 1), istride=3 * (top + 1), ws_bytes=1 << 30)),
           (-2, dict(h=top + 1, w=1, rstride=3, istride=3 * (top + 1), ws_bytes=1 << 30))]
    for code, change in bad:
        a = dict(good, **change)
        rc = lib().sf_jpeg_decode_split(a["data"], a["data_bytes"], a["desc"], a["n_int"], a["tables"], a["n_sets"], a["n"], a["h"], a["w"],
                                        a["c"], a["hs"], a["vs"], a["out"], a["istride"], a["rstride"], a["oc"], a["status"], a["seg"],
                                        a["smin"], a["ws"], a["ws_bytes"], torch.cuda.current_stream().cuda_stream)
        assert rc == code, (change, rc, lib().sf_last_error())
    torch.cuda.synchronize()
    assert (out.view() == FILL).all() and (ws.view() == 0x3C).all() and (status.view() == 0x77).all()
    assert out.guards_unchanged() and ws.guards_unchanged() and status.guards_unchanged()
    size = lib().sf_jpeg_decode_split_ws_bytes
    assert size(0, 8, 8, 3, 1, 1, 100, 1, 64) == -1 and size(1, 8, 8, 3, 1, 2, 100, 1, 64) == -1 and size(1, 8, 8, 3, 1, 1, -1, 1, 64) == -1
    assert size(1, 8, 8, 3, 1, 1, 100, 0, 64) == -1 and size(1, 8, 8, 3, 1, 1, 100, 1, 48) == -1 and size(1, 8, 8, 3, 1, 1, 100, 1, 4) == -1
    assert size(1, 8, 8, 3, 1, 1, 1 << 20, 1, 8) > size(1, 8, 8, 3, 1, 1, 1 << 20, 1, 4096) > lib().sf_jpeg_decode_ws_bytes(1, 8, 8, 3, 1, 1) + (1 << 20)


def test_malformed_streams_fail_alone(dev, tmp_path):
    """The 34 deterministic mutations of jpeg_decode_cases.mutations(), every interval split: each call first runs clean through the
    sanitized host program; then on the device every image's status is zero exactly where sf_jpeg_decode's is on the same call (and
    equals the host program's word), the undamaged images are bitwise right and every guard band is intact (decode() asserts that)."""
    muts = dc.mutations()
    assert len(muts) == 34
    exe = sc.host_program(tmp_path)
    want = [dc.decode_ref(dc.load(n)) for n in dc.MUTATED]
    waves = [decode(dev, sc.Call.of(c), split=False, row_gap=2, image_gap=7) for _, c in muts]
    for S in (8, 128):
        calls = [sc.Call.of(c, S, 0) for _, c in muts]
        host = sc.run_host(exe, calls, tmp_path, f"mutations{S}")           # asserts a clean exit without a sanitizer report
        failed = 0
        for (label, _), call, h, (wpixels, wstatus) in zip(muts, calls, host, waves):
            pixels, status = decode(dev, call, row_gap=2, image_gap=7)
            assert np.array_equal(status == 0, wstatus == 0), (label, S, status, wstatus)
            assert np.array_equal(status, h["status"]), (label, S, status, h["status"])
            for i in np.flatnonzero(status == 0):
                assert np.array_equal(pixels[i], wpixels[i]), (label, S, i)
                if i != 1:                                                  # image 1 is the damaged one: a flipped bit may still decode
                    assert np.array_equal(pixels[i], want[i]), (label, S, i)
            assert status[0] == 0 or label == "image-negative"
            failed += int(status[1] != 0)
        assert failed >= len(muts) - 8                                      # only a flipped bit may go unnoticed


def test_ops_and_decode_batch_split_always_is_split_never(dev):
    from streamflow_amd import jpeg_gpu, ops
    call = sc.Call(dc.MUTATED)
    want = np.stack([dc.decode_ref(dc.load(n)) for n in dc.MUTATED])
    args = (torch.from_numpy(call.data).to(dev), torch.from_numpy(call.desc).to(dev), torch.from_numpy(call.tables).to(dev), 3, 33, 33, 3, 2, 2)
    for kw in (dict(segment_bytes=16), dict(split_min_bytes=100), dict(segment_bytes=8, split_min_bytes=0)):
        out, status = ops.jpeg_decode(*args, **kw)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (3, 33, 33, 3) and not status.any() and np.array_equal(out.cpu().numpy(), want), kw
    for kw in (dict(segment_bytes=24), dict(segment_bytes=4), dict(split_min_bytes=-1)):
        with pytest.raises(RuntimeError):
            ops.jpeg_decode(*args, **kw)
    for names in (dc.MUTATED, ("sync-444-96x128-q90",), ("sync-420-96x128-q90",), ("sync-grey-96x128-q90", "sync-grey-96x128-q90")):
        blobs = [sc.load(n) for n in names]
        never = jpeg_gpu.decode_batch(blobs, dev, split="never")
        for kw in (dict(split="always"), dict(split="always", segment_bytes=16), dict(split="auto")):
            assert torch.equal(jpeg_gpu.decode_batch(blobs, dev, **kw), never), (names, kw)
        assert np.array_equal(never[0].cpu().numpy(), dc.decode_ref(blobs[0]))
    with pytest.raises(ValueError, match="the broken one.*status"):
        jpeg_gpu.decode_batch([sc.load("sync-420-96x128-q90"), sc.load("sync-420-96x128-q90")[:-900] + b"\xff\xd9"], dev, split="always",
                              names=["good", "the broken one"])


def test_predict_video_on_a_reader_that_splits_is_the_existing_path(dev, tmp_path):
    """Five 132 x 196 wheels encoded on the GPU, written as an AVI file and as a directory: predict_video on
    MjpegReader(split="always") and JpegDir(split="always") -- every interval of every frame on the split route -- equals
    predict_video on the split="never" reader bit for bit.  The tiny synthetic-weight model of the video tests."""
    from streamflow_amd import avi, jpeg_gpu, synthetic as syn, video
    from streamflow_amd.model import SKFlow_MF8, default_args
    H, W, T, n, iters = 132, 196, 3, 5, 3
    images = torch.from_numpy(np.stack([dc.jc.make("wheel", H, W, 3, 10 + s) for s in range(n)])).to(dev)
    (tmp_path / "frames").mkdir()
    files = jpeg_gpu.encode_batch(images, [str(tmp_path / "frames" / f"{i:04d}.jpg") for i in range(n)], quality=85)
    with avi.MjpegWriter(str(tmp_path / "in.avi"), W, H, 25) as v:
        for blob in files:
            v.add(blob)
    model = SKFlow_MF8(default_args(T=T, Encoder="PatchEncoder")).to(dev)
    model.load_state_dict(dict(syn.make_params(41, T)), strict=True)
    never = avi.MjpegReader(str(tmp_path / "in.avi"), split="never")
    want = video.predict_video(model, never, T=T, iters=iters, clips_per_step=2)
    assert want.shape == (n - 1, 2, H, W) and torch.isfinite(want).all()
    reader = video.open_frames(str(tmp_path / "in.avi"), jpeg_split="always")
    assert isinstance(reader, avi.MjpegReader) and reader.split == "always"
    assert torch.equal(video.predict_video(model, reader, T=T, iters=iters, clips_per_step=2), want)
    frames = video.open_frames(str(tmp_path / "frames"), jpeg_split="always")
    assert isinstance(frames, video.JpegDir) and frames.split == "always"
    assert torch.equal(video.predict_video(model, frames, T=T, iters=iters, clips_per_step=2), want)
    assert np.array_equal(reader[3], never[3]) and np.array_equal(frames[-1], dc.decode_ref(files[-1]))
    reader.close()
    never.close()
