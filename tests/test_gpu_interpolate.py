"""ops.frame_interp, streamflow_amd.interpolate and the demo's slow-motion output: 9 frames of 64 x 96, T = 4 (three clips, the
last one a tail clip that overlaps).  Everything is compared BITWISE: the wrapper with the raw C ABI call and with the numpy
restatement (tests/interp_cases.py), `between` with per-pair calls, interpolate_video with `between` on the flows of
predict_video(bidirectional=True), the written files with those tensors.

The model.  At 64 x 96 the flow network itself cannot run: its feature grid of 8 x 12 leaves a one-pixel coarsest correlation level
and the engine refuses it (it needs 128 pixels per side).  The library tests therefore use the seeded stand-in of the existing video
tests at that size (tests/video_cases.py stub_model: a fixed function of the clip batch with the model's interface, whose flows are
sub-pixel to two pixels long and differ in every pixel).  The demo builds StreamFlowT4 from a checkpoint itself, so its two tests run
the seeded Twins model of tests/test_gpu_video.py at 128 x 192, the size that test's 124 x 188 frames are padded to."""
import os

import numpy as np
import pytest
import torch

from tests import avi_walk
from tests import interp_cases as ic
from tests import video_cases as vc

pytestmark = pytest.mark.gpu

H, W, T, N, ITERS = 64, 96, 4, 9, 3
DEMO_H, DEMO_W = 128, 192


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def frames():
    return vc.random_frames(17, N, H, W)                                  # uint8 [N, H, W, 3] on the host


@pytest.fixture(scope="module")
def model():
    return vc.stub_model


@pytest.fixture(scope="module")
def flows(model, frames):
    """(fwd, bwd) [N - 1, 2, H, W] of the video, computed once and left unchanged."""
    from streamflow_amd import video
    fwd, bwd = video.predict_video(model, frames, T=T, iters=ITERS, clips_per_step=8, bidirectional=True)
    assert torch.isfinite(fwd).all() and 0.3 < float(fwd.abs().mean()) < 2 and not torch.equal(fwd[0], fwd[1])
    return fwd, bwd


def raw_call(a, b, fwd, bwd, num, den, cls=None, imp=(16, 1, 16)):
    """sf_frame_interp on dense device tensors -> (out, cover, stats)."""
    from streamflow_amd import _lib
    lib = _lib.load()
    n, _, h, w = fwd.shape
    a, b, fwd, bwd = a.contiguous(), b.contiguous(), fwd.contiguous(), bwd.contiguous()
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=fwd.device)
    cover = torch.empty(n, h, w, dtype=torch.uint8, device=fwd.device)
    stats = torch.zeros(n, ic.LEN, dtype=torch.float64, device=fwd.device)
    ws = torch.empty(lib.sf_frame_interp_ws_bytes(n, h, w), dtype=torch.uint8, device=fwd.device)
    st = lib.sf_frame_interp(a.data_ptr(), 3 * h * w, 3 * w, 3, 1, b.data_ptr(), 3 * h * w, 3 * w, 3, 1, fwd.data_ptr(), 2 * h * w, h * w, w,
                             bwd.data_ptr(), 2 * h * w, h * w, w, n, h, w, num, den, None if cls is None else cls[0].data_ptr(),
                             None if cls is None else cls[1].data_ptr(), 0, 1, imp[0], imp[1], imp[2], out.data_ptr(), cover.data_ptr(),
                             stats.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.sf_last_error()
    return out, cover, stats


def test_wrapper_equals_the_raw_call_and_the_restatement(dev, frames, flows):
    from streamflow_amd import _lib, consistency, ops
    fwd, bwd = flows
    dframes = frames.to(dev)
    a, b = dframes[:-1], dframes[1:]
    (cls_f, _), (cls_b, _) = consistency.check_pairs(fwd, bwd)
    cls = (cls_f, cls_b)
    host = [t.cpu().numpy() for t in (a, b, fwd, bwd, cls_f, cls_b)]
    per4 = int(_lib.load().sf_frame_interp_ws_bytes(4, H, W))
    for num, den, use_cls, imp in ((1, 2, True, (16, 1, 16)), (2, 3, False, (16, 1, 16)), (63, 64, True, (3, 7, 1))):
        want = raw_call(a, b, fwd, bwd, num, den, cls if use_cls else None, imp)
        restated = ic.restate(*host[:4], num, den, tuple(host[4:]) if use_cls else None, imp=imp)
        for x, y in zip(want, restated):
            assert np.array_equal(x.cpu().numpy(), y)
        chw = dframes.permute(0, 3, 1, 2).contiguous()
        for aa, bb, kw in ((a, b, {}), (a, b, dict(max_ws_bytes=per4)), (a, b, dict(max_ws_bytes=1)),
                           (chw[:-1], chw[1:], dict(channels_last=False)), (chw.permute(0, 2, 3, 1)[:-1], b, {})):
            out, cover, stats = ops.frame_interp(aa, bb, fwd, bwd, num, den, cls=cls if use_cls else None, importance=imp, cover=True, **kw)
            assert torch.equal(out, want[0]) and torch.equal(cover, want[1]) and torch.equal(stats, want[2])
        out, none, stats = ops.frame_interp(a, b, fwd, bwd, num, den, cls=cls if use_cls else None, importance=imp, stats=want[2].clone())
        assert none is None and torch.equal(out, want[0]) and torch.equal(stats, 2 * want[2])
    # other class bytes: a mask image's codes
    table = torch.tensor([255, 0, 128], dtype=torch.uint8, device=dev)
    out, _, _ = ops.frame_interp(a, b, fwd, bwd, 1, 2, cls=(table[cls_f.long()], table[cls_b.long()]), codes=(255, 0))
    assert torch.equal(out, raw_call(a, b, fwd, bwd, 1, 2, cls)[0])
    for bad, match in ((dict(num=0), "0 < num"), (dict(den=65), "0 < num"), (dict(importance=(0, 1, 1)), "importance"),
                       (dict(cls=(cls_f,)), "pair"), (dict(cls=(cls_f, cls_b[:2])), "class map"), (dict(stats=torch.zeros(2, 5)), "stats")):
        kw = dict(dict(num=1, den=2), **bad)
        with pytest.raises(RuntimeError, match=match):
            ops.frame_interp(a, b, fwd, bwd, **kw)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.frame_interp(a.float(), b, fwd, bwd, 1, 2)
    with pytest.raises(RuntimeError, match="frames of"):
        ops.frame_interp(a[:3], b, fwd, bwd, 1, 2)
    with pytest.raises(RuntimeError, match="bwd"):
        ops.frame_interp(a, b, fwd, bwd[:2], 1, 2)


@pytest.mark.parametrize("masks", [True, False], ids=["masks", "nomasks"])
def test_between_equals_per_pair_calls(dev, frames, flows, masks):
    from streamflow_amd import consistency, interpolate, ops
    fwd, bwd = flows
    dframes = frames.to(dev)
    factor = 4
    mid, stats = interpolate.between(dframes, fwd, bwd, factor, masks=masks)
    assert mid.shape == (N - 1, factor - 1, H, W, 3) and mid.dtype == torch.uint8 and stats.shape == (N - 1, factor - 1, ic.LEN)
    assert torch.equal(mid, interpolate.between(dframes.permute(0, 3, 1, 2).contiguous(), fwd, bwd, factor, masks=masks)[0])
    for j in range(N - 1):
        f, b = fwd[j:j + 1], bwd[j:j + 1]
        cls = None
        if masks:
            (cf, _), (cb, _) = consistency.check_pairs(f, b)
            cls = (cf, cb)
        for i in range(1, factor):
            out, cover, st = raw_call(dframes[j:j + 1], dframes[j + 1:j + 2], f, b, i, factor, cls)
            assert torch.equal(mid[j, i - 1], out[0]) and torch.equal(stats[j, i - 1], st[0]), (j, i)
    assert float(stats[..., ic.PIXELS].sum()) == (N - 1) * (factor - 1) * H * W
    with pytest.raises(RuntimeError, match="one frame more"):
        interpolate.between(dframes[:-1], fwd, bwd, factor)


def test_interpolate_video_passes_frames_through_and_fills_in_between(dev, model, frames, flows):
    from streamflow_amd import interpolate
    fwd, bwd = flows
    factor = 3
    dframes = frames.to(dev)
    want_mid, want_stats = interpolate.between(dframes, fwd, bwd, factor)
    got = interpolate.interpolate_video(model, frames, factor=factor, T=T, iters=ITERS)
    assert got.shape == ((N - 1) * factor + 1, H, W, 3) and got.dtype == torch.uint8 and got.device == dev
    assert torch.equal(got[::factor], dframes)
    for i in range(1, factor):
        assert torch.equal(got[i::factor], want_mid[:, i - 1]), i
    for clips_per_step in (1, 8):
        calls = []
        sink_frames = frames.to(dev).permute(0, 3, 1, 2).contiguous() if clips_per_step == 1 else frames
        res = interpolate.interpolate_video(model, sink_frames, factor=factor, T=T, iters=ITERS, clips_per_step=clips_per_step,
                                            emit=lambda first, batch: calls.append((first, batch.clone())))
        assert res is None
        at = 0
        for first, batch in calls:                                        # in order, without gaps or repeats
            assert first == at and batch.dtype == torch.uint8 and tuple(batch.shape[1:]) == (H, W, 3)
            at += batch.shape[0]
        assert at == got.shape[0] and calls[-1][1].shape[0] == 1
        assert torch.equal(torch.cat([b for _, b in calls]), got)
    # the sink's report: shares of the cover codes over all interpolated pixels
    sink = interpolate.InterpSink(factor, lambda first, batch: None)
    sink(0, fwd, bwd, dframes)
    sink.finish()
    rep = sink.report()
    s = want_stats.sum((0, 1)).cpu().numpy()
    assert rep["pixels"] == (N - 1) * (factor - 1) * H * W == s[ic.PIXELS]
    assert [rep[k] for k in interpolate.COVER_NAMES] == [s[k] / s[ic.PIXELS] for k in (ic.BOTH, ic.A_ONLY, ic.B_ONLY, ic.HOLES)]
    assert abs(sum(rep[k] for k in interpolate.COVER_NAMES) - 1) < 1e-12
    assert interpolate.report_line(rep).startswith("Interpolation cover, pixels: %d" % rep["pixels"])


@pytest.fixture(scope="module")
def demo_inputs(tmp_path_factory):
    """A directory of PNG frames and a checkpoint of a seeded StreamFlowT4, as tests/test_gpu_video.py makes them."""
    from streamflow_amd import flow_io, synthetic as syn
    root = tmp_path_factory.mktemp("slowmo")
    os.makedirs(root / "frames")
    frames = vc.random_frames(18, N, DEMO_H, DEMO_W)
    for i, f in enumerate(frames.numpy()):
        flow_io.write_png(str(root / "frames" / ("%04d.png" % i)), f)
    sd = dict(syn.make_params(51, 4))
    sd.update({"fnet." + k: v for k, v in syn.make_twins_params(52).items()})
    sd.update({"cnet." + k: v for k, v in syn.make_twins_params(53).items()})
    ckpt = str(root / "ckpt.pth")
    torch.save({"model": {"module." + k: v for k, v in sd.items()}}, ckpt)
    return root, ckpt, frames


@pytest.fixture(scope="module")
def demo_video(dev, demo_inputs):
    """What the demo must write for --interpolate 2: interpolate_video with its model, computed once."""
    from streamflow_amd import interpolate
    from streamflow_amd.model import StreamFlowT4
    model = StreamFlowT4(demo_inputs[1]).to(dev).eval()
    got = interpolate.interpolate_video(model, demo_inputs[2], factor=2, T=T, iters=ITERS).cpu().numpy()
    assert got.shape == (2 * N - 1, DEMO_H, DEMO_W, 3)
    return got


@pytest.mark.parametrize("png_encode", ["gpu", "host"])
def test_demo_writes_the_slow_motion_frames(dev, demo_inputs, demo_video, png_encode, capsys):
    from streamflow_amd import demo, flow_io
    root, ckpt, _ = demo_inputs
    out = root / ("slow_" + png_encode)
    argv = ["--frames", str(root / "frames"), "--ckpt", ckpt, "--interpolate", "2", "--slowmo", str(out), "--iters", str(ITERS),
            "--png-encode", png_encode] + (["--report"] if png_encode == "gpu" else [])
    assert demo.main(argv) == 0
    text = capsys.readouterr().out
    assert "%d flow fields" % (N - 1) in text and ("Interpolation cover, pixels: %d" % ((N - 1) * DEMO_H * DEMO_W) in text) == (png_encode == "gpu")
    assert sorted(os.listdir(out)) == ["slow_%06d.png" % i for i in range(2 * N - 1)]
    for i in range(2 * N - 1):
        assert np.array_equal(flow_io.read_png(str(out / ("slow_%06d.png" % i))), demo_video[i]), i


def test_demo_writes_the_slow_motion_video(dev, demo_inputs, demo_video, capsys):
    from streamflow_amd import demo, jpeg_gpu
    root, ckpt, _ = demo_inputs
    path = root / "slow.avi"
    assert demo.main(["--frames", str(root / "frames"), "--ckpt", ckpt, "--interpolate", "2", "--slowmo-video", str(path), "--iters",
                      str(ITERS), "--fps", "24", "--jpeg-quality", "85", "--out", str(root / "colour")]) == 0
    capsys.readouterr()
    info = avi_walk.walk(open(path, "rb").read())
    assert (info["width"], info["height"]) == (DEMO_W, DEMO_H) and len(info["frames"]) == 2 * N - 1
    assert info["rate"] / info["scale"] == 24
    blobs = jpeg_gpu.encode_batch(torch.from_numpy(demo_video).to(dev), quality=85)
    assert [bytes(x) for x in info["frames"]] == [bytes(x) for x in blobs]
    assert len(os.listdir(root / "colour")) == N - 1                     # the colour-wheel images are written as before
