"""Video inference at a chosen resolution: ops.resize_frames / ops.resize_flows, video.predict_video(size=...) and the --scale
switch of streamflow_amd.demo.

Criterion: every comparison is BITWISE.  predict_video(size=...) must be the composition resize_frames -> predict_video on the
resized frames -> resize_flows, whatever the batching; the wrappers must give the bytes of the numpy restatement
(tests/resize_cases.py) for the u8 side; size=None must be the call without the keyword."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import resize_cases as rc
from tests import video_cases as vc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, T, N = 60, 90, 4, 11                                               # 4 clips, the last one a tail clip
SIZE = (32, 48)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def frames():
    return vc.random_frames(33, N, H, W)


def compose(model, frames_dev, size, frame_filter, flow_filter, bidirectional=False, **kw):
    """The definition: frames to the working size, the video path there, flows back to the frames' grid."""
    from streamflow_amd import ops, video
    small = ops.resize_frames(frames_dev, size, frame_filter)
    assert small.shape == (frames_dev.shape[0],) + tuple(size) + (3,) and small.dtype == torch.uint8
    low = video.predict_video(model, small, T=T, bidirectional=bidirectional, **kw)
    back = lambda f: ops.resize_flows(f, (H, W), flow_filter)
    return tuple(back(f) for f in low) if bidirectional else back(low)


def test_wrappers_match_the_restatement(dev, frames):
    from streamflow_amd import ops
    for name in ("bilinear", "lanczos"):
        want = rc.resize_u8(frames.numpy()[:3], SIZE, name)
        for src in (frames[:3].to(dev), frames[:3].permute(0, 3, 1, 2).contiguous().to(dev), frames.to(dev)[:3, :, :, :]):
            got = ops.resize_frames(src, SIZE, name)
            assert np.array_equal(got.cpu().numpy(), want), name
        out = torch.empty(3, *SIZE, 3, dtype=torch.uint8, device=dev)
        assert ops.resize_frames(frames[:3].to(dev), SIZE, name, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    flow = torch.from_numpy(rc.f32_input(((37, 53), (16, 24)))).to(dev)
    got = ops.resize_flows(flow, (16, 24), "bicubic").cpu().numpy().astype(np.float64)
    sx, sy = 24 / 53, 16 / 37
    assert (np.abs(got - rc.resize_f64(flow.cpu().numpy(), (16, 24), "bicubic", sx, sy))
            <= rc.bound_f32(flow.cpu().numpy(), (16, 24), "bicubic", sx, sy)).all()
    plain = ops.resize_flows(flow, (16, 24), "bicubic", rescale=False).cpu().numpy()
    assert plain.tobytes() == rc.emulate_f32(flow.cpu().numpy(), (16, 24), "bicubic").tobytes()      # the stated fp32 arithmetic, exactly
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resize_frames(frames[:2], SIZE)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resize_flows(flow.cpu(), SIZE)
    with pytest.raises(ValueError):
        ops.resize_frames(frames[:2].to(dev), SIZE, "nearest")


@pytest.mark.parametrize("clips_per_step", [1, 8])
def test_predict_video_at_a_size_is_the_composition(dev, frames, clips_per_step):
    from streamflow_amd import video
    shapes = []

    def model(imgs):
        shapes.append(tuple(imgs.shape[-2:]))
        return vc.stub_model(imgs)

    fd = frames.to(dev)
    for ff, lf in (("bilinear", "bilinear"), ("lanczos", "bicubic")):
        want = compose(vc.stub_model, fd, SIZE, ff, lf, clips_per_step=clips_per_step)
        assert want.shape == (N - 1, 2, H, W)
        for name, src in (("host", frames), ("device", fd), ("device chw", fd.permute(0, 3, 1, 2).contiguous()), ("list", list(frames.numpy()))):
            del shapes[:]
            got = video.predict_video(model, src, T=T, clips_per_step=clips_per_step, size=SIZE, frame_filter=ff, flow_filter=lf)
            assert got.dtype == torch.float32 and torch.equal(got, want), (ff, lf, name)
            assert shapes and set(shapes) == {SIZE}, shapes              # the model is called with (h, w) clips
    # a size that is no multiple of 8: the padder works at (h, w)
    del shapes[:]
    odd = (27, 44)
    got = video.predict_video(model, fd, T=T, clips_per_step=clips_per_step, size=odd)
    assert set(shapes) == {(32, 48)} and torch.equal(got, compose(vc.stub_model, fd, odd, "bilinear", "bilinear", clips_per_step=clips_per_step))
    # enlarging
    big = (96, 144)
    assert torch.equal(video.predict_video(vc.stub_model, fd, T=T, clips_per_step=clips_per_step, size=big),
                       compose(vc.stub_model, fd, big, "bilinear", "bilinear", clips_per_step=clips_per_step))


def test_sink_receives_full_size_flows_and_the_original_frames(dev, frames):
    from streamflow_amd import video
    fd = frames.to(dev)
    want = compose(vc.stub_model, fd, SIZE, "bilinear", "bilinear", clips_per_step=3)
    calls = []
    res = video.predict_video(vc.stub_model, frames, T=T, clips_per_step=3, size=SIZE, sink=lambda first, f: calls.append((first, f)))
    assert res is None and [c[0] for c in calls] == [b[4] for b in video.plan_batches(N, T, 3)]
    assert torch.equal(torch.cat([c[1] for c in calls]), want)
    wf, wb = compose(vc.stub_model, fd, SIZE, "bilinear", "bilinear", bidirectional=True, clips_per_step=3)
    assert torch.equal(wf, want) and not torch.equal(wb, want)
    for src in (frames, fd, fd.permute(0, 3, 1, 2).contiguous()):
        gf, gb = video.predict_video(vc.stub_model, src, T=T, clips_per_step=3, size=SIZE, bidirectional=True)
        assert torch.equal(gf, wf) and torch.equal(gb, wb)
        calls = []
        res = video.predict_video(vc.stub_model, src, T=T, clips_per_step=3, size=SIZE, bidirectional=True,
                                  sink=lambda first, f, b, held: calls.append((first, f, b, held.clone())))
        assert res is None and torch.equal(torch.cat([c[1] for c in calls]), wf) and torch.equal(torch.cat([c[2] for c in calls]), wb)
        for first, f, b, held in calls:
            assert held.dtype == torch.uint8 and held.shape == (f.shape[0] + 1, H, W, 3)
            assert torch.equal(held, fd[first:first + f.shape[0] + 1]), first        # the ORIGINAL bytes


def test_size_none_is_the_call_without_the_keyword(dev, frames):
    from streamflow_amd import video
    for kw in (dict(), dict(bidirectional=True), dict(mode="kitti", clips_per_step=3)):
        a = video.predict_video(vc.stub_model, frames, T=T, **kw)
        b = video.predict_video(vc.stub_model, frames, T=T, size=None, frame_filter="lanczos", flow_filter="box", **kw)
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert torch.equal(x, y)
    with pytest.raises(ValueError):
        video.predict_video(vc.stub_model, frames, T=T, size=(0, 8))
    with pytest.raises(ValueError):
        video.predict_video(vc.stub_model, frames, T=T, size=SIZE, frame_filter="nearest")


def test_command_line_scale(tmp_path, dev):
    """python -m streamflow_amd.demo --scale 0.5 over five 256 x 384 PNG frames: .flo files and colour images of the ORIGINAL size whose
    flows are predict_video(size=scaled_size(...)) in this process; --scale together with --max-side is a usage error."""
    from streamflow_amd import flow_io, resize, synthetic as syn, video
    from streamflow_amd.model import StreamFlowT4
    h0, w0, n, iters = 256, 384, 5, 2
    fr = vc.random_frames(6, n, h0, w0).numpy()
    os.makedirs(tmp_path / "frames")
    for i, f in enumerate(fr):
        flow_io.write_png(str(tmp_path / "frames" / ("%04d.png" % i)), f)
    sd = dict(syn.make_params(51, 4))
    sd.update({"fnet." + k: v for k, v in syn.make_twins_params(52).items()})
    sd.update({"cnet." + k: v for k, v in syn.make_twins_params(53).items()})
    ckpt = str(tmp_path / "ckpt.pth")
    torch.save({"model": {"module." + k: v for k, v in sd.items()}}, ckpt)
    base = [sys.executable, "-m", "streamflow_amd.demo", "--frames", str(tmp_path / "frames"), "--ckpt", ckpt, "--out", str(tmp_path / "png"),
            "--flo", str(tmp_path / "flo"), "--iters", str(iters)]
    r = subprocess.run(base + ["--scale", "0.5", "--max-side", "128"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--scale and --max-side" in r.stderr and not os.path.exists(tmp_path / "flo")
    r = subprocess.run(base + ["--scale", "0.5", "--resize-filter", "bicubic"], cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert sorted(os.listdir(tmp_path / "flo")) == ["frame_%04d.flo" % i for i in range(n - 1)]
    size = resize.scaled_size((h0, w0), scale=0.5)
    assert size == (128, 192)
    model = StreamFlowT4(ckpt).to(dev).eval()
    want = video.predict_video(model, torch.from_numpy(fr), T=4, iters=iters, size=size, frame_filter="bicubic", flow_filter="bicubic")
    assert want.shape == (n - 1, 2, h0, w0) and torch.isfinite(want).all()
    for i in range(n - 1):
        flo = flow_io.read_flo(str(tmp_path / "flo" / ("frame_%04d.flo" % i)))
        assert np.array_equal(flo, want[i].permute(1, 2, 0).cpu().numpy()), i
        assert flow_io.read_png(str(tmp_path / "png" / ("frame_%04d.png" % i))).shape[:2] == (h0, w0)
