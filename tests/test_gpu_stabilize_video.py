"""streamflow_amd.stabilize on the GPU and the demo's --stabilize output.

The library tests use a stand-in for the model whose flows are EXACT: the video shows one textured image through a window that
jitters by whole pixels, frame k carries k in a tag byte, and the stand-in returns for every pair the constant flow between the two
windows it reads from the tags (forwards or, for time-reversed clips, backwards).  11 frames of 40 x 64 (no padding), T = 4: four
clips, the last one a tail clip that overlaps.  In tripod mode with zoom 1 and the constant border every output frame must then be
frame 0 BITWISE wherever its source is inside the frame: that pins the signs and the order of composition from the flow to the
rendered byte.  stabilize_video must be BITWISE the composition of predict_video, ops.motion_fit, camera_path and ops.warp_affine.
The demo builds StreamFlowT4 from a checkpoint itself, so its test runs the seeded Twins model of tests/test_gpu_video.py at
128 x 192 in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import avi_walk
from tests import video_cases as vc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, T, N, MARGIN = 40, 64, 4, 11, 8
JITTER = np.array([[0, 0], [3, -2], [-1, 4], [5, 1], [2, 2], [-4, -3], [0, 5], [6, -1], [-2, 0], [1, -5], [3, 3]])     # (x, y) per frame


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def jitter_video():
    """uint8 [N, H, W, 3]: frame k shows the window of a fixed noise image at offset MARGIN + JITTER[k]; its red byte at (0, 0) is 8 k."""
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, size=(H + 2 * MARGIN, W + 2 * MARGIN, 3), dtype=np.uint8)
    frames = np.stack([base[MARGIN + jy:MARGIN + jy + H, MARGIN + jx:MARGIN + jx + W] for jx, jy in JITTER]).copy()
    frames[:, 0, 0, 0] = 8 * np.arange(N)
    return torch.from_numpy(frames)


def jitter_model(imgs: torch.Tensor) -> list:
    """The exact flows of jitter_video's clips: a scene point seen at p in frame a is seen at p + JITTER[a] - JITTER[b] in frame b."""
    B, Tc, _, Hp, Wp = imgs.shape
    index = torch.round((imgs[:, :, 0, 0, 0] + 1.0) * (255.0 / 2.0) / 8.0).long().clamp(0, N - 1)       # [B, T] frame numbers
    table = torch.from_numpy(JITTER).to(imgs.device, torch.float32)
    out = []
    for k in range(Tc - 1):
        d = table[index[:, k]] - table[index[:, k + 1]]                  # [B, 2]
        out.append(d.view(B, 2, 1, 1).expand(B, 2, Hp, Wp).contiguous())
    return out


@pytest.mark.parametrize("clips_per_step", [1, 8])
@pytest.mark.parametrize("kind", ["translation", "similarity"])
def test_tripod_mode_reproduces_frame_zero_bitwise(dev, clips_per_step, kind):
    from streamflow_amd import stabilize
    frames = jitter_video()
    got = {}
    res = stabilize.stabilize_video(jitter_model, frames, lambda first, out: got.update({first: out.cpu().numpy()}), kind=kind, sigma=None,
                                    zoom=1.0, border="constant", fill=(1, 2, 3), T=T, clips_per_step=clips_per_step)
    out = np.concatenate([got[k] for k in sorted(got)])
    assert out.shape == (N, H, W, 3) and sorted(got)[0] == 0
    want_models = np.tile(np.eye(3)[:2], (N - 1, 1, 1))
    want_models[:, :, 2] = JITTER[:-1] - JITTER[1:]
    assert np.abs(res.models - want_models).max() <= 1e-12 and res.zoom == 1.0
    assert (res.fit_info["status"] == 0).all() and (res.fit_info["inlier_share"] == 1.0).all()
    f0 = frames[0].numpy()
    ys, xs = np.mgrid[0:H, 0:W]
    outside = 0
    for k in range(N):
        dx, dy = JITTER[0] - JITTER[k]                                   # output pixel p reads frame k at p + JITTER[0] - JITTER[k]
        inside = (xs + dx >= 0) & (xs + dx <= W - 1) & (ys + dy >= 0) & (ys + dy <= H - 1)
        outside += int((~inside).sum())
        assert (out[k][~inside] == (1, 2, 3)).all(), k
        same = inside.copy()
        same[0, 0] = False                                               # frame 0's tag
        if 0 <= -dy < H and 0 <= -dx < W:
            same[-dy, -dx] = False                                       # where frame k's tag lands
        assert np.array_equal(out[k][same], f0[same]), (k, int((out[k][same] != f0[same]).sum()))
    assert np.array_equal(out[0], f0)
    rep = res.report()
    assert rep["frames"] == N and rep["bad_fields"] == 0 and rep["zoom"] == 1.0 and rep["inlier_share"] == 1.0
    assert rep["outside"] == outside / (N * H * W)
    assert abs(rep["max_correction"] - np.linalg.norm(JITTER - JITTER[0], axis=1).max()) <= 1e-9
    assert res.report_line().startswith("Stabilisation frames: %d" % N)


@pytest.mark.parametrize("clips_per_step", [1, 8])
def test_stabilize_video_is_the_composition_of_its_parts(dev, clips_per_step):
    """(A field's fit and a frame's rendering do not depend on the batch they run in: with so few fields the grid per field is the same.)"""
    from streamflow_amd import ops, stabilize, video
    frames = vc.random_frames(31, N, H, W)
    got = {}
    res = stabilize.stabilize_video(vc.stub_model, frames, lambda first, out: got.update({first: out.clone()}), kind="affine", sigma=2.0,
                                    zoom="auto", border="replicate", T=T, clips_per_step=clips_per_step, step=2)
    out = torch.cat([got[k] for k in sorted(got)])
    flows = video.predict_video(vc.stub_model, frames, T=T, clips_per_step=clips_per_step)
    models, info = ops.motion_fit(flows, kind="affine", step=2)
    assert np.array_equal(res.models, models.cpu().numpy())
    inv_maps, zoom = stabilize.camera_path(models, sigma=2.0, zoom="auto", hw=(H, W))
    assert np.array_equal(res.inv_maps, inv_maps) and res.zoom == zoom and 1.0 <= zoom <= stabilize.MAX_ZOOM
    want, counts = ops.warp_affine(frames.to(dev), inv_maps, border="replicate")
    assert torch.equal(out, want) and res.outside == int(counts.sum())
    assert not torch.equal(out, frames.to(dev))
    # a sink alone: the models of a video without keeping its flows
    sink = stabilize.MotionSink(kind="affine", step=2)
    assert video.predict_video(vc.stub_model, frames, T=T, clips_per_step=clips_per_step, sink=sink) is None
    assert np.array_equal(sink.models(), res.models) and np.array_equal(sink.info()["status"], info["status"].cpu().numpy())


def test_size_and_occlusion_go_through(dev):
    from streamflow_amd import consistency, ops, stabilize, video
    frames = jitter_video()
    got = {}
    res = stabilize.stabilize_video(jitter_model, frames, lambda first, out: got.update({first: out.clone()}), kind="similarity", sigma=None,
                                    zoom=1.0, border="constant", occlusion=True, T=T, clips_per_step=3)
    out = torch.cat([got[k] for k in sorted(got)])
    fwd, bwd = video.predict_video(jitter_model, frames, T=T, clips_per_step=3, bidirectional=True)
    assert torch.equal(bwd, -fwd)
    cls = consistency.check_pairs(fwd, bwd)[0][0]
    models, info = ops.motion_fit(fwd, cls=cls, kind="similarity")
    assert np.array_equal(res.models, models.cpu().numpy()) and (info["inlier_share"] == 1.0).all()
    assert (info["trace"][:, 0, ops.MOT_N] < H * W).all()                # the pixels that leave the frame stayed out of the fit
    assert torch.equal(out, ops.warp_affine(frames.to(dev), stabilize.camera_path(models, None, 1.0, (H, W))[0], border="constant")[0])
    # size=: the model runs at another resolution, the fit sees flows on the frames' own grid, the frames keep their size
    frames2 = vc.random_frames(32, N, 48, 80)
    got2 = {}
    res2 = stabilize.stabilize_video(vc.stub_model, frames2, lambda first, out: got2.update({first: out.clone()}), size=(40, 64), T=T,
                                     clips_per_step=8, sigma=1.5)
    out2 = torch.cat([got2[k] for k in sorted(got2)])
    flows2 = video.predict_video(vc.stub_model, frames2, T=T, clips_per_step=8, size=(40, 64))
    assert tuple(out2.shape) == (N, 48, 80, 3) and np.array_equal(res2.models, ops.motion_fit(flows2)[0].cpu().numpy())
    assert res2.report()["frames"] == N


def test_command_line_writes_the_stabilised_frames_and_video(tmp_path, dev):
    """python -m streamflow_amd.demo --stabilize DIR --stabilize-video FILE --report in a child process over six 128 x 192 PNG frames:
    the PNGs decode to stabilize_video's frames with the same model and options in this process, the AVI passes tests/avi_walk.py
    and holds the JPEG streams of those frames (so its frames decode to their JPEG round trip)."""
    from streamflow_amd import avi, flow_io, jpeg_gpu, stabilize, synthetic as syn
    from streamflow_amd.model import StreamFlowT4
    Hd, Wd, n, iters = 128, 192, 6, 3
    frames = vc.random_frames(6, n, Hd, Wd).numpy()
    os.makedirs(tmp_path / "frames")
    for i, f in enumerate(frames):
        flow_io.write_png(str(tmp_path / "frames" / ("%04d.png" % i)), f)
    sd = dict(syn.make_params(51, 4))
    sd.update({"fnet." + k: v for k, v in syn.make_twins_params(52).items()})
    sd.update({"cnet." + k: v for k, v in syn.make_twins_params(53).items()})
    ckpt = str(tmp_path / "ckpt.pth")
    torch.save({"model": {"module." + k: v for k, v in sd.items()}}, ckpt)
    cmd = [sys.executable, "-m", "streamflow_amd.demo", "--frames", str(tmp_path / "frames"), "--ckpt", ckpt, "--stabilize",
           str(tmp_path / "stab"), "--stabilize-video", str(tmp_path / "stab.avi"), "--stabilize-model", "affine", "--smooth-sigma", "2",
           "--stabilize-zoom", "1.1", "--stabilize-border", "black", "--report", "--iters", str(iters), "--fps", "12", "--jpeg-quality",
           "85"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "5 flow fields" in r.stdout and "Stabilisation frames: 6" in r.stdout and "Consistency" not in r.stdout
    assert sorted(os.listdir(tmp_path / "stab")) == ["stab_%06d.png" % i for i in range(n)]
    model = StreamFlowT4(ckpt).to(dev).eval()
    got = {}
    res = stabilize.stabilize_video(model, torch.from_numpy(frames), lambda first, out: got.update({first: out.clone()}), kind="affine",
                                    sigma=2.0, zoom=1.1, border="constant", T=4, iters=iters, clips_per_step=8)
    want = torch.cat([got[k] for k in sorted(got)])
    assert res.zoom == 1.1 and not torch.equal(want.cpu(), torch.from_numpy(frames))
    for i in range(n):
        assert np.array_equal(flow_io.read_png(str(tmp_path / "stab" / ("stab_%06d.png" % i))), want[i].cpu().numpy()), i
    info = avi_walk.walk(open(tmp_path / "stab.avi", "rb").read())
    assert (info["width"], info["height"]) == (Wd, Hd) and len(info["frames"]) == n and info["rate"] / info["scale"] == 12
    blobs = jpeg_gpu.encode_batch(want, quality=85)
    assert [bytes(x) for x in info["frames"]] == [bytes(x) for x in blobs]
    trip = jpeg_gpu.decode_batch([bytes(x) for x in blobs], dev)          # the emitted frames' JPEG round trip
    assert torch.equal(avi.MjpegReader(str(tmp_path / "stab.avi")).device_batch(0, n, dev), trip)
    assert float((trip.float() - want.float()).abs().mean()) < 16        # (and the round trip is the frames, as far as JPEG goes)
