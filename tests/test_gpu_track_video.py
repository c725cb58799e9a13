"""streamflow_amd.track on the GPU and the demo's --track outputs.

The library tests use stand-ins for the model, as tests/test_gpu_stabilize_video.py does: `shift_model` returns one constant
whole-pixel flow for every pair (negated for time-reversed clips, which it tells from the frame numbers tests/video_cases.py's
random_frames writes into the first pixel), so tracks are exactly q + n d until a point leaves the frame; vc.stub_model returns a
fixed function of the clip batch, sub-pixel flows that differ in every pixel, for the comparisons that must be BITWISE the
composition of predict_video and one ops.track_advance.  11 frames of 40 x 64, T = 4: four clips, the last one a tail clip that
overlaps; clips_per_step 1 and 8 puts the batch boundaries in different places.  The demo builds StreamFlowT4 from a checkpoint
itself, so its test runs the seeded Twins model of tests/test_gpu_video.py at 128 x 192 in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import avi_walk
from tests import track_cases as tc
from tests import video_cases as vc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, T, N = 40, 64, 4, 11
SHIFT = (2.0, -1.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def shift_model(imgs: torch.Tensor) -> list:
    B, Tc, _, Hp, Wp = imgs.shape
    index = torch.round((imgs[:, :, 0, 0, 0] + 1.0) * (255.0 / 2.0))     # [B, T] frame numbers
    d = torch.tensor(SHIFT, device=imgs.device)
    out = []
    for k in range(Tc - 1):
        sign = torch.where(index[:, k + 1] > index[:, k], 1.0, -1.0)
        out.append((sign.view(B, 1, 1, 1) * d.view(1, 2, 1, 1)).expand(B, 2, Hp, Wp).contiguous())
    return out


def queries():
    from streamflow_amd import track
    q = track.grid_queries((H, W), 7)
    q[:, 0] = np.arange(len(q)) % 6                                      # starts spread over the first batches
    extra = np.array([[0, W - 1, H - 1], [2, 0, 0], [4, 70, 3], [1, np.nan, 3], [10, 5, 5]], np.float32)
    return np.concatenate([q, extra])


@pytest.mark.parametrize("clips_per_step", [1, 8])
def test_a_constant_shift_gives_exact_tracks(dev, clips_per_step):
    from streamflow_amd import track
    frames = vc.random_frames(3, N, H, W)
    q = queries()
    t = track.track_points(shift_model, frames, q, T=T, clips_per_step=clips_per_step).numpy()
    assert t.xy.shape == (N, len(q), 2) and t.status.shape == (N, len(q))
    for i, (t0, x0, y0) in enumerate(q):
        ok0 = 0 <= x0 <= W - 1 and 0 <= y0 <= H - 1
        steps, lost = 0, not ok0
        for n in range(N):
            if n < t0:
                assert t.status[n, i] == tc.PENDING
                continue
            if n > t0 and not lost:
                if 0 <= x0 + (steps + 1) * SHIFT[0] <= W - 1 and 0 <= y0 + (steps + 1) * SHIFT[1] <= H - 1:
                    steps += 1
                else:
                    lost = True
            assert t.status[n, i] == (tc.LOST if lost else tc.VISIBLE), (i, n)
            if ok0:
                assert tuple(t.xy[n, i]) == (x0 + steps * SHIFT[0], y0 + steps * SHIFT[1]), (i, n)
    assert (t.status[-1] == tc.VISIBLE).any() and (t.status[-1] == tc.LOST).any() and not (t.status == tc.OCCLUDED).any()
    rep = t.report()
    assert rep["frames"] == N and rep["points"] == len(q) and abs(rep["visible"] + rep["lost"] + rep["occluded"] - 1.0) < 1e-12


def _compose(dev, frames, q, occlusion, **predict):
    """predict_video, then ONE ops.track_advance over the whole video."""
    from streamflow_amd import ops, video
    got = video.predict_video(vc.stub_model, frames, T=T, bidirectional=occlusion, **predict)
    fwd, bwd = got if occlusion else (got, None)
    h, w = fwd.shape[-2:]
    sxy, sst, start = (torch.from_numpy(a).to(dev) for a in tc.initial_state(q, h, w))
    xy, st, _ = ops.track_advance(fwd, bwd, state=(sxy, sst), start=start, frame0=0)
    return xy, st, fwd


@pytest.mark.parametrize("clips_per_step", [1, 8])
def test_track_points_is_predict_video_then_one_advance(dev, clips_per_step):
    from streamflow_amd import track
    frames = vc.random_frames(41, N, H, W)
    q = queries()
    for occlusion in (True, False):
        t = track.track_points(vc.stub_model, frames, q, T=T, clips_per_step=clips_per_step, occlusion=occlusion)
        xy, st, fwd = _compose(dev, frames, q, occlusion, clips_per_step=clips_per_step)
        assert torch.equal(t.xy[1:].permute(0, 2, 1).contiguous().view(torch.int32), xy.view(torch.int32))
        assert torch.equal(t.status[1:], st)
        # row 0: the queries, started or pending
        assert torch.equal(t.xy[0].cpu().contiguous().view(torch.int32), torch.from_numpy(q[:, 1:].copy()).view(torch.int32))
        started, inside = q[:, 0] <= 0, (q[:, 1] >= 0) & (q[:, 1] <= W - 1) & (q[:, 2] >= 0) & (q[:, 2] <= H - 1)
        assert np.array_equal(t.status[0].cpu().numpy(), np.where(started, np.where(inside, tc.VISIBLE, tc.LOST), tc.PENDING))
        # ... and the GPU rows are the restatement's, on the flows the model gave
        f = fwd.cpu().numpy()
        if not occlusion:
            want = tc.advance32(f, None, *tc.initial_state(q, H, W))
            assert np.array_equal(xy.cpu().numpy().view(np.uint32), want[0].view(np.uint32)) and np.array_equal(st.cpu().numpy(), want[1])
            assert not (t.status == tc.OCCLUDED).any()
        else:
            assert (t.status == tc.OCCLUDED).any()                      # the stand-in's two directions are not consistent everywhere


def test_size_goes_through(dev):
    from streamflow_amd import track
    frames = vc.random_frames(42, N, 48, 80)
    q = track.grid_queries((48, 80), 9)
    t = track.track_points(vc.stub_model, frames, q, T=T, clips_per_step=3, size=(40, 64))
    xy, st, fwd = _compose(dev, frames, q, True, clips_per_step=3, size=(40, 64))
    assert tuple(fwd.shape) == (N - 1, 2, 48, 80)                        # flows on the frames' own grid: tracks in original pixels
    assert torch.equal(t.xy[1:].permute(0, 2, 1).contiguous().view(torch.int32), xy.view(torch.int32)) and torch.equal(t.status[1:], st)


def test_dense_tracks_and_the_long_range_flow(dev):
    from streamflow_amd import ops, track, video
    frames = vc.random_frames(43, N, H, W)
    fwd, bwd = video.predict_video(vc.stub_model, frames, T=T, clips_per_step=2, bidirectional=True)
    for anchor, last in ((0, None), (3, 8)):
        d = track.dense_tracks(vc.stub_model, frames, anchor=anchor, last=last, T=T, clips_per_step=2)
        n = (N - 1 if last is None else last) - anchor
        assert tuple(d.xy.shape) == (n, 2, H, W) and tuple(d.status.shape) == (n, H, W)
        xy, st, _ = ops.track_advance(fwd[anchor:anchor + n], bwd[anchor:anchor + n], frame0=anchor)
        assert torch.equal(d.xy.view(n, 2, -1).view(torch.int32), xy.view(torch.int32)) and torch.equal(d.status.view(n, -1), st)
        # row 0: an integer position reads its own tap exactly, so it is float32(grid) + fwd bitwise wherever that lands inside
        gy, gx = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev), indexing="ij")
        grid = torch.stack([gx, gy])
        want = grid + fwd[anchor]
        inside = (want[0] >= 0) & (want[0] <= W - 1) & (want[1] >= 0) & (want[1] <= H - 1)
        assert torch.equal(d.xy[0][:, inside], want[:, inside]) and torch.equal(d.xy[0][:, ~inside], grid[:, ~inside])
        assert bool((d.status[0][~inside] == tc.LOST).all()) and bool((d.status[0][inside] <= tc.OCCLUDED).all()) and bool(inside.any())
        assert torch.equal(d.long_range_flow()[0][:, inside], (want - grid)[:, inside])
    with pytest.raises(MemoryError, match="bytes"):
        track.dense_tracks(vc.stub_model, frames, budget_bytes=1 << 10)


@pytest.mark.parametrize("clips_per_step", [1, 8])
def test_track_sink_with_emit_delivers_the_same_rows(dev, clips_per_step):
    from streamflow_amd import track, video
    frames = vc.random_frames(44, N, H, W)
    q = queries()
    t = track.track_points(vc.stub_model, frames, q, T=T, clips_per_step=clips_per_step, sticky=True)
    got = {}
    sink = track.TrackSink(q, (H, W), N, sticky=True, emit=lambda first, xy, st: got.update({first: (xy.clone(), st.clone())}))
    assert video.predict_video(vc.stub_model, frames, T=T, clips_per_step=clips_per_step, sink=sink, bidirectional=True) is None
    assert sorted(got)[0] == 0 and sink.xy is None
    xy = torch.cat([got[k][0] for k in sorted(got)])
    st = torch.cat([got[k][1] for k in sorted(got)])
    assert [k for k in sorted(got)] == list(np.cumsum([0] + [int(got[k][1].shape[0]) for k in sorted(got)])[:-1])
    assert torch.equal(xy.permute(0, 2, 1).contiguous().view(torch.int32), t.xy.contiguous().view(torch.int32)) and torch.equal(st, t.status)
    with pytest.raises(RuntimeError, match="not complete|nothing is kept"):
        sink.tracks()
    with pytest.raises(RuntimeError, match="bidirectional"):
        video.predict_video(vc.stub_model, frames, T=T, sink=track.TrackSink(q, (H, W), N))


def test_draw_wrapper_matches_the_restatement(dev):
    from streamflow_amd import track
    frames = vc.random_frames(45, N, H, W)
    t = track.track_points(shift_model, frames, queries(), T=T, occlusion=False)
    out = track.draw(frames[2:7].to(dev), t, first_frame=2, trail=5, radius=2)
    xy, st = (a.cpu().numpy() for a in t.planar())
    want = tc.draw32(frames[2:7].numpy(), 2, xy, st, 0, 5, 2, 1, track.default_palette(), track.alpha_fade(5))
    assert np.array_equal(out.cpu().numpy(), want) and (want != frames[2:7].numpy()).any()
    # channel-first frames, as a view
    chw = frames[2:7].to(dev).permute(0, 3, 1, 2)
    assert torch.equal(track.draw(chw.contiguous(), t, first_frame=2, trail=5, radius=2), out)


def test_command_line_writes_tracks_frames_and_video(tmp_path, dev):
    """python -m streamflow_amd.demo --track grid:24 --tracks-out --track-frames --track-video --report in a child process over six
    128 x 192 PNG frames, without --out: the .npz holds track_points' arrays for the same model and options in this process, the PNGs
    decode to track.draw's frames, the AVI passes tests/avi_walk.py and holds the JPEG streams of those frames."""
    from streamflow_amd import flow_io, jpeg_gpu, synthetic as syn, track
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
    cmd = [sys.executable, "-m", "streamflow_amd.demo", "--frames", str(tmp_path / "frames"), "--ckpt", ckpt, "--track", "grid:24",
           "--tracks-out", str(tmp_path / "tracks.npz"), "--track-frames", str(tmp_path / "drawn"), "--track-video", str(tmp_path / "drawn.avi"),
           "--track-trail", "4", "--track-radius", "2", "--report", "--iters", str(iters), "--fps", "12", "--jpeg-quality", "85"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "5 flow fields" in r.stdout and "Tracks points: 48, frames: 6" in r.stdout and "Consistency" not in r.stdout
    assert sorted(os.listdir(tmp_path / "drawn")) == ["track_%06d.png" % i for i in range(n)]
    model = StreamFlowT4(ckpt).to(dev).eval()
    q = track.grid_queries((Hd, Wd), 24)
    t = track.track_points(model, torch.from_numpy(frames), q, T=4, iters=iters, clips_per_step=8)
    with np.load(tmp_path / "tracks.npz") as z:
        assert sorted(z.files) == ["queries", "status", "xy"] and np.array_equal(z["queries"], q)
        assert np.array_equal(z["xy"].view(np.uint32), t.numpy().xy.view(np.uint32)) and np.array_equal(z["status"], t.numpy().status)
    want = track.draw(torch.from_numpy(frames).to(dev), t, 0, trail=4, radius=2)
    assert not torch.equal(want.cpu(), torch.from_numpy(frames))
    for i in range(n):
        assert np.array_equal(flow_io.read_png(str(tmp_path / "drawn" / ("track_%06d.png" % i))), want[i].cpu().numpy()), i
    info = avi_walk.walk(open(tmp_path / "drawn.avi", "rb").read())
    assert (info["width"], info["height"]) == (Wd, Hd) and len(info["frames"]) == n and info["rate"] / info["scale"] == 12
    assert [bytes(x) for x in info["frames"]] == [bytes(x) for x in jpeg_gpu.encode_batch(want, quality=85)]
