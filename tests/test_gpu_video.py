"""The video path on the GPU: sf_frames_to_clips / sf_clips_to_flows (csrc/video_io.hip), video.predict_video and the command line
of streamflow_amd.demo against the torch restatement of the reference's read_video_and_group_predict (tests/video_cases.py).

Criterion: every comparison is BITWISE (torch.equal / np.array_equal).  The kernels move values and look them up in a table that
torch itself filled; nothing is rounded on the way, so there is no tolerance to choose.  Outputs sit between guard words that must
be intact afterwards."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import video_cases as vc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x7FC5A5A5                                                   # a NaN payload no computation produces
GUARD = 4096                                                            # floats on either side (a multiple of 4: the view stays 16-byte aligned)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _guarded(dev, shape):
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    return buf, buf[GUARD:GUARD + numel].view(shape)


def _guards_intact(buf):
    raw = buf.view(torch.int32)
    return bool((raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all())


def _written(view):
    return not bool((view.contiguous().view(torch.int32) == SENTINEL).any())


def test_every_byte_value_equals_the_device_expression(dev):
    """All 256 byte values, in every channel and in the pad columns: the clip holds exactly 2 * (x / 255.0) - 1.0 as the device
    computes it (whichever way its division by a scalar rounds)."""
    from streamflow_amd import ops
    vals = torch.arange(256, dtype=torch.uint8)
    frames = torch.stack([vals.view(8, 32, 1).expand(8, 32, 3), vals.flip(0).view(8, 32, 1).expand(8, 32, 3)]).contiguous().to(dev)
    got = ops.frames_to_clips(frames, 2, 2, 0, 1)
    want = (2 * (frames.float() / 255.0) - 1.0).permute(0, 3, 1, 2)[None]
    assert got.shape == (1, 2, 3, 8, 32) and torch.equal(got, want)
    lut = ops.norm_lut(dev)
    assert torch.equal(lut, 2 * (torch.arange(256, device=dev).float() / 255.0) - 1.0) and ops.norm_lut(dev) is lut
    assert torch.equal(got[0, 0, 0].reshape(-1), lut)


# (H, W, mode, channels_last, T, n, first_clip, n_clips (None: to the end), frames held from, odd byte offset)
FRAME_CASES = [
    (436, 1024, "sintel", True, 4, 8, 0, None, 0, False),                # tail clip; rows of 3072 bytes: dword loads
    (436, 1024, "kitti", False, 4, 7, 0, None, 0, False),                # CHW, no tail clip, all padding at the bottom
    (436, 1024, "sintel", True, 3, 6, 0, None, 0, True),                 # the same rows one byte off: byte loads
    (375, 1242, "kitti", True, 3, 7, 0, None, 0, False),                 # pad left 3: unaligned interior, 3 W = 3726
    (375, 1242, "kitti", False, 2, 4, 1, 2, 1, True),
    (37, 53, "sintel", True, 2, 5, 0, None, 0, False),                   # W % 4 = 1
    (37, 53, "sintel", False, 4, 9, 1, 2, 3, False),                     # clips 1 and 2 (the tail) from a buffer holding frames 3..8
    (37, 53, "kitti", True, 4, 9, 1, 1, 2, True),
    (30, 50, "sintel", True, 3, 8, 2, 2, 4, False),                      # W % 4 = 2, middle clips, frames 4..7 held
    (40, 64, "sintel", True, 4, 10, 0, None, 0, False),                  # no padding at all
    (8, 8, "sintel", True, 2, 2, 0, None, 0, False),
]


@pytest.mark.parametrize("case", FRAME_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_frames_to_clips_matches_the_restatement(dev, case):
    from streamflow_amd import ops, video
    from streamflow_amd.utils import InputPadder
    H, W, mode, channels_last, T, n, first, n_clips, held_from, odd = case
    nc = video.clip_count(n, T)
    n_clips = nc - first if n_clips is None else n_clips
    frames = vc.random_frames(H * 7 + W + T, n, H, W).to(dev)             # [n, H, W, 3]
    want = vc.clips(frames, T, mode)[first:first + n_clips]
    held_to = video.clip_start(first + n_clips - 1, n, T) + T
    assert held_from <= video.clip_start(first, n, T)
    part = frames[held_from:held_to]
    part = part.contiguous() if channels_last else part.permute(0, 3, 1, 2).contiguous()
    if odd:                                                              # the same bytes in a view that starts at an odd address
        raw = torch.empty(part.numel() + 1, dtype=torch.uint8, device=dev)
        raw[1:].copy_(part.reshape(-1))
        part = raw[1:].view(part.shape)
        assert part.data_ptr() % 2 == 1
    pad = InputPadder((H, W), mode=mode)._pad
    buf, out = _guarded(dev, want.shape)
    got = ops.frames_to_clips(part, n, T, first, n_clips, pad, frame0=held_from, channels_last=channels_last, out=out)
    assert got is out and _written(out)
    assert torch.equal(out, want), f"{int((out != want).sum())} of {want.numel()} values differ"
    assert _guards_intact(buf)
    if not odd:                                                          # without `out`: a fresh tensor, the same values
        assert torch.equal(ops.frames_to_clips(part, n, T, first, n_clips, pad, frame0=held_from, channels_last=channels_last), want)


def test_frames_to_clips_takes_strided_views(dev):
    """A crop of larger frames (row and frame strides of the parent) and frames with a channel stride of 2 (BGRA-like storage)."""
    from streamflow_amd import ops
    big = vc.random_frames(5, 6, 50, 70).to(dev)
    crop = big[:, 5:45, 3:67]                                            # [6, 40, 64, 3], strides of the parent
    assert not crop.is_contiguous()
    assert torch.equal(ops.frames_to_clips(crop, 6, 4, 0, 2), vc.clips(crop.contiguous(), 4, "sintel"))
    wide = torch.zeros(6, 40, 64, 6, dtype=torch.uint8, device=dev)
    wide[..., ::2] = crop
    assert torch.equal(ops.frames_to_clips(wide[..., ::2], 6, 4, 0, 2), vc.clips(crop.contiguous(), 4, "sintel"))


def test_wrappers_reject_bad_tensors(dev):
    from streamflow_amd import ops
    frames = vc.random_frames(0, 6, 16, 24).to(dev)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.frames_to_clips(frames.float(), 6, 4, 0, 2)
    with pytest.raises(RuntimeError, match="channel dimension"):
        ops.frames_to_clips(frames, 6, 4, 0, 2, channels_last=False)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.frames_to_clips(frames, 6, 4, 0, 2, out=torch.empty(2, 4, 3, 16, 16, device=dev))
    with pytest.raises(RuntimeError, match="need frames 2 .. 5"):
        ops.frames_to_clips(frames[:5], 6, 4, 1, 1)
    pairs = [torch.zeros(2, 2, 16, 24, device=dev) for _ in range(3)]
    with pytest.raises(RuntimeError, match="pair tensors for clips"):
        ops.clips_to_flows(pairs[:2], 6, 4, 0, 0, 5, (16, 24))
    with pytest.raises(RuntimeError, match="differ in shape"):
        ops.clips_to_flows(pairs[:2] + [torch.zeros(1, 2, 16, 24, device=dev)], 6, 4, 0, 0, 5, (16, 24))
    with pytest.raises(RuntimeError, match="is not the pair tensors'"):
        ops.clips_to_flows(pairs, 6, 4, 0, 0, 5, (16, 20))
    with pytest.raises(RuntimeError, match="belong to clips 0 .. 1"):
        ops.clips_to_flows([p[:1] for p in pairs], 6, 4, 0, 0, 5, (16, 24))
    with pytest.raises(RuntimeError, match="contiguous rows"):
        ops.clips_to_flows([p.half() for p in pairs], 6, 4, 0, 0, 5, (16, 24))


# (H, W, mode, T, n, first_clip, n_clips, extra rows / columns of the allocation the pair tensors are views of, view offset)
FLOW_CASES = [
    (436, 1024, "sintel", 4, 8, 0, 3, (0, 0), (0, 0)),                   # the model's own layout: float4 both ways; ends in the tail clip
    (436, 1024, "sintel", 4, 11, 1, 2, (2, 8), (1, 4)),                  # views of a larger allocation, still 16-byte aligned
    (436, 1024, "sintel", 3, 9, 0, 4, (3, 5), (2, 3)),                   # odd row stride and offset: scalar loads, float4 stores
    (375, 1242, "kitti", 3, 8, 2, 2, (0, 0), (0, 0)),                    # pad left 3, W % 4 = 2: scalar both ways; tail clip
    (37, 53, "sintel", 4, 9, 0, 3, (1, 3), (1, 1)),
    (37, 53, "kitti", 2, 5, 1, 3, (0, 0), (0, 0)),
    (30, 52, "sintel", 9, 12, 0, 2, (0, 0), (0, 0)),                     # eight pairs per clip (the most); pad left 2: scalar loads
    (40, 64, "sintel", 4, 10, 0, 3, (0, 4), (0, 4)),
]


@pytest.mark.parametrize("case", FLOW_CASES, ids=lambda c: "-".join(str(x) for x in c).replace(" ", ""))
def test_clips_to_flows_matches_slicing(dev, case):
    from streamflow_amd import ops, video
    from streamflow_amd.utils import InputPadder
    H, W, mode, T, n, first, n_clips, extra, off = case
    left, right, top, bottom = pad = InputPadder((H, W), mode=mode)._pad
    Hp, Wp = H + top + bottom, W + left + right
    g = torch.Generator().manual_seed(H + W + T + n)
    alloc = [torch.randn(n_clips, 2, Hp + extra[0], Wp + extra[1], generator=g).to(dev) for _ in range(T - 1)]
    pairs = [a[:, :, off[0]:off[0] + Hp, off[1]:off[1] + Wp] for a in alloc]
    assert extra == (0, 0) or not pairs[0].is_contiguous()
    assert first + n_clips <= video.clip_count(n, T)
    p_lo, p_hi = first * (T - 1), min((first + n_clips) * (T - 1), n - 1)         # the pairs this batch of clips produces
    want = []
    for j in range(p_lo, p_hi):
        c, k = video.pair_clip(j, n, T)
        want.append(pairs[k][c - first][:, top:top + H, left:left + W])
    want = torch.stack(want)
    buf, out = _guarded(dev, want.shape)
    got = ops.clips_to_flows(pairs, n, T, first, p_lo, p_hi - p_lo, (H, W), pad, out=out)
    assert got is out and _written(out) and torch.equal(out, want) and _guards_intact(buf)
    # a sub-range of the pairs, into a fresh tensor
    if p_hi - p_lo > 2:
        assert torch.equal(ops.clips_to_flows(pairs, n, T, first, p_lo + 1, p_hi - p_lo - 2, (H, W), pad), want[1:-1])


@pytest.mark.parametrize("clips_per_step", [1, 3, 8])
def test_predict_video_with_a_stub_model(dev, clips_per_step):
    """Host and device frames, HWC and CHW, a list of frames; with and without a sink: all the restatement's flows."""
    from streamflow_amd import video
    H, W, T, n = 60, 90, 4, 11                                            # 4 clips, the last one a tail clip
    frames = vc.random_frames(21, n, H, W)
    for mode in ("sintel", "kitti"):
        want = vc.flows(vc.stub_model, frames.to(dev), T, mode, clips_per_step)
        assert want.shape == (n - 1, 2, H, W)
        chw = frames.permute(0, 3, 1, 2).contiguous()
        for name, src in (("host", frames), ("device", frames.to(dev)), ("numpy", frames.numpy()), ("host chw", chw),
                          ("device chw", chw.to(dev)), ("list", list(frames.numpy())), ("device list", list(frames.to(dev)))):
            got = video.predict_video(vc.stub_model, src, T=T, clips_per_step=clips_per_step, mode=mode)
            assert got.device == dev and got.dtype == torch.float32 and torch.equal(got, want), (mode, name)
        calls = []
        res = video.predict_video(vc.stub_model, frames, T=T, clips_per_step=clips_per_step, mode=mode,
                                  sink=lambda first, f: calls.append((first, f)))
        assert res is None and [c[0] for c in calls] == [b[4] for b in video.plan_batches(n, T, clips_per_step)]
        assert torch.equal(torch.cat([c[1] for c in calls]), want)
    # other clip lengths, a video without a tail clip
    for T2, n2 in ((2, 5), (3, 7), (5, 11)):
        f2 = vc.random_frames(T2, n2, 33, 47)
        assert torch.equal(video.predict_video(vc.stub_model, f2, T=T2, clips_per_step=clips_per_step),
                           vc.flows(vc.stub_model, f2.to(dev), T2, "sintel", clips_per_step))


def test_predict_video_with_the_model(dev):
    """SKFlow_MF8 with the patch encoder on seeded synthetic weights, 132 x 196 frames (padded to 136 x 200), T = 3, 8 frames: four
    clips, the last one a tail clip.  The model must be repeatable on a batch first; then predict_video equals the restatement
    driving the same forward_normalised calls (clips_per_step = 3: batches of 3 and 1), and at one clip per call equals
    demo.predict_frames given the device-normalised frames."""
    from streamflow_amd import synthetic as syn, video
    from streamflow_amd.demo import predict_frames
    from streamflow_amd.model import SKFlow_MF8, default_args
    H, W, T, n, iters = 132, 196, 3, 8, 3
    model = SKFlow_MF8(default_args(T=T, Encoder="PatchEncoder")).to(dev)
    model.load_state_dict(dict(syn.make_params(41, T)), strict=True)
    frames = vc.random_frames(8, n, H, W)
    batch = vc.clips(frames.to(dev), T, "sintel")[:3].contiguous()
    first, second = model.forward_normalised(batch, iters), model.forward_normalised(batch, iters)
    assert len(first) == T - 1 and first[0].shape == (3, 2, 136, 200)
    for a, b in zip(first, second):
        assert torch.equal(a, b), "the model is not repeatable on one batch"
    assert torch.isfinite(first[0]).all() and float(first[0].abs().max()) > 0
    call = lambda imgs: model.forward_normalised(imgs, iters)
    got3 = video.predict_video(model, frames, T=T, iters=iters, clips_per_step=3)
    assert got3.shape == (n - 1, 2, H, W) and torch.equal(got3, vc.flows(call, frames.to(dev), T, "sintel", 3))
    assert torch.equal(video.predict_video(model, frames.to(dev), T=T, iters=iters, clips_per_step=3), got3)
    got1 = video.predict_video(model, frames, T=T, iters=iters, clips_per_step=1)
    normalised = [vc.normalise(f.permute(2, 0, 1)) for f in frames.to(dev)]
    want1 = predict_frames(call, normalised, T=T, device=dev)
    assert torch.equal(got1.cpu(), torch.stack(want1))
    # iters=None is the class's default
    default, twelve = model.forward_normalised(batch), model.forward_normalised(batch, 12)
    assert len(default) == len(twelve) == T - 1 and all(torch.equal(a, b) for a, b in zip(default, twelve))


def test_command_line_writes_the_flows_of_predict_video(tmp_path, dev):
    """python -m streamflow_amd.demo over six 124 x 188 PNG frames and a checkpoint saved from a seeded StreamFlowT4 (Twins_CSC
    encoders): five colour PNGs and five .flo files that decode to what a direct predict_video call returns in this process."""
    from streamflow_amd import flow_io, synthetic as syn, video
    from streamflow_amd.demo import colour_images
    from streamflow_amd.model import StreamFlowT4
    H, W, n, iters = 124, 188, 6, 3
    frames = vc.random_frames(5, n, H, W).numpy()
    os.makedirs(tmp_path / "frames")
    for i, f in enumerate(frames):
        flow_io.write_png(str(tmp_path / "frames" / ("%04d.png" % i)), f if i != 2 else f[:, :, 0])       # one grey frame
    frames[2] = frames[2][:, :, :1]
    sd = dict(syn.make_params(51, 4))
    sd.update({"fnet." + k: v for k, v in syn.make_twins_params(52).items()})
    sd.update({"cnet." + k: v for k, v in syn.make_twins_params(53).items()})
    ckpt = str(tmp_path / "ckpt.pth")
    torch.save({"model": {"module." + k: v for k, v in sd.items()}}, ckpt)
    cmd = [sys.executable, "-m", "streamflow_amd.demo", "--frames", str(tmp_path / "frames"), "--ckpt", ckpt, "--out",
           str(tmp_path / "png"), "--flo", str(tmp_path / "flo"), "--iters", str(iters), "--clips-per-step", "8"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "5 flow fields" in r.stdout
    assert sorted(os.listdir(tmp_path / "png")) == ["frame_%04d.png" % i for i in range(n - 1)]
    assert sorted(os.listdir(tmp_path / "flo")) == ["frame_%04d.flo" % i for i in range(n - 1)]
    model = StreamFlowT4(ckpt).to(dev).eval()
    want = video.predict_video(model, video.FrameDir(str(tmp_path / "frames")), T=4, iters=iters, clips_per_step=8)
    assert want.shape == (n - 1, 2, H, W) and torch.isfinite(want).all()
    assert torch.equal(want, video.predict_video(model, torch.from_numpy(frames), T=4, iters=iters, clips_per_step=8))
    images = colour_images(list(want))
    for i in range(n - 1):
        flo = flow_io.read_flo(str(tmp_path / "flo" / ("frame_%04d.flo" % i)))
        assert np.array_equal(flo, want[i].permute(1, 2, 0).cpu().numpy()), i
        assert np.array_equal(flow_io.read_png(str(tmp_path / "png" / ("frame_%04d.png" % i))), images[i]), i
