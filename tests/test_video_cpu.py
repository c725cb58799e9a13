"""The video path on the CPU side: the closed-form clip schedule and the batching against demo.group_clips, FrameDir on PNG files,
the argument checks of sf_frames_to_clips / sf_clips_to_flows (which run before any device is touched), and loud failure of
predict_video without a GPU or with bad arguments."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import video_cases as vc


@pytest.fixture(scope="module")
def lib():
    from streamflow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_schedule_equals_group_clips():
    """T = 2..7, n = T..79: clip starts, and (clip, slot) of every pair = the kept slots of group_clips in order."""
    from streamflow_amd import video
    from streamflow_amd.demo import group_clips
    for T in range(2, 8):
        for n in range(T, 80):
            sched = group_clips(n, T)
            assert video.clip_count(n, T) == len(sched)
            assert [video.clip_start(c, n, T) for c in range(len(sched))] == [s for s, _ in sched]
            want = [(c, k) for c, (_, keep) in enumerate(sched) for k in range(T - 1) if keep[k]]
            assert [video.pair_clip(j, n, T) for j in range(n - 1)] == want
            # every kept slot is the pair it claims to be
            assert [sched[c][0] + k for c, k in want] == list(range(n - 1))
    with pytest.raises(ValueError):
        video.clip_count(3, 4)
    with pytest.raises(ValueError):
        video.clip_start(2, 7, 4)
    with pytest.raises(ValueError):
        video.pair_clip(6, 7, 4)


def test_plan_batches_tiles_the_video():
    """clips_per_step = 1..9: the batches' clips are consecutive, every pair appears exactly once and in order, every clip's frames
    and every pair's clip lie inside the batch."""
    from streamflow_amd import video
    for T in range(2, 8):
        for n in range(T, 80):
            nc = video.clip_count(n, T)
            for cps in range(1, 10):
                plan = video.plan_batches(n, T, cps)
                assert len(plan) == -(-nc // cps)
                next_clip, pairs = 0, []
                for first, k, f_lo, f_hi, p_lo, p_hi in plan:
                    assert first == next_clip and 1 <= k <= cps and p_lo < p_hi
                    next_clip += k
                    for c in range(first, first + k):
                        s = video.clip_start(c, n, T)
                        assert f_lo <= s and s + T <= f_hi <= n
                    assert f_lo == video.clip_start(first, n, T)
                    for j in range(p_lo, p_hi):
                        assert first <= video.pair_clip(j, n, T)[0] < first + k
                    pairs += list(range(p_lo, p_hi))
                assert next_clip == nc and pairs == list(range(n - 1))
                assert all(k == cps for _, k, *_ in plan[:-1])
    with pytest.raises(ValueError, match="clips_per_step"):
        video.plan_batches(10, 4, 0)


def test_frame_dir_reads_grey_rgb_and_rgba(tmp_path):
    from streamflow_amd import flow_io, video
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, size=(9, 14, 3), dtype=np.uint8)
    grey = rng.integers(0, 256, size=(9, 14), dtype=np.uint8)
    rgba = rng.integers(0, 256, size=(9, 14, 4), dtype=np.uint8)
    flow_io.write_png(str(tmp_path / "f_0002.png"), rgba)                 # written out of order: the directory is sorted by name
    flow_io.write_png(str(tmp_path / "f_0000.png"), rgb)
    flow_io.write_png(str(tmp_path / "f_0001.png"), grey)
    (tmp_path / "notes.txt").write_text("not a frame")
    fd = video.FrameDir(str(tmp_path))
    assert len(fd) == 3 and fd.hw == (9, 14)
    for i, want in enumerate((rgb, np.repeat(grey[:, :, None], 3, axis=2), rgba[:, :, :3])):
        got = fd[i]
        assert got.dtype == np.uint8 and got.shape == (9, 14, 3) and got.flags["C_CONTIGUOUS"] and np.array_equal(got, want)
    assert np.array_equal(fd[-1], rgba[:, :, :3])
    with pytest.raises(IndexError):
        fd[3]
    assert len(video.FrameDir(str(tmp_path), pattern="f_000[01].png")) == 2
    with pytest.raises(FileNotFoundError):
        video.FrameDir(str(tmp_path), pattern="*.jpg")


def test_frame_dir_rejects_mixed_sizes(tmp_path):
    from streamflow_amd import flow_io, video
    flow_io.write_png(str(tmp_path / "a.png"), np.zeros((8, 12, 3), np.uint8))
    flow_io.write_png(str(tmp_path / "b.png"), np.zeros((8, 13, 3), np.uint8))
    with pytest.raises(ValueError, match="differs"):
        video.FrameDir(str(tmp_path))
    (tmp_path / "b.png").write_bytes(b"not a png at all, but long enough to hold a header")
    with pytest.raises(IOError, match="not a PNG"):
        video.FrameDir(str(tmp_path))


def _frames_call(lib, **kw):
    """sf_frames_to_clips on dummy, never dereferenced pointers: a video of 10 HWC frames of 36 x 52 held whole, clips of 4, pad to
    40 x 56; keywords override."""
    a = dict(frames=0x10000, fs=36 * 52 * 3, rs=52 * 3, ps=3, cs=1, frame0=0, n_buf=10, n=10, T=4, first_clip=0, n_clips=3, H=36, W=52,
             pad_top=2, pad_left=2, Hp=40, Wp=56, lut=0x20000, out=0x30000)
    a.update(kw)
    return lib.sf_frames_to_clips(a["frames"], a["fs"], a["rs"], a["ps"], a["cs"], a["frame0"], a["n_buf"], a["n"], a["T"], a["first_clip"],
                                  a["n_clips"], a["H"], a["W"], a["pad_top"], a["pad_left"], a["Hp"], a["Wp"], a["lut"], a["out"], None)


def test_frames_to_clips_rejects_bad_arguments(lib):
    for name in ("frames", "lut", "out"):
        assert _frames_call(lib, **{name: None}) == -1 and b"null" in lib.sf_last_error()
    assert _frames_call(lib, T=1) == -1 and b"T = 1" in lib.sf_last_error()
    assert _frames_call(lib, n=3, n_buf=3) == -1 and b"shorter than one clip" in lib.sf_last_error()
    assert _frames_call(lib, first_clip=1, n_clips=3) == -1 and b"of a video with 3" in lib.sf_last_error()
    assert _frames_call(lib, first_clip=-1) == -1 and _frames_call(lib, n_clips=0) == -1
    # the third clip starts at frame 6 (10 - 4) and needs frames 6..9
    assert _frames_call(lib, n_buf=9) == -1 and b"the buffer holds 0 .. 8" in lib.sf_last_error()
    assert _frames_call(lib, frame0=1, n_buf=9) == -1 and b"need frames 0 .. 9" in lib.sf_last_error()
    assert _frames_call(lib, first_clip=2, n_clips=1, frame0=7, n_buf=3) == -1 and b"need frames 6 .. 9" in lib.sf_last_error()
    assert _frames_call(lib, Hp=44, Wp=60) == -1 and b"multiple of 8" in lib.sf_last_error()
    assert _frames_call(lib, Hp=32) == -1 and b"smaller than the frame" in lib.sf_last_error()
    assert _frames_call(lib, pad_left=8) == -1 and b"smaller than the frame" in lib.sf_last_error()
    assert _frames_call(lib, pad_top=-1) == -1 and _frames_call(lib, H=0) == -1
    assert _frames_call(lib, rs=-156) == -1 and b"negative stride" in lib.sf_last_error()
    assert _frames_call(lib, out=0x30004) == -1 and b"aligned" in lib.sf_last_error()
    assert _frames_call(lib, n=70000, n_buf=70000, n_clips=22000) == -1 and b"65535" in lib.sf_last_error()


def _flows_call(lib, npairs_set=3, **kw):
    """sf_clips_to_flows on dummy pointers: the whole 10-frame video of above in one batch of 3 clips."""
    from streamflow_amd._lib import SfPairPtrs
    a = dict(clip=2 * 40 * 56, ch=40 * 56, row=56, n=10, T=4, first_clip=0, n_clips=3, pair0=0, n_pairs=9, H=36, W=52, pad_top=2,
             pad_left=2, out=0x30000)
    a.update(kw)
    ptrs = SfPairPtrs()
    for k in range(npairs_set):
        ptrs.p[k] = 0x40000 + 0x10000 * k
    return lib.sf_clips_to_flows(ctypes.byref(ptrs), a["clip"], a["ch"], a["row"], a["n"], a["T"], a["first_clip"], a["n_clips"],
                                 a["pair0"], a["n_pairs"], a["H"], a["W"], a["pad_top"], a["pad_left"], a["out"], None)


def test_clips_to_flows_rejects_bad_arguments(lib):
    assert lib.sf_clips_to_flows(None, 1, 1, 1, 10, 4, 0, 3, 0, 9, 36, 52, 2, 2, 0x30000, None) == -1 and b"null" in lib.sf_last_error()
    assert _flows_call(lib, out=None) == -1 and b"null" in lib.sf_last_error()
    assert _flows_call(lib, npairs_set=2) == -1 and b"null pointer for pair 2" in lib.sf_last_error()
    assert _flows_call(lib, T=10, n=20, npairs_set=8) == -2 and b"at most 8" in lib.sf_last_error()
    assert _flows_call(lib, T=1) == -1
    assert _flows_call(lib, n=3) == -1 and b"shorter than one clip" in lib.sf_last_error()
    assert _flows_call(lib, n_pairs=10) == -1 and b"of a video with 9" in lib.sf_last_error()
    assert _flows_call(lib, n_pairs=0) == -1 and _flows_call(lib, pair0=-1) == -1
    # pairs 6..8 belong to the tail clip 2
    assert _flows_call(lib, n_clips=2, n_pairs=7) == -1 and b"belong to clips 0 .. 2" in lib.sf_last_error()
    assert _flows_call(lib, first_clip=1, n_clips=2, pair0=2, n_pairs=7) == -1 and b"belong to clips 0 .. 2" in lib.sf_last_error()
    assert _flows_call(lib, first_clip=1, n_clips=3) == -1 and b"of a video with 3" in lib.sf_last_error()
    assert _flows_call(lib, row=53) == -1 and b"bad strides" in lib.sf_last_error()
    assert _flows_call(lib, H=0) == -1 and _flows_call(lib, pad_left=-1) == -1


def test_signatures_match_the_struct():
    from streamflow_amd import _lib, video
    assert ctypes.sizeof(_lib.SfPairPtrs) == 8 * ctypes.sizeof(ctypes.c_void_p) and len(_lib.SfPairPtrs().p) == video.MAX_PAIRS
    assert len(_lib.SIGNATURES["sf_frames_to_clips"][1]) == 20 and len(_lib.SIGNATURES["sf_clips_to_flows"][1]) == 16


def test_model_has_forward_normalised():
    import streamflow_amd as sfa
    assert sfa.SKFlow_MF8.default_iters == 12 and sfa.StreamFlowT4.default_iters == 15
    seen = {}

    class Probe(sfa.SKFlow_MF8):
        def __init__(self):                                              # no layers: only the call forwarding is looked at
            torch.nn.Module.__init__(self)

        def _forward_normalised(self, imgs, iters, flow_init, test_mode):
            seen.update(iters=iters, flow_init=flow_init, test_mode=test_mode)
            return ["flows"]

    assert Probe().forward_normalised(torch.zeros(1, 2, 3, 8, 8)) == ["flows"]
    assert seen == dict(iters=12, flow_init=None, test_mode=True)
    Probe().forward_normalised(torch.zeros(1, 2, 3, 8, 8), 5)
    assert seen["iters"] == 5


def test_predict_video_fails_loudly_without_a_gpu(monkeypatch):
    from streamflow_amd import ops, video
    frames = vc.random_frames(0, 6, 16, 24)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback.*predict_frames"):
        video.predict_video(vc.stub_model, frames)
    with pytest.raises(RuntimeError, match="predict_frames"):
        video.predict_video(vc.stub_model, list(frames), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frames_to_clips(frames, 6, 4, 0, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.clips_to_flows([torch.zeros(1, 2, 16, 24)] * 3, 6, 4, 0, 0, 3, (16, 24))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.norm_lut("cpu")


def test_predict_video_rejects_bad_arguments():
    """Every one of these is refused before the device is looked at (they raise the same way with and without a GPU)."""
    from streamflow_amd import video
    frames = vc.random_frames(0, 6, 16, 24)
    with pytest.raises(ValueError, match="at least T=4"):
        video.predict_video(vc.stub_model, frames[:3])
    with pytest.raises(TypeError, match="uint8"):
        video.predict_video(vc.stub_model, frames.float())
    with pytest.raises(TypeError, match="uint8"):
        video.predict_video(vc.stub_model, frames.numpy().astype(np.float32))
    with pytest.raises(TypeError, match="uint8"):
        video.predict_video(vc.stub_model, [f.float() for f in frames])
    with pytest.raises(ValueError, match=r"\[N, H, W, 3\]"):
        video.predict_video(vc.stub_model, frames[..., :2])
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        video.predict_video(vc.stub_model, [f.permute(2, 0, 1) for f in frames])
    mixed = list(frames)
    mixed[4] = mixed[4][:, :20]
    with pytest.raises(ValueError, match="frame 4 is"):
        video.predict_video(vc.stub_model, mixed)
    with pytest.raises(ValueError, match="clips_per_step"):
        video.predict_video(vc.stub_model, frames, clips_per_step=0)
    with pytest.raises(ValueError, match="at most 8 pairs"):
        video.predict_video(vc.stub_model, vc.random_frames(0, 12, 8, 8), T=10)
    with pytest.raises(TypeError, match="sequence"):
        video.predict_video(vc.stub_model, iter(list(frames)))


def test_restatement_is_the_frame_by_frame_pipeline():
    """tests/video_cases.py against demo.predict_frames on the host (normalised fp32 frames, one clip per call): the same fields."""
    from streamflow_amd.demo import predict_frames
    frames = vc.random_frames(3, 9, 19, 26)
    for T in (2, 3, 4):
        for mode in ("sintel", "kitti"):
            want = predict_frames(vc.stub_model, [vc.normalise(f.permute(2, 0, 1)) for f in frames], T=T, mode=mode)
            for cps in (1, 3):
                got = vc.flows(vc.stub_model, frames, T, mode, cps)
                assert got.shape == (8, 2, 19, 26) and torch.equal(got, torch.stack(want))
