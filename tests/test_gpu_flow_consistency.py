"""sf_flow_consistency / sf_warp_frames (csrc/flow_consistency.hip) through the C ABI with raw strides and guard bands, the ops
wrappers, video.predict_video(bidirectional=True), consistency.video_report and the demo's --occlusion / --warp output.

Criteria.  Class bytes and warped bytes: BITWISE the numpy float32 restatement's (tests/consistency_cases.py; its agreement with an
independent float64 formulation is tests/test_consistency_cases_cpu.py).  Counts: exactly equal.  The fp64 sums: within
terms * 2^-52 relative of numpy's fp64 sum of the same float32 terms -- the terms are non-negative, so two orders of summation differ by
at most (terms - 1) * 2^-53 relative each.  Flows of predict_video: bitwise.  Operands are placed in NaN-filled allocations, outputs
between sentinel bands; everything outside the views must come back unchanged.  NaN, Inf and huge flows are ordinary inputs with
defined results (class outside, byte 0): nothing here is meant to fault."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import consistency_cases as cc
from tests import video_cases as vc
from tests.guarded import GuardedBytes

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 7), (5, 1), (13, 37), (17, 65), (33, 130)]
BAND, SENT = 512, 0x5A


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from streamflow_amd import _lib
    return _lib.load()


class Bytes:
    """`size` bytes holding SENT between two bands of BAND sentinel bytes, `shift` bytes off the allocation's alignment."""

    def __init__(self, dev, size, shift=0):
        self.lo, self.size = BAND + shift, size
        self.buf = torch.full((self.lo + size + BAND,), SENT, dtype=torch.uint8, device=dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo

    def view(self):
        return self.buf[self.lo:self.lo + self.size]

    def bands_intact(self):
        return bool((self.buf[:self.lo] == SENT).all() and (self.buf[self.lo + self.size:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


class Rows:
    """Stats rows float64 [n, length] holding `start` between two bands of sentinel doubles."""

    def __init__(self, dev, n, length, start=0.0):
        self.buf = torch.full((8 + n * length + 8,), 777.25, dtype=torch.float64, device=dev)
        self.rows = self.buf[8:8 + n * length].view(n, length)
        self.rows.fill_(start)

    @property
    def ptr(self):
        return self.rows.data_ptr()

    def bands_intact(self):
        return bool((self.buf[:8] == 777.25).all() and (self.buf[-8:] == 777.25).all())


def _bits_equal(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def _frames(arr_hwc, dev, chw_odd):
    """uint8 [n, h, w, 3] -> (device tensor keeping the allocation alive, ptr, byte strides (frame, row, px, ch))."""
    t = torch.from_numpy(arr_hwc)
    n, h, w, _ = t.shape
    if not chw_odd:
        d = t.contiguous().to(dev)
        return d, d.data_ptr(), (3 * h * w, 3 * w, 3, 1)
    raw = torch.full((3 + t.numel() + 8,), 0xEE, dtype=torch.uint8, device=dev)
    raw[3:3 + t.numel()].copy_(t.permute(0, 3, 1, 2).contiguous().reshape(-1).to(dev))
    return raw, raw.data_ptr() + 3, (3 * h * w, w, 1, h * w)


def run_case(lib, dev, fwd, bwd, src, ref, strided, codes=(0, 1, 2), alpha=cc.ALPHA, beta=cc.BETA, start=0.0):
    """Both entry points through the C ABI on one case; returns what they wrote and asserts every guard."""
    n, _, h, w = fwd.shape
    pad, base = (3, 1) if strided else (0, 0)
    fbuf, fv = cc.place(torch.from_numpy(fwd), dev, pad, base)
    bbuf, bv = cc.place(torch.from_numpy(bwd), dev, pad, base)
    fsnap, bsnap = fbuf.clone(), bbuf.clone()
    assert (fv.data_ptr() % 16 != 0) == strided
    cls = Bytes(dev, n * h * w, shift=1 if strided else 0)
    stats = Rows(dev, n, cc.LEN, start)
    ws = GuardedBytes(dev, lib.sf_flow_consistency_ws_bytes(n, h, w), guard=4096)
    st = lib.sf_flow_consistency(fv.data_ptr(), fv.stride(0), fv.stride(1), fv.stride(2), bv.data_ptr(), bv.stride(0), bv.stride(1),
                                 bv.stride(2), n, h, w, alpha, beta, codes[0], codes[1], codes[2], cls.ptr, stats.ptr, ws.ptr, ws.size,
                                 torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.sf_last_error()
    skeep, sptr, ss = _frames(src, dev, strided)
    rkeep, rptr, rs = _frames(ref, dev, strided)
    out = Bytes(dev, n * h * w * 3, shift=1 if strided else 0)
    wstats = Rows(dev, n, 2, start)
    wws = GuardedBytes(dev, lib.sf_warp_frames_ws_bytes(n, h, w), guard=4096)
    st = lib.sf_warp_frames(sptr, ss[0], ss[1], ss[2], ss[3], fv.data_ptr(), fv.stride(0), fv.stride(1), fv.stride(2), n, h, w, out.ptr,
                            cls.ptr, codes[0], rptr, rs[0], rs[1], rs[2], rs[3], wstats.ptr, wws.ptr, wws.size,
                            torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.sf_last_error()
    plain = Bytes(dev, n * h * w * 3, shift=1 if strided else 0)          # without the optional arguments: the same bytes
    st = lib.sf_warp_frames(sptr, ss[0], ss[1], ss[2], ss[3], fv.data_ptr(), fv.stride(0), fv.stride(1), fv.stride(2), n, h, w, plain.ptr,
                            None, 0, None, 0, 0, 0, 0, None, None, 0, torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.sf_last_error()
    torch.cuda.synchronize()
    assert _bits_equal(fbuf, fsnap) and _bits_equal(bbuf, bsnap), "an operand was written"
    assert cls.bands_intact() and out.bands_intact() and plain.bands_intact() and stats.bands_intact() and wstats.bands_intact()
    assert ws.guards_unchanged() and wws.guards_unchanged()
    assert torch.equal(out.view(), plain.view())
    return (cls.view().view(n, h, w).cpu().numpy(), stats.rows.cpu().numpy(), out.view().view(n, h, w, 3).cpu().numpy(),
            wstats.rows.cpu().numpy())


def check_against_restatement(got, fwd, bwd, src, ref, codes=(0, 1, 2), start=0.0, calls=1):
    cls, stats, warped, wstats = got
    want_cls, want_stats, _, _ = cc.restate32(fwd, bwd, codes=codes)
    want_warped, want_wstats = cc.warp32(src, fwd, want_cls, ref, visible=codes[0])
    assert np.array_equal(cls, want_cls), f"{int((cls != want_cls).sum())} of {cls.size} class bytes differ"
    assert np.array_equal(warped, want_warped), f"{int((warped != want_warped).sum())} of {warped.size} warped bytes differ"
    n, h, w = cls.shape
    for i in range(n):
        for k in (cc.PIXELS, cc.VISIBLE, cc.OCCLUDED, cc.OUTSIDE, cc.FINITE):
            assert stats[i, k] == start + calls * want_stats[i, k], (i, k, stats[i], want_stats[i])
        assert wstats[i, 1] == start + calls * want_wstats[i, 1], (i, wstats[i], want_wstats[i])
        if start == 0.0 and calls == 1:
            for g, wnt, terms in ((stats[i, cc.SUM_FB], want_stats[i, cc.SUM_FB], want_stats[i, cc.VISIBLE]),
                                  (stats[i, cc.SUM_MAG], want_stats[i, cc.SUM_MAG], want_stats[i, cc.FINITE]),
                                  (wstats[i, 0], want_wstats[i, 0], want_wstats[i, 1])):
                print(f"field {i}: sum {g!r} vs {wnt!r}, terms {terms}")
                assert abs(g - wnt) <= terms * 2.0 ** -52 * abs(wnt), (i, g, wnt, terms)


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("n", [1, 3, 25])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "%dx%d" % s)
def test_kernels_match_the_restatement_bitwise(lib, dev, hw, n, strided):
    h, w = hw
    fwd, bwd, src, ref = cc.make_case(100 + h + w, n, h, w)
    check_against_restatement(run_case(lib, dev, fwd, bwd, src, ref, strided), fwd, bwd, src, ref)


def _special_case():
    h, w = 6, 12
    fwd, bwd, src, ref = cc.make_case(7, 2, h, w)
    fwd *= np.float32(0.1)
    bwd *= np.float32(0.1)
    for x, bad in enumerate([np.nan, np.inf, -np.inf, 1e30, -1e30]):
        fwd[0, 0, 0, x] = bad
        fwd[0, 1, 1, x] = bad
        fwd[1, :, 2, x] = bad
    fwd[0, :, 3, 0] = (w - 1, 0.0)                                       # exactly on the last column
    fwd[0, :, 3, 1] = (0.0, 2.0)                                         # exactly on the last row
    fwd[0, :, 4, 0] = (-0.0, -0.0)
    fwd[0, :, 4, w - 1] = (0.0, 1.0)                                     # the last corner
    bwd[0, :, 3, w - 1] = (-(w - 1), 0.0)
    bwd[0, :, h - 1, 1] = (0.0, -2.0)
    bwd[0, :, h - 1, w - 1] = (-0.0, -1.0)
    fwd[1, :, 4, 4] = (0.0, 0.0)
    bwd[1, 0, 4, 4] = np.nan                                             # a NaN tap: occluded
    return fwd, bwd, src, ref


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
def test_special_values_have_defined_results(lib, dev, strided):
    fwd, bwd, src, ref = _special_case()
    got = run_case(lib, dev, fwd, bwd, src, ref, strided)
    check_against_restatement(got, fwd, bwd, src, ref)
    cls, stats, warped, _ = got
    assert (cls[0, 0, :5] == 2).all() and (cls[0, 1, :5] == 2).all() and (cls[1, 2, :5] == 2).all()
    assert not warped[0, 0, :5].any() and not warped[0, 1, :5].any() and not warped[1, 2, :5].any()
    assert cls[0, 3, 0] == 0 and cls[0, 3, 1] == 0 and cls[0, 4, 0] != 2 and cls[0, 4, 11] == 0
    assert (warped[0, 3, 0] == src[0, 3, 11]).all() and (warped[0, 3, 1] == src[0, 5, 1]).all() and (warped[0, 4, 11] == src[0, 5, 11]).all()
    assert cls[1, 4, 4] == 1
    assert stats[0, cc.FINITE] == 6 * 12 - 10 and np.isfinite(stats).all()


def test_custom_codes_accumulation_and_repeatability(lib, dev):
    fwd, bwd, src, ref = cc.make_case(150, 3, 17, 65)
    first = run_case(lib, dev, fwd, bwd, src, ref, False, codes=(255, 0, 128))
    check_against_restatement(first, fwd, bwd, src, ref, codes=(255, 0, 128))
    assert set(np.unique(first[0])) == {0, 128, 255}
    again = run_case(lib, dev, fwd, bwd, src, ref, False, codes=(255, 0, 128))
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes(), "two runs differ"
    # rows are ADDED to: a start value of 1000 in every entry, and a second call on the same rows through the wrapper
    check_against_restatement(run_case(lib, dev, fwd, bwd, src, ref, True, start=1000.0), fwd, bwd, src, ref, start=1000.0)
    from streamflow_amd import ops
    f, b = torch.from_numpy(fwd).to(dev), torch.from_numpy(bwd).to(dev)
    cls, stats = ops.flow_consistency(f, b)
    once = stats.clone()
    cls2, stats2 = ops.flow_consistency(f, b, stats=stats)
    assert stats2 is stats and torch.equal(cls, cls2)
    counts = [cc.PIXELS, cc.VISIBLE, cc.OCCLUDED, cc.OUTSIDE, cc.FINITE]
    assert torch.equal(stats[:, counts], 2 * once[:, counts]) and torch.equal(stats[:, [cc.SUM_FB, cc.SUM_MAG]], once[:, [cc.SUM_FB, cc.SUM_MAG]] * 2)
    assert np.array_equal(once.cpu().numpy(), first[1])


def test_bad_arguments_write_nothing(lib, dev):
    n, h, w = 2, 9, 20
    fwd = torch.zeros(n, 2, h, w, device=dev)
    cls, out = Bytes(dev, n * h * w), Bytes(dev, n * h * w * 3)
    stats, ws = Rows(dev, n, cc.LEN), Bytes(dev, 1 << 16)
    src = torch.zeros(n, h, w, 3, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    ok = dict(fwd=fwd.data_ptr(), fr=w, n=n, h=h, w=w, cls=cls.ptr, stats=stats.ptr, ws=ws.ptr, ws_bytes=ws.size, alpha=0.01)

    def fbc(**kw):
        a = dict(ok, **kw)
        return lib.sf_flow_consistency(a["fwd"], 2 * h * w, h * w, a["fr"], fwd.data_ptr(), 2 * h * w, h * w, w, a["n"], a["h"], a["w"],
                                       a["alpha"], 0.5, 0, 1, 2, a["cls"], a["stats"], a["ws"], a["ws_bytes"], s)

    for bad in (dict(fwd=None), dict(cls=None), dict(stats=None), dict(ws=None), dict(n=0), dict(n=65536), dict(h=0), dict(w=0),
                dict(fr=w - 1), dict(ws_bytes=lib.sf_flow_consistency_ws_bytes(n, h, w) - 1), dict(alpha=float("nan"))):
        assert fbc(**bad) == -1, bad

    def warp(**kw):
        a = dict(dict(src=src.data_ptr(), out=out.ptr, cls=None, ref=None, stats=None, ws=None, ws_bytes=0, n=n, fr=w), **kw)
        return lib.sf_warp_frames(a["src"], 3 * h * w, 3 * w, 3, 1, fwd.data_ptr(), 2 * h * w, h * w, a["fr"], a["n"], h, w, a["out"],
                                  a["cls"], 0, a["ref"], 3 * h * w, 3 * w, 3, 1, a["stats"], a["ws"], a["ws_bytes"], s)

    for bad in (dict(src=None), dict(out=None), dict(n=0), dict(fr=w - 1), dict(cls=cls.ptr), dict(ref=src.data_ptr()),
                dict(cls=cls.ptr, ref=src.data_ptr()), dict(cls=cls.ptr, ref=src.data_ptr(), stats=stats.ptr, ws=ws.ptr, ws_bytes=8)):
        assert warp(**bad) == -1, bad
    torch.cuda.synchronize()
    assert cls.untouched() and out.untouched() and ws.untouched() and bool((stats.rows == 0).all()) and stats.bands_intact()
    # ... and the good calls do write
    assert fbc() == 0 and warp() == 0
    torch.cuda.synchronize()
    assert bool((cls.view() == 0).all()) and bool((out.view() == 0).all()) and float(stats.rows[0, cc.VISIBLE]) == h * w


def test_wrappers_take_hwc_and_chw_frames_and_views(dev):
    from streamflow_amd import consistency, ops
    n, h, w = 3, 17, 65
    fwd, bwd, src, ref = cc.make_case(11, n, h, w)
    want_cls, want_stats, _, _ = cc.restate32(fwd, bwd, codes=(255, 0, 128))
    want_warped, want_w = cc.warp32(src, fwd, want_cls, ref, visible=255)
    f, b = torch.from_numpy(fwd).to(dev), torch.from_numpy(bwd).to(dev)
    s, r = torch.from_numpy(src).to(dev), torch.from_numpy(ref).to(dev)
    _, fview = cc.place(f, dev, 3, 1)                                    # a view with odd strides
    for ff in (f, fview):
        cls, stats = ops.flow_consistency(ff, b, codes=(255, 0, 128))
        assert cls.dtype == torch.uint8 and np.array_equal(cls.cpu().numpy(), want_cls)
        assert np.array_equal(stats.cpu().numpy()[:, :4], want_stats[:, :4])
        for frames, refs, cl in ((s, r, None), (s.permute(0, 3, 1, 2).contiguous(), r.permute(0, 3, 1, 2).contiguous(), False),
                                 (s.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1), r, None)):
            warped, ws = ops.warp_frames(frames, ff, cls=cls, ref=refs, channels_last=cl, visible=255)
            assert np.array_equal(warped.cpu().numpy(), want_warped)
            assert ws[:, 1].cpu().tolist() == want_w[:, 1].tolist()
            plain, none = ops.warp_frames(frames, ff, channels_last=cl)
            assert none is None and torch.equal(plain, warped)
    # consistency.check_pairs: the second direction is the kernel with the arguments swapped; warp_back slices the frames
    (cf, sf_), (cb, sb) = consistency.check_pairs(f, b)
    assert np.array_equal(cf.cpu().numpy(), cc.restate32(fwd, bwd)[0]) and np.array_equal(cb.cpu().numpy(), cc.restate32(bwd, fwd)[0])
    video = torch.from_numpy(np.concatenate([ref[:1], src])).to(dev)     # n + 1 frames
    wb, st = consistency.warp_back(video, f, cf)
    assert np.array_equal(wb.cpu().numpy(), cc.warp32(video[1:].cpu().numpy(), fwd)[0]) and st.shape == (n, 2)
    wr, _ = consistency.warp_back(video, b, reverse=True)
    assert np.array_equal(wr.cpu().numpy(), cc.warp32(video[:-1].cpu().numpy(), bwd)[0])
    with pytest.raises(RuntimeError, match="fp32"):
        ops.flow_consistency(f.double(), b)
    with pytest.raises(RuntimeError, match="bwd"):
        ops.flow_consistency(f, b[:2])
    with pytest.raises(RuntimeError, match="come together"):
        ops.warp_frames(s, f, cls=cf)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.warp_frames(s.float(), f)
    with pytest.raises(RuntimeError, match="frames of"):
        ops.warp_frames(s[:2], f)


def backward_flows(call, frames_hwc, T, mode, clips_per_step):
    """The definition of predict_video's bwd: the forward schedule's clips, reversed in time, `clips_per_step` per call; the outputs
    of a reversed clip in reversed order are the backward flows of the forward clip's pairs."""
    n = frames_hwc.shape[0]
    all_clips = vc.clips(frames_hwc, T, mode)
    _, padder = vc.padded_frames(frames_hwc[:1], mode)
    fields = []
    for first in range(0, all_clips.shape[0], clips_per_step):
        outs = list(call(all_clips[first:first + clips_per_step].flip(1).contiguous()))[::-1]
        fields += vc.kept(outs, first, n, T, padder)
    return torch.stack(fields)


@pytest.mark.parametrize("clips_per_step", [1, 3, 8])
def test_bidirectional_predict_video_with_a_stub_model(dev, clips_per_step):
    from streamflow_amd import video
    H, W, T, n = 60, 90, 4, 11                                            # 4 clips, the last one a tail clip that overlaps
    frames = vc.random_frames(21, n, H, W)
    for mode in ("sintel", "kitti"):
        one = video.predict_video(vc.stub_model, frames, T=T, clips_per_step=clips_per_step, mode=mode)
        fwd, bwd = video.predict_video(vc.stub_model, frames, T=T, clips_per_step=clips_per_step, mode=mode, bidirectional=True)
        assert torch.equal(fwd, one) and torch.equal(fwd, vc.flows(vc.stub_model, frames.to(dev), T, mode, clips_per_step))
        want_b = backward_flows(vc.stub_model, frames.to(dev), T, mode, 1)                    # a per-clip loop
        assert bwd.shape == fwd.shape and torch.equal(bwd, want_b)
        assert not torch.equal(bwd, fwd)
        # the stub's flows are frame differences: the backward flow of a pair is the negated forward one
        assert torch.equal(bwd, -fwd)
        calls = []
        chw = frames.permute(0, 3, 1, 2).contiguous()
        for src in (frames, frames.to(dev), chw.to(dev), list(frames.numpy())):
            calls.clear()
            res = video.predict_video(vc.stub_model, src, T=T, clips_per_step=clips_per_step, mode=mode, bidirectional=True,
                                      sink=lambda *a: calls.append(a))
            plan = video.plan_batches(n, T, clips_per_step)
            assert res is None and [c[0] for c in calls] == [b[4] for b in plan]
            assert torch.equal(torch.cat([c[1] for c in calls]), fwd) and torch.equal(torch.cat([c[2] for c in calls]), bwd)
            for (first, f, b, held), batch in zip(calls, plan):
                assert held.dtype == torch.uint8 and held.device == dev and tuple(held.shape) == (f.shape[0] + 1, H, W, 3)
                assert torch.equal(held.cpu(), frames[first:first + f.shape[0] + 1])
    # a video without a tail clip, other clip lengths
    for T2, n2 in ((2, 5), (3, 7), (5, 11)):
        f2 = vc.random_frames(T2, n2, 33, 47)
        fwd, bwd = video.predict_video(vc.stub_model, f2, T=T2, clips_per_step=clips_per_step, bidirectional=True)
        assert torch.equal(fwd, vc.flows(vc.stub_model, f2.to(dev), T2, "sintel", 1))
        assert torch.equal(bwd, backward_flows(vc.stub_model, f2.to(dev), T2, "sintel", 1))


def test_bidirectional_predict_video_with_the_model(dev):
    """SKFlow_MF8 with the patch encoder on seeded synthetic weights, 132 x 196 frames, T = 3, 8 frames (four clips, a tail clip), as
    tests/test_gpu_video.py: fwd is the unidirectional call's, bwd the reversed clips' outputs in reversed order."""
    from streamflow_amd import synthetic as syn, video
    from streamflow_amd.model import SKFlow_MF8, default_args
    H, W, T, n, iters = 132, 196, 3, 8, 3
    model = SKFlow_MF8(default_args(T=T, Encoder="PatchEncoder")).to(dev)
    model.load_state_dict(dict(syn.make_params(41, T)), strict=True)
    frames = vc.random_frames(8, n, H, W)
    call = lambda imgs: model.forward_normalised(imgs, iters)
    one = video.predict_video(model, frames, T=T, iters=iters, clips_per_step=3)
    fwd, bwd = video.predict_video(model, frames, T=T, iters=iters, clips_per_step=3, bidirectional=True)
    assert torch.equal(fwd, one) and torch.isfinite(bwd).all()
    assert torch.equal(bwd, backward_flows(call, frames.to(dev), T, "sintel", 3))
    assert not torch.equal(bwd, fwd)


def shifting_video(n, H, W, shift, seed=3):
    """Frame k shows a fixed random image moved `shift` pixels to the left per frame; the blue byte of pixel (0, 0) holds 20 k."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(H, W + n * shift, 3), dtype=np.uint8)
    frames = np.stack([base[:, k * shift:k * shift + W] for k in range(n)]).copy()
    frames[:, 0, 0, 2] = 20 * np.arange(n)
    return torch.from_numpy(frames)


def make_shift_model(shift, back_extra):
    def model(imgs):
        """Pair k of a clip: u = -shift where the later frame follows (the tag grows), shift + back_extra where time runs backwards."""
        B, T, _, H, W = imgs.shape
        out = []
        for k in range(T - 1):
            fwd_in_time = imgs[:, k + 1, 2, 0, 0] > imgs[:, k, 2, 0, 0]
            u = torch.where(fwd_in_time, torch.full_like(fwd_in_time, -shift, dtype=torch.float32),
                            torch.full_like(fwd_in_time, shift + back_extra, dtype=torch.float32))
            flow = torch.zeros(B, 2, H, W, device=imgs.device)
            flow[:, 0] = u.view(B, 1, 1)
            out.append(flow)
        return out
    return model


def test_video_report_on_a_translating_video(dev, capsys):
    """A constant shift of 6 pixels per frame: the true forward flow is (-6, 0), its inverse (+6, 0); the stub returns (-6, 0) and
    (6.25, 0).  Forward: the 6 leftmost columns leave the frame, everything else is visible with |f + b| = 0.25 and the warped
    frame equals the frame (integer shift) but for the tagged pixel.  Backward: x + 6.25 <= W - 1 fails for the 7 rightmost columns."""
    from streamflow_amd import consistency
    n, H, W, shift = 9, 40, 64, 6                                         # no padding at 40 x 64
    frames = shifting_video(n, H, W, shift)
    rep = consistency.video_report(make_shift_model(shift, 0.25), frames.to(dev), T=4, clips_per_step=2)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("Consistency (forward)") and lines[1].startswith("Consistency (backward)")
    f, b = rep["forward"], rep["backward"]
    assert f["pairs"] == b["pairs"] == n - 1 and f["pixels"] == b["pixels"] == (n - 1) * H * W
    assert f["visible"] == (W - shift) / W and f["occluded"] + f["outside"] == shift / W and f["occluded"] == 0
    assert b["visible"] == (W - shift - 1) / W and b["occluded"] + b["outside"] == (shift + 1) / W
    assert abs(f["fb_error"] - 0.25) < 1e-6 and abs(b["fb_error"] - 0.25) < 1e-6
    assert abs(f["mean_flow"] - shift) < 1e-6 and abs(b["mean_flow"] - (shift + 0.25)) < 1e-6
    assert 0 <= f["photo_error"] < 255.0 / (H * (W - shift))              # one tagged byte per frame at most
    assert 1.0 < b["photo_error"] < 255.0                                 # a quarter-pixel blend of noise


def test_command_line_writes_masks_and_warped_frames(tmp_path, dev):
    """python -m streamflow_amd.demo --occlusion --warp --report over six 124 x 188 PNG frames (as tests/test_gpu_video.py): the
    written PNGs decode to the kernels' bytes for the flows a direct bidirectional predict_video call returns in this process."""
    from streamflow_amd import consistency, flow_io, ops, synthetic as syn, video
    from streamflow_amd.model import StreamFlowT4
    H, W, n, iters = 124, 188, 6, 3
    frames = vc.random_frames(5, n, H, W).numpy()
    os.makedirs(tmp_path / "frames")
    for i, f in enumerate(frames):
        flow_io.write_png(str(tmp_path / "frames" / ("%04d.png" % i)), f)
    sd = dict(syn.make_params(51, 4))
    sd.update({"fnet." + k: v for k, v in syn.make_twins_params(52).items()})
    sd.update({"cnet." + k: v for k, v in syn.make_twins_params(53).items()})
    ckpt = str(tmp_path / "ckpt.pth")
    torch.save({"model": {"module." + k: v for k, v in sd.items()}}, ckpt)
    cmd = [sys.executable, "-m", "streamflow_amd.demo", "--frames", str(tmp_path / "frames"), "--ckpt", ckpt, "--out",
           str(tmp_path / "png"), "--flo", str(tmp_path / "flo"), "--occlusion", str(tmp_path / "occ"), "--warp", str(tmp_path / "warp"),
           "--report", "--iters", str(iters), "--clips-per-step", "8"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "5 flow fields" in r.stdout and "Consistency (forward)" in r.stdout and "Consistency (backward)" in r.stdout
    names = ["frame_%04d" % i for i in range(n - 1)]
    assert sorted(os.listdir(tmp_path / "occ")) == [x + ".png" for x in names] == sorted(os.listdir(tmp_path / "warp"))
    assert sorted(os.listdir(tmp_path / "flo")) == sorted([x + ".flo" for x in names] + [x + "_bwd.flo" for x in names])
    model = StreamFlowT4(ckpt).to(dev).eval()
    fwd, bwd = video.predict_video(model, torch.from_numpy(frames), T=4, iters=iters, clips_per_step=8, bidirectional=True)
    cls, _ = ops.flow_consistency(fwd, bwd, codes=consistency.MASK_CODES)
    warped, _ = consistency.warp_back(torch.from_numpy(frames).to(dev), fwd)
    cls, warped = cls.cpu().numpy(), warped.cpu().numpy()
    for i, x in enumerate(names):
        assert np.array_equal(flow_io.read_flo(str(tmp_path / "flo" / (x + "_bwd.flo"))), bwd[i].permute(1, 2, 0).cpu().numpy()), i
        occ = flow_io.read_png(str(tmp_path / "occ" / (x + ".png")))
        assert occ.shape[:2] == (H, W) and np.array_equal(occ.reshape(H, W), cls[i]), i
        assert np.array_equal(flow_io.read_png(str(tmp_path / "warp" / (x + ".png"))), warped[i]), i
