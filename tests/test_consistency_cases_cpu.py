"""CPU: the float32 restatement of sf_flow_consistency / sf_warp_frames (tests/consistency_cases.py) against an independent float64
formulation through grid_sample; the case generator covers all three classes; the Python layers fail loudly without a GPU; the
demo's new flags; the header and the library carry the new entry points.

Tolerances.  Classes: the float32 and float64 evaluations of lhs - rhs differ by a few float32 roundings of terms of size
<= 1 + rhs (bilinear weights, two squares, a sum), far below 1e-4 (1 + rhs); a pixel whose float64 margin |lhs - rhs| exceeds that
must get the same class.  The inside test is the same kind of comparison: px = x + u rounds by <= 2^-24 |px| < 1e-5 for these sizes, so
targets within 1e-4 of a frame edge (in float64) but not exactly on it are left aside, all others must agree.  Warped bytes: the float32 value is within
a few 2^-24 * 255 of the float64 one, so the rounded bytes differ by at most 1 (only next to a .5 boundary)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import consistency_cases as cc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 7), (5, 1), (13, 37), (17, 65), (33, 130)]


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "%dx%d" % s)
def test_float32_restatement_agrees_with_the_float64_formulation(hw):
    h, w = hw
    fwd, bwd, src, ref = cc.make_case(100 + h + w, 3, h, w)
    cls, stats, lhs32, rhs32 = cc.restate32(fwd, bwd)
    warped, _ = cc.warp32(src, fwd)
    inside64, lhs, rhs, vals, dist = cc.formulate64(fwd, bwd, src)
    clear_edge = (dist == 0) | (np.abs(dist) > 1e-4)                      # (exactly on an edge: the float32 sum is exact too)
    assert clear_edge.mean() > 0.99
    # outside: equal wherever the target is clear of the frame edge
    assert np.array_equal((cls == 2)[clear_edge], ~inside64[clear_edge])
    # visible / occluded: equal wherever the float64 margin is clear
    clear = clear_edge & inside64 & (np.abs(lhs - rhs) > 1e-4 * (1 + rhs))
    assert clear.sum() >= 0.9 * (clear_edge & inside64).sum()
    assert np.array_equal((cls == 0)[clear], (lhs <= rhs)[clear])
    assert np.array_equal((cls == 1)[clear], (lhs > rhs)[clear])
    # warped bytes within 1 of the rounded float64 values; 0 outside
    want = np.where(inside64[..., None], np.floor(vals + 0.5), 0.0)
    diff = np.abs(warped.astype(np.int64) - want.astype(np.int64))[clear_edge]
    assert diff.max() <= 1, f"warped bytes differ by {diff.max()}"
    # the stats rows restate the class map
    for i in range(3):
        assert stats[i, cc.PIXELS] == h * w == stats[i, cc.VISIBLE] + stats[i, cc.OCCLUDED] + stats[i, cc.OUTSIDE]
        assert stats[i, cc.VISIBLE] == (cls[i] == 0).sum() and stats[i, cc.FINITE] == h * w
    # the sums agree with float64 to float32 accuracy (sums of non-negative terms)
    vis = cls == 0
    fb64 = np.sqrt(lhs)[vis & clear].sum()
    fb32 = np.sqrt(lhs32.astype(np.float64))[vis & clear].sum()
    assert abs(fb64 - fb32) <= 1e-4 * (1 + fb64)


@pytest.mark.parametrize("hw", [s for s in SIZES if not cc.degenerate(*s)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("n", [1, 3, 25])
def test_generator_covers_all_three_classes(hw, n):
    """So that the GPU test cannot pass on trivial inputs: every non-degenerate case has at least 5 % of its pixels in each class,
    in both directions of the photometric statistic's mask as well (visible pixels exist in every field)."""
    h, w = hw
    fwd, bwd, _, _ = cc.make_case(100 + h + w, n, h, w)
    cls, stats, _, _ = cc.restate32(fwd, bwd)
    for k in (0, 1, 2):
        share = (cls == k).mean()
        assert share >= 0.05, f"class {k}: {share:.3f} of the pixels"
    assert (stats[:, cc.VISIBLE] > 0).all()


def test_thin_cases_keep_pixels_inside():
    for h, w in [s for s in SIZES if cc.degenerate(*s)]:
        fwd, bwd, _, _ = cc.make_case(100 + h + w, 3, h, w)
        if h == 1:
            assert not fwd[:, 1].any()
        if w == 1:
            assert not fwd[:, 0].any()
        cls, _, _, _ = cc.restate32(fwd, bwd)
        assert (cls != 2).any()


def test_special_values_in_the_restatement():
    """NaN, +-Inf and +-1e30 forward flows are outside (no index is formed from them); a NaN backward tap is occluded; a target
    exactly on the last row / column is inside; -0.0 behaves as 0."""
    h, w = 6, 9
    fwd = np.zeros((1, 2, h, w), np.float32)
    bwd = np.zeros((1, 2, h, w), np.float32)
    for x, bad in enumerate([np.nan, np.inf, -np.inf, 1e30, -1e30]):
        fwd[0, 0, 0, x] = bad
        fwd[0, 1, 1, x] = bad
    fwd[0, 0, 2, 0] = w - 1                                              # lands exactly on the last column
    fwd[0, 1, 2, 1] = h - 1 - 2                                          # ... on the last row
    fwd[0, 0, 3, 0] = -0.0
    bwd[0, 0, 2, w - 1] = -(w - 1)
    bwd[0, 1, h - 1, 1] = -(h - 1 - 2)
    bwd[0, 0, 4, 4] = np.nan
    cls, stats, _, _ = cc.restate32(fwd, bwd)
    assert (cls[0, 0, :5] == 2).all() and (cls[0, 1, :5] == 2).all()
    assert cls[0, 2, 0] == 0 and cls[0, 2, 1] == 0 and cls[0, 3, 0] == 0
    assert cls[0, 4, 4] == 1
    assert stats[0, cc.FINITE] == h * w - 10 and np.isfinite(stats[0, cc.SUM_MAG])
    warped, _ = cc.warp32(np.full((1, h, w, 3), 200, np.uint8), fwd)
    assert (warped[0, 0, :5] == 0).all() and (warped[0, 2, 0] == 200).all()


def test_python_layers_fail_loudly_without_a_gpu():
    from streamflow_amd import consistency, ops, video
    f = torch.zeros(2, 2, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.flow_consistency(f, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.warp_frames(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        consistency.check_pairs(f, f)
    if not torch.cuda.is_available():
        frames = torch.zeros(5, 8, 8, 3, dtype=torch.uint8)
        with pytest.raises(RuntimeError, match="no CPU"):
            video.predict_video(lambda x: [], frames, T=2, bidirectional=True)
        with pytest.raises(RuntimeError, match="no CPU"):
            consistency.video_report(lambda x: [], frames, T=2)
    # argument errors come before the device check
    with pytest.raises(TypeError, match="uint8"):
        video.predict_video(lambda x: [], torch.zeros(5, 8, 8, 3), T=2, bidirectional=True)
    with pytest.raises(ValueError, match="at least T"):
        video.predict_video(lambda x: [], torch.zeros(1, 8, 8, 3, dtype=torch.uint8), T=2, bidirectional=True)
    import inspect
    assert inspect.signature(video.predict_video).parameters["bidirectional"].default is False


def test_demo_parser_takes_the_new_flags(capsys):
    from streamflow_amd import demo
    ap = demo.arg_parser()
    base = ["--frames", "f", "--ckpt", "c", "--out", "o"]
    a = ap.parse_args(base)
    assert a.bidirectional is False and a.occlusion is None and a.warp is None and a.report is False
    a = ap.parse_args(base + ["--bidirectional", "--occlusion", "occ", "--warp", "wrp", "--report"])
    assert a.bidirectional and a.occlusion == "occ" and a.warp == "wrp" and a.report
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--occlusion"])
    assert "--occlusion" in capsys.readouterr().err
    import inspect
    params = inspect.signature(demo.read_frames_and_group_predict).parameters
    for name, default in (("bidirectional", False), ("occlusion_dir", None), ("warp_dir", None), ("report", False)):
        assert params[name].default is default


def test_header_and_library_carry_the_entry_points():
    from streamflow_amd import _lib, build, ops
    hdr = open(os.path.join(REPO, "include", "streamflow_hip.h")).read()
    for name in ("sf_flow_consistency", "sf_warp_frames"):
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES
        assert f"int64_t {name}_ws_bytes(" in hdr and name + "_ws_bytes" in _lib.SIGNATURES
    assert int(re.search(r"SF_FBC_LEN = (\d+)", hdr).group(1)) == ops.FBC_LEN == cc.LEN
    assert int(re.search(r"SF_WARP_LEN = (\d+)", hdr).group(1)) == ops.WARP_LEN
    assert "flow_consistency.hip" in build.SOURCES
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.load()
    for name in ("sf_flow_consistency", "sf_warp_frames"):
        assert hasattr(lib, name)
    # host-side argument checks run before any launch (dummy, never dereferenced pointers)
    assert lib.sf_flow_consistency_ws_bytes(3, 13, 37) == 3 * 4 * 7 * 8 and lib.sf_warp_frames_ws_bytes(3, 13, 37) == 3 * 1 * 2 * 8
    assert lib.sf_flow_consistency_ws_bytes(1, 1088, 1920) == 2048 * 7 * 8 and lib.sf_flow_consistency_ws_bytes(24, 436, 1024) == 24 * 85 * 7 * 8
    assert lib.sf_warp_frames_ws_bytes(1, 1088, 1920) == 2040 * 2 * 8
    assert lib.sf_warp_frames_ws_bytes(0, 4, 4) == -1 and lib.sf_flow_consistency_ws_bytes(65536, 4, 4) == -1
    assert lib.sf_flow_consistency_ws_bytes(1, 1 << 15, 1 << 15) == -1
    P = 0x10000
    ok = dict(fwd=P, ff=800, fc=400, fr=20, bwd=P, bf=800, bc=400, br=20, n=2, h=20, w=20, alpha=0.01, beta=0.5, cls=P, stats=P,
              ws=P, ws_bytes=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sf_flow_consistency(a["fwd"], a["ff"], a["fc"], a["fr"], a["bwd"], a["bf"], a["bc"], a["br"], a["n"], a["h"], a["w"],
                                       a["alpha"], a["beta"], 0, 1, 2, a["cls"], a["stats"], a["ws"], a["ws_bytes"], None)

    for bad in (dict(fwd=None), dict(bwd=None), dict(cls=None), dict(stats=None), dict(ws=None), dict(n=0), dict(n=65536), dict(h=0),
                dict(w=-1), dict(h=1 << 15, w=1 << 15, fr=1 << 15, br=1 << 15), dict(fr=19), dict(br=19), dict(ws_bytes=111),
                dict(fwd=P + 2), dict(stats=P + 4), dict(alpha=float("nan")), dict(fc=0)):
        assert call(**bad) == -1, bad
        assert b"sf_flow_consistency" in lib.sf_last_error()

    def warp(**kw):
        a = dict(dict(src=P, flows=P, out=P, cls=None, ref=None, stats=None, ws=None, ws_bytes=0, n=2, h=20, w=20, fr=20), **kw)
        return lib.sf_warp_frames(a["src"], 1200, 60, 3, 1, a["flows"], 800, 400, a["fr"], a["n"], a["h"], a["w"], a["out"], a["cls"], 0,
                                  a["ref"], 1200, 60, 3, 1, a["stats"], a["ws"], a["ws_bytes"], None)

    for bad in (dict(src=None), dict(flows=None), dict(out=None), dict(n=0), dict(h=0), dict(fr=19), dict(cls=P), dict(ref=P),
                dict(cls=P, ref=P), dict(cls=P, ref=P, stats=P), dict(cls=P, ref=P, stats=P, ws=P, ws_bytes=8),
                dict(flows=P + 1)):
        assert warp(**bad) == -1, bad
        assert b"sf_warp_frames" in lib.sf_last_error()
