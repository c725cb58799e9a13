"""CPU: the two restatements of sf_frame_interp (tests/interp_cases.py) against each other and against a float64 ideal; exact
properties of the contract (zero flow, integer translations, constant colours, non-finite flows); the Python layers fail loudly
without a GPU; the demo's new flags; the header and the library carry the new entry points and refuse bad arguments before a launch.

Margin against the float64 ideal (dyadic cases: t in {1/2, 1/4, 3/4}, flows multiples of 1/16, so t * flow is a multiple of 1/64
and the integer weights are exactly 4096 times the real ones).  Every output byte is the exact rational value rounded ONCE, half
up: a side's mean C / W as (2 C + W) / (2 W), the blend of two sides as one quotient of products of the sums (the sides are NOT
rounded to bytes first), a hole as the blend of two bytes.  So every byte lies within 0.5 of the ideal; 1e-9 covers the float64
evaluation of the ideal itself (values up to 255, a few roundings of 2^-53 relative)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import interp_cases as ic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ic.CASES + ic.DYADIC


@pytest.fixture(scope="module")
def dyadic():
    """{case id: (restatement, ideal)} with class maps and the default importances, computed once."""
    res = {}
    for case in ic.DYADIC:
        a, b, fwd, bwd, num, den, cls = ic.build(case, True)
        res[case[0]] = (ic.restate(a, b, fwd, bwd, num, den, cls), ic.ideal64(a, b, fwd, bwd, num, den, cls))
    return res


@pytest.mark.parametrize("case", ALL, ids=ic.case_ids(ALL))
def test_the_two_restatements_agree_bitwise(case):
    for with_cls, imp in ic.VARIANTS:
        a, b, fwd, bwd, num, den, cls = ic.build(case, with_cls)
        vec = ic.restate(a, b, fwd, bwd, num, den, cls, imp=imp)
        loop = ic.restate_scalar(a, b, fwd, bwd, num, den, cls, imp=imp)
        for name, x, y in zip(("out", "cover", "stats"), vec, loop):
            assert x.dtype == y.dtype and np.array_equal(x, y), (name, with_cls, imp)
        n, _, h, w = fwd.shape
        assert (vec[2][:, ic.PIXELS] == h * w).all() and (vec[2][:, 1:].sum(1) == h * w).all()


@pytest.mark.parametrize("case", ic.BIG, ids=ic.case_ids(ic.BIG))
def test_the_two_restatements_agree_under_heavy_contention(case):
    """... and the cases do what they are for: a one-sided W of at least 2^31 whose dark channels keep 2 C + W below 2^32 (mean 0),
    or both-sided targets with W on both sides of 2^24."""
    a, b, fwd, bwd, num, den, _ = ic.build(case)
    vec, loop = ic.restate(a, b, fwd, bwd, num, den), ic.restate_scalar(a, b, fwd, bwd, num, den)
    for x, y in zip(vec, loop):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    tf, tb = ic.ts_pair(num, den)
    full = np.full(fwd[:, 0].shape, 16, np.uint64)
    (WA, CA), (WB, _) = ic.splat32(a, fwd, tf, full), ic.splat32(b, bwd, tb, full)
    if case[1] == "dark-one-side":
        q = int(np.argmax(WA[0]))
        W, C = int(WA[0].reshape(-1)[q]), CA[0].reshape(-1, 3)[q]
        assert W == fwd.shape[2] * fwd.shape[3] << 16 >= 1 << 31 and not WB.any() and (WA > 0).sum() == 1
        assert 2 * int(C[0]) + W < 1 << 32 and 2 * int(C[1]) + W < 1 << 32 and 2 * int(C[2]) + W >= 1 << 32
        assert vec[0][0].reshape(-1, 3)[q].tolist()[:2] == [0, 0] and 100 < vec[0][0].reshape(-1, 3)[q][2] < 155
        assert vec[1][0].reshape(-1)[q] == 1
    else:
        both = (WA > 0) & (WB > 0)
        assert both.sum() >= 40 and (WA[both] < 1 << 24).any() and (WA[both] >= 1 << 24).sum() >= 30 and (WB[both] >= 1 << 24).sum() >= 30


def test_cases_reach_every_cover_code_and_every_class():
    """So that the GPU test cannot pass on trivial inputs."""
    seen = np.zeros(4)
    for case in ic.CASES:
        a, b, fwd, bwd, num, den, cls = ic.build(case, True)
        seen += ic.restate(a, b, fwd, bwd, num, den, cls)[2][:, 1:].sum(0)
        if case[1] == "smooth" and min(fwd.shape[2:]) >= 5:
            assert len(np.unique(cls[0])) >= 2
    assert (seen > 100).all(), seen
    a, b, fwd, bwd, num, den, _ = ic.build(ic.CASES[10])                  # converge: one accumulator takes every pixel of pair 0
    W, _ = ic.splat32(a, fwd, ic.ts_pair(num, den)[0], np.full(fwd[:, 0].shape, 16, np.uint64))
    assert W[0].max() == 13 * 37 * 4096 * 16 and (W[0] > 0).sum() == 1 and (W[1] > 0).sum() == 4


@pytest.mark.parametrize("case", ic.DYADIC, ids=ic.case_ids(ic.DYADIC))
def test_dyadic_bytes_lie_within_half_a_level_of_the_float64_ideal(dyadic, case):
    """The margin 0.5 + 1e-9 on every byte, whichever sides are present (module docstring).  A resolve that rounds each side to a
    byte before blending misses it where both sides are present (up to 0.994 on these cases)."""
    (out, cover, _), (ideal, _, _, cover64) = dyadic[case[0]]
    assert np.array_equal(cover, cover64)
    d = np.abs(out.astype(np.float64) - ideal)
    for k, name in enumerate(("both", "a only", "b only", "holes")):
        if (cover == k).any():
            print(f"{case[0]} {name}: max |byte - ideal| = {d[cover == k].max():.6f} over {(cover == k).sum()} pixels")
    assert d.max() <= 0.5 + 1e-9, f"max |byte - ideal| = {d.max():.6f}"


@pytest.mark.parametrize("case", ic.DYADIC, ids=ic.case_ids(ic.DYADIC))
def test_dyadic_side_colours_are_the_rounded_ideal_means(case):
    """Each side's integer mean (2 C + W) / (2 W) is within 0.5 + 1e-9 of the float64 mean with unquantised weights."""
    a, b, fwd, bwd, num, den, cls = ic.build(case, True)
    _, ma, mb, _ = ic.ideal64(a, b, fwd, bwd, num, den, cls)
    tf, tb = ic.ts_pair(num, den)
    for img, flow, ts, c, want in ((a, fwd, tf, cls[0], ma), (b, bwd, tb, cls[1], mb)):
        W, C = ic.splat32(img, flow, ts, ic._importance(c, (0, 1), (16, 1, 16), c.shape))
        assert np.array_equal(W > 0, ~np.isnan(want[..., 0]))
        Ws = np.where(W > 0, W, np.uint64(1))[..., None]
        got = ((np.uint64(2) * C + Ws) // (np.uint64(2) * Ws)).astype(np.float64)
        assert np.abs(got - want)[W > 0].max() <= 0.5 + 1e-9


@pytest.mark.parametrize("t", [(1, 2), (1, 3), (3, 4), (63, 64)], ids=lambda t: "%d/%d" % t)
def test_zero_flow_is_the_integer_cross_fade(t):
    num, den = t
    a, b, fwd, bwd = ic.make("zero", 5, 2, 9, 21, num, den)
    out, cover, stats = ic.restate(a, b, fwd, bwd, num, den)
    want = (a.astype(np.int64) * (den - num) + b.astype(np.int64) * num + den // 2) // den
    assert np.array_equal(out, want) and not cover.any()
    assert (stats[:, ic.BOTH] == 9 * 21).all()


@pytest.mark.parametrize("shift", [(2, 0), (-4, 2), (6, -2)], ids=str)
def test_even_translation_at_half_time_reproduces_the_shifted_image(shift):
    """Frame b is frame a moved by (sx, sy); at t = 1/2 the image moved by half of that appears exactly wherever both sides cover."""
    sx, sy = shift
    h, w = 12, 30
    rng = np.random.default_rng(9)
    big = rng.integers(0, 256, size=(h + 16, w + 16, 3), dtype=np.uint8)
    cut = lambda dx, dy: big[8 - dy:8 - dy + h, 8 - dx:8 - dx + w][None].copy()
    a, b, mid = cut(0, 0), cut(sx, sy), cut(sx // 2, sy // 2)
    fwd = np.zeros((1, 2, h, w), np.float32)
    fwd[0, 0], fwd[0, 1] = sx, sy
    out, cover, _ = ic.restate(a, b, fwd, -fwd, 1, 2)
    both = cover[0] == 0
    assert both.sum() >= (h - abs(sy)) * (w - abs(sx))
    assert np.array_equal(out[0][both], mid[0][both])
    # one side alone is the shifted image too
    one = (cover[0] == 1) | (cover[0] == 2)
    assert one.any() and np.array_equal(out[0][one], mid[0][one])


@pytest.mark.parametrize("case", [c for c in ic.CASES if c[1] in ("smooth", "edges", "holes", "converge")][::2], ids=lambda c: c[0])
def test_constant_colours_come_back_at_every_pixel(case):
    """The weights are a partition of unity: the mean of equal bytes is that byte, and so is every blend."""
    a, b, fwd, bwd, num, den, cls = ic.build(case, True)
    colour = np.array([7, 130, 255], np.uint8)
    a[:], b[:] = colour, colour
    out, _, _ = ic.restate(a, b, fwd, bwd, num, den, cls)
    assert (out == colour).all()


def test_non_finite_and_huge_flows_contribute_nothing():
    h, w = 5, 8
    a = np.full((1, h, w, 3), 200, np.uint8)
    b = np.full((1, h, w, 3), 100, np.uint8)
    fwd = np.zeros((1, 2, h, w), np.float32)
    bwd = np.zeros((1, 2, h, w), np.float32)
    for x, bad in enumerate(ic.SPECIALS):
        fwd[0, 0, 0, x] = bad
        fwd[0, 1, 1, x] = bad
        bwd[0, :, 2, x] = bad
    out, cover, stats = ic.restate(a, b, fwd, bwd, 1, 2)
    assert (cover[0, 0, :5] == 2).all() and (cover[0, 1, :5] == 2).all() and (cover[0, 2, :5] == 1).all()
    assert (out[0, 0, :5] == 100).all() and (out[0, 2, :5] == 200).all() and (out[0, 3] == 150).all()
    assert stats[0].tolist() == [40, 25, 5, 10, 0]


def test_python_layers_fail_loudly_without_a_gpu():
    from streamflow_amd import interpolate, ops
    f = torch.zeros(2, 2, 8, 8)
    fr = torch.zeros(3, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_interp(fr[:-1], fr[1:], f, f, 1, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        interpolate.between(fr, f, f, 2, masks=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        interpolate.between(fr, f, f, 2)
    for bad in (1, 0, 65, 2.0, True):
        with pytest.raises(ValueError, match="factor"):
            interpolate.interpolate_video(lambda x: [], fr, factor=bad)
        with pytest.raises(ValueError, match="factor"):
            interpolate.between(fr, f, f, bad)
    with pytest.raises(ValueError, match="factor"):
        interpolate.InterpSink(1, print)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU"):
            interpolate.interpolate_video(lambda x: [], torch.zeros(5, 8, 8, 3, dtype=torch.uint8), factor=2, T=2)
    import inspect
    p = inspect.signature(ops.frame_interp).parameters
    assert p["importance"].default == (16, 1, 16) and p["max_ws_bytes"].default == 1 << 30 and p["cover"].default is False
    assert inspect.signature(interpolate.interpolate_video).parameters["factor"].default == 2


def test_demo_parser_takes_the_new_flags(capsys):
    from streamflow_amd import demo
    ap = demo.arg_parser()
    base = ["--frames", "f", "--ckpt", "c"]
    a = ap.parse_args(base + ["--out", "o"])
    assert a.interpolate is None and a.slowmo is None and a.slowmo_video is None
    a = ap.parse_args(base + ["--interpolate", "4", "--slowmo", "d", "--slowmo-video", "v.avi"])
    assert a.interpolate == 4 and a.slowmo == "d" and a.slowmo_video == "v.avi" and a.out is None
    for bad in (["--interpolate", "1"], ["--interpolate", "65"], ["--interpolate", "x"]):
        with pytest.raises(SystemExit):
            ap.parse_args(base + ["--slowmo", "d"] + bad)
        assert "--interpolate" in capsys.readouterr().err
    # neither --out nor --video nor a slow-motion output; a slow-motion output without --interpolate and the reverse
    for argv in (base, base + ["--interpolate", "2"], base + ["--slowmo", "d"], base + ["--out", "o", "--interpolate", "2"],
                 base + ["--out", "o", "--slowmo-video", "v.avi"]):
        with pytest.raises(SystemExit):
            demo.main(argv)
        capsys.readouterr()
    import inspect
    params = inspect.signature(demo.read_frames_and_group_predict).parameters
    for name in ("interpolate", "slowmo_dir", "slowmo_video"):
        assert params[name].default is None


def test_header_and_library_carry_the_entry_points():
    from streamflow_amd import _lib, build, ops
    hdr = open(os.path.join(REPO, "include", "streamflow_hip.h")).read()
    assert "int sf_frame_interp(" in hdr and "int64_t sf_frame_interp_ws_bytes(" in hdr
    assert "sf_frame_interp" in _lib.SIGNATURES and "sf_frame_interp_ws_bytes" in _lib.SIGNATURES
    assert int(re.search(r"SF_INTERP_LEN = (\d+)", hdr).group(1)) == ops.INTERP_LEN == ic.LEN
    for name, value in (("PIXELS", ic.PIXELS), ("BOTH", ic.BOTH), ("A_ONLY", ic.A_ONLY), ("B_ONLY", ic.B_ONLY), ("HOLES", ic.HOLES)):
        assert int(re.search(r"SF_INTERP_%s = (\d+)" % name, hdr).group(1)) == getattr(ops, "INTERP_" + name) == value
    assert "frame_interp.hip" in build.SOURCES
    for kernel in ("splat_kernel", "resolve_kernel"):
        assert kernel in build.HOT_KERNELS                                # the build fails if they use scratch memory
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.load()
    # 2 sides x 4 planes x 8 bytes per pixel and pair, plus blocks-per-pair partial rows of SF_INTERP_LEN doubles
    assert lib.sf_frame_interp_ws_bytes(1, 1, 1) == 64 + 40
    assert lib.sf_frame_interp_ws_bytes(3, 13, 37) == 64 * 3 * 13 * 37 + 3 * 4 * 40
    assert lib.sf_frame_interp_ws_bytes(3, 5, 260) == 64 * 3 * 5 * 260 + 3 * 3 * 40
    assert lib.sf_frame_interp_ws_bytes(1, 1088, 1920) == 64 * 1088 * 1920 + 2048 * 40
    assert lib.sf_frame_interp_ws_bytes(24, 436, 1024) == 64 * 24 * 436 * 1024 + 24 * 85 * 40
    for bad in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, -1), (1, 1 << 15, 1 << 15)):
        assert lib.sf_frame_interp_ws_bytes(*bad) == -1, bad
        assert b"sf_frame_interp_ws_bytes" in lib.sf_last_error()
    P = 0x10000
    ok = dict(a=P, b=P, fs=1200, rs=60, ps=3, cs=1, fwd=P, bwd=P, ff=800, fc=400, fr=20, n=2, h=20, w=20, num=1, den=2, cls_f=None,
              cls_b=None, imp=(16, 1, 16), out=P, cover=None, stats=P, ws=P, ws_bytes=1 << 20)

    def call(**kw):
        q = dict(ok, **kw)
        return lib.sf_frame_interp(q["a"], q["fs"], q["rs"], q["ps"], q["cs"], q["b"], q["fs"], q["rs"], q["ps"], q["cs"], q["fwd"], q["ff"],
                                   q["fc"], q["fr"], q["bwd"], q["ff"], q["fc"], q["fr"], q["n"], q["h"], q["w"], q["num"], q["den"],
                                   q["cls_f"], q["cls_b"], 0, 1, q["imp"][0], q["imp"][1], q["imp"][2], q["out"], q["cover"], q["stats"],
                                   q["ws"], q["ws_bytes"], None)

    need = lib.sf_frame_interp_ws_bytes(2, 20, 20)
    for bad in (dict(a=None), dict(b=None), dict(fwd=None), dict(bwd=None), dict(out=None), dict(stats=None), dict(ws=None),
                dict(n=0), dict(n=65536), dict(h=0), dict(w=-1), dict(h=1 << 15, w=1 << 15, fr=1 << 15),
                dict(fr=19), dict(fc=0), dict(ff=-1), dict(fs=-1), dict(rs=-1), dict(ps=-1), dict(cs=-1),
                dict(fwd=P + 2), dict(bwd=P + 1), dict(stats=P + 4), dict(ws=P + 4),
                dict(num=0), dict(num=2), dict(num=-1), dict(den=65, num=3), dict(den=1, num=1), dict(num=3, den=2),
                dict(imp=(0, 1, 1)), dict(imp=(1, 17, 1)), dict(imp=(1, 1, -3)),
                dict(cls_f=P), dict(cls_b=P), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(**bad) == -1, bad
        assert b"sf_frame_interp" in lib.sf_last_error(), bad
