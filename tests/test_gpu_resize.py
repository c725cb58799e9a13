"""sf_resize_u8 / sf_resize_f32 (csrc/resize.hip) through the C ABI with raw strides; every buffer is a guard-banded allocation of
tests/guarded.py, the frame and flow layouts (plain / hwc / chw, plain / strided) are those of tests/test_gpu_frame_interp.py.

Criteria.  u8: the output is BITWISE the numpy restatement's (tests/resize_cases.py, which is PIL.Image.resize byte for byte:
tests/test_resize_cases_cpu.py); all arithmetic is integer, there is no tolerance.  f32: every element within (T_h + T_v + 6) *
2^-24 * |s| * A of the float64 result computed from the same fp32-rounded tables (resize_cases.bound_f32 has the derivation).  The
tables handed to the kernels are the RESTATEMENT's, not the product's.  Operands, guards and everything outside the output and the
workspace must come back unchanged.  No test passes a malformed table; nothing here is meant to fault."""
import numpy as np
import pytest
import torch

from tests import resize_cases as rc
from tests.guarded import GuardedBytes
from tests.test_gpu_frame_interp import place_flows, place_frames

pytestmark = pytest.mark.gpu

OUT_FILL, WS_FILL = 0x5A, 0x7F


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from streamflow_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Tables:
    """The restatement's tables of one (H, W) -> (h, w) and filter on the device: int32 fixed point (u8) or fp32."""

    def __init__(self, dev, H, W, h, w, name, kind):
        self.keep, self.args = [], []
        for a, b in ((W, w), (H, h)):
            if a == b:
                self.args += [None, None, 0]
                continue
            bounds, k = rc.table(a, b, name)
            kk = rc.fixed(k) if kind == "u8" else k.astype(np.float32)
            tb, tk = torch.from_numpy(bounds).to(dev), torch.from_numpy(np.ascontiguousarray(kk)).to(dev)
            self.keep += [tb, tk]
            self.args += [tb.data_ptr(), tk.data_ptr(), int(k.shape[1])]
        self.snap = [t.clone() for t in self.keep]

    def unchanged(self):
        return all(torch.equal(a, b) for a, b in zip(self.keep, self.snap))


class CallU8:
    def __init__(self, lib, dev, img, hw, name, layout="plain"):
        self.lib, self.n, (self.H, self.W), (self.h, self.w) = lib, img.shape[0], img.shape[1:3], hw
        self.src, self.strides = place_frames(img, dev, layout)
        self.snap = self.src.buf.clone()
        self.tab = Tables(dev, self.H, self.W, self.h, self.w, name, "u8")
        self.out = GuardedBytes(dev, self.n * self.h * self.w * 3, fill=OUT_FILL)
        self.need = lib.sf_resize_u8_ws_bytes(self.n, self.H, self.W, self.h, self.w)
        assert self.need == (3 * self.n * self.H * self.w if (self.h != self.H and self.w != self.W) else 0)
        self.ws = GuardedBytes(dev, self.need, fill=WS_FILL) if self.need else None

    def run(self, **kw):
        q = dict(src=self.src.ptr, n=self.n, H=self.H, W=self.W, h=self.h, w=self.w, tab=list(self.tab.args), out=self.out.ptr,
                 ws=None if self.ws is None else self.ws.ptr, ws_bytes=self.need, rs=self.strides[1])
        q.update(kw)
        fs, _, ps, cs = self.strides
        return self.lib.sf_resize_u8(q["src"], fs, q["rs"], ps, cs, q["n"], q["H"], q["W"], q["h"], q["w"], *q["tab"], q["out"], q["ws"],
                                     q["ws_bytes"], stream())

    def result(self):
        torch.cuda.synchronize()
        assert torch.equal(self.src.buf, self.snap), "the source was written"
        assert self.tab.unchanged(), "a table was written"
        assert self.out.guards_unchanged() and (self.ws is None or self.ws.guards_unchanged())
        return self.out.view().view(self.n, self.h, self.w, 3).cpu().numpy()


U8_LAYOUTS = {((37, 53), (16, 24)): ("plain", "hwc", "chw"), ((70, 33), (20, 33)): ("plain", "hwc", "chw"),
              ((33, 70), (33, 31)): ("plain", "chw"), ((50, 61), (50, 61)): ("plain", "hwc", "chw"),
              ((150, 530), (75, 265)): ("plain", "hwc")}


@pytest.mark.parametrize("name", rc.FILTER_NAMES)
@pytest.mark.parametrize("case", rc.U8_SHAPES, ids=rc.shape_id)
def test_u8_is_the_restatement_bitwise(lib, dev, case, name):
    img = rc.u8_input(case, "noise")
    img[0, : max(1, img.shape[1] // 3)] = rc.u8_input(case, "extremes")[0, : max(1, img.shape[1] // 3)]      # 0 / 255 runs: the overshoots
    want = rc.resize_u8(img, case[1], name)
    for layout in U8_LAYOUTS.get(case[:2], ("plain",)):
        call = CallU8(lib, dev, img, case[1], name, layout)
        assert call.run() == 0, lib.sf_last_error()
        got = call.result()
        assert np.array_equal(got, want), (layout, f"{int((got != want).sum())} of {got.size} bytes differ")


def test_u8_repeated_calls_and_stale_workspace(lib, dev):
    """The workspace is written before it is read: a second call on the same buffers gives the same bytes."""
    case = rc.U8_SHAPES[2]
    img = rc.u8_input(case, "noise")
    call = CallU8(lib, dev, img, case[1], "bicubic", "hwc")
    assert call.run() == 0, lib.sf_last_error()
    first = call.result()
    call.ws.view().fill_(0xFF)
    call.out.view().fill_(0)
    assert call.run() == 0, lib.sf_last_error()
    assert np.array_equal(call.result(), first) and np.array_equal(first, rc.resize_u8(img, case[1], "bicubic"))


class CallF32:
    def __init__(self, lib, dev, flow, hw, name, strided=False):
        self.lib, self.n, (self.H, self.W), (self.h, self.w) = lib, flow.shape[0], flow.shape[2:], hw
        self.g, self.ptr, self.strides = place_flows(flow, dev, strided)
        self.tab = Tables(dev, self.H, self.W, self.h, self.w, name, "f32")
        self.out = GuardedBytes(dev, self.n * 2 * self.h * self.w * 4, fill=OUT_FILL)
        self.need = lib.sf_resize_f32_ws_bytes(self.n, self.H, self.W, self.h, self.w)
        assert self.need == (8 * self.n * self.H * self.w if (self.h != self.H and self.w != self.W) else 0)
        self.ws = GuardedBytes(dev, self.need, fill=WS_FILL) if self.need else None

    def run(self, sx=1.0, sy=1.0, **kw):
        q = dict(src=self.ptr, n=self.n, H=self.H, W=self.W, h=self.h, w=self.w, tab=list(self.tab.args), out=self.out.ptr,
                 ws=None if self.ws is None else self.ws.ptr, ws_bytes=self.need, rs=self.strides[2], cs=self.strides[1])
        q.update(kw)
        return self.lib.sf_resize_f32(q["src"], self.strides[0], q["cs"], q["rs"], q["n"], q["H"], q["W"], q["h"], q["w"], *q["tab"],
                                      float(sx), float(sy), q["out"], q["ws"], q["ws_bytes"], stream())

    def result(self):
        torch.cuda.synchronize()
        assert self.g.outside_unchanged() and torch.equal(self.g.buf.view(torch.int32), self.g.snap.view(torch.int32)), "the source was written"
        assert self.tab.unchanged(), "a table was written"
        assert self.out.guards_unchanged() and (self.ws is None or self.ws.guards_unchanged())
        return self.out.view().view(torch.float32).view(self.n, 2, self.h, self.w).cpu().numpy()


@pytest.mark.parametrize("name", rc.FILTER_NAMES)
@pytest.mark.parametrize("case", rc.F32_SHAPES, ids=rc.shape_id)
def test_f32_is_within_the_bound_of_float64(lib, dev, case, name):
    flow = rc.f32_input(case)
    for sx, sy in rc.F32_SCALES:
        want = rc.resize_f64(flow, case[1], name, sx, sy)
        bound = rc.bound_f32(flow, case[1], name, sx, sy)
        for strided in (False, True):
            call = CallF32(lib, dev, flow, case[1], name, strided)
            assert call.run(sx, sy) == 0, lib.sf_last_error()
            err = np.abs(call.result().astype(np.float64) - want)
            worst = float((err / np.maximum(bound, 1e-300)).max())
            print(f"{rc.shape_id(case)} {name} s=({sx}, {sy}) strided={strided}: max err / bound = {worst:.3f}")
            assert (err <= bound).all(), (sx, sy, strided, worst)


def test_f32_copy_scales_the_planes(lib, dev):
    """Neither axis changes: the planes, channel 0 times sx and channel 1 times sy (one fp32 multiply: exact against numpy)."""
    flow = rc.f32_input(((9, 200), (9, 31)))
    call = CallF32(lib, dev, flow, flow.shape[2:], "bilinear", True)
    assert call.run(1.75, 0.4) == 0, lib.sf_last_error()
    want = flow * np.array([1.75, 0.4], np.float32)[None, :, None, None]
    assert call.result().tobytes() == want.astype(np.float32).tobytes()


@pytest.mark.parametrize("case,name", [(rc.F32_SHAPES[0], "lanczos"), (rc.F32_SHAPES[1], "bilinear"), (rc.F32_SHAPES[4], "bicubic")],
                         ids=lambda v: v if isinstance(v, str) else rc.shape_id(v))
def test_f32_nan_and_inf_follow_the_table(lib, dev, case, name):
    """NaN and Inf entries are ordinary inputs: NaN exactly where the restatement has NaN (every tap inside the bounds is multiplied,
    zero coefficients included), the same infinities, and the bounded values everywhere else."""
    flow = rc.f32_input(case)
    H, W = flow.shape[2:]
    flow[0, 0, H // 2, W // 3] = np.nan
    flow[0, 1, H // 4, W // 2] = np.inf
    flow[1, 0, H - 1, W - 1] = -np.inf
    flow[1, 1, 0, 0] = np.nan
    flow[1, 1, H // 2, W // 2:W // 2 + 2] = (np.inf, -np.inf)
    want = rc.resize_f64(flow, case[1], name, 1.75, 0.4)
    bound = rc.bound_f32(flow, case[1], name, 1.75, 0.4)
    call = CallF32(lib, dev, flow, case[1], name, True)
    assert call.run(1.75, 0.4) == 0, lib.sf_last_error()
    got = call.result().astype(np.float64)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).sum() > want.size // 2
    assert np.array_equal(np.isnan(got), np.isnan(want))
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf])
    fin = np.isfinite(want)
    assert np.isfinite(bound[fin]).all() and (np.abs(got[fin] - want[fin]) <= bound[fin]).all()


def test_bad_arguments_launch_nothing(lib, dev):
    case = rc.U8_SHAPES[2]
    img = rc.u8_input(case, "noise")
    call = CallU8(lib, dev, img, case[1], "lanczos", "hwc")
    tab = list(call.tab.args)

    def with_tab(i, v):
        t = list(tab)
        t[i] = v
        return dict(tab=t)

    for bad in (dict(src=None), dict(out=None), dict(ws=None), dict(n=0), dict(n=65536), dict(H=0), dict(W=0), dict(h=0), dict(w=0), dict(rs=-1),
                with_tab(0, None), with_tab(1, None), with_tab(3, None), with_tab(4, None), with_tab(2, 0), with_tab(2, 98), with_tab(5, 98),
                dict(out=call.out.ptr + 1), dict(ws=call.ws.ptr + 2), dict(ws_bytes=call.need - 1)):
        assert call.run(**bad) == -1, bad
        assert b"sf_resize_u8" in lib.sf_last_error(), bad
    call.result()
    assert bool((call.out.view() == OUT_FILL).all()) and bool((call.ws.view() == WS_FILL).all())
    assert lib.sf_resize_u8_ws_bytes(0, 4, 4, 2, 2) == -1 and lib.sf_resize_u8_ws_bytes(1, 1 << 15, 1 << 15, 2, 2) == -1
    assert call.run() == 0, lib.sf_last_error()                          # ... and the good call does write
    assert np.array_equal(call.result(), rc.resize_u8(img, case[1], "lanczos"))

    fcase = rc.F32_SHAPES[0]
    flow = rc.f32_input(fcase)
    fc = CallF32(lib, dev, flow, fcase[1], "lanczos", True)
    tab = list(fc.tab.args)
    for bad in (dict(src=None), dict(out=None), dict(ws=None), dict(n=0), dict(n=32768), dict(H=0), dict(W=0), dict(h=0), dict(w=0),
                dict(rs=fc.W - 1), dict(cs=0), with_tab(0, None), with_tab(1, None), with_tab(3, None), with_tab(4, None), with_tab(2, 98),
                with_tab(5, 0), dict(out=fc.out.ptr + 2), dict(src=fc.ptr + 2), dict(ws=fc.ws.ptr + 2), dict(ws_bytes=fc.need - 1)):
        assert fc.run(**bad) == -1, bad
        assert b"sf_resize_f32" in lib.sf_last_error(), bad
    fc.result()
    assert bool((fc.out.view() == OUT_FILL).all()) and bool((fc.ws.view() == WS_FILL).all())
    assert lib.sf_resize_f32_ws_bytes(32768, 4, 4, 2, 2) == -1
    assert fc.run() == 0, lib.sf_last_error()
    assert (np.abs(fc.result() - rc.resize_f64(flow, fcase[1], "lanczos")) <= rc.bound_f32(flow, fcase[1], "lanczos")).all()
