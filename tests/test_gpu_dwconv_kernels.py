"""The depthwise 15 x 15 / 7 x 7 layer of the SK blocks -- sf_dwconv_res_gelu, sf_dwconv_res_gelu_f16in (csrc/conv.hip: the fp32 stencil
and the banded-Toeplitz kernel on the matrix cores) -- through the C ABI (-m gpu): raw pointers and strides handed to
streamflow_amd._lib.load(), not ops.dwconv_res_gelu (which only ever passes tight strides and offset 0), at the smallest shapes that
reach each branch of dwconv_dispatch (tests/dwconv_cases.py: plan() restates it; tests/test_dwconv_cases_cpu.py pins the case table,
the models, the bound and its teeth).

x, wgt and bias sit in guard-banded buffers whose padding holds 3e4 (a read outside a view that reaches a result moves it by
thousands of bounds; NaN would not show: see the last test), y in one filled with NaN.  Every run asserts: status 0; every element of
the y view finite; nothing outside any view changed and no input changed; the bound of tests/dwconv_cases.py per element against
model64 (the class's operand model in float64).  Bitwise: the placed run (base off the allocation's start, image strides beyond the
span, different for x and y) equals the contiguous one wherever both take the same arithmetic form -- vector and scalar stores of the
stencil, float4 and element staging of the matrix-core kernel, a DMA placement that keeps the DMA form; image z of a batch equals the
run on image z alone; FP32 and F16X3 at K = 7 (both the stencil); the widest accepted planes against a plane one tile narrower.  Pair
rules of tests/test_gpu_parity.py: fp16 y against fp32 y of the same call (erf forms), fp16 input against fp32 input of the same
values, the DMA form against the register form.  One non-finite value: see test_one_bad_value_stays_in_its_window.

err / tol is printed per run ("DWCONV ..."), the worst per kernel form and class at the end ("DWCONV WORST ...").  On an MI355X,
70 tests in 10 s, the slowest 1.1 s (ipw_reg 8 x 8, C 324, n 15, K 15: 90 single-image runs):
    fp32 output (erf form): stencil and every matrix-core form at most 0.17 (F16X2, K 15, ragged 17 x 33, std; 0.174 on 33 x 248, gain).
    fp16 output: 0.96 .. 0.99 in every form and class but mean100 (0.66) -- the bound's fp16 rounding term is attained (half an
        ulp): stencil 0.988 (1000 x 4, K 15, gain), F16X3 0.988 (8 x 8, C 324, std), two / one product on fp32 input 0.991 (8 x 8,
        C 640, K 7, tiny), fp16 rows through registers 0.976 (40 x 240, K 7, gain), by DMA 0.981 (80 x 8, C 128, n 13, K 15, gain).
    No case exceeded its bound: the residual's split (2^-20 |x| in F16X3) is part of the operand model, so the mean100 class holds.
    One bad value: asserted by test_one_bad_value_stays_in_its_window (225 / 49 outputs change in the stencil, 480 / 224 on the
        matrix cores; none is NaN).
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests import dwconv_cases as dc
from tests import test_dwconv_cases_cpu as ref
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 3.0e4                                                   # around the input views: finite (both GELU forms turn a NaN pre-activation into
                                                              # a number near zero, so a NaN would hide), exact in fp16, and thousands of
                                                              # bounds large in any result it reaches
TAIL = 64
CASES = dc.cases()
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "dwconv_stencil_v126.json")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _lib():
    from streamflow_amd import _lib as L
    return L


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b.to(a.device))))


def _untouched(G):
    return _same(G.buf, G.snap if hasattr(G, "snap") else torch.full_like(G.buf, G.fill))


class Run:
    """One call.  x [n][C][h w] float32 numpy (fp16 values for the fp16 entry point)."""

    def __init__(self, dev, x, wgt, b, h, w, entry, precision, y_f16, xform=None, yform=None, placed=False):
        lib = _lib().load()
        n, C, _ = x.shape
        k = wgt.shape[-1]
        y_f16 = 1 if entry == "f16in" else y_f16
        xdt = torch.float16 if entry == "f16in" else torch.float32
        ydt = torch.float16 if y_f16 else torch.float32
        xform = xform or ("f16_any" if entry == "f16in" else "f32_any")
        yform = yform or ("f16_any" if y_f16 else "f32_any")
        span = C * h * w
        xo, xs = dc.place(xform, span, placed, 0)
        yo, ys = dc.place(yform, span, placed, 1)
        wo = 1 if placed else 0
        self.X = Guarded(dev, n, C, h * w, xo, h * w, xs, PAD, xdt, tail=TAIL).put(torch.from_numpy(x))
        self.W = Guarded(dev, 1, 1, C * k * k, wo, C * k * k, C * k * k, PAD, tail=TAIL).put(torch.from_numpy(wgt))
        self.B = Guarded(dev, 1, 1, C, 3 * wo, C, C, PAD, tail=TAIL).put(torch.from_numpy(b))
        self.Y = Guarded(dev, n, C, h * w, yo, h * w, ys, NAN, ydt, tail=TAIL)
        assert self.X.buf.data_ptr() % 16 == 0 and self.Y.buf.data_ptr() % 16 == 0
        self.plan = dc.plan(entry, precision, k, y_f16, n, C, h, w, self.X.ptr % 16, self.Y.ptr % 16, xs, ys)
        self.y_f16, self.shape = y_f16, (n, C, h, w)
        if entry == "f16in":
            self.status = lib.sf_dwconv_res_gelu_f16in(self.X.ptr, xs, self.W.ptr, self.B.ptr, self.Y.ptr, ys, n, C, h, w, k, precision, _lib().stream())
        else:
            self.status = lib.sf_dwconv_res_gelu(self.X.ptr, xs, self.W.ptr, self.B.ptr, self.Y.ptr, ys, y_f16, n, C, h, w, k, precision, _lib().stream())
        torch.cuda.synchronize()
        self.msg = lib.sf_last_error().decode(errors="replace") if self.status else ""

    def y(self):
        return self.Y.region().view(self.shape)

    def check(self, what, finite=True):
        assert self.plan["refused"] is None, (what, self.plan)
        assert self.status == 0, (what, self.status, self.msg)
        if finite:
            assert bool(torch.isfinite(self.y().float()).all()), (what, "a cell of y was not written")
        assert self.Y.outside_unchanged(), (what, "an element outside the y view changed")
        for f in (self.X, self.W, self.B):
            assert _untouched(f), (what, "an input buffer changed")
        return self


WORST = {}


def _bound(what, run, cid, cls):
    c = ref.BY_ID[cid]
    pl = run.plan
    _, _, _, _, y64, tol, _, _ = ref.expect(cid, cls, ref.key(pl, run.y_f16))
    err = (run.y().double().cpu() - y64).abs().numpy()
    r = float((err / tol).max())
    print(f"DWCONV {pl['kernel']} prod{pl['prod']} {pl['form']} {pl['gelu']} {what}: err {float(err.max()):.3e} ratio {r:.3f}")
    kk = (pl["kernel"], pl["prod"], pl["form"], pl["gelu"], cls)
    if r > WORST.get(kk, (0.0, ""))[0]:
        WORST[kk] = (r, what)
    assert r <= 1.0, (what, c["id"], r, float(err.max()))


def _pair(what, a, b, rel, absolute, vs="b"):
    a, b = a.float(), b.float()
    scale = b.abs() if vs == "b" else torch.maximum(a.abs(), b.abs())
    d = (a - b).abs()
    assert bool((d <= rel * scale + absolute).all()), (what, float(d.max()))


# ---- every case ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case(dev, case):
    c = case
    n, C, h, w, k, entry = c["n"], c["C"], c["h"], c["w"], c["k"], c["entry"]
    small = n * C * h * w <= dc.ALL_CLASSES_BELOW
    for cls in c["classes"]:
        x, wgt, b = dc.draw(c, cls)
        kept = {}
        for precision, y_f16 in c["variants"]:
            what = f"{c['id']} {dc.PREC_NAME[precision]} y16={y_f16} {cls}"
            stencil = c["family"] == "stencil"
            vec_x = "f16_dma" if entry == "f16in" else ("f32_vec" if w % 4 == 0 else "f32_any")
            vec_y = ("f16_vec" if y_f16 else "f32_vec") if stencil and w % 4 == 0 else None
            r0 = Run(dev, x, wgt, b, h, w, entry, precision, y_f16).check(what)
            assert r0.plan["kernel"] == c["family"]
            _bound(what, r0, c["id"], cls)
            y0 = kept[(precision, y_f16)] = r0.y().clone()
            dma = r0.plan["form"] == "f16dma"
            # placed: the same access width where the shape allows one ...
            r1 = Run(dev, x, wgt, b, h, w, entry, precision, y_f16, vec_x if (dma or entry == "f32") else None, vec_y, placed=True).check(what + " placed")
            assert r1.plan["form"] == r0.plan["form"] and r1.X.stride != r1.Y.stride and r1.X.stride > C * h * w
            if stencil and w % 4 == 0:
                assert r0.plan["vec_store"] and r1.plan["vec_store"]
            if not stencil and entry == "f32" and w % 4 == 0:
                assert r0.plan["vec_ok"] and r1.plan["vec_ok"]
            assert _same(r1.y(), y0), (what, "the placed run is not bitwise the contiguous one")
            # ... and the element-wise one (scalar stores, element staging)
            if (stencil or entry == "f32") and w % 4 == 0 and (small or cls == "std"):
                r2 = Run(dev, x, wgt, b, h, w, entry, precision, y_f16, placed=True).check(what + " placed, one element off")
                assert not (r2.plan["vec_store"] if stencil else r2.plan["vec_ok"])
                assert _same(r2.y(), y0), (what, "vector and element-wise access differ")
            # fp16 rows that leave the DMA form by their base, then by their stride: the register form
            if dma and small:
                regs = []
                for form in ("f16_halfoff", "f16_oddstride"):
                    r3 = Run(dev, x, wgt, b, h, w, entry, precision, 1, form, placed=True).check(what + " " + form)
                    assert r3.plan["form"] == "f16reg", form
                    _bound(what + " " + form, r3, c["id"], cls)
                    _pair(what + " dma / registers", r3.y(), y0, dc.PAIR_IN_REL, dc.PAIR_IN_ABS, vs="max")
                    regs.append(r3.y().clone())
                assert _same(regs[0], regs[1]), (what, "two placements of the register form differ")
            # image z of the batch alone
            if n > 1 and cls == "std":
                for z in range(n):
                    rz = Run(dev, x[z:z + 1], wgt, b, h, w, entry, precision, y_f16).check(f"{what} image {z}")
                    assert rz.plan["form"] == r0.plan["form"]
                    assert _same(rz.y(), y0[z:z + 1]), (what, z, "an image of a batch differs from the image alone")
            # the fp32 entry point on the same fp16 values
            if entry == "f16in" and cls == "std" and (small or c["name"] in ("cliff", "wide15", "wide7")):
                rf = Run(dev, x, wgt, b, h, w, "f32", precision, 1).check(what + " as fp32 input")
                _pair(what + " fp16 / fp32 input", y0, rf.y(), dc.PAIR_IN_REL, dc.PAIR_IN_ABS, vs="max")
        for precision in {p for p, _ in c["variants"]}:                        # fp16 y against fp32 y, erf forms
            if (precision, 0) in kept and (c["family"] == "stencil" or precision == dc.F16X3):
                _pair(f"{c['id']} {cls} fp16 y / fp32 y", kept[(precision, 1)], kept[(precision, 0)], dc.PAIR_F16_Y_REL, dc.PAIR_F16_Y_ABS)
        if c["family"] == "stencil" and k == 7:
            for y_f16 in (0, 1):
                assert _same(kept[(dc.FP32, y_f16)], kept[(dc.F16X3, y_f16)]), (c["id"], cls, "FP32 and F16X3 at K = 7 both run the stencil")


# ---- the stencil before its strip was shortened to fit ----------------------------------------------------------------------------------
def _digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def recorded_runs(dev):
    """{key: digest of y} for the recorded cases, every variant, the existing tests' class, contiguous."""
    out = {}
    for c in CASES:
        if c["name"] in dc.RECORDED:
            x, wgt, b = dc.draw(c, "std")
            out[c["id"] + " inputs"] = hashlib.sha256(x.tobytes() + wgt.tobytes() + b.tobytes()).hexdigest()
            for precision, y_f16 in c["variants"]:
                r = Run(dev, x, wgt, b, c["h"], c["w"], "f32", precision, y_f16)
                assert r.status == 0, (c["id"], r.status, r.msg)
                out[f"{c['id']} {dc.PREC_NAME[precision]} y16={y_f16}"] = _digest(r.y())
    return out


def test_stencil_results_of_shapes_accepted_before_are_bitwise_what_they_were(dev):
    """33 x 256 and 40 x 604 against the digests of a run of the library before the strip was shortened to fit LDS (SF_VERSION 126),
    recorded once on an MI355X: tests/golden/dwconv_stencil_v126.json."""
    want = json.load(open(GOLDEN))
    got = recorded_runs(dev)
    assert got.keys() == want.keys() and len(got) == 8 + 3
    for f in want:
        assert got[f] == want[f], f


# ---- the widest planes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", dc.KSIZES)
def test_widest_plane_against_one_tile_narrower(dev, k):
    """16 x 480 (K = 15) / 16 x 704 (K = 7): the columns whose footprint lies inside the first w - 16 columns are bitwise those of
    the plane made of these columns alone."""
    w, h, R = dc.MFMA_WIDEST[k], 16, k // 2
    for entry in ("f32", "f16in"):
        (c,) = [c for c in CASES if c["name"] == f"wide{k}" and c["entry"] == entry]
        x, wgt, b = dc.draw(c, "std")
        xn = np.ascontiguousarray(x.reshape(1, 1, h, w)[..., : w - 16]).reshape(1, 1, -1)
        for precision, y_f16 in c["variants"]:
            what = f"wide K{k} {entry} {dc.PREC_NAME[precision]} y16={y_f16}"
            a = Run(dev, x, wgt, b, h, w, entry, precision, y_f16).check(what)
            n_ = Run(dev, xn, wgt, b, h, w - 16, entry, precision, y_f16).check(what + " narrower")
            assert a.plan["form"] == n_.plan["form"] or entry == "f16in"
            if a.plan["form"] == n_.plan["form"]:
                assert _same(a.y()[..., : w - 16 - R], n_.y()[..., : w - 16 - R]), what
            else:
                _pair(what, a.y()[..., : w - 16 - R], n_.y()[..., : w - 16 - R], dc.PAIR_IN_REL, dc.PAIR_IN_ABS, vs="max")


# ---- one bad value ------------------------------------------------------------------------------------------------------------------------
# (entry, precision, K, y_f16, placement of x): fp16 rows dense take the DMA form, one half off the register form
POISON_RUNS = [("f32", dc.FP32, 15, 0, None), ("f32", dc.FP32, 7, 1, None), ("f32", dc.F16X3, 15, 0, None), ("f32", dc.F16X2, 15, 0, None),
               ("f32", dc.F16X2, 7, 1, None), ("f32", dc.F16, 15, 1, None), ("f16in", dc.F16X2, 15, 1, None), ("f16in", dc.F16X2, 7, 1, None),
               ("f16in", dc.F16, 7, 1, None), ("f16in", dc.F16X2, 15, 1, "f16_halfoff"), ("f16in", dc.F16, 7, 1, "f16_halfoff")]


@pytest.mark.parametrize("entry,precision,k,y_f16,xform", POISON_RUNS,
                         ids=[f"{e}-{dc.PREC_NAME[p]}-K{k}-y16={y}-{f or 'dense'}" for e, p, k, y, f in POISON_RUNS])
def test_one_bad_value_stays_in_its_window(dev, entry, precision, k, y_f16, xform):
    """One NaN, then one +inf (fp32 input on the matrix cores: also one 1e5, beyond fp16) at pixel (y0, x0) of one plane.  Asserted:
    no output of any plane is NaN -- both GELU forms clamp their argument with max / med3, which return the other operand for a
    NaN, so a NaN (and a -inf) pre-activation leaves as a number within the form's absolute error of zero;
    the set of outputs that differ bitwise from the clean run is EXACTLY the K x K footprint (stencil; F16X3 with 1e5, whose
    truncating split keeps it finite) or EXACTLY rows y0 +- R of the 16-column tiles whose 32-column window holds x0 (matrix cores:
    the band's structural zeros times a non-finite value are NaN); every other plane is bitwise clean;
    NaN: every changed output is that near-zero number;
    +inf (and 1e5 in the two- and one-product forms, whose hi half is inf): a changed output is +inf or near zero, near zero where
    its tap weight is negative and outside the footprint; stencil: +inf wherever the tap weight is positive (at the pixel itself
    only if the centre tap is: inf - inf otherwise); F16X3: near zero everywhere (lo = inf - inf)."""
    n, C, h, w = dc.POISON_SHAPE
    zi, ci, y0, x0 = dc.POISON_AT
    R = k // 2
    rng = np.random.default_rng(77 + k)
    x = rng.standard_normal((n, C, h * w)).astype(np.float32)
    if entry == "f16in":
        x = x.astype(np.float16).astype(np.float32)
    wgt = (rng.standard_normal((C, k, k)) / k).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    go = lambda xx: Run(dev, xx, wgt, b, h, w, entry, precision, y_f16, xform, None, placed=xform is not None)   # noqa: E731
    clean = go(x).check("clean")
    pl = clean.plan
    kernel = pl["kernel"]
    if entry == "f16in":
        assert pl["form"] == ("f16reg" if xform else "f16dma")
    may, foot = dc.poison_sets(h, w, k, y0, x0, kernel)
    may_t, foot_t = torch.from_numpy(may).to(dev), torch.from_numpy(foot).to(dev)
    near0 = dc.ERF_ABS if pl["gelu"] == "erf" else dc.POLY_ABS
    ys, xs = np.nonzero(foot)
    tap = torch.from_numpy(wgt[ci][y0 - ys + R, x0 - xs + R].copy()).to(dev)       # output (y, x) holds x0 through tap (y0 - y + R, x0 - x + R)
    pixel = torch.from_numpy((ys == y0) & (xs == x0)).to(dev)
    yc = clean.y()
    others = torch.ones(n, C, dtype=torch.bool, device=dev)
    others[zi, ci] = False
    for v in [NAN, float("inf")] + ([1e5] if entry == "f32" and kernel == "mfma" else []):
        what = f"{kernel} {entry} {dc.PREC_NAME[precision]} K{k} {pl['form']} value {v}"
        xb = x.copy()
        xb.reshape(n, C, h, w)[zi, ci, y0, x0] = v
        r = go(xb).check(what, finite=False)
        yb = r.y()
        assert not bool(torch.isnan(yb.float()).any()), (what, "an output is NaN")
        assert _same(yb[others], yc[others]), (what, "another plane changed")
        got = yb[zi, ci].float()
        changed = _bits(yb[zi, ci]) != _bits(yc[zi, ci])
        finite_1e5 = v == 1e5 and pl["prod"] == 3
        want = foot_t if kernel == "stencil" or finite_1e5 else may_t
        print(f"DWCONV poison {what}: {int(changed.sum())} outputs changed, window {int(want.sum())}, {int(torch.isinf(got).sum())} inf")
        assert bool((changed == want).all()), (what, int(changed.sum()), int(want.sum()), "the changed outputs are not exactly the window")
        if finite_1e5:
            assert bool(torch.isfinite(got).all())
            continue
        ch = got[changed]
        assert bool(((ch == float("inf")) | (ch.abs() <= near0)).all()), (what, "a changed output is neither +inf nor near zero")
        inside = got[foot_t]
        if v != v or pl["prod"] == 3:
            assert not bool(torch.isinf(got).any()), what
        else:
            assert bool((got[changed & ~foot_t].abs() <= near0).all()), what
            assert bool((inside[(tap < 0) & ~pixel].abs() <= near0).all()), (what, "a negative tap of +inf is not near zero")
            pos = inside[(tap > 0) & ~pixel] == float("inf")
            assert float(pos.float().mean()) >= 0.9, (what, "positive taps of +inf are not +inf")
            if kernel == "stencil":
                assert bool(pos.all())
                centre = float(wgt[ci, R, R])
                assert (float(got[y0, x0]) == float("inf")) == (centre > 0), (what, centre)


# ---- refusals on real buffers -------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(dev):
    """The refused argument sets of tests/dwconv_cases.py with real guard-banded buffers: SF_ERR_BAD_ARG, y bitwise untouched."""
    lib = _lib().load()
    X = Guarded(dev, 1, 1, 4096, 0, 4096, 4096, NAN, tail=TAIL).put(torch.zeros(1, 1, 4096))
    W = Guarded(dev, 1, 1, 4096, 0, 4096, 4096, NAN, tail=TAIL).put(torch.zeros(1, 1, 4096))
    B = Guarded(dev, 1, 1, 64, 0, 64, 64, NAN, tail=TAIL).put(torch.zeros(1, 1, 64))
    Y = Guarded(dev, 1, 1, 4096, 0, 4096, 4096, NAN, tail=TAIL)
    ptrs = {"x": (X.ptr, 4096), "wgt": (W.ptr, 0), "bias": (B.ptr, 0), "y": (Y.ptr, 4096)}
    for r in dc.refusals():
        st, msg = ref.call_refused(lib, r, ptrs)
        torch.cuda.synchronize()
        assert st == dc.SF_ERR_BAD_ARG and msg, (r, st, msg)
        assert _untouched(Y) and _untouched(X), r


def test_zz_worst_ratios():
    """Prints the worst err / tol per kernel form and class of this session's runs (the docstring's table)."""
    for kk, (r, what) in sorted(WORST.items()):
        print(f"DWCONV WORST {kk}: {r:.3f} at {what}")
    assert all(r <= 1.0 for r, _ in WORST.values())
