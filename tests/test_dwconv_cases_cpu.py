"""CPU: the restatement, operand models, bounds, plan and case lists of tests/test_gpu_dwconv_kernels.py (tests/dwconv_cases.py).

1. ref_dwconv -- y = gelu(x + dwconv(x) + b) with zero padding, written tap by tap -- equals F.conv2d in float64 and, put in place of
   the depthwise steps of the oracle's SK block, reproduces the reference's golden SK blocks (tests/golden/skblock.npz).
2. split8 / split8_rn emulated bit by bit: the halves are fp16 values, hi + lo is within 2^-20 / 2^-22 of x, truncation and rounding
   go the way csrc/split_operand.h says.
3. Both GELU forms of csrc/sf_common.h restated; their errors on a grid over [-12, 12] against the figures the bound uses.
4. The kernel emulated (the class's operand model in torch float32, the GELU form in fp32, the output rounded) sits inside HALF the
   bound around model64 for fp32 output; for fp16 output inside the bound with its accumulation term counted by half (the half-ulp
   rounding and the polynomial's minimax error are attained by a right kernel).  On the existing tests' class the derived bound is
   under its cap without being cut.
5. Teeth: each wrong kernel of the list is at least TEN bounds off somewhere on a named case of every class it applies to.
6. plan(): every branch of the case table is reached by a named case, with the facts the table states.
7. Refusals: the library answers SF_ERR_BAD_ARG, with a message, for every argument set of dwconv_cases.refusals(), called with
   dummy pointers that are never dereferenced (no accepted argument set is ever called that way), and plan() refuses the same sets."""
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dwconv_cases as dc

F64, F32 = torch.float64, torch.float32
CASES = dc.cases()
BY_ID = {c["id"]: c for c in CASES}


def _named(name, k=None, entry=None):
    return [c for c in CASES if c["name"] == name and (k is None or c["k"] == k) and (entry is None or c["entry"] == entry)]


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def conv_taps(x, wgt, rows=None):
    """x [n][C][h][w], wgt [C][K][K]: out[y][x] = sum over (ky, kx), in that order, of wgt[ky][kx] * x[y + ky - R][x + kx - R], zero
    outside the plane.  rows: {ky: [h] mask} -- tap row ky only counts for the output rows of the mask (wrong kernels)."""
    K = wgt.shape[-1]
    R = K // 2
    n, C, h, w = x.shape
    xp = F.pad(x, (R, R, R, R))
    out = torch.zeros_like(x)
    for ky in range(K):
        for kx in range(K):
            t = xp[:, :, ky:ky + h, kx:kx + w] * wgt[:, ky, kx].view(1, C, 1, 1)
            if rows is not None and ky in rows:
                t = t * rows[ky].to(x.dtype).view(1, 1, h, 1)
            out = out + t
    return out


def ref_dwconv(x, wgt, b):
    """update.py:33-34 with kernel 15 / 7: gelu(x + dwconv(x) + b)."""
    return gelu(x + conv_taps(x, wgt) + b.view(1, -1, 1, 1))


# ---- the models -------------------------------------------------------------------------------------------------------------------
WRONG = ("flip", "halo", "band_shift", "no_res", "fold_and_res", "bias_twice", "w_f16", "x_f16", "res_hi", "neighbour", "stale_row")


def applies(wrong, pl, case):
    two_strips = pl["strips"] > 1
    return {"fold_and_res": pl["fold"], "w_f16": pl["prod"] == 2, "x_f16": pl["prod"] == 3, "res_hi": pl["kernel"] == "mfma" and pl["form"] == "f32",
            "neighbour": case["C"] > 1, "halo": two_strips, "stale_row": two_strips}.get(wrong, True)


def model_pre(pl, x, wgt, b, h, w, dtype, wrong=None):
    """The pre-activation as the kernel of plan `pl` forms it, evaluated in `dtype`: the products one after the other into one
    accumulator, the bias, then the residual.  x [n][C][h w], wgt [C][K][K], b [C] numpy float32."""
    n, C, _ = x.shape
    K = wgt.shape[-1]
    R = K // 2
    if wrong == "flip":
        wgt = wgt[:, ::-1, ::-1].copy()
    elif wrong == "band_shift":
        wgt = np.concatenate([wgt[:, :, 1:], np.zeros_like(wgt[:, :, :1])], axis=2)
    elif wrong == "neighbour":
        wgt = np.roll(wgt, -1, axis=0)
    prods, res = dc.operands(pl, x, wgt, wrong if wrong in ("w_f16", "x_f16", "res_hi", "no_res") else None)
    T = lambda a, shape: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).view(shape)   # noqa: E731
    rows = None
    ys = torch.arange(h)
    first = (ys % pl["strip_h"] == 0) & (ys > 0)
    last = (ys % pl["strip_h"] == pl["strip_h"] - 1) & (ys < h - 1)
    if wrong == "halo":                                       # a halo of R - 1: the strip's outermost halo rows are missing
        rows = {0: ~first, K - 1: ~last}
    acc = None
    for xp, wp in prods:
        t = conv_taps(T(xp, (n, C, h, w)), T(wp, (C, K, K)), rows)
        acc = t if acc is None else acc + t
    if wrong == "stale_row":                                  # a strip's first staged row is still the previous strip's first row
        xp, wp = prods[-1]
        xt = F.pad(T(xp, (n, C, h, w)), (R, R, R + pl["strip_h"], 0))
        for y0 in ys[first].tolist():
            good, stale = xt[:, :, y0 + pl["strip_h"]], xt[:, :, y0]         # input rows y0 - R and y0 - strip_h - R
            for kx in range(K):
                acc[:, :, y0] += T(wp, (C, K, K))[:, 0, kx].view(1, C, 1) * (stale - good)[:, :, kx:kx + w]
    pre = acc + T(b, (1, C, 1, 1)) * (2 if wrong == "bias_twice" else 1)
    if res is not None and wrong != "no_res":
        pre = (T(res[0], (n, C, h, w)) + T(res[1], (n, C, h, w))) + pre
    if wrong == "fold_and_res":
        pre = T(x, (n, C, h, w)) + pre
    return pre


@functools.lru_cache(maxsize=6)
def expect(cid, cls, pl_key):
    """(x, wgt, b, pre64, y64, tol [n][C][h][w]) for case `cid`, class `cls` and the plan given as a sorted item tuple."""
    c, pl = BY_ID[cid], dict(pl_key)
    x, wgt, b = dc.draw(c, cls)
    pre64 = model_pre(pl, x, wgt, b, c["h"], c["w"], F64)
    pre32 = model_pre(pl, x, wgt, b, c["h"], c["w"], F32)
    y64 = gelu(pre64)
    ptol = dc.pre_tol(pre32.numpy(), pre64.numpy())
    tol = dc.bound(pre64.numpy(), y64.numpy(), ptol, pl["gelu"], pl["y_f16"], cls)
    return x, wgt, b, pre64, y64, tol, pre32, ptol


def key(pl, y_f16):
    return tuple(sorted({**pl, "y_f16": y_f16}.items(), key=lambda kv: kv[0]))


def plan_of(c, precision, y_f16, **kw):
    return dc.plan(c["entry"], precision, c["k"], y_f16, c["n"], c["C"], c["h"], c["w"], **kw)


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", dc.KSIZES)
def test_restatement_equals_conv2d(k):
    g = torch.Generator().manual_seed(k)
    n, C, h, w = 2, 3, 9, 20
    x, wgt, b = torch.randn(n, C, h, w, generator=g).double(), torch.randn(C, k, k, generator=g).double() / k, torch.randn(C, generator=g).double()
    want = F.gelu(x + F.conv2d(x, wgt.view(C, 1, k, k), b, padding=k // 2, groups=C))
    assert float((ref_dwconv(x, wgt, b) - want).abs().max()) < 1e-13


def test_restatement_reproduces_the_golden_sk_blocks(golden, monkeypatch):
    """The oracle's SK block with its depthwise steps computed by ref_dwconv: tolerance of test_oracle_golden.py::test_skblocks."""
    from oracle import streamflow_oracle as orc
    from streamflow_amd import synthetic as syn
    from tests import cases
    g = golden("skblock")
    P = syn.make_params(cases.SKBLOCK_SEED, 4)
    real = F.conv2d
    used = []

    def conv2d(x, wgt, bias=None, stride=1, padding=0, dilation=1, groups=1):
        if groups > 1 and wgt.shape[-1] in dc.KSIZES:
            used.append(wgt.shape[-1])
            return conv_taps(x, wgt[:, 0]) + bias.view(1, -1, 1, 1)
        return real(x, wgt, bias, stride, padding, dilation, groups)

    monkeypatch.setattr(orc.F, "conv2d", conv2d)
    for name, cin, cout, kc in cases.SKBLOCK_CASES:
        out = orc.skblock(cases.skblock_inputs(name, cin), P, "update_block." + name, kc)
        want = g[name.replace(".", "_")]
        assert bool((np.abs(out.numpy() - want) <= 2e-5 + 1e-5 * np.abs(want)).all()), name
    assert set(used) == set(dc.KSIZES)


# ---- 2. the splits ------------------------------------------------------------------------------------------------------------------
def test_splits_bit_by_bit():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(4000) * s for s in (1.0, 100.0, 1e-4, 3e3)]).astype(np.float32)
    x = np.concatenate([x, np.float32([0.0, -0.0, 1.0, 65504.0, 2.0 ** -14, 2.0 ** -24, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11])]).astype(np.float64)
    for fn, rel in ((dc.split8, 2.0 ** -20), (dc.split8_rn, 2.0 ** -22)):
        hi, lo = fn(x)
        for part in (hi, lo):
            assert np.array_equal(part.astype(np.float16).astype(np.float64), part)
        assert bool((np.abs(x - (hi + lo)) <= rel * np.abs(x) + 2.0 ** -24).all()), fn.__name__
    hi, lo = dc.split8(x)
    assert bool((np.abs(hi) <= np.abs(x)).all()) and bool((np.abs(hi + lo) <= np.abs(x)).all())          # towards zero, twice
    big = np.abs(x) >= 2.0 ** -14
    assert np.array_equal(hi[big], (x[big].astype(np.float32).view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32).astype(np.float64))
    hi, lo = dc.split8_rn(x)
    assert np.array_equal(hi, x.astype(np.float16).astype(np.float64))                                  # to nearest, ties to even
    assert dc.split8_rn(np.float64([1.0 + 2.0 ** -11]))[0][0] == 1.0 and dc.split8_rn(np.float64([1.0 + 3 * 2.0 ** -11]))[0][0] == 1.0 + 2.0 ** -9
    assert bool((np.abs(lo) <= 2.0 ** -11 * np.abs(x) + 2.0 ** -25).all())


# ---- 3. the GELU forms --------------------------------------------------------------------------------------------------------------
def test_gelu_forms_on_a_grid():
    """What csrc/sf_common.h states, and where it did not hold (its comments now carry the measured figures)."""
    x = np.linspace(-12.0, 12.0, 480001)
    exact = gelu(torch.from_numpy(x)).numpy()
    for single in (False, True):
        e = np.abs(dc.gelu_erf_form(x, single) - exact)
        assert e[x <= 4.0].max() <= 1.3e-6                                       # the stated absolute figure, up to the fit's range
        assert bool((e <= dc.gelu_term(x, exact, "erf") - 2.0 ** -25 * np.abs(x)).all())                # (v_rcp_f32's ulp left over)
        p = np.abs(dc.gelu_poly_form(x, single) - exact)
        assert p[x <= 8.0].max() <= dc.POLY_ABS and bool((p <= dc.gelu_term(x, exact, "poly")).all())
    # findings: 2.25e-7 |x| (erf form) and "5.2e-5 for every x", "1.1e-5 relative" (polynomial) are exceeded
    e = np.abs(dc.gelu_erf_form(x, True) - exact)
    assert (e / np.maximum(np.abs(x), 1e-9))[x > 4].max() > 2.25e-7
    p = np.abs(dc.gelu_poly_form(x, False) - exact)
    assert p.max() > 5.2e-5 and (p[x > 0.01] / exact[x > 0.01]).max() > 1.1e-5
    assert bool((dc.gelu_poly_form(x, False)[x < -4.3] > -5.2e-5).all())          # the far negative tail stays inside the absolute figure


# ---- 4. models inside half the bound, bounds under the caps -------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_models_inside_half_the_bound_and_bounds_under_the_caps(case):
    c = case
    for precision, y_f16 in c["variants"]:
        pl = plan_of(c, precision, y_f16)
        assert pl["refused"] is None and pl["kernel"] == c["family"], (c["id"], precision, pl)
        for cls in c["classes"]:
            x, wgt, b, pre64, y64, tol, pre32, ptol = expect(c["id"], cls, key(pl, y_f16))
            form = dc.gelu_erf_form if pl["gelu"] == "erf" else dc.gelu_poly_form
            emu = dc.round_out(form(pre32.numpy(), single=True), y_f16)
            err = np.abs(emu - y64.numpy())
            # fp32 output: inside half the bound, as the rule is worded.  fp16 output: the half-ulp rounding and the polynomial's
            # minimax error are attained by a right kernel, so they count in full and the accumulation term P by half
            limit = 0.5 * tol if not y_f16 else tol - 0.5 * 1.13 * ptol
            assert bool((err <= limit).all()), (c["id"], dc.PREC_NAME[precision], y_f16, cls, float((err / tol).max()))
            if cls == "std":                                 # the cap never binds: the derived bound is under it as it stands
                free = dc.bound(pre64.numpy(), y64.numpy(), ptol, pl["gelu"], y_f16, None)
                assert bool((free <= (dc.cap_f16(y64.numpy()) if y_f16 else dc.CAP_F32)).all()) and np.array_equal(free, tol)


# ---- 5. teeth -----------------------------------------------------------------------------------------------------------------------
TEETH_CASES = ("ragged", "exact", "strip1row15", "strip1row7", "s_ragged", "s_strips")
TEETH_CLASSES = ("std", "gain")


def _klass(c, pl):
    return (pl["kernel"], pl["prod"], pl["form"])


@functools.lru_cache(maxsize=None)
def _worst_ratios():
    """{(wrong, class): (largest err / tol, case)} over the teeth cases."""
    out = {}
    for c in CASES:
        if c["name"] not in TEETH_CASES:
            continue
        for precision, y_f16 in c["variants"]:
            pl = plan_of(c, precision, y_f16)
            for cls in TEETH_CLASSES:
                if cls not in c["classes"]:
                    continue
                x, wgt, b, pre64, y64, tol, _, _ = expect(c["id"], cls, key(pl, y_f16))
                for wrong in WRONG:
                    if not applies(wrong, pl, c):
                        continue
                    bad = gelu(model_pre(pl, x, wgt, b, c["h"], c["w"], F64, wrong))
                    r = float(((bad - y64).abs().numpy() / tol).max())
                    k = (wrong, _klass(c, pl))
                    if r > out.get(k, (0.0, None))[0]:
                        out[k] = (r, f"{c['id']} {dc.PREC_NAME[precision]} y16={y_f16} {cls}")
    return out


@pytest.mark.parametrize("wrong", WRONG)
def test_wrong_kernel_is_ten_bounds_off(wrong):
    got = {k: v for k, v in _worst_ratios().items() if k[0] == wrong}
    klasses = {k[1] for k in _worst_ratios()}
    want = {kl for kl in klasses if any(applies(wrong, plan_of(c, p, y), c) and _klass(c, plan_of(c, p, y)) == kl
                                        for c in CASES if c["name"] in TEETH_CASES for p, y in c["variants"])}
    assert want and {k[1] for k in got} == want
    for k, (r, where) in got.items():
        print(f"TEETH {wrong} {k[1]}: {r:.1f} bounds at {where}")
        assert r >= 10.0, (wrong, k[1], r, where)


def test_teeth_cover_every_class():
    klasses = {k[1] for k in _worst_ratios()}
    assert klasses == {("stencil", 0, "f32"), ("mfma", 3, "f32"), ("mfma", 2, "f32"), ("mfma", 1, "f32"), ("mfma", 2, "f16reg"),
                       ("mfma", 1, "f16reg"), ("mfma", 2, "f16dma"), ("mfma", 1, "f16dma")}


# ---- 6. the plan and the case table -------------------------------------------------------------------------------------------------
def _pl(name, k, entry, precision=dc.F16X2, y_f16=1, **kw):
    (c,) = _named(name, k, entry)
    return plan_of(c, precision, y_f16, **kw), c


def test_case_table_facts():
    assert len(CASES) == len({c["id"] for c in CASES}) == len({c["seed"] for c in CASES}) == 54
    assert {c["name"] for c in CASES} == {s[0] for s in dc.MFMA_SHAPES} | {s[0] for s in dc.STENCIL_SHAPES}
    for c in CASES:                                          # every variant of every case takes the family's kernel
        assert c["classes"][0] == "std" and all(plan_of(c, p, y)["kernel"] == c["family"] for p, y in c["variants"]), c["id"]
    assert {cls for c in CASES for cls in c["classes"]} == set(dc.CLASSES)
    for k in dc.KSIZES:
        assert {(p, y) for c in CASES if c["family"] == "mfma" and c["k"] == k and c["entry"] == "f32" for p, y in c["variants"]} == \
            {(p, y) for p in ((dc.F16X3, dc.F16X2, dc.F16) if k == 15 else (dc.F16X2, dc.F16)) for y in (0, 1)}
        assert {(p, y) for c in CASES if c["family"] == "stencil" and c["k"] == k for p, y in c["variants"]} == \
            {(p, y) for p in ((dc.FP32,) if k == 15 else (dc.FP32, dc.F16X3)) for y in (0, 1)}
        # halo only, single row / column, exact and ragged tiles
        assert _pl("halo", k, "f32")[0]["ngroups"] == 1 and _pl("exact", k, "f32")[0]["ntx"] == 1
        p = _pl("ragged", k, "f32")[0]
        assert p["ntx"] == 3 and p["nty"] == 2 and p["groups_per_wave"] == (1, 1, 0, 0)       # 4 tiles a wave: one past the edge; idle waves
        # fp16 rows: width, base, stride decide the form
        assert _pl("odd_width", k, "f16in")[0]["form"] == "f16reg"
        p, c = _pl("exact", k, "f16in")
        span = c["C"] * c["h"] * c["w"]
        assert p["form"] == "f16dma" and p["fold"] and _pl("exact", k, "f16in", precision=dc.F16)[0]["fold"] is False
        assert plan_of(c, dc.F16X2, 1, x_base=2)["form"] == "f16reg" and plan_of(c, dc.F16X2, 1, x_stride=span + 3)["form"] == "f16reg"
        assert plan_of(c, dc.F16X2, 1, x_base=0, x_stride=span + 24)["form"] == "f16dma"
        for form in ("f16_dma", "f16_halfoff", "f16_oddstride"):
            off, stride = dc.place(form, span, True)
            assert plan_of(c, dc.F16X2, 1, x_base=2 * off % 16, x_stride=stride)["form"] == ("f16dma" if form == "f16_dma" else "f16reg"), form
        # images per workgroup, the ragged last workgroup, groups per wave
        p = _pl("ipw_dma", k, "f16in")[0]
        assert (p["form"], p["imgs_per_wg"], p["grid_z"], p["last_wg_imgs"], p["groups_per_wave"]) == ("f16dma", 4, 2, 3, (1, 0, 0, 0))
        p = _pl("gpw_dma", k, "f16in")[0]
        assert (p["form"], p["imgs_per_wg"], p["grid_z"], p["last_wg_imgs"], p["groups_per_wave"]) == ("f16dma", 3, 5, 1, (2, 1, 1, 1))
        p = _pl("ipw_reg", k, "f32", y_f16=0)[0]
        assert (p["form"], p["imgs_per_wg"], p["grid_z"]) == ("f32", 3, 5)
        # float4 against element staging
        p, c = _pl("exact", k, "f32", y_f16=0)
        assert p["vec_ok"] and not plan_of(c, dc.F16X2, 0, x_base=4)["vec_ok"] and not plan_of(c, dc.F16X2, 0, x_stride=c["C"] * 256 + 3)["vec_ok"]
        # the widest planes and one column more
        w = dc.MFMA_WIDEST[k]
        for entry in ("f32", "f16in"):
            assert dc.plan(entry, dc.F16X2, k, 1, 1, 1, 16, w)["refused"] is None and dc.plan(entry, dc.F16X2, k, 1, 1, 1, 16, w + 1)["refused"] == "width"
        ws = dc.STENCIL_WIDEST[k]
        for h in (1, 40, 1000):                              # one interval per K, for every h
            ok = [dc.plan("f32", dc.FP32, k, 0, 1, 1, h, w_)["refused"] is None for w_ in range(1, ws + 40)]
            assert all(ok[:ws]) and not any(ok[ws:]), (k, h)
        # the stencil: strips, vector stores
        p, c = _pl("s_strips", k, "f32", precision=dc.FP32, y_f16=0)
        assert (p["strips"], p["last_strip_rows"], p["vec_store"], p["parent_refused"]) == (2, 1, True, False)
        assert not plan_of(c, dc.FP32, 0, y_base=4)["vec_store"] and not plan_of(c, dc.FP32, 1, y_base=2)["vec_store"] and plan_of(c, dc.FP32, 1, y_base=8)["vec_store"]
        assert _pl("s_tall", k, "f32", precision=dc.FP32, y_f16=0)[0]["refused"] is None
    p = _pl("strip1row15", 15, "f16in")[0]
    assert (p["form"], p["pieces"], p["strips"], p["last_strip_rows"]) == ("f16dma", 7, 2, 1)
    p = _pl("strip1row15", 15, "f32", y_f16=0)[0]
    assert (p["strips"], p["last_strip_rows"]) == (2, 1)
    for entry in ("f32", "f16in"):
        p = _pl("strip1row7", 7, entry)[0]
        assert (p["strips"], p["last_strip_rows"]) == (2, 1)
    p15, p7 = _pl("cliff", 15, "f16in")[0], _pl("cliff", 7, "f16in")[0]                     # two rounded planes no longer fit LDS
    assert (p15["form"], p15["strips"]) == ("f16dma", 2) and (p7["form"], p7["strips"]) == ("f16reg", 1)
    p = _pl("ipw_reg7", 7, "f32", y_f16=0)[0]
    assert (p["imgs_per_wg"], p["grid_z"]) == (3, 3)
    p = _pl("s_ldslimit", 15, "f32", precision=dc.FP32, y_f16=0)[0]
    assert 65000 < p["lds"] <= 65536 and not p["parent_refused"]
    # what the dispatch refused before its strip was shortened: K = 15 and h = 40 took w = 1..604 and 681..716
    was = [not dc.plan("f32", dc.FP32, 15, 0, 1, 1, 40, w)["parent_refused"] for w in range(1, 720)]
    assert [w for w in range(1, 720) if was[w - 1]] == list(range(1, 605)) + list(range(681, 717))
    assert _pl("s_wide", 15, "f32", precision=dc.FP32, y_f16=0)[0]["parent_refused"] and _pl("s_tall", 15, "f32", precision=dc.FP32, y_f16=0)[0]["parent_refused"]


def test_placements():
    for form, (off, mult) in dc.FORMS.items():
        assert dc.place(form, 1000, False) == (0, 1000)
        (o0, s0), (o1, s1) = dc.place(form, 1000, True, 0), dc.place(form, 1000, True, 1)
        assert o0 == o1 == off and s0 > 1000 and s1 > 1000 and s0 != s1 and s0 % mult == 0 and s1 % mult == 0
        if mult == 1:
            assert s0 % 2 == 1 and s1 % 2 == 1                                    # odd where allowed (the span is even here)


def test_poison_sets():
    may, foot = dc.poison_sets(33, 40, 15, 20, 17, "mfma")
    assert foot.sum() == 15 * 15 and bool((foot <= may).all())
    assert sorted(set(np.argwhere(may)[:, 1] // 16)) == [0, 1] and may[:, 32:].sum() == 0      # windows -8..23 and 8..39 hold column 17
    assert np.array_equal(*dc.poison_sets(33, 40, 7, 20, 17, "stencil"))


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from streamflow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


DUMMY = 0x10000                                              # never dereferenced: every call below ends before a launch


def call_refused(lib, r, ptrs=None):
    """ptrs: {name: (address, stride)} of real buffers, or None for dummy pointers."""
    assert plan_refuses(r), r                                # no argument set that the library accepts is called with dummy pointers
    span = max(r["C"], 1) * max(r["h"], 1) * max(r["w"], 1)
    p = {f: ((DUMMY * (i + 1), span) if ptrs is None else ptrs[f]) for i, f in enumerate(("x", "wgt", "bias", "y"))}
    a = {f: (None if r["null"] == f else p[f][0]) for f in p}
    if r["entry"] == "f16in":
        st = lib.sf_dwconv_res_gelu_f16in(a["x"], p["x"][1], a["wgt"], a["bias"], a["y"], p["y"][1], r["n"], r["C"], r["h"], r["w"], r["k"], r["precision"], None)
    else:
        st = lib.sf_dwconv_res_gelu(a["x"], p["x"][1], a["wgt"], a["bias"], a["y"], p["y"][1], r["y_f16"], r["n"], r["C"], r["h"], r["w"], r["k"],
                                    r["precision"], None)
    return st, lib.sf_last_error().decode(errors="replace")


def plan_refuses(r):
    return r["null"] is not None or dc.plan(r["entry"], r["precision"], r["k"], r["y_f16"], r["n"], r["C"], r["h"], r["w"])["refused"] is not None


def test_refusals_list():
    rs = dc.refusals()
    assert {r["why"] for r in rs} == {"ksize", "precision", "y_f16", "null", "dims", "fp16 input", "width", "lds", "plane", "span", "grid"}
    for r in rs:
        if r["null"] is None:
            assert dc.plan(r["entry"], r["precision"], r["k"], r["y_f16"], r["n"], r["C"], r["h"], r["w"])["refused"] == r["why"], r
    # the span rule is its own: the same plane with fp16 output (half the bytes) is accepted
    assert dc.plan("f32", dc.F16X2, 7, 1, 1, 1, 800000, 704)["refused"] is None


def test_library_refuses_what_the_plan_refuses(lib):
    words = {"ksize": "kernel size", "precision": "precision", "y_f16": "y_f16", "null": "null", "dims": "dims", "fp16 input": "fp16 input",
             "width": "too large", "lds": "LDS", "plane": "plane too large", "span": "32-bit", "grid": "grid too large"}
    for r in dc.refusals():
        st, msg = call_refused(lib, r)
        assert st == dc.SF_ERR_BAD_ARG and words[r["why"]] in msg, (r, st, msg)
