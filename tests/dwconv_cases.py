"""Case lists, launch plan, placements, operand models and the per-element bound of tests/test_gpu_dwconv_kernels.py: the depthwise
15 x 15 / 7 x 7 layer of the SK blocks, y = gelu(x + dwconv(x) + b), through the C ABI -- sf_dwconv_res_gelu and
sf_dwconv_res_gelu_f16in (csrc/conv.hip: an fp32 stencil and a banded-Toeplitz kernel on the matrix cores).  Pure numpy: no torch,
no device.  tests/test_dwconv_cases_cpu.py pins what is here (the float64 restatement, the models inside half the bound, the bounds
under the caps, wrong kernels outside ten bounds, plan() against the library's refusals, the facts of the case table).

PLAN.  plan() restates dwconv_dispatch: which kernel, how many products, the input form (fp32 planes split while staged / fp16 rows
through registers / fp16 rows by DMA, double-buffered, the residual folded into the centre tap at two products), strips, images per
workgroup, tile groups per wave, LDS bytes, vector staging and stores, refused or not.

OPERAND MODEL, per class (split8 / split8_rn of csrc/split_operand.h emulated bit by bit; the products are the ones the kernel
issues, exact in float64):

    stencil (FP32; F16X3 at K = 7)   x and w as they are, the residual x itself
    F16X3 (K = 15)                   x = hi + lo by split8, w = hi + lo by split8: al bh + ah bl + ah bh; residual hi + lo of x
    F16X2                            x = hi of split8_rn alone, w = hi + lo by split8: ah bl + ah bh
    F16                              x = fp16_rn(x), w = fp16_rn(w): one product
        residual of F16X2 / F16:     fp32 input: hi + lo of split8_rn(x); fp16 input through registers, and the one-product DMA
                                     form: the fp16 value itself; DMA form at two products: none, the centre tap is
                                     split8(fp32(w_c + 1))

BOUND, per element, against the model evaluated in float64 (model64):

    pre-activation   P = 4 max|model32 - model64| + 4 * 2^-24 max|model64|      (the project's rule; model32 = the same model in
                                                                                 torch float32: two fp32 summation orders)
    through GELU     1.13 P                                                     (|gelu'| <= 1.13)
    GELU itself      erf form:        max(1.3e-6, 3.0e-7 |pre|)
                     polynomial form: max(5.2e-5, 6.6e-6 |pre|), for pre > 0 at most 1.35e-5 gelu(pre): the form of a two- or
                                      one-product matrix-core result that leaves as fp16.  (Both as measured on the restated
                                      polynomials, see gelu_term(): two of the figures csrc/sf_common.h stated did not hold.)
    output rounding  fp32: 2^-24 |y|;  fp16: 2^-11 |y| + 2^-25

CAPS on the class of the existing tests (tests/test_gpu_parity.py): 2e-5 for fp32 output, 2^-11 * 1.03 |ref| + 8e-5 for fp16 output.
"""
import numpy as np

from tests.attn_cases import f16, f32
from tests.corr_cases import f16z

FP32, F16X3, F16X2, F16 = 0, 1, 2, 3                        # SF_PRECISION_*
PREC_NAME = {FP32: "fp32", F16X3: "f16x3", F16X2: "f16x2", F16: "f16"}
SF_OK, SF_ERR_BAD_ARG, SF_ERR_HIP = 0, -1, -3
KSIZES = (15, 7)
CLASSES = ("std", "mean100", "gain", "tiny")
ALL_CLASSES_BELOW = 40000                                   # cells of a case (n C h w) up to which it runs every class
CAP_F32 = 2e-5
PAIR_F16_Y_REL, PAIR_F16_Y_ABS = 2.0 ** -11 * (1 + 1e-3), 3e-7     # fp16 y against fp32 y of the same call, erf forms
PAIR_IN_REL, PAIR_IN_ABS = 2.0 ** -9, 2.5e-5                # fp16 input against fp32 input of the same values; DMA against registers


def cap_f16(ref):
    return 2.0 ** -11 * 1.03 * np.abs(ref) + 8e-5


def _cdiv(a, b):
    return -(-a // b)


# ---- the launch plan ---------------------------------------------------------------------------------------------------------------
def plan(entry, precision, ksize, y_f16, n_img, C, h, w, x_base=0, y_base=0, x_stride=None, y_stride=None):
    """dwconv_dispatch restated.  entry 'f32' / 'f16in'; x_base, y_base: the base addresses modulo 16 (bytes); strides in elements
    (None: dense).  Returns a dict; d['refused'] is None or the reason."""
    x_f16 = entry == "f16in"
    if x_f16:
        y_f16 = 1
    x_stride = C * h * w if x_stride is None else x_stride
    y_stride = C * h * w if y_stride is None else y_stride

    def no(why):
        return dict(refused=why)

    if y_f16 not in (0, 1):
        return no("y_f16")
    if min(n_img, C, h, w) <= 0:
        return no("dims")
    if ksize not in (7, 15):
        return no("ksize")
    if not FP32 <= precision <= F16:
        return no("precision")
    if h * w >= 1 << 30:
        return no("plane")
    two = precision in (F16X2, F16)
    one = precision == F16
    if x_f16 and not two:
        return no("fp16 input")
    if precision != FP32 and (ksize == 15 or two):
        if h * w * (2 if y_f16 else 4) > 2 ** 31 - 1 or (x_f16 and h * w * 2 > 1 << 30):
            return no("span")
        w16 = _cdiv(w, 16) * 16
        base16 = (w16 + 16) // 8
        stride16 = base16 if base16 % 4 == 2 else base16 + (2 - base16 % 4 + 4) % 4
        strip = _cdiv(h, 16) * 16
        while strip > 16 and 2 * (strip + ksize - 1) * stride16 * 16 > 60 * 1024:
            strip -= 16
        plane = (strip + ksize - 1) * stride16 * 16
        pieces = _cdiv(plane, 4096)
        use_dma = (x_f16 and w % 8 == 0 and x_stride % 8 == 0 and x_base % 16 == 0 and pieces <= 8
                   and 2 * pieces * 4096 + ksize * 256 <= 64 * 1024)
        if use_dma:
            plane = pieces * 4096
        lds = 2 * plane + ksize * 256
        if lds > 64 * 1024:
            return no("width")
        strips = _cdiv(h, strip)
        groups = max(1, min(n_img, _cdiv(768 if use_dma else 2048, C * strips)))
        ipw = _cdiv(n_img, groups)
        gz = _cdiv(n_img, ipw)
        if strips > 65535 or gz > 65535:
            return no("grid")
        ntx, nty = w16 // 16, strip // 16
        ngroups = nty * _cdiv(ntx, 4)
        prod = 1 if one else 2 if two else 3
        return dict(refused=None, kernel="mfma", prod=prod, form="f16dma" if use_dma else "f16reg" if x_f16 else "f32",
                    fold=use_dma and prod == 2, gelu="poly" if prod <= 2 and y_f16 else "erf", strip_h=strip, strips=strips,
                    last_strip_rows=h - (strips - 1) * strip, imgs_per_wg=ipw, grid_z=gz, last_wg_imgs=n_img - (gz - 1) * ipw,
                    ntx=ntx, nty=nty, ngroups=ngroups, groups_per_wave=tuple((ngroups - wv + 3) // 4 for wv in range(4)),
                    vec_ok=w % 4 == 0 and x_stride % 4 == 0 and x_base % 16 == 0, vec_store=None, lds=lds,
                    pieces=pieces if use_dma else 0, parent_refused=False)
    tiles_x = _cdiv(w, 4)
    if tiles_x > 512:
        return no("width")
    tiles_y = _cdiv(h, 4)
    if tiles_y * tiles_x > 512:
        tiles_y = 512 // tiles_x
    wp4 = (tiles_x * 4 + ksize - 1 + 3) // 4

    def lds_of(ty):
        return ((ty * 4 + ksize - 1) * wp4 * 4 + 8 + ksize * ksize + 8) * 4

    parent_refused = lds_of(tiles_y) > 64 * 1024             # the dispatch before the strip was shortened to fit
    while tiles_y > 1 and lds_of(tiles_y) > 64 * 1024:
        tiles_y -= 1
    if lds_of(tiles_y) > 64 * 1024:
        return no("lds")
    strip = tiles_y * 4
    strips = _cdiv(h, strip)
    if strips > 65535:
        return no("grid")
    return dict(refused=None, kernel="stencil", prod=0, form="f32", fold=False, gelu="erf", strip_h=strip, strips=strips,
                last_strip_rows=h - (strips - 1) * strip, imgs_per_wg=1, grid_z=1, last_wg_imgs=1, ntx=tiles_x, nty=tiles_y, ngroups=0,
                groups_per_wave=(), vec_ok=None, vec_store=w % 4 == 0 and y_stride % 4 == 0 and y_base % (8 if y_f16 else 16) == 0,
                lds=lds_of(tiles_y), pieces=0, threads=_cdiv(tiles_y * tiles_x, 64) * 64, parent_refused=parent_refused)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# (name, n, C, h, w, ksizes, entries)
MFMA_SHAPES = (
    ("halo", 2, 3, 1, 1, KSIZES, ("f32", "f16in")),
    ("row", 2, 2, 1, 17, KSIZES, ("f32", "f16in")),
    ("col", 2, 2, 17, 1, KSIZES, ("f32", "f16in")),
    ("exact", 2, 2, 16, 16, KSIZES, ("f32", "f16in")),
    ("ragged", 2, 2, 17, 33, KSIZES, ("f32", "f16in")),
    ("strip1row15", 2, 1, 33, 248, (15,), ("f32", "f16in")),
    ("strip1row7", 2, 1, 49, 248, (7,), ("f32", "f16in")),
    ("cliff", 2, 1, 40, 240, KSIZES, ("f16in",)),
    ("ipw_dma", 7, 384, 8, 8, KSIZES, ("f16in",)),
    ("gpw_dma", 13, 128, 80, 8, KSIZES, ("f16in",)),
    ("ipw_reg", 15, 324, 8, 8, KSIZES, ("f32",)),
    ("ipw_reg7", 9, 640, 8, 8, (7,), ("f32",)),
    ("odd_width", 2, 2, 9, 12, KSIZES, ("f16in",)),
    ("wide15", 1, 1, 16, 480, (15,), ("f32", "f16in")),
    ("wide7", 1, 1, 16, 704, (7,), ("f32", "f16in")),
)
STENCIL_SHAPES = (
    ("s_one", 2, 3, 1, 1, KSIZES),
    ("s_small", 2, 2, 3, 5, KSIZES),
    ("s_vec", 2, 2, 6, 8, KSIZES),
    ("s_ragged", 2, 2, 17, 33, KSIZES),
    ("s_strips", 2, 2, 33, 256, KSIZES),
    ("s_ldslimit", 1, 2, 40, 604, (15,)),
    ("s_wide", 1, 1, 40, 640, KSIZES),
    ("s_tall", 1, 2, 1000, 4, KSIZES),
)
RECORDED = ("s_strips", "s_ldslimit")                       # results recorded from the library before the stencil strip fix
WAS_REFUSED = ("s_wide", "s_tall")
MFMA_WIDEST = {15: 480, 7: 704}                             # at h = 16; one more column is refused
STENCIL_WIDEST = {15: 880, 7: 1620}                         # any h


def mfma_variants(entry, ksize):
    """(precision, y_f16) that take the matrix-core kernel."""
    if entry == "f16in":
        return ((F16X2, 1), (F16, 1))
    v = [(F16X2, 0), (F16X2, 1), (F16, 0), (F16, 1)]
    return ([(F16X3, 0), (F16X3, 1)] if ksize == 15 else []) + v


def stencil_variants(ksize):
    v = [(FP32, 0), (FP32, 1)]
    return v + ([(F16X3, 0), (F16X3, 1)] if ksize == 7 else [])


def cases():
    out = []
    for i, (name, n, C, h, w, ks, entries) in enumerate(MFMA_SHAPES):
        for k in ks:
            for e in entries:
                out.append(dict(id=f"{name}-{h}x{w}-n{n}C{C}-K{k}-{e}", name=name, family="mfma", entry=e, n=n, C=C, h=h, w=w, k=k,
                                seed=7000 + 10 * i + (k == 7) + 2 * (e == "f16in"), variants=mfma_variants(e, k)))
    for i, (name, n, C, h, w, ks) in enumerate(STENCIL_SHAPES):
        for k in ks:
            out.append(dict(id=f"{name}-{h}x{w}-n{n}C{C}-K{k}", name=name, family="stencil", entry="f32", n=n, C=C, h=h, w=w, k=k,
                            seed=7500 + 10 * i + (k == 7), variants=stencil_variants(k)))
    for j, c in enumerate(out):
        small = c["n"] * c["C"] * c["h"] * c["w"] <= ALL_CLASSES_BELOW
        c["classes"] = CLASSES if small else ("std", CLASSES[1 + j % 3])
    return out


def draw(case, cls):
    """(x [n][C][h w], wgt [C][K][K], bias [C]) float32; for the fp16 entry point x holds fp16 values."""
    rng = np.random.default_rng(case["seed"] * 8 + CLASSES.index(cls))
    n, C, h, w, k = case["n"], case["C"], case["h"], case["w"], case["k"]
    x = rng.standard_normal((n, C, h * w))
    wgt = rng.standard_normal((C, k, k)) / k
    b = 0.1 * rng.standard_normal(C)
    if cls == "mean100":
        x, wgt = x + 100.0, wgt * 1e-3
    elif cls == "gain":
        x = x * 8.0
    elif cls == "tiny":
        x = x * 1e-4
    x = x.astype(np.float32)
    if case["entry"] == "f16in":
        x = x.astype(np.float16).astype(np.float32)
    return x, wgt.astype(np.float32), b.astype(np.float32)


# ---- placements --------------------------------------------------------------------------------------------------------------------
# form -> (elements per 16 bytes' smallest allowed step off the allocation, multiple the image stride must keep).  "any": nothing
# demanded -- one element off, odd gaps.
FORMS = {
    "f32_vec": (4, 4),        # fp32 rows 16-byte aligned: float4 staging (matrix cores) / float4 stores (stencil)
    "f32_any": (1, 1),
    "f16_dma": (8, 8),        # fp16 rows of whole 16-byte aligned octets: the DMA form
    "f16_vec": (4, 4),        # fp16 y of the stencil: 8-byte stores
    "f16_any": (1, 1),
    "f16_oddstride": (0, 1),  # base aligned, odd image stride: leaves the DMA form by the stride alone
    "f16_halfoff": (1, 8),    # base one half off, stride a multiple of 8: leaves the DMA form by the base alone
}


def place(form, span, placed, k=0):
    """(off, stride) in elements for an image of `span` elements.  placed = False: (0, span)."""
    if not placed:
        return 0, span
    off, mult = FORMS[form]
    gap = mult * (3 + 2 * k)                                  # odd where the form allows, different for x (k = 0) and y (k = 1)
    return off, span + gap


# ---- split8 / split8_rn, bit by bit ------------------------------------------------------------------------------------------------
def split8(x):
    """hi = the fp32 bits & 0xFFFFE000 cut to fp16, lo = x - hi (exact in fp32) cut to fp16, both towards zero (v_cvt_pkrtz)."""
    x32 = np.asarray(x, np.float64).astype(np.float32)
    ah = (x32.view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32).astype(np.float64)
    return f16z(ah), f16z(x32.astype(np.float64) - ah)


def split8_rn(x):
    """hi = x rounded to nearest fp16, lo = the fp32 difference rounded to nearest fp16."""
    x32 = np.asarray(x, np.float64).astype(np.float32).astype(np.float64)
    hi = f16(x32)
    return hi, f16(f32(x32 - hi))


def operands(pl, x, wgt, wrong=None):
    """What the kernel of plan `pl` multiplies and adds, as float64 arrays (every value exact in fp32):
    (products [(x part, w part), ...] in issue order, residual parts (a, b) with residual = fp32(a + b) or None).
    wrong: 'w_f16' (weights rounded once where the class splits them), 'x_f16' (x rounded once where the class says F16X3),
    'res_hi' (the residual as hi alone), 'no_res' (the folded form without its + 1)."""
    x, wgt = np.asarray(x, np.float64), np.asarray(wgt, np.float64)
    k = wgt.shape[-1]
    if pl["kernel"] == "stencil":
        return [(x, wgt)], (x, np.zeros_like(x))
    if pl["fold"] and wrong != "no_res":
        wgt = wgt.copy()
        wgt[:, k // 2, k // 2] = f32(wgt[:, k // 2, k // 2] + 1.0)
    if pl["prod"] == 3:
        xh, xl = split8(x)
        wh, wl = split8(wgt)
        if wrong == "x_f16":
            xh, xl = f16(x), np.zeros_like(x)
        prods = [(xl, wh), (xh, wl), (xh, wh)]
    else:
        xh, xl = split8_rn(x)
        if pl["prod"] == 2 and wrong != "w_f16":
            wh, wl = split8(wgt)
            prods = [(xh, wl), (xh, wh)]
        else:
            prods = [(xh, f16(wgt))]
    if pl["form"] != "f32":
        xl = np.zeros_like(x)                               # fp16 rows: the value is its own hi half
    if wrong == "res_hi":
        xl = np.zeros_like(x)
    return prods, (None if pl["fold"] else (xh, xl))


# ---- the two GELUs of csrc/sf_common.h, restated ------------------------------------------------------------------------------------
ERF_P = (-2.72614225801306e-10, 2.77068142495902e-08, -2.10102402082508e-06, -5.69250639462346e-05, -7.34990630326855e-04,
         -2.95459980854025e-03, -1.60960333262415e-02)
ERF_Q = (-1.45660718464996e-05, -2.13374055278905e-04, -1.68282697438203e-03, -7.37332916720468e-03, -1.42647390514189e-02)
POLY = (1.12535e-10, -1.074371e-08, 4.5365834e-07, -1.12924145e-05, 0.0001871811, -0.0022188, 0.019636236, -0.13269384, 0.79780626)
POLY_CLAMP = 4.2426405
ERF_HALF_CLAMP = -5.6568542


def _r(v, single):
    return f32(v) if single else v


def gelu_erf_form(x, single=False):
    """gelu_erf2: 0.5 max(x, -5.657) (1 + erf_fast(x / sqrt 2)); single: every operation rounded to fp32 (an fma rounds once)."""
    x = _r(np.asarray(x, np.float64), single)
    z = np.clip(_r(x * _r(0.70710678118654752440, single), single), -4.0, 4.0)
    z2 = _r(z * z, single)
    p = _r(ERF_P[0], single)
    for c in ERF_P[1:]:
        p = _r(p * z2 + _r(c, single), single)
    q = _r(ERF_Q[0], single)
    for c in ERF_Q[1:]:
        q = _r(q * z2 + _r(c, single), single)
    e = _r(_r(z * p, single) * _r(1.0 / q, single), single)
    return _r(_r(0.5 * np.maximum(x, _r(ERF_HALF_CLAMP, single)), single) * _r(1.0 + e, single), single)


def gelu_poly_form(x, single=False):
    """gelu_poly2: h + h (xc D(xc^2)), h = max(x, -4.243) / 2, xc = x clamped to +-4.243."""
    x = _r(np.asarray(x, np.float64), single)
    cl = _r(POLY_CLAMP, single)
    xc = np.clip(x, -cl, cl)
    t = _r(xc * xc, single)
    p = _r(POLY[0], single)
    for c in POLY[1:]:
        p = _r(p * t + _r(c, single), single)
    hh = _r(0.5 * np.maximum(x, -cl), single)
    return _r(hh * _r(xc * p, single) + hh, single)


# csrc/sf_common.h stated 1.3e-6 for the erf form "for every x" and, from the fit's 4.5e-7, 2.25e-7 |x|; 5.2e-5 "for EVERY x" and
# 1.1e-5 relative for x > 0 for the polynomial.  Restated and measured on a grid over [-12, 12] (tests/test_dwconv_cases_cpu.py):
#   erf form    1.06e-6 for x <= 0; for x > 0 the error is relative, 2.6e-7 x evaluated in fp32 with an exact reciprocal (3.2e-8 x
#               in float64: the rest is the rounding of the fit's own operations), + 2^-25 x for v_rcp_f32's ulp: 3.0e-7 |x|
#   polynomial  5.0e-5 up to the clamp of xc (4.243); beyond it the residue of erf(3) != 1 times x / 2 = 6.5e-6 x, which passes
#               5.2e-5 at x = 8; relative to gelu(x), x > 0: 1.35e-5 (1.2e-5 of x)
# The comments there now say so, and the bound uses these.
ERF_ABS, ERF_REL = 1.3e-6, 3.0e-7
POLY_ABS, POLY_REL_FAR, POLY_REL_GELU = 5.2e-5, 6.6e-6, 1.35e-5


def gelu_term(pre, y, form):
    """|kernel's GELU - gelu| for the pre-activation `pre` (y = gelu(pre))."""
    pre, y = np.asarray(pre, np.float64), np.abs(np.asarray(y, np.float64))
    if form == "erf":
        return np.maximum(ERF_ABS, ERF_REL * np.abs(pre))
    t = np.maximum(POLY_ABS, POLY_REL_FAR * np.abs(pre))
    return np.where(pre > 0, np.minimum(t, POLY_REL_GELU * y + 2.0 ** -149), t)


def pre_tol(m32, m64):
    """The project's rule on the pre-activation: 4 x the error of the float32 evaluation + 4 fp32 ulps of the largest value."""
    m64 = np.asarray(m64, np.float64)
    return 4.0 * float(np.abs(np.asarray(m32, np.float64) - m64).max()) + 4.0 * 2.0 ** -24 * float(np.abs(m64).max())


def bound(pre64, y64, ptol, form, y_f16, cls):
    """Per element; capped on the existing tests' class by what they allow."""
    y = np.abs(np.asarray(y64, np.float64))
    t = 1.13 * ptol + gelu_term(pre64, y, form) + out_rounding(y, y_f16)
    if cls == "std":
        t = np.minimum(t, cap_f16(y) if y_f16 else CAP_F32)
    return t


def out_rounding(y, y_f16):
    y = np.abs(np.asarray(y, np.float64))
    return 2.0 ** -11 * y + 2.0 ** -25 if y_f16 else 2.0 ** -24 * y


def round_out(y, y_f16):
    return f16(y) if y_f16 else f32(y)


# ---- how far a non-finite input value may spread -----------------------------------------------------------------------------------
POISON_SHAPE = (3, 3, 33, 40)                               # n, C, h, w
POISON_AT = (1, 2, 20, 17)                                  # image, channel, y0, x0


def poison_sets(h, w, k, y0, x0, kernel):
    """(rows_cols mask [h][w] of outputs that MAY differ from the clean run, footprint mask [h][w]).  Stencil: the K x K footprint.
    Matrix cores: rows y0 - R .. y0 + R, and the columns of every 16-column tile whose 32-column window (columns 16 t - 8 .. 16 t + 23)
    holds x0: the band multiplies the whole window, 0 * NaN = NaN."""
    R = k // 2
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rows = np.abs(yy - y0) <= R
    foot = rows & (np.abs(xx - x0) <= R)
    if kernel == "stencil":
        return foot, foot
    t = xx // 16
    return rows & (16 * t - 8 <= x0) & (x0 <= 16 * t + 23), foot


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _rf(why, entry="f32", precision=F16X2, k=15, y_f16=0, n=1, C=1, h=16, w=16, null=None):
    return dict(why=why, entry=entry, precision=precision, k=k, y_f16=y_f16, n=n, C=C, h=h, w=w, null=null)


def refusals():
    """Argument sets the library refuses before any launch (SF_ERR_BAD_ARG with a message)."""
    r = [_rf("ksize", k=9), _rf("ksize", k=0), _rf("ksize", k=15 * 7, precision=FP32), _rf("ksize", k=3, entry="f16in", y_f16=1),
         _rf("precision", precision=-1), _rf("precision", precision=4), _rf("precision", precision=4, entry="f16in", y_f16=1),
         _rf("y_f16", y_f16=2), _rf("y_f16", y_f16=-1, precision=FP32)]
    r += [_rf("null", null=p) for p in ("x", "wgt", "bias", "y")] + [_rf("null", null="x", entry="f16in", y_f16=1)]
    for d in ("n", "C", "h", "w"):
        r += [_rf("dims", **{d: 0}), _rf("dims", **{d: -1}, precision=FP32)]
    r += [_rf("fp16 input", entry="f16in", precision=FP32, y_f16=1), _rf("fp16 input", entry="f16in", precision=F16X3, y_f16=1)]
    for k, wmax in MFMA_WIDEST.items():
        r += [_rf("width", k=k, w=wmax + 1), _rf("width", k=k, w=wmax + 1, precision=F16, y_f16=1),
              _rf("width", k=k, w=wmax + 1, entry="f16in", y_f16=1)]
    r += [_rf("width", k=15, w=481, precision=F16X3)]
    for k, wmax in STENCIL_WIDEST.items():
        r += [_rf("lds", k=k, w=wmax + 1, precision=FP32, h=40), _rf("lds", k=k, w=wmax + 1, precision=FP32, h=1, y_f16=1),
              _rf("width", k=k, w=2049, precision=FP32)]
    r += [_rf("lds", k=7, w=1621, precision=F16X3)]
    r += [_rf("plane", h=32768, w=32768), _rf("plane", h=32768, w=32768, precision=FP32)]
    # the matrix-core kernel's 32-bit byte offsets and `int` record counts: h w 4 bytes of fp32 output beyond 2^31 - 1, and for fp16
    # input h w 2 bytes beyond 2^30 (the offset its DMA uses for "outside the plane")
    r += [_rf("span", k=7, h=800000, w=704), _rf("span", k=7, h=800000, w=704, precision=F16),
          _rf("span", k=7, h=900000, w=608, entry="f16in", y_f16=1)]
    r += [_rf("grid", k=7, h=200000000, w=1, precision=FP32), _rf("grid", k=15, h=16 * 65536, w=480, y_f16=1)]      # more than 65535 strips
    return r
