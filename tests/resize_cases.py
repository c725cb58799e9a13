"""A numpy restatement of the resize kernels (csrc/resize.hip; include/streamflow_hip.h, "resize"), written independently of
streamflow_amd/resize.py, with the case lists and the error bound of the fp32 kernel.

Tables: Pillow's precompute_coeffs (Resample.c) as scalar Python loops over `math` functions.  resize_u8: Pillow's 8-bit resampler
in integers (bitwise PIL.Image.resize: tests/test_resize_cases_cpu.py).  resize_float: Pillow's mode-F resampler, float64 sums with
a float32 intermediate (bitwise PIL on mode F).  resize_f64 / resize_abs: the float64 result from fp32-rounded tables and its
magnitude companion for the bound of sf_resize_f32; emulate_f32: the kernel's stated fp32 arithmetic in numpy."""
import math

import numpy as np

PRECISION_BITS = 22
FILTER_NAMES = ("box", "bilinear", "bicubic", "lanczos")


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"box": (_box, 0.5), "bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}


def table(in_size, out_size, name):
    """(bounds int32 [out, 2], k float64 [out, ksize]): one axis, scalar loops."""
    f, fsupport = FILTERS[name]
    scale = float(in_size) / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.float64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        xmin = 0 if xmin < 0 else xmin
        xmax = int(center + support + 0.5)
        xmax = in_size if xmax > in_size else xmax
        xmax -= xmin
        ww = 0.0
        for x in range(xmax):
            w = f((x + xmin - center + 0.5) * ss)
            kk[xx, x] = w
            ww += w
        for x in range(xmax):
            if ww != 0.0:
                kk[xx, x] /= ww
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def fixed(kk):
    """The 8-bit resampler's coefficients: (int)(k * 2^22 +- 0.5), scalar."""
    out = np.zeros(kk.shape, np.int32)
    for idx in np.ndindex(*kk.shape):
        v = float(kk[idx])
        out[idx] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return out


def _pass_u8(img, bounds, k, axis):
    """One integer pass along `axis` of uint8 [..]: clip8(2^21 + sum pixel * k)."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.zeros((bounds.shape[0],) + src.shape[1:], np.uint8)
    for o in range(bounds.shape[0]):
        first, cnt = int(bounds[o, 0]), int(bounds[o, 1])
        ss = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for i in range(cnt):
            ss = ss + src[first + i] * int(k[o, i])
        assert ss.size == 0 or (np.abs(ss).max() < (1 << 31))             # the kernel's (and Pillow's) sums are 32-bit
        out[o] = np.clip(ss >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_u8(img, hw, name):
    """uint8 [n, H, W, 3] -> [n, h, w, 3]: horizontal pass if w != W, then vertical pass if h != H; a copy with neither."""
    h, w = hw
    out = img
    if w != img.shape[2]:
        b, k = table(img.shape[2], w, name)
        out = _pass_u8(out, b, fixed(k), 2)
    if h != img.shape[1]:
        b, k = table(img.shape[1], h, name)
        out = _pass_u8(out, b, fixed(k), 1)
    return np.ascontiguousarray(out).copy()


def _pass_f64(x, bounds, k, axis, inter=None):
    """One float64 pass along `axis`: every tap inside the bounds is multiplied (zeros included), summed in tap order."""
    src = np.moveaxis(x, axis, 0).astype(np.float64)
    out = np.zeros((bounds.shape[0],) + src.shape[1:], np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for o in range(bounds.shape[0]):
            first, cnt = int(bounds[o, 0]), int(bounds[o, 1])
            ss = np.zeros(src.shape[1:], np.float64)
            for i in range(cnt):
                ss = ss + src[first + i] * float(k[o, i])
            out[o] = ss
        if inter is not None:
            out = out.astype(inter).astype(np.float64)
    return np.moveaxis(out, 0, axis)


def resize_float(x, hw, name):
    """Pillow's mode-F resampler for float32 [.., H, W]: float64 tables and sums, float32 after each pass."""
    h, w = hw
    out = x
    if w != x.shape[-1]:
        b, k = table(x.shape[-1], w, name)
        out = _pass_f64(out, b, k, out.ndim - 1, np.float32)
    if h != x.shape[-2]:
        b, k = table(x.shape[-2], h, name)
        out = _pass_f64(out, b, k, out.ndim - 2, np.float32)
    return np.asarray(out, np.float32)


def tables_f32(H, W, h, w, name):
    """((bounds_x, kx fp32) or None, (bounds_y, ky fp32) or None): the float64 tables rounded once."""
    tx = ty = None
    if w != W:
        b, k = table(W, w, name)
        tx = (b, k.astype(np.float32))
    if h != H:
        b, k = table(H, h, name)
        ty = (b, k.astype(np.float32))
    return tx, ty


def resize_f64(flow, hw, name, sx=1.0, sy=1.0, absolute=False):
    """float64 result of the two passes on fp32 [n, 2, H, W] with the fp32-ROUNDED tables and an exact (float64) intermediate;
    channel 0 times fp32(sx), channel 1 times fp32(sy).  absolute=True: the same resample of |v| with |k| and |s| (the A |s| of
    the bound)."""
    H, W = flow.shape[2:]
    tx, ty = tables_f32(H, W, hw[0], hw[1], name)
    out = np.abs(flow.astype(np.float64)) if absolute else flow.astype(np.float64)
    for t, axis in ((tx, 3), (ty, 2)):
        if t is not None:
            k = t[1].astype(np.float64)
            out = _pass_f64(out, t[0], np.abs(k) if absolute else k, axis)
    s = np.array([float(np.float32(sx)), float(np.float32(sy))], np.float64)
    with np.errstate(invalid="ignore"):
        return out * (np.abs(s) if absolute else s)[None, :, None, None]


def bound_f32(flow, hw, name, sx=1.0, sy=1.0):
    """(T_h + T_v + 6) * 2^-24 * |s| * A per output element: first-order rounding of every product and sum of the two passes (a
    term of a pass with T taps goes through one product and at most T - 1 sums), of the intermediate and of the final multiply.
    T_h, T_v: the tap counts of the element's column and row (0 for an axis that has no pass)."""
    H, W = flow.shape[2:]
    h, w = hw
    tx, ty = tables_f32(H, W, h, w, name)
    th = tx[0][:, 1].astype(np.float64) if tx is not None else np.zeros(w)
    tv = ty[0][:, 1].astype(np.float64) if ty is not None else np.zeros(h)
    taps = th[None, None, None, :] + tv[None, None, :, None] + 6.0
    return taps * 2.0 ** -24 * resize_f64(flow, hw, name, sx, sy, absolute=True)


def emulate_f32(flow, hw, name, sx=1.0, sy=1.0):
    """The kernel's stated arithmetic in numpy float32: acc = acc + v * k with every product and sum rounded, fp32 intermediate, one
    multiply by fp32(sx) / fp32(sy) at the end."""
    H, W = flow.shape[2:]
    tx, ty = tables_f32(H, W, hw[0], hw[1], name)
    out = flow.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t, axis in ((tx, 3), (ty, 2)):
            if t is None:
                continue
            src = np.moveaxis(out, axis, 0)
            res = np.zeros((t[0].shape[0],) + src.shape[1:], np.float32)
            for o in range(t[0].shape[0]):
                first, cnt = int(t[0][o, 0]), int(t[0][o, 1])
                acc = np.zeros(src.shape[1:], np.float32)
                for i in range(cnt):
                    acc = (acc + (src[first + i] * np.float32(t[1][o, i])).astype(np.float32)).astype(np.float32)
                res[o] = acc
            out = np.moveaxis(res, 0, axis)
        s = np.array([np.float32(sx), np.float32(sy)], np.float32)
        return np.ascontiguousarray((out * s[None, :, None, None]).astype(np.float32))


# ---- cases ------------------------------------------------------------------------------------------------------------------------
# ((H, W), (h, w), n)
U8_SHAPES = [((1, 1), (5, 7), 1), ((7, 5), (1, 1), 1), ((37, 53), (16, 24), 1), ((37, 53), (80, 99), 1),
             ((64, 96), (9, 13), 1),                                     # 47 taps with the 3-lobe filter
             ((33, 70), (33, 31), 1),                                    # horizontal pass only
             ((70, 33), (20, 33), 1),                                    # vertical pass only
             ((50, 61), (50, 61), 1),                                    # copy
             ((20, 300), (17, 41), 1), ((3, 2), (64, 64), 1),
             ((150, 530), (75, 265), 3)]                                 # more than one block in both directions; 3 w % 4 != 0
U8_KINDS = ("noise", "extremes")

F32_SHAPES = [((37, 53), (16, 24)), ((16, 24), (37, 53)), ((55, 128), (109, 255)), ((1, 1), (4, 4)), ((9, 200), (9, 31))]
F32_SCALES = ((1.0, 1.0), (1.75, 0.4))
F32_N = 2


def shape_id(case):
    (H, W), (h, w) = case[0], case[1]
    return f"{H}x{W}-{h}x{w}"


def u8_input(case, kind):
    """Seeded uint8 [n, H, W, 3]: uniform noise, or only the values 0 and 255 (the largest over- and undershoots)."""
    (H, W), (h, w), n = case
    rng = np.random.default_rng([H, W, h, w, U8_KINDS.index(kind)])
    if kind == "noise":
        return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    return (rng.integers(0, 2, (n, H, W, 3)) * 255).astype(np.uint8)


def f32_input(case, n=F32_N):
    """Seeded flow-like fp32 [n, 2, H, W]: a smooth part of tens of pixels plus noise, both signs."""
    (H, W), (h, w) = case
    rng = np.random.default_rng([H, W, h, w, 7])
    y, x = np.mgrid[0:H, 0:W]
    smooth = 20.0 * np.sin(x / 9.0 + rng.uniform(0, 6, (n, 2, 1, 1))) * np.cos(y / 7.0)
    return (smooth + rng.normal(0, 3.0, (n, 2, H, W))).astype(np.float32)


def golden_name(case, kind):
    return f"u8_{shape_id(case)}_{kind}.npz"


def golden_name_f32(case):
    return f"f32_{shape_id(case)}.npz"
