"""Case lists, float64 references, layout decoders and per-element bounds of tests/test_gpu_corr_kernels.py: the correlation family
through the C ABI -- sf_corr_build_pyramid[_pitched] / sf_corr_lookup[_pitched] (csrc/corr.hip), sf_corr_build_blocked /
sf_corr_lookup_blocked (csrc/corr_blocked.hip), sf_corr_build_blocked32 / sf_corr_lookup_blocked32 (csrc/corr_blocked32.hip).  Pure
numpy on the CPU; tests/test_corr_cases_cpu.py pins what is here (oracle and golden equality, decoders against independent encoders,
rounding models inside half the bound, bounds under the caps, wrong kernels outside ten bounds, the case sets).

REFERENCE (include/streamflow_hip.h, in pixel space, float64).  C0[i][j] = <f1[:, i], f2[:, j]> / sqrt(D); level l + 1 = the 2 x 2 mean
of level l over the target dims with floor; lookup channel l * 81 + a * 9 + b' samples level l at (x / 2^l + a - 4, y / 2^l + b' - 4):
floor, fraction, four taps, zero outside; a scaled coordinate that is not strictly inside (-1e6, 1e6) samples zero.  No round trip
through grid_sample's normalised coordinates.

BUILD BOUND, per cell.  With S = sum_k |f1_k| |f2_k| / sqrt(D) (float64) and R = |reference cell|:

    level 0, before the cell is stored:   B0 = OPER + (STEPS + 4) 2^-24 S
        OPER   operand rounding, evaluated on the operands AS THE KERNEL HOLDS THEM (x' = pre * x, pre the folded power of two, 1 else):
                   sum_k (dx(a'_k) |b'_k| + |a'_k| dx(b'_k)) * post,   post = (1 / sqrt(D)) / (pre_a pre_b)
               dx(x) = 0                                for fp32 operands (FP32)
                     = max(2^-11 |x|, 2^-25)            one fp16 rounding; 2^-25 = half the spacing of fp16's subnormals (F16, blocked fp16)
                     = max(2^-20 |x|, 2^-24) [+ 2^-24]  the hi + lo split of the correlation builds (F16X3, blocked fp32).  It is NOT
                                                        the round-to-nearest split of the attention kernels (2^-21, tests/attn_cases.py)
                                                        but csrc/split_operand.h split8(): hi = x cut to 10 mantissa bits, lo = x - hi cut
                                                        to fp16, both towards zero -- |x - (hi + lo)| < 2^-10 |lo| <= 2^-20 |x| as that
                                                        file states, or < 2^-24 (the SPACING of fp16's subnormals, not half of it) where lo
                                                        is subnormal; for |x| < 2^-14 hi itself is cut to the subnormal grid and lo
                                                        (< 2^-24) is cut to zero: another 2^-24.  The dropped product lo * lo, |lo| <
                                                        2^-10 |x|, adds 2^-20 S to OPER
        STEPS  fp32 accumulation steps, 2^-24 of the running sum (<= S) each: D for one product per k (FP32, F16, blocked fp16), 3 D for
               the three products of the split classes (MFMA-internal partial sums count as steps: the worst case)
        4      the scale: sqrtf, the division and the float conversion of 1 / sqrt(D) (3) and the multiplication (1); an exact power
               of two folded into the operands costs nothing, the term is kept for every class
    level l > 0, pooled in fp32 from the UNROUNDED level-0 values, two additions per level (the factor 0.25 is exact):
                                          Bl = pool(B(l-1)) + 2 * 2^-24 pool(S(l-1) + B(l-1)),   S(l) = pool(S(l-1))
    stored cell:                          fp32 cells: 2 Bl;   fp16 cells: 2 (Bl + max(2^-11 (R + Bl), 2^-25))   (rounded ONCE)

    The factor 2, as in tests/attn_cases.py: every term above is first order and ATTAINED (D = 1 with fp16 operands: the error is the two
    operand roundings and the cell's, nothing averages out), so the sum is what a right kernel may reach; the factor covers second
    order and is the margin tests/test_corr_cases_cpu.py demands of the rounding models (inside HALF the bound).

    pool() is the same floor 2 x 2 mean: the error of a mean is at most the mean of the errors.  Nothing here comes from a kernel.

LOOKUP BOUND, per output channel, on the STORED cells c_1..c_4 of the four taps (float64 lookup of the decoded volume):

    L = 9 * 2^-24 * sum_i |c_i| + 2^-126
        3   a weight: the roundings of 1 - fx, 1 - fy and of their product (two-step kernels round the same three)
        1   the cell-weight product
        3   the three additions (partial sums <= sum |c_i| w_i <= sum |c_i|)
        1   the fraction c - floor(c): exact for c >= 0 and c <= -1, but for -1 < c < 0 the fp32 sum c + 1 rounds (half an ulp of a
            number below 1: 2^-25 in fx and in fy, 2^-24 in a weight)
        1   second order of the seven relative terms and fused multiply-adds contracting differently from this count
    A fp16 cell converts to fp32 exactly.

CAPS (what the suite already allows; a derived bound above its cap would hide nothing but is refused: tests/test_corr_cases_cpu.py):
1e-5 for cells of the split classes, 2^-11 R + 3e-5 for fp16 cells, 5e-5 for the lookup.  The worst-case bounds above are linear in D
where the existing tolerances count on sqrt(D): features are unit normal times AMP = 2^-6, at which every case is under its cap (the
fp16 terms 2 (2^-10 S + 2^-11 R) - 2^-11 R <= 3e-5 need S <= 0.012).  At that scale the caps are a formality (the GPU assertions use
the derived bounds alone), and every lo half of the split is an fp16 subnormal: the 2^-24 branch of dx is what the 13 cases measure.
The normal-lo branch (2^-20 |x|) is run by the cross-layout tests, which build the same cases from unit-normal features (amp = 1, the
scale the existing 2e-6 / 2e-5 / one-fp16-ulp tolerances were written for; no cap applies there) and hold them to the same bounds.

CROSS-LAYOUT limits (CROSS_CELLS, CROSS_LOOKUP, cross_f16_ulp), at unit-normal features only: blocked fp32 cells against pitched F16X3 cells
2e-6, their looked-up features 2e-5 (tests/test_gpu_corr_blocked32.py), blocked fp16 cells against dense fp16 cells 2^-10 |x| + 1e-6
(tests/test_gpu_corr_blocked.py).  A build with ONE fp16 product per k in place of the split is beyond them
(tests/test_corr_cases_cpu.py).

FOLD (csrc/corr_blocked.hip, host side, restated in blocked_fold): sf_corr_build_blocked packs every FRAME once (shared) iff pairs > 1,
f2 == f1 + f_pair_stride and (sqrt(scale) is a power of two or scale is not); the factor folded into the packed features is sqrt(scale)
on both sides (shared, D = 16, 256), scale on the f1 side (not shared, D = 1, 4, 16, 64, 256), else 1 and the epilogue multiplies.
"""
import math

import numpy as np

from tests.attn_cases import ACC, EPS, SUB, f16, f32, koct_alone_bound  # noqa: F401  (the same quantities: 2^-24, 2^-11 / 2^-21, 2^-25)

AMP = 2.0 ** -6
CAP_SPLIT, CAP_F16_ABS, CAP_LOOKUP = 1e-5, 3e-5, 5e-5
CROSS_AMP, CROSS_CELLS, CROSS_LOOKUP = 1.0, 2e-6, 2e-5


def cross_f16_ulp(x):
    """The one-fp16-ulp rule of test_blocked_matches_row_major_fp16_path, for cells x of unit-normal features."""
    return 2.0 ** -10 * np.abs(x) + 1e-6
LOOKUP_MULT = 9
FP32, F16X3, F16 = 0, 1, 3                                   # SF_PRECISION_*

# ---- case sets (asserted in tests/test_corr_cases_cpu.py) ------------------------------------------------------------------------
GRIDS = ((8, 8), (8, 9), (9, 8), (8, 16), (8, 17), (15, 17), (16, 24), (11, 36), (17, 33), (24, 40))
DEPTHS = (1, 8, 24, 40, 64, 256)
DEPTH_256_GRIDS = ((8, 8), (8, 9))                           # the two smallest grids (both N % 4 == 0: D = 256 is exempt from that rule)
IMAGES = ((1, 1), (2, 1), (1, 3), (2, 2))
FAMILIES = ("pyramid", "blocked16", "blocked32")
# (h, w, D, B, pairs): every grid once, then the two grids with N % 4 != 0 again until every D and every (B, pairs) has one
SHAPES = ((8, 8, 256, 1, 3), (8, 9, 256, 2, 1), (9, 8, 1, 1, 1), (8, 16, 64, 2, 2), (8, 17, 8, 1, 1), (15, 17, 1, 2, 2),
          (16, 24, 24, 2, 1), (11, 36, 40, 1, 3), (17, 33, 8, 1, 3), (24, 40, 64, 1, 1),
          (15, 17, 24, 1, 1), (15, 17, 64, 1, 3), (17, 33, 40, 2, 1))
COORD_NAMES = ("partly_outside", "fully_outside", "integer", "last_cell", "nan_x", "last_block_row", "ys_mod4_3",
               "minus_one", "w_minus_1_plus_eps", "level3_outside", "pos_inf_x", "neg_inf_x", "pos_inf_y", "nan_y", "1e6", "-1e6", "9.9e5",
               "minus_zero", "large_negative", "neg_inf_y")


def cases():
    """The same shapes for every family (FAMILIES): the GPU test runs each of them through each family's entry points."""
    return [dict(id=f"{h}x{w}-D{D}-B{B}p{pairs}", h=h, w=w, D=D, B=B, pairs=pairs, seed=4000 + i)
            for i, (h, w, D, B, pairs) in enumerate(SHAPES)]


def features(case):
    """Frames [B][pairs + 1][D][N] fp32, unit normal times AMP (times case["amp"] where a case names one: the cross-layout runs use 1,
    the scale of the existing tolerances): pair t of clip b correlates frame t (f1) with frame t + 1 (f2)."""
    rng = np.random.default_rng(case["seed"])
    return (case.get("amp", AMP) * rng.standard_normal((case["B"], case["pairs"] + 1, case["D"], case["h"] * case["w"]))).astype(np.float32)


def fixed_coords(h, w):
    """{name: ((y, x) pixel, (cx, cy))}: the six fixed pixels of the existing _coords helpers and the ys % 4 == 3 one on the diagonal,
    the rest in row 7 and row 0 -- every grid has those pixels (h, w >= 8)."""
    inf, nan = float("inf"), float("nan")
    far = 8.0 * ((w >> 3) + 5) + 0.5                         # level 3: x / 8 - 4 >= w >> 3, every tap of every window outside
    vals = [(-6.0, 2.0), (w + 9.0, h + 9.0), (3.0, 4.0), (w - 1.0, h - 1.0), (nan, 1.0), (3.0, h - 0.5), (5.25, 11.75),
            (-1.0, 3.0), (w - 1.0 + 2.0 ** -10, 2.5), (far, 1.0), (inf, 2.0), (-inf, 2.0), (2.0, inf), (2.0, nan), (1.0e6, 1.0),
            (1.0, -1.0e6), (9.9e5, 9.9e5), (-0.0, -0.0), (-12345.678, 3.25), (2.0, -inf)]
    pix = [(i, i) for i in range(7)] + [(7, j) for j in range(8)] + [(0, j) for j in range(1, 6)]
    assert len(vals) == len(pix) == len(COORD_NAMES)
    return {n: (p, v) for n, p, v in zip(COORD_NAMES, pix, vals)}


def coords(case):
    """[B * pairs][2][N] fp32: identity plus noise (sigma 3), then the fixed pixels (the same in every image)."""
    h, w, n = case["h"], case["w"], case["B"] * case["pairs"]
    rng = np.random.default_rng(case["seed"] + 500)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    c = np.stack([xs, ys])[None] + 3.0 * rng.standard_normal((n, 2, h, w))
    for (y, x), (cx, cy) in fixed_coords(h, w).values():
        c[:, 0, y, x], c[:, 1, y, x] = cx, cy
    return c.reshape(n, 2, h * w).astype(np.float32)


# ---- the float64 reference ------------------------------------------------------------------------------------------------------
def pool(x):
    """Floor 2 x 2 mean over the last two dims."""
    H2, W2 = x.shape[-2] // 2, x.shape[-1] // 2
    x = x[..., : 2 * H2, : 2 * W2].reshape(*x.shape[:-2], H2, 2, W2, 2)
    return (x[..., 0, :, 0] + x[..., 0, :, 1] + x[..., 1, :, 0] + x[..., 1, :, 1]) * 0.25


def pyramid(f1, f2, h, w):
    """f1, f2 [D][N] -> four float64 levels [N][h >> l][w >> l]."""
    f1, f2 = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    lv = [(f1.T @ f2 / math.sqrt(f1.shape[0])).reshape(-1, h, w)]
    for _ in range(3):
        lv.append(pool(lv[-1]))
    return lv


def lookup(levels, xy, wrong=None):
    """levels: four [N][hl][wl] float64 maps of ONE image; xy [2][N] fp32.  Returns (out [324][N], asum [324][N] = sum of |cell| over the
    four taps, dead [324][N] = every tap outside).  wrong: 'swap_ab', 'drop_tap4', 'clamp'."""
    N = xy.shape[1]
    out, asum, dead = np.zeros((324, N)), np.zeros((324, N)), np.ones((324, N), bool)
    pix = np.arange(N)
    for l, m in enumerate(levels):
        hl, wl = m.shape[1:]
        c = np.asarray(xy, np.float64) * 2.0 ** -l
        c = np.where((c > -1.0e6) & (c < 1.0e6), c, -1.0e6)
        c0 = np.floor(c)
        fx, fy = c[0] - c0[0], c[1] - c0[1]
        x0, y0 = c0[0].astype(np.int64), c0[1].astype(np.int64)
        P = np.zeros((N, hl + 2, wl + 2))
        P[:, 1:-1, 1:-1] = m
        if wrong == "clamp":
            P = np.pad(m, ((0, 0), (1, 1), (1, 1)), mode="edge")
        for a in range(9):
            for b in range(9):
                ch = l * 81 + (b * 9 + a if wrong == "swap_ab" else a * 9 + b)
                for k, (dy, dx, wt) in enumerate(((0, 0, (1 - fx) * (1 - fy)), (0, 1, fx * (1 - fy)), (1, 0, (1 - fx) * fy), (1, 1, fx * fy))):
                    if wrong == "drop_tap4" and k == 3:
                        continue
                    yy, xx = y0 + b - 4 + dy, x0 + a - 4 + dx
                    v = P[pix, np.clip(yy, -1, hl) + 1, np.clip(xx, -1, wl) + 1]
                    out[ch] += v * wt
                    asum[ch] += np.abs(v)
                    dead[ch] &= ~((yy >= 0) & (yy < hl) & (xx >= 0) & (xx < wl))
    return out, asum, dead


def lookup_bound(asum):
    return LOOKUP_MULT * ACC * asum + 2.0 ** -126


# ---- arithmetic classes ---------------------------------------------------------------------------------------------------------
def blocked_fold(D, pairs, frames_shared):
    """csrc/corr_blocked.hip (host side), restated: (shared, pre_a, pre_b, post) -- post is what the epilogue multiplies with."""
    scale = np.float32(1.0) / np.sqrt(np.float32(D))
    root = np.sqrt(scale)
    pow2, root_pow2 = math.frexp(float(scale))[0] == 0.5, math.frexp(float(root))[0] == 0.5
    shared = bool(pairs > 1 and frames_shared and (root_pow2 or not pow2))
    fold = root_pow2 if shared else pow2
    if not fold:
        return shared, 1.0, 1.0, float(scale)
    return (shared, float(root), float(root), 1.0) if shared else (shared, float(scale), 1.0, 1.0)


def klass(name, D=1, pairs=1, frames_shared=False):
    """name: 'fp32', 'x3' (F16X3 and blocked fp32), 'f16' (dense fp16 cells), 'b16' (blocked fp16 cells).  Returns a dict: how the
    operands are held, the powers of two folded into them, products per k, the cell format."""
    if name == "b16":
        shared, pa, pb, _ = blocked_fold(D, pairs, frames_shared)
        return dict(name=name, oper="f16", pa=pa, pb=pb, prod=1, cell16=True, shared=shared)
    return dict(name=name, oper={"fp32": "f32", "x3": "split", "f16": "f16", "x1": "f16"}[name], pa=1.0, pb=1.0, prod=3 if name == "x3" else 1,
                cell16=name == "f16", shared=False)                                # 'x1': a wrong kernel -- one fp16 product, fp32 cells


def _dx(x, how):
    if how == "split":                                       # split8(): towards zero twice
        return np.maximum(2.0 ** -20 * np.abs(x), 2.0 * SUB) + np.where(np.abs(x) < 2.0 ** -14, 2.0 * SUB, 0.0)
    return np.zeros_like(x) if how == "f32" else np.maximum(EPS[how] * np.abs(x), SUB)


def build_bound(f1, f2, h, w, K):
    """Per stored cell of the four levels: (bounds, exact levels)."""
    f1, f2 = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    D = f1.shape[0]
    s = 1.0 / math.sqrt(D)
    a, b = np.abs(f1) * K["pa"], np.abs(f2) * K["pb"]
    post = s / (K["pa"] * K["pb"])
    S = (a.T @ b * post).reshape(-1, h, w)
    oper = ((_dx(a, K["oper"]).T @ b + a.T @ _dx(b, K["oper"])) * post).reshape(-1, h, w)
    if K["oper"] == "split":
        oper = oper + 2.0 ** -20 * S
    B = oper + (K["prod"] * D + 4) * ACC * S
    exact = pyramid(f1, f2, h, w)
    out = []
    for l in range(4):
        if l:
            B, S = pool(B) + 2 * ACC * pool(S + B), pool(S)
        out.append(2.0 * (B + np.maximum(2.0 ** -11 * (np.abs(exact[l]) + B), SUB) if K["cell16"] else B))
    return out, exact


def build_cap(exact, K):
    return 2.0 ** -11 * np.abs(exact) + CAP_F16_ABS if K["cell16"] else np.full_like(exact, CAP_SPLIT)


def f16z(x):
    """Round towards zero to IEEE fp16 (v_cvt_pkrtz_f16_f32), subnormals kept; returned as float64."""
    x = np.asarray(x, np.float64)
    h = x.astype(np.float16)
    return np.where(np.abs(h.astype(np.float64)) > np.abs(x), np.nextafter(h, np.float16(0.0)), h).astype(np.float64)


def _parts(x, how):
    if how == "f32":
        return f32(x), None
    if how == "f16":
        return f16(x), None
    x32 = np.asarray(x, np.float64).astype(np.float32)       # split8(): hi = the fp32 bits & 0xFFFFE000, lo = x - hi (exact), both cut
    ah = (x32.view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32).astype(np.float64)
    return f16z(ah), f16z(x32.astype(np.float64) - ah)


def model(f1, f2, h, w, K, wrong=None):
    """Numpy emulation of what the kernel rounds: operands times the folded power of two THEN rounded, one fp32 rounding per k of the
    running sum, the fp32 scale, fp32 pooling of the unrounded level-0 values (vertical pair, horizontal pair, times 0.25), the cell
    rounded once.  wrong: 'inv_d' (1 / D), 'ceil_pool', 'shift_l2' (level 2 from level 0, origin one column on), 'fold_twice'."""
    D = f1.shape[0]
    pa, pb = (K["pa"] ** 2, K["pb"] ** 2) if wrong == "fold_twice" else (K["pa"], K["pb"])
    ah, al = _parts(np.asarray(f1, np.float64) * pa, K["oper"])
    bh, bl = _parts(np.asarray(f2, np.float64) * pb, K["oper"])
    acc = np.zeros((ah.shape[1], bh.shape[1]))
    for k in range(D):
        p = np.outer(ah[k], bh[k])
        if al is not None:
            p += np.outer(ah[k], bl[k]) + np.outer(al[k], bh[k])
        acc = f32(acc + p)
    s32 = np.float32(1.0) / (np.float32(D) if wrong == "inv_d" else np.sqrt(np.float32(D)))
    post = 1.0 if K["pa"] * K["pb"] != 1.0 else float(s32)
    lv = [f32(acc * post).reshape(-1, h, w)]
    for l in range(1, 4):
        x = lv[-1]
        if wrong == "ceil_pool":
            x = np.pad(x, ((0, 0), (0, x.shape[1] % 2), (0, x.shape[2] % 2)))
        H2, W2 = x.shape[1] // 2, x.shape[2] // 2
        x = x[:, : 2 * H2, : 2 * W2].reshape(-1, H2, 2, W2, 2)
        v = f32(x[:, :, 0] + x[:, :, 1])
        lv.append(f32(0.25 * f32(v[..., 0] + v[..., 1])))
    if wrong == "shift_l2":
        x = lv[0][:, :, 1:]
        for _ in range(2):
            x = pool(x)
        lv[2] = np.pad(x, ((0, 0), (0, lv[2].shape[1] - x.shape[1]), (0, lv[2].shape[2] - x.shape[2])))
    return [f16(x) for x in lv] if K["cell16"] else lv


# ---- sizes and geometry, restated (include/streamflow_hip.h; the workspace formulas from the three host entry points) ------------
def _up(x, m):
    return -(-x // m) * m


def build_ws_bytes(B, pairs, D, h, w):
    """(f1, f2) x images x (hi, lo) fp16 planes of D rounded up to 32 rows."""
    return 2 * B * pairs * _up(D, 32) * h * w * 4


def blocked_geometry(h, w, f32cells):
    """Blocks of 8 x 8 fp16 cells, or of 4 rows x 8 columns fp32 cells: 128 bytes either way."""
    rows = 4 if f32cells else 8
    nby = [_up(h >> l, rows) // rows for l in range(4)]
    nbx = [_up(w >> l, 8) // 8 for l in range(4)]
    off = [sum(nby[k] * nbx[k] * 128 for k in range(l)) for l in range(5)]
    return dict(rec_bytes=off[4], lvl_off=off[:4], nby=nby, nbx=nbx, src_rows=_up(h * w, 128))


def blocked_bytes(n_img, h, w, f32cells):
    g = blocked_geometry(h, w, f32cells)
    return n_img * g["src_rows"] * g["rec_bytes"]


def blocked_ws_bytes(n_img, D, h, w):
    """Two fp16 k-octet images [256 / 8][Np][8] per image, Np = N + 1 zero pixel rounded up to 8."""
    return 2 * n_img * 32 * _up(h * w + 1, 8) * 16


def blocked32_ws_bytes(n_img, D, h, w):
    return 2 * n_img * 2 * (_up(D, 32) // 8) * h * w * 16


# ---- decoders: raw bytes -> cells [n_img][N][hl][wl] float64 --------------------------------------------------------------------
def decode_rows(raw, dtype, B, pairs, N, hl, wl, pitch=None, pair_stride=0, base=0):
    """raw: the level's whole buffer (uint8).  Level map of (pair t, clip b, source i): hl rows of `pitch` cells at cell
    base + t * pair_stride + (b * N + i) * hl * pitch; cell (y, x) at y * pitch + x."""
    pitch = wl if pitch is None else pitch
    cells = np.frombuffer(np.ascontiguousarray(raw).tobytes(), dtype=dtype)
    t = np.arange(pairs)[None, :, None, None, None]
    b = np.arange(B)[:, None, None, None, None]
    i = np.arange(N)[None, None, :, None, None]
    y = np.arange(hl)[None, None, None, :, None]
    x = np.arange(wl)[None, None, None, None, :]
    idx = base + t * pair_stride + (b * N + i) * hl * pitch + y * pitch + x
    return cells[idx].reshape(B * pairs, N, hl, wl).astype(np.float64)


def decode_dense_f32(raw, B, pairs, N, hl, wl, pair_stride=0, base=0):
    return decode_rows(raw, np.float32, B, pairs, N, hl, wl, None, pair_stride, base)


def decode_dense_f16(raw, B, pairs, N, hl, wl, pair_stride=0, base=0):
    return decode_rows(raw, np.float16, B, pairs, N, hl, wl, None, pair_stride, base)


def decode_pitched_f32(raw, B, pairs, N, hl, wl, pitch, pair_stride=0, base=0):
    return decode_rows(raw, np.float32, B, pairs, N, hl, wl, pitch, pair_stride, base)


def blocked_cell_bytes(h, w, f32cells, l, wrong=None):
    """Byte offset inside a record of every cell (ty, tx) of level l: [hl][wl] int64."""
    g = blocked_geometry(h, w, f32cells)
    ty, tx = np.meshgrid(np.arange(h >> l), np.arange(w >> l), indexing="ij")
    if f32cells:
        return g["lvl_off"][l] + ((ty // 4) * g["nbx"][l] + tx // 8) * 128 + ((tx % 8) * 4 + ty % 4) * 4
    cell = (ty % 8) * 8 + tx % 8 if wrong == "cell_order" else (tx % 8) * 8 + ty % 8
    return g["lvl_off"][l] + ((ty // 8) * g["nbx"][l] + tx // 8) * 128 + cell * 2


def decode_blocked(raw, f32cells, n_img, h, w, img_stride=None, wrong=None):
    """raw: uint8 from the volume's base.  Four levels [n_img][N][hl][wl] float64."""
    g = blocked_geometry(h, w, f32cells)
    img_stride = g["src_rows"] * g["rec_bytes"] if img_stride is None else img_stride
    es = 4 if f32cells else 2
    cells = np.frombuffer(np.ascontiguousarray(raw).tobytes(), dtype=np.float32 if f32cells else np.float16)
    out = []
    for l in range(4):
        cb = blocked_cell_bytes(h, w, f32cells, l, wrong)[None, None]
        idx = np.arange(n_img)[:, None, None, None] * img_stride + np.arange(h * w)[None, :, None, None] * g["rec_bytes"] + cb
        out.append(cells[idx // es].astype(np.float64))
    return out


def blocked_data_mask(n_img, h, w, f32cells, img_stride=None):
    """bool per byte of n_img images at img_stride: True where the header calls the byte data (a cell of a level of a source pixel)."""
    g = blocked_geometry(h, w, f32cells)
    img_stride = g["src_rows"] * g["rec_bytes"] if img_stride is None else img_stride
    es = 4 if f32cells else 2
    m = np.zeros(n_img * img_stride, bool)
    for l in range(4):
        cb = blocked_cell_bytes(h, w, f32cells, l).reshape(-1)
        idx = (np.arange(n_img)[:, None, None] * img_stride + np.arange(h * w)[None, :, None] * g["rec_bytes"] + cb[None, None]).reshape(-1)
        for e in range(es):
            m[idx + e] = True
    return m


def decode_koct(halves, n_img, N, img_stride):
    """k-octet planes [41][N][8] per image (fp16 array from the view's base) -> ([n_img][324][N], [n_img][4][N] rows 324..327)."""
    r = np.arange(328)[None, :, None]
    idx = np.arange(n_img)[:, None, None] * img_stride + ((r // 8) * N + np.arange(N)[None, None, :]) * 8 + r % 8
    v = np.asarray(halves)[idx]
    return v[:, :324], v[:, 324:]
