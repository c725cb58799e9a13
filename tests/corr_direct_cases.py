"""Case lists, float64 reference, rounding models and the per-channel bound of tests/test_gpu_corr_direct.py: the volume-free
correlation route through the C ABI -- sf_corr_direct_ws_bytes / sf_corr_direct_pack / sf_corr_direct_lookup (csrc/corr_direct.hip).
Pure numpy on the CPU; tests/test_corr_direct_cases_cpu.py pins what is here.

REFERENCE.  corr_cases.pyramid + corr_cases.lookup, as for the volume routes (float64, in pixel space).  The direct route computes
level l at target cell J as <f1_i, pool_l(f2)_J> / sqrt(D), pool_l the floor 2 x 2 mean applied l times to the FEATURES of frame 2:
pooling is linear, so this is the same mathematics (feature_pyramid() below agrees with corr_cases.pyramid to 1e-12 on every case).

BOUND, per cell of level l (source pixel i, target cell J), with s = 1 / sqrt(D), p = pool_l(f2) in float64, A = pool_l(|f2|):

    E_l    what the fp32 pooling of the features adds to a pooled value: two additions per level, 2^-24 of the partial sums each (the
           factor 0.25 is exact); the partial sums are at most the pooled MAGNITUDES A:   E_0 = 0,
           E_l = pool(E_(l-1)) + 2 * 2^-24 (A_l + pool(E_(l-1)))
    q      the pooled value as the kernel holds it before it is rounded: |q| <= |p| + E
    OPER   s * sum_k ( dx(f1_ik) (|p_kJ| + E_kJ) + |f1_ik| (dx(|p_kJ| + E_kJ) + E_kJ) ):  the operand rounding of f1 and of the pooled f2
           (rounded ONCE), dx of the class as in corr_cases._dx (one fp16 rounding: max(2^-11 |x|, 2^-25); split8(): max(2^-20 |x|,
           2^-24) + 2^-24 below 2^-14), and the pooling error itself
    S      s * sum_k |f1_ik| (|p_kJ| + E_kJ)
    STEPS  (prod * D + 4) * 2^-24 * S: fp32 accumulation steps (MFMA-internal partial sums count as steps), prod = 1 (F16) or 3
           (F16X3); 4 = the scale (sqrtf, division, conversion, multiplication)
    DROP   2^-20 * S in the split class: the dropped lo * lo product
    B = OPER + STEPS + DROP.  Cells are never rounded to fp16 and never stored: no cell term.

per output channel:  2 * sum_taps w_t B_t  +  corr_cases.lookup_bound(sum_taps (|c_t| + B_t))
    w_t the bilinear weights (the output is LINEAR in the cells with exactly these weights, so the cell errors enter weighted;
    evaluated by running corr_cases.lookup over the maps B); the factor 2 as in corr_cases: every term is first order and attained,
    the factor covers second order and is the margin the rounding models must keep (inside HALF the bound); the blend's own nine
    roundings on the cells as the kernel holds them (|c| + B).  Nothing here comes from a kernel.

CAP.  corr_cases.CAP_LOOKUP (5e-5) on every case: a formality at the feature scale of the cases (2^-6); the GPU assertions use the
derived bound alone.

CASES.  corr_cases.cases() as they are (13 shapes, their features, `noise` = their coordinates: identity + sigma-3 noise + the 20
fixed edge / NaN / inf / 1e6 pixels), and three coordinate sets aimed at the lookup's tiles of 16 consecutive pixels and their
bounding boxes: `uniform` (every pixel uniformly random over [-8, w + 8) x [-8, h + 8): the box is the whole level), `dead_tile`
(noise, but every pixel of the second tile NaN or far outside, alternating), `corner` (noise around the top-left corner for the
first tile, but its pixel 5 points to the bottom-right corner).
"""
import functools
import math

import numpy as np

from tests import corr_cases as cc
from tests.corr_cases import ACC, F16, F16X3, f16, f32  # noqa: F401

COORD_SETS = ("noise", "uniform", "dead_tile", "corner")
TILE = 16
KLASSES = {"f16": dict(name="f16", oper="f16", prod=1, precision=F16), "x3": dict(name="x3", oper="split", prod=3, precision=F16X3)}


def cases():
    return cc.cases()


def coords(case, name):
    """[B * pairs][2][N] fp32."""
    h, w, n = case["h"], case["w"], case["B"] * case["pairs"]
    N = h * w
    if name == "noise":
        return cc.coords(case)
    rng = np.random.default_rng(case["seed"] + 900 + COORD_SETS.index(name))
    if name == "uniform":
        c = np.stack([rng.uniform(-8.0, w + 8.0, (n, N)), rng.uniform(-8.0, h + 8.0, (n, N))], 1)
        return c.astype(np.float32)
    c = cc.coords(case).astype(np.float64)
    if name == "dead_tile":
        t = np.arange(TILE, 2 * TILE)
        c[:, 0, t[0::2]], c[:, 1, t[0::2]] = np.nan, 3.0
        c[:, 0, t[1::2]], c[:, 1, t[1::2]] = w + 40.5, -(h + 40.25)
    else:
        t = np.arange(TILE)
        c[:, 0, t] = 1.5 + rng.standard_normal((n, TILE))
        c[:, 1, t] = 1.25 + rng.standard_normal((n, TILE))
        c[:, 0, 5], c[:, 1, 5] = w - 1.75, h - 1.5
    return c.astype(np.float32)


def ws_bytes(B, pairs, D, h, w, precision):
    """include/streamflow_hip.h, restated: parts * (Dp / 8) * 16 bytes per cell, 2 N + N1 + N2 + N3 cells per image."""
    parts = 2 if precision == F16X3 else 1
    cells = 2 * h * w + sum((h >> l) * (w >> l) for l in range(1, 4))
    return B * pairs * parts * (cc._up(D, 32) // 8) * 16 * cells


# ---- float64 ---------------------------------------------------------------------------------------------------------------------
def feature_pyramid(f1, f2, h, w):
    """The direct formulation in float64: four levels [N][hl][wl] from the pooled FEATURES of frame 2."""
    f1 = np.asarray(f1, np.float64)
    p = np.asarray(f2, np.float64).reshape(-1, h, w)
    s = 1.0 / math.sqrt(f1.shape[0])
    out = []
    for l in range(4):
        if l:
            p = cc.pool(p)
        out.append((f1.T @ p.reshape(p.shape[0], -1) * s).reshape(-1, h >> l, w >> l))
    return out


def cell_bound(f1, f2, h, w, K):
    """B per cell of the four levels: list of [N][hl][wl]."""
    f1 = np.abs(np.asarray(f1, np.float64))
    D = f1.shape[0]
    s = 1.0 / math.sqrt(D)
    p = np.asarray(f2, np.float64).reshape(-1, h, w)
    A, E = np.abs(p), np.zeros_like(p)
    out = []
    for l in range(4):
        if l:
            p, A = cc.pool(p), cc.pool(A)
            E = cc.pool(E)
            E = E + 2 * ACC * (A + E)
        q = (np.abs(p) + E).reshape(D, -1)
        e = E.reshape(D, -1)
        oper = s * (cc._dx(f1, K["oper"]).T @ q + f1.T @ (cc._dx(q, K["oper"]) + e))
        S = s * (f1.T @ q)
        B = oper + (K["prod"] * D + 4) * ACC * S
        if K["oper"] == "split":
            B = B + 2.0 ** -20 * S
        out.append(B.reshape(-1, h >> l, w >> l))
    return out


def channel_bound(Bmaps, asum, xy):
    """[324][N] from the cell bounds, the reference's sum of |cell| over the taps and the image's coordinates."""
    wsum, usum, _ = cc.lookup(Bmaps, xy)
    return 2.0 * wsum + cc.lookup_bound(asum + usum)


@functools.lru_cache(maxsize=None)
def _levels(case_id, amp):
    case = dict(next(c for c in cases() if c["id"] == case_id), amp=amp)
    F = cc.features(case)
    lv = []
    for b in range(case["B"]):
        for t in range(case["pairs"]):
            ex = cc.pyramid(F[b, t], F[b, t + 1], case["h"], case["w"])
            lv.append((ex, {k: cell_bound(F[b, t], F[b, t + 1], case["h"], case["w"], K) for k, K in KLASSES.items()}))
    return case, F, lv


@functools.lru_cache(maxsize=None)
def reference(case_id, coord_set, amp=cc.AMP):
    """Computed once per (case, coordinate set), shared and never modified: dict(case, F [B][pairs + 1][D][N] fp32, xy [n][2][N] fp32,
    out [n][324][N] float64, dead [n][324][N] bool, bound {'f16' | 'x3': [n][324][N]})."""
    case, F, lv = _levels(case_id, amp)
    xy = coords(case, coord_set)
    out, dead, bound = [], [], {k: [] for k in KLASSES}
    for img, (ex, Bm) in enumerate(lv):
        o, asum, d = cc.lookup(ex, xy[img])
        out.append(o)
        dead.append(d)
        for k in KLASSES:
            bound[k].append(channel_bound(Bm[k], asum, xy[img]))
    r = dict(case=case, F=F, xy=xy, out=np.stack(out), dead=np.stack(dead), bound={k: np.stack(v) for k, v in bound.items()})
    for a in (r["F"], r["xy"], r["out"], r["dead"], *r["bound"].values()):
        a.setflags(write=False)
    return r


# ---- rounding model --------------------------------------------------------------------------------------------------------------
def _pool32(x, wrong=None):
    """One level of the kernel's fp32 pooling: vertical pair, horizontal pair, times 0.25."""
    if wrong == "ceil_pool":
        x = np.pad(x, ((0, 0), (0, x.shape[1] % 2), (0, x.shape[2] % 2)))
    H2, W2 = x.shape[1] // 2, x.shape[2] // 2
    x = x[:, : 2 * H2, : 2 * W2].reshape(-1, H2, 2, W2, 2)
    v = f32(x[:, :, 0] + x[:, :, 1])
    return f32(0.25 * f32(v[..., 0] + v[..., 1]))


def _held(x, how):
    """The value an operand stands for after its rounding: fp16(x), or hi + lo of split8()."""
    hi, lo = cc._parts(x, how)
    return hi if lo is None else hi + lo


def model(f1, f2, h, w, K, wrong=None):
    """Numpy emulation of what the kernels round: fp32 pooling of the features, operands rounded once, one fp32 rounding per k of the
    running sum (hi hi + hi lo + lo hi per k in the split class), the fp32 scale.  Four levels [N][hl][wl] float64.
    wrong: 'inv_d' (1 / D), 'ceil_pool', 'stride' (level l = the unpooled features at stride 2^l), 'round_each' (the pooled features
    rounded to the operand format at EVERY level, the next level pooled from the rounded one)."""
    D = f1.shape[0]
    ah, al = cc._parts(np.asarray(f1, np.float64), K["oper"])
    p = f32(np.asarray(f2, np.float64).reshape(D, h, w))
    s32 = np.float32(1.0) / (np.float32(D) if wrong == "inv_d" else np.sqrt(np.float32(D)))
    out = []
    for l in range(4):
        if l:
            if wrong == "stride":
                p = p[:, : 2 * (p.shape[1] // 2): 2, : 2 * (p.shape[2] // 2): 2]
            else:
                p = _pool32(_held(p, K["oper"]) if wrong == "round_each" else p, wrong)
        bh, bl = cc._parts(p.reshape(D, -1), K["oper"])
        acc = np.zeros((ah.shape[1], bh.shape[1]))
        for k in range(D):
            q = np.outer(ah[k], bh[k])
            if al is not None:
                q += np.outer(ah[k], bl[k]) + np.outer(al[k], bh[k])
            acc = f32(acc + q)
        out.append(f32(acc * float(s32)).reshape(-1, *p.shape[1:]))
    return out


@functools.lru_cache(maxsize=None)
def _model_levels(case_id, amp, klass, wrong):
    case, F, _ = _levels(case_id, amp)
    return [model(F[b, t], F[b, t + 1], case["h"], case["w"], KLASSES[klass], wrong)
            for b in range(case["B"]) for t in range(case["pairs"])]


def model_out(ref, klass, wrong=None, lookup_wrong=None):
    """[n][324][N]: the model's levels (class `klass`: 'f16' | 'x3'; computed once per case, class and `wrong`) looked up in float64 at
    the reference's coordinates."""
    case = ref["case"]
    lv = _model_levels(case["id"], case.get("amp", cc.AMP), klass, wrong)
    return np.stack([cc.lookup(m, ref["xy"][img], lookup_wrong)[0] for img, m in enumerate(lv)])
