"""Cases and a numpy restatement of csrc/stabilize.hip (include/streamflow_hip.h, "video stabilisation") for
tests/test_stabilize_cases_cpu.py, tests/test_gpu_stabilize.py and tests/test_gpu_stabilize_video.py:

* `weights32` / `moments64`: the per-pixel weight in float32 operation by operation (every numpy operation rounds once, as the kernel
  does with contraction off), the thirteen sums in float64 of float64 products in the header's order, with the sum of the terms'
  magnitudes and their number next to every sum (the reordering bound `terms * 2^-52 * sum |term|` needs them);
* `solve64`: the header's closed forms and Cholesky factor in float64; `fit`: the chain, round by round, as a trace like the kernel's;
* `warp_affine32`: sf_warp_affine_u8 in float32 operation by operation: bytes and outside counts must be BITWISE the kernel's;
* `lstsq64`: an independent float64 weighted least squares through numpy.linalg.lstsq on the design matrix;
* `robust_case`: an affine camera plus a rectangle of a quarter of the area that moves on its own, plus noise.

This is the project's own code: nothing here is taken from the reference's text."""
import numpy as np

f32, f64 = np.float32, np.float64
TRANSLATION, SIMILARITY, AFFINE = 0, 1, 2
(S1, SX, SY, SXX, SXY, SYY, SU, SXU, SYU, SV, SXV, SYV, SQQ, N) = range(14)
LEN, TRACE_LEN = 14, 23
T_MODEL, T_C, T_INV_C2, T_STATUS = 14, 20, 21, 22
OK, DEGENERATE, EMPTY = 0, 1, 2
CONSTANT, REPLICATE = 0, 1


def coords32(h, w, step=1):
    """(xs, ys integer sample positions; xn, yn float32 normalised coordinates of them)."""
    xs, ys = np.arange(0, w, step), np.arange(0, h, step)
    cx, cy = f32(w - 1) * f32(0.5), f32(h - 1) * f32(0.5)
    s = f32(2.0) / f32(max(w - 1, h - 1, 1))
    return xs, ys, (xs.astype(f32) - cx) * s, (ys.astype(f32) - cy) * s


def weights32(flows, cls=None, codes=(0, 1, 2), class_weights=(1.0, 0.0, 0.0), step=1, max_mag=None, model=None, inv_c2=None):
    """(wt float32 [n, hs, ws]; xn [ws], yn [hs]; u, v float32 [n, hs, ws]) of the pixels that take part."""
    flows = np.asarray(flows, f32)
    n, _, h, w = flows.shape
    max_mag = f32(4.0 * max(h, w) if max_mag is None else max_mag)
    xs, ys, xn, yn = coords32(h, w, step)
    u, v = flows[:, 0][:, ys][:, :, xs], flows[:, 1][:, ys][:, :, xs]
    with np.errstate(all="ignore"):
        valid = (np.abs(u) <= max_mag) & (np.abs(v) <= max_mag)
        if cls is None:
            wt = np.ones(u.shape, f32)
        else:
            b = np.asarray(cls)[:, ys][:, :, xs]
            wt = np.where(b == codes[0], f32(class_weights[0]), np.where(b == codes[1], f32(class_weights[1]),
                          np.where(b == codes[2], f32(class_weights[2]), f32(0)))).astype(f32)
        if model is not None:
            a = np.asarray(model, f32).reshape(n, 6)[:, :, None, None]
            X, Y = xn[None, None, :], yn[None, :, None]
            pu = a[:, 0] + (a[:, 1] * X + a[:, 2] * Y)
            pv = a[:, 3] + (a[:, 4] * X + a[:, 5] * Y)
            ru, rv = u - pu, v - pv
            r2 = ru * ru + rv * rv
            t = r2 * np.asarray(inv_c2, f32).reshape(n, 1, 1)
            g = f32(1) - t
            wr = np.where(t < f32(1), g * g, f32(0)).astype(f32)
            wt = wt * wr
        wt = np.where(valid, wt, f32(0)).astype(f32)
    return wt, xn, yn, u, v


def moments64(wt, xn, yn, u, v):
    """(moments, sum of |term|, number of terms) float64 [n, LEN] each, from weights32's outputs."""
    n = wt.shape[0]
    mom, mag, cnt = np.zeros((n, LEN)), np.zeros((n, LEN)), np.zeros((n, LEN))
    for i in range(n):
        take = wt[i] > 0
        W = wt[i][take].astype(f64)
        X = np.broadcast_to(xn[None, :], wt[i].shape)[take].astype(f64)
        Y = np.broadcast_to(yn[:, None], wt[i].shape)[take].astype(f64)
        U, V = u[i][take].astype(f64), v[i][take].astype(f64)
        WX, WY = W * X, W * Y
        terms = [W, WX, WY, WX * X, WX * Y, WY * Y, W * U, WX * U, WY * U, W * V, WX * V, WY * V, W * (U * U + V * V)]
        for k, t in enumerate(terms):
            mom[i, k], mag[i, k] = t.sum(), np.abs(t).sum()
        mom[i, N] = mag[i, N] = W.size
        cnt[i] = W.size
    return mom, mag, cnt


def solve64(m, kind, kappa=2.0, c_floor=1.0):
    """One field: moments [LEN] -> (model float64 [6], c, inv_c2 float32, status, rss / S1), the header's formulas in float64."""
    m = np.asarray(m, f64)
    s1, sx, sy, sxx, sxy, syy, su, sxu, syu, sv, sxv, syv, sqq = (m[k] for k in range(13))
    a = np.zeros(6)
    status, rss = OK, 0.0
    with np.errstate(all="ignore"):
        if not s1 > 0.0:
            status = EMPTY
        else:
            thr = 2.0 ** -40 * s1
            done = kind == TRANSLATION
            if kind == AFFINE:
                l00 = np.sqrt(s1)
                l10, l20 = sx / l00, sy / l00
                d1 = sxx - l10 * l10
                if d1 > thr:
                    l11 = np.sqrt(d1)
                    l21 = (sxy - l20 * l10) / l11
                    d2 = (syy - l20 * l20) - l21 * l21
                    if d2 > thr:
                        l22 = np.sqrt(d2)
                        for o, (b0, b1, b2) in ((0, (su, sxu, syu)), (3, (sv, sxv, syv))):
                            z0 = b0 / l00
                            z1 = (b1 - l10 * z0) / l11
                            z2 = ((b2 - l20 * z0) - l21 * z1) / l22
                            a[o + 2] = z2 / l22
                            a[o + 1] = (z1 - l21 * a[o + 2]) / l11
                            a[o] = ((z0 - l10 * a[o + 1]) - l20 * a[o + 2]) / l00
                        done = True
            elif kind == SIMILARITY:
                D = (sxx + syy) - (sx * sx + sy * sy) / s1
                if D > thr:
                    p = ((sxu + syv) - (sx * su + sy * sv) / s1) / D
                    q = ((syu - sxv) - (sy * su - sx * sv) / s1) / D
                    a[0] = ((su - p * sx) - q * sy) / s1
                    a[3] = ((sv + q * sx) - p * sy) / s1
                    a[1], a[5], a[2], a[4] = p, p, q, -q
                    done = True
            if not done:
                status = DEGENERATE
            if not done or kind == TRANSLATION:
                a[:] = 0.0
                a[0], a[3] = su / s1, sv / s1
            pb = ((a[0] * su + a[1] * sxu) + a[2] * syu) + ((a[3] * sv + a[4] * sxv) + a[5] * syv)
            quad = lambda p0, p1, p2: ((p0 * ((s1 * p0 + sx * p1) + sy * p2) + p1 * ((sx * p0 + sxx * p1) + sxy * p2))
                                       + p2 * ((sy * p0 + sxy * p1) + syy * p2))
            rss = max(0.0, (sqq - 2.0 * pb) + (quad(a[0], a[1], a[2]) + quad(a[3], a[4], a[5]))) / s1
        c = max(c_floor, kappa * np.sqrt(rss)) if rss == rss else c_floor
    return a, c, f32(1.0 / (c * c)), status, rss


def normal_matrix(m, kind):
    """(the normal equations' matrix of `kind` from a moment row, its right-hand sides): what numpy.linalg.solve gets in the tests."""
    s1, sx, sy, sxx, sxy, syy = (m[k] for k in range(6))
    M3 = np.array([[s1, sx, sy], [sx, sxx, sxy], [sy, sxy, syy]])
    if kind == TRANSLATION:
        return np.array([[s1]]), [np.array([m[SU]]), np.array([m[SV]])]
    if kind == AFFINE:
        return M3, [m[[SU, SXU, SYU]], m[[SV, SXV, SYV]]]
    t = sxx + syy                                                        # unknowns (a0, a3, a, b)
    M4 = np.array([[s1, 0, sx, sy], [0, s1, sy, -sx], [sx, sy, t, 0], [sy, -sx, 0, t]])
    return M4, [np.array([m[SU], m[SV], m[SXU] + m[SYV], m[SYU] - m[SXV]])]


def unknowns(a, kind):
    """A model [6] as the unknown vectors of normal_matrix's systems."""
    if kind == TRANSLATION:
        return [a[[0]], a[[3]]]
    if kind == AFFINE:
        return [a[:3], a[3:]]
    return [np.array([a[0], a[3], a[1], a[2]])]


def fit(flows, kind, rounds=6, kappa=2.0, c_floor=1.0, **weights):
    """The chain: trace float64 [n, rounds, TRACE_LEN] as sf_motion_fit writes it."""
    n = np.asarray(flows).shape[0]
    trace = np.zeros((n, rounds, TRACE_LEN))
    model, inv_c2 = None, None
    for r in range(rounds):
        mom, _, _ = moments64(*weights32(flows, model=model, inv_c2=inv_c2, **weights))
        trace[:, r, :LEN] = mom
        for i in range(n):
            a, c, ic, status, _ = solve64(mom[i], kind, kappa, c_floor)
            trace[i, r, T_MODEL:T_MODEL + 6], trace[i, r, T_C], trace[i, r, T_INV_C2], trace[i, r, T_STATUS] = a, c, f64(ic), status
        model, inv_c2 = trace[:, r, T_MODEL:T_MODEL + 6].astype(f32), trace[:, r, T_INV_C2].astype(f32)
    return trace


def to_pixels(a, h, w):
    """Normalised model [6] -> float64 [2, 3] with p' = M [x, y, 1] in pixels."""
    a = np.asarray(a, f64)
    cx, cy, s = (w - 1) * 0.5, (h - 1) * 0.5, 2.0 / max(w - 1, h - 1, 1)
    return np.array([[1.0 + a[1] * s, a[2] * s, a[0] - a[1] * s * cx - a[2] * s * cy],
                     [a[4] * s, 1.0 + a[5] * s, a[3] - a[4] * s * cx - a[5] * s * cy]])


def corner_error(Ma, Mb, h, w):
    """The largest distance (px) between where two pixel models [2, 3] send the four frame corners."""
    q = np.array([[0, 0, 1], [w - 1, 0, 1], [0, h - 1, 1], [w - 1, h - 1, 1]], f64)
    return float(np.linalg.norm(q @ np.asarray(Ma, f64).T - q @ np.asarray(Mb, f64).T, axis=1).max())


def lstsq64(wt, xn, yn, u, v, kind):
    """One field, independent of the normal equations: numpy.linalg.lstsq on sqrt(w)-scaled rows of the design matrix, float64."""
    take = wt > 0
    sw = np.sqrt(wt[take].astype(f64))
    X = np.broadcast_to(xn[None, :], wt.shape)[take].astype(f64)
    Y = np.broadcast_to(yn[:, None], wt.shape)[take].astype(f64)
    U, V = u[take].astype(f64), v[take].astype(f64)
    one, zero = np.ones_like(X), np.zeros_like(X)
    if kind == TRANSLATION:
        cols_u, cols_v = [one, zero], [zero, one]
    elif kind == SIMILARITY:                                             # unknowns (a0, a3, a, b)
        cols_u, cols_v = [one, zero, X, Y], [zero, one, Y, -X]
    else:
        cols_u, cols_v = [one, X, Y, zero, zero, zero], [zero, zero, zero, one, X, Y]
    A = np.concatenate([np.stack(cols_u, 1) * sw[:, None], np.stack(cols_v, 1) * sw[:, None]])
    p = np.linalg.lstsq(A, np.concatenate([U * sw, V * sw]), rcond=None)[0]
    if kind == TRANSLATION:
        return np.array([p[0], 0, 0, p[1], 0, 0])
    if kind == SIMILARITY:
        return np.array([p[0], p[2], p[3], p[1], -p[3], p[2]])
    return p


def model_flow(Mpx, h, w):
    """The flow field float64 [2, h, w] of a pixel model [2, 3]: p' - p."""
    x, y = np.arange(w, dtype=f64)[None, :], np.arange(h, dtype=f64)[:, None]
    M = np.asarray(Mpx, f64)
    return np.stack([M[0, 0] * x + M[0, 1] * y + M[0, 2] - x, M[1, 0] * x + M[1, 1] * y + M[1, 2] - y + 0 * x])


def camera(seed, h, w, kind=AFFINE):
    """A seeded camera motion [2, 3] of the given kind: a few pixels of shift, about a degree of rotation, a percent of scale."""
    rng = np.random.default_rng(seed)
    tx, ty = rng.uniform(-4, 4, 2)
    if kind == TRANSLATION:
        return np.array([[1, 0, tx], [0, 1, ty]], f64)
    th, sc = rng.uniform(-0.03, 0.03), 1.0 + rng.uniform(-0.02, 0.02)
    A = sc * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    if kind == AFFINE:
        A = A + rng.uniform(-0.01, 0.01, (2, 2))
    c = np.array([(w - 1) * 0.5, (h - 1) * 0.5])
    return np.concatenate([A, (c - A @ c + [tx, ty])[:, None]], axis=1)


def make_fields(seed, n, h, w, noise=0.3, kind=AFFINE):
    """n seeded fields float32 [n, 2, h, w]: a camera each plus Gaussian noise; and the cameras [n, 2, 3]."""
    rng = np.random.default_rng(seed)
    cams = np.stack([camera(seed * 100 + i, h, w, kind) for i in range(n)])
    flows = np.stack([model_flow(cams[i], h, w) for i in range(n)]) + noise * rng.standard_normal((n, 2, h, w))
    return flows.astype(f32), cams


def robust_case(seed, h, w):
    """(flow float32 [1, 2, h, w], camera [2, 3]): an affine camera, a rectangle of 25 % of the area (half the height, half the width,
    seeded position) moving by (+9, -6) px on its own, 0.05 px Gaussian noise."""
    rng = np.random.default_rng(seed)
    cam = camera(seed, h, w, AFFINE)
    flow = model_flow(cam, h, w)
    rh, rw = h // 2, w // 2
    y0, x0 = int(rng.integers(0, h - rh + 1)), int(rng.integers(0, w - rw + 1))
    flow[0, y0:y0 + rh, x0:x0 + rw] += 9.0
    flow[1, y0:y0 + rh, x0:x0 + rw] -= 6.0
    flow += 0.05 * rng.standard_normal(flow.shape)
    return flow[None].astype(f32), cam


def make_cls(seed, n, h, w, codes=(0, 1, 2)):
    """A seeded class map uint8 [n, h, w]: mostly the first code, blobs of the second, a border strip of the third, a few other bytes."""
    rng = np.random.default_rng(seed)
    r = rng.random((n, h, w))
    cls = np.where(r < 0.7, codes[0], np.where(r < 0.85, codes[1], np.where(r < 0.97, codes[2], 200))).astype(np.uint8)
    return cls


def warp_affine32(src_hwc, maps, border=REPLICATE, fill=(0, 0, 0)):
    """(out uint8 [n, h, w, 3], outside int64 [n]) of sf_warp_affine_u8, float32 operation by operation."""
    src = np.asarray(src_hwc)
    n, h, w, _ = src.shape
    m = np.asarray(maps, f32).reshape(n, 6)[:, :, None, None]
    x, y = np.arange(w, dtype=f32)[None, None, :], np.arange(h, dtype=f32)[None, :, None]
    xmax, ymax = f32(w - 1), f32(h - 1)
    with np.errstate(all="ignore"):
        px = m[:, 0] * x + (m[:, 1] * y + m[:, 2])
        py = m[:, 3] * x + (m[:, 4] * y + m[:, 5])
        inside = (px >= f32(0)) & (px <= xmax) & (py >= f32(0)) & (py <= ymax)
        take = inside.copy()
        if border == REPLICATE:
            ok = ~inside & ~np.isnan(px) & ~np.isnan(py)
            px = np.where(ok, np.minimum(np.maximum(px, f32(0)), xmax), px)
            py = np.where(ok, np.minimum(np.maximum(py, f32(0)), ymax), py)
            take |= ok
        pxs, pys = np.where(take, px, f32(0)).astype(f32), np.where(take, py, f32(0)).astype(f32)
        fx0, fy0 = np.floor(pxs), np.floor(pys)
        tx, ty = pxs - fx0, pys - fy0
        x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        i = np.arange(n)[:, None, None]
        gx, gy = f32(1) - tx, f32(1) - ty
        out = np.empty((n, h, w, 3), np.uint8)
        for c in range(3):
            p = src[..., c].astype(f32)
            top = gx * p[i, y0, x0] + tx * p[i, y0, x1]
            bot = gx * p[i, y1, x0] + tx * p[i, y1, x1]
            val = gy * top + ty * bot
            out[..., c] = np.where(take, np.floor(val + f32(0.5)), f32(fill[c])).astype(np.uint8)
    return out, (~inside).sum(axis=(1, 2)).astype(np.int64)
