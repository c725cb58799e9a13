"""Cases and independent statements of sf_frame_interp (include/streamflow_hip.h, "frame interpolation") for
tests/test_interp_cases_cpu.py, tests/test_gpu_frame_interp.py and tests/test_gpu_interpolate.py:

* `make`: seeded generators of frame pairs and flows -- smooth sub-pixel flows, every pixel aimed at one target, flows that leave
  the frame on every edge by less and by more than a pixel, NaN / Inf / 1e30 entries, diverging flows that leave holes, zero flows,
  integer translations, and dyadic flows (multiples of 1/16, for t in {1/2, 1/4, 3/4}: the 1/64 weights are then exact).
* `restate`: the header's steps operation by operation -- float32 coordinates (every numpy operation rounds once, as the kernel does
  with contraction off), then integers, np.add.at on uint64.  The kernel must reproduce its bytes, cover codes and counts BITWISE.
* `restate_scalar`: the same contract as a pixel-by-pixel loop with Python ints (no vectorisation, no uint64 wrap-around to hide).
* `ideal64`: float64 splat with unquantised bilinear weights and real division, no rounding anywhere.

This is the project's own code: nothing here is taken from the reference's text."""
import numpy as np

from tests import consistency_cases as cc

f32 = np.float32
LEN, PIXELS, BOTH, A_ONLY, B_ONLY, HOLES = 5, 0, 1, 2, 3, 4
SPECIALS = (np.nan, np.inf, -np.inf, 1e30, -1e30)

# (id, kind, n, h, w, num, den): the smallest shapes at which each mechanism can go wrong -- one pixel; a row longer than one
# 256-pixel unit and a one-column field; a field that is no multiple of 4 or 64; several pairs with more than one unit per row
CASES = [
    ("1x1-zero", "zero", 1, 1, 1, 1, 2),
    ("1x1-smooth", "smooth", 2, 1, 1, 1, 3),
    ("1x300-smooth", "smooth", 1, 1, 300, 1, 2),
    ("1x300-edges", "edges", 1, 1, 300, 3, 4),
    ("300x1-smooth", "smooth", 1, 300, 1, 1, 3),
    ("300x1-edges", "edges", 2, 300, 1, 63, 64),
    ("13x37-smooth-1/2", "smooth", 2, 13, 37, 1, 2),
    ("13x37-smooth-1/3", "smooth", 2, 13, 37, 1, 3),
    ("13x37-smooth-3/4", "smooth", 1, 13, 37, 3, 4),
    ("13x37-smooth-63/64", "smooth", 1, 13, 37, 63, 64),
    ("13x37-converge-1/2", "converge", 2, 13, 37, 1, 2),
    ("13x37-converge-3/4", "converge", 1, 13, 37, 3, 4),
    ("13x37-edges-1/2", "edges", 1, 13, 37, 1, 2),
    ("13x37-edges-1/3", "edges", 1, 13, 37, 1, 3),
    ("13x37-special", "special", 2, 13, 37, 1, 3),
    ("13x37-holes", "holes", 2, 13, 37, 1, 2),
    ("13x37-holes-63/64", "holes", 1, 13, 37, 63, 64),
    ("13x37-zero", "zero", 1, 13, 37, 3, 4),
    ("5x260-smooth-1/2", "smooth", 3, 5, 260, 1, 2),
    ("5x260-smooth-1/3", "smooth", 3, 5, 260, 1, 3),
    ("5x260-special-3/4", "special", 3, 5, 260, 3, 4),
    ("5x260-holes-63/64", "holes", 3, 5, 260, 63, 64),
]
DYADIC = [("dyadic-%dx%d-%d/%d" % (h, w, num, den), "dyadic", n, h, w, num, den)
          for (n, h, w) in ((2, 13, 37), (1, 1, 300), (1, 300, 1), (3, 5, 260)) for (num, den) in ((1, 2), (1, 4), (3, 4))]
# Heavy contention, where the resolve leaves its 32-bit / 64-bit fast paths (run without class maps, importance 16):
# * dark-one-side: every pixel of a dark frame A (bytes 0 / 1, one noisy channel) lands on ONE pixel centre and nothing of B stays
#   in the frame: W = h * w * 4096 * 16 is exactly 2^31 at 128 x 256 and just above it at 130 x 256, so 2 W passes 32 bits while
#   2 C + W of the dark channels does not;
# * converge-grid: every pixel of both sides lands on one of 8 x 4 sub-pixel targets: about a hundred accumulators with W around
#   2^24 .. 2^26, on both sides of the threshold between the 64-bit blend and the 128-bit one, at every one of them.
BIG = [
    ("128x256-dark-one-side", "dark-one-side", 1, 128, 256, 1, 2),
    ("130x256-dark-one-side", "dark-one-side", 1, 130, 256, 1, 2),
    ("128x256-converge-grid-1/2", "converge-grid", 1, 128, 256, 1, 2),
    ("96x256-converge-grid-1/3", "converge-grid", 2, 96, 256, 1, 3),
]
# (class maps?, importances)
VARIANTS = [(False, (16, 1, 16)), (True, (16, 1, 16)), (True, (1, 1, 1))]


def case_ids(cases=CASES):
    return [c[0] for c in cases]


def _seed(name: str) -> int:
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (1 << 31)


def make(kind: str, seed: int, n: int, h: int, w: int, num: int, den: int):
    """(a, b uint8 [n, h, w, 3]; fwd, bwd fp32 [n, 2, h, w]) as numpy arrays."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    b = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    fwd = np.zeros((n, 2, h, w), f32)
    bwd = np.zeros((n, 2, h, w), f32)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    tf, tb = num / den, (den - num) / den
    if kind == "zero":
        pass
    elif kind in ("smooth", "special"):
        for i in range(n):
            tx, ty = rng.uniform(-2.5, 2.5, size=2)
            ph = rng.uniform(0, 2 * np.pi, size=4)
            su = tx + 0.8 * np.sin(2 * np.pi * xs / max(w, 8) + ph[0]) + 0.6 * np.cos(2 * np.pi * ys / max(h, 8) + ph[1])
            sv = ty + 0.7 * np.cos(2 * np.pi * xs / max(w, 8) + ph[2]) + 0.5 * np.sin(2 * np.pi * ys / max(h, 8) + ph[3])
            fwd[i, 0], fwd[i, 1] = su, sv
            bwd[i, 0] = -su + 0.05 * rng.standard_normal((h, w))
            bwd[i, 1] = -sv + 0.05 * rng.standard_normal((h, w))
        if kind == "special":
            for field in (fwd, bwd):
                for i in range(n):
                    pos = rng.choice(h * w, size=min(h * w, 3 * len(SPECIALS)), replace=False)
                    for k, q in enumerate(pos):
                        bad = SPECIALS[k % len(SPECIALS)]
                        comp = (k // len(SPECIALS)) % 3                   # u, v, both
                        if comp in (0, 2):
                            field[i, 0].reshape(-1)[q] = bad
                        if comp in (1, 2):
                            field[i, 1].reshape(-1)[q] = bad
    elif kind == "converge":
        # every pixel of both sides lands on one target at time t: on a pixel centre for pair 0 (one accumulator takes h * w adds
        # of weight 4096), a quarter pixel off it for the others (four accumulators)
        for i in range(n):
            cx, cy = (w // 2, h // 2) if i == 0 else (w // 3 + 0.25, h // 3 + 0.75)
            fwd[i, 0], fwd[i, 1] = (cx - xs) / tf, (cy - ys) / tf
            bwd[i, 0], bwd[i, 1] = (cx - xs) / tb, (cy - ys) / tb
    elif kind == "dark-one-side":
        a[..., :2] = rng.random((n, h, w, 2)) < 0.1                       # bytes 0 / 1: the true means are 0; channel 2 stays noise
        fwd[:, 0], fwd[:, 1] = (w // 2 - xs) / tf, (h // 2 - ys) / tf
        bwd[:] = 1e30
    elif kind == "converge-grid":
        for i in range(n):
            tx, ty = w // 2 + xs % 8 + 0.25, h // 2 + ys % 4 + 0.5
            fwd[i, 0], fwd[i, 1] = (tx - xs) / tf, (ty - ys) / tf
            bwd[i, 0], bwd[i, 1] = (tx + 0.5 - xs) / tb, (ty - 0.25 - ys) / tb
    elif kind == "edges":
        # the two outermost columns / rows are pushed over their edge by half a pixel and by two and a half pixels (the next ring by
        # one and a half): partly outside, more than a pixel outside, and wholly outside
        dx = np.zeros((h, w))
        dy = np.zeros((h, w))
        for ring, d in ((0, 0.5), (1, 2.5), (2, 3.5)):
            if w > 2 * ring + 1:
                dx[:, ring], dx[:, w - 1 - ring] = -d, d
            if h > 2 * ring + 1:
                dy[ring, :], dy[h - 1 - ring, :] = -d, d
        for i in range(n):
            jit = 0.01 * rng.standard_normal((2, h, w))
            fwd[i, 0], fwd[i, 1] = dx / tf + jit[0], dy / tf + jit[1]
            bwd[i, 0], bwd[i, 1] = dx / tb + jit[1], dy / tb + jit[0]
    elif kind == "holes":
        # both sides move away from the middle column / row: a band in the middle is reached by nothing
        sx = np.where(xs >= w / 2, 1.0, -1.0) * (0.0 if w == 1 else 3.0)
        sy = np.where(ys >= h / 2, 1.0, -1.0) * (0.0 if h == 1 else 2.0)
        for i in range(n):
            fwd[i, 0], fwd[i, 1] = sx / tf + 0.1 * rng.standard_normal((h, w)), sy / tf
            bwd[i, 0], bwd[i, 1] = sx / tb, sy / tb + 0.1 * rng.standard_normal((h, w))
    elif kind == "dyadic":
        fwd[:] = rng.integers(-48, 49, size=fwd.shape) / 16.0
        bwd[:] = rng.integers(-48, 49, size=bwd.shape) / 16.0
    else:
        raise ValueError(kind)
    return a, b, fwd, bwd


def build(case, with_cls=False):
    """(a, b, fwd, bwd, num, den, cls or None) of an entry of CASES / DYADIC; the class maps are the consistency restatement's."""
    name, kind, n, h, w, num, den = case
    a, b, fwd, bwd = make(kind, _seed(name), n, h, w, num, den)
    cls = (cc.restate32(fwd, bwd)[0], cc.restate32(bwd, fwd)[0]) if with_cls else None
    return a, b, fwd, bwd, num, den, cls


def _importance(cls, codes, imp, shape):
    if cls is None:
        return np.full(shape, imp[0], np.uint64)
    return np.where(cls == codes[0], imp[0], np.where(cls == codes[1], imp[1], imp[2])).astype(np.uint64)


def _axis32(p, ok):
    """floor, fraction and the two 1/64 weights of one coordinate, float32 step by step (0 where not ok)."""
    ps = np.where(ok, p, f32(0))
    f0 = np.floor(ps)
    fr = ps - f0
    w1 = np.floor(fr * f32(64) + f32(0.5)).astype(np.int64)
    return f0.astype(np.int64), 64 - w1, w1


def splat32(img, flow, ts, imp_map):
    """One side's accumulators (W uint64 [n, h, w], C uint64 [n, h, w, 3]): float32 coordinates, integer weights, np.add.at."""
    n, _, h, w = flow.shape
    ts = f32(ts)
    with np.errstate(all="ignore"):
        px = np.arange(w, dtype=f32)[None, None, :] + ts * flow[:, 0]
        py = np.arange(h, dtype=f32)[None, :, None] + ts * flow[:, 1]
        ok = (px > f32(-1)) & (px < f32(w)) & (py > f32(-1)) & (py < f32(h))
        x0, wx0, wx1 = _axis32(px, ok)
        y0, wy0, wy1 = _axis32(py, ok)
    W = np.zeros(n * h * w, np.uint64)
    C = np.zeros((n * h * w, 3), np.uint64)
    pair = np.broadcast_to(np.arange(n)[:, None, None], ok.shape)
    for ty, wy in ((0, wy0), (1, wy1)):
        for tx, wx in ((0, wx0), (1, wx1)):
            xi, yi, wt = x0 + tx, y0 + ty, wx * wy
            m = ok & (wt > 0) & (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            idx = (pair[m] * h + yi[m]) * w + xi[m]
            wi = wt[m].astype(np.uint64) * imp_map[m]
            np.add.at(W, idx, wi)
            np.add.at(C, idx, wi[:, None] * img[m].astype(np.uint64))
    return W.reshape(n, h, w), C.reshape(n, h, w, 3)


def ts_pair(num, den):
    """(tf, tb): the two scale factors as the host computes them in float32."""
    return f32(num) / f32(den), f32(den - num) / f32(den)


def restate(a, b, fwd, bwd, num, den, cls=None, codes=(0, 1), imp=(16, 1, 16)):
    """(out uint8 [n, h, w, 3], cover uint8 [n, h, w], stats float64 [n, LEN]) of sf_frame_interp."""
    fwd, bwd = np.asarray(fwd, f32), np.asarray(bwd, f32)
    n, _, h, w = fwd.shape
    tf, tb = ts_pair(num, den)
    WA, CA = splat32(a, fwd, tf, _importance(None if cls is None else cls[0], codes, imp, (n, h, w)))
    WB, CB = splat32(b, bwd, tb, _importance(None if cls is None else cls[1], codes, imp, (n, h, w)))
    one, two = np.uint64(1), np.uint64(2)

    def mean(W, C):
        Ws = np.where(W > 0, W, one)[..., None]
        return (two * C + Ws) // (two * Ws)

    ha, hb = WA > 0, WB > 0
    hole = ~ha & ~hb
    fade = (a.astype(np.uint64) * np.uint64(den - num) + b.astype(np.uint64) * np.uint64(num) + np.uint64(den // 2)) // np.uint64(den)
    # both sides: one rounding of ((den - num) CA / WA + num CB / WB) / den; the products pass 64 bits, so Python ints (object arrays)
    wa, wb = np.where(ha & hb, WA, one).astype(object)[..., None], np.where(ha & hb, WB, one).astype(object)[..., None]
    N = (den - num) * CA.astype(object) * wb + num * CB.astype(object) * wa
    D = den * wa * wb
    both = ((2 * N + D) // (2 * D)).astype(np.uint64)
    out = np.where(hole[..., None], fade, np.where((ha & ~hb)[..., None], mean(WA, CA), np.where((hb & ~ha)[..., None], mean(WB, CB), both)))
    assert out.max() <= 255
    cover = np.where(ha, np.where(hb, 0, 1), np.where(hb, 2, 3)).astype(np.uint8)
    stats = np.zeros((n, LEN), np.float64)
    for i in range(n):
        stats[i] = [h * w] + [(cover[i] == k).sum() for k in range(4)]
    return out.astype(np.uint8), cover, stats


def restate_scalar(a, b, fwd, bwd, num, den, cls=None, codes=(0, 1), imp=(16, 1, 16)):
    """The same contract pixel by pixel: np.float32 scalars for the coordinates, Python ints for everything after them."""
    n, _, h, w = fwd.shape
    tf, tb = ts_pair(num, den)
    out = np.zeros((n, h, w, 3), np.uint8)
    cover = np.zeros((n, h, w), np.uint8)
    stats = np.zeros((n, LEN), np.float64)
    half, sixty4, minus1 = f32(0.5), f32(64), f32(-1)
    for i in range(n):
        acc = [[[0, 0, 0, 0] for _ in range(h * w)] for _ in range(2)]
        for sd, (img, flow, ts, c) in enumerate(((a, fwd, tf, None if cls is None else cls[0]),
                                                 (b, bwd, tb, None if cls is None else cls[1]))):
            for y in range(h):
                for x in range(w):
                    with np.errstate(all="ignore"):
                        px = f32(x) + f32(ts * f32(flow[i, 0, y, x]))
                        py = f32(y) + f32(ts * f32(flow[i, 1, y, x]))
                    if not (px > minus1 and px < f32(w) and py > minus1 and py < f32(h)):
                        continue
                    fx0, fy0 = np.floor(px), np.floor(py)
                    wx1 = int(np.floor(f32(f32(px - fx0) * sixty4) + half))
                    wy1 = int(np.floor(f32(f32(py - fy0) * sixty4) + half))
                    wx, wy = (64 - wx1, wx1), (64 - wy1, wy1)
                    weight = imp[0]
                    if c is not None:
                        k = int(c[i, y, x])
                        weight = imp[0] if k == codes[0] else (imp[1] if k == codes[1] else imp[2])
                    for ty in (0, 1):
                        for tx in (0, 1):
                            xi, yi, wt = int(fx0) + tx, int(fy0) + ty, wx[tx] * wy[ty]
                            if wt == 0 or not (0 <= xi < w and 0 <= yi < h):
                                continue
                            t = acc[sd][yi * w + xi]
                            t[0] += wt * weight
                            for ch in range(3):
                                t[1 + ch] += wt * weight * int(img[i, y, x, ch])
        counts = [0, 0, 0, 0]
        for y in range(h):
            for x in range(w):
                ta, tb_ = acc[0][y * w + x], acc[1][y * w + x]
                code = (0 if tb_[0] else 1) if ta[0] else (2 if tb_[0] else 3)
                for ch in range(3):
                    if code == 3:
                        val = (int(a[i, y, x, ch]) * (den - num) + int(b[i, y, x, ch]) * num + den // 2) // den
                    elif code == 1:
                        val = (2 * ta[1 + ch] + ta[0]) // (2 * ta[0])
                    elif code == 2:
                        val = (2 * tb_[1 + ch] + tb_[0]) // (2 * tb_[0])
                    else:
                        nn = (den - num) * ta[1 + ch] * tb_[0] + num * tb_[1 + ch] * ta[0]
                        dd = den * ta[0] * tb_[0]
                        val = (2 * nn + dd) // (2 * dd)
                    out[i, y, x, ch] = val
                cover[i, y, x] = code
                counts[code] += 1
        stats[i] = [h * w] + counts
    return out, cover, stats


def ideal64(a, b, fwd, bwd, num, den, cls=None, codes=(0, 1), imp=(16, 1, 16)):
    """Float64, unquantised bilinear weights, real division, nothing rounded: (value float64 [n, h, w, 3], the two sides' means
    float64 [n, h, w, 3] (NaN where a side is absent), cover)."""
    n, _, h, w = fwd.shape
    t = num / den

    def side(img, flow, ts, c):
        flow = np.asarray(flow, np.float64)
        with np.errstate(all="ignore"):
            px = np.arange(w, dtype=np.float64)[None, None, :] + ts * flow[:, 0]
            py = np.arange(h, dtype=np.float64)[None, :, None] + ts * flow[:, 1]
            ok = (px > -1) & (px < w) & (py > -1) & (py < h)
        px, py = np.where(ok, px, 0.0), np.where(ok, py, 0.0)
        x0, y0 = np.floor(px), np.floor(py)
        fx, fy = px - x0, py - y0
        x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
        W = np.zeros(n * h * w)
        C = np.zeros((n * h * w, 3))
        pair = np.broadcast_to(np.arange(n)[:, None, None], ok.shape)
        weight = _importance(c, codes, imp, (n, h, w)).astype(np.float64)
        for ty, wy in ((0, 1 - fy), (1, fy)):
            for tx, wx in ((0, 1 - fx), (1, fx)):
                xi, yi, wt = x0 + tx, y0 + ty, wx * wy
                m = ok & (wt > 0) & (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
                idx = (pair[m] * h + yi[m]) * w + xi[m]
                np.add.at(W, idx, wt[m] * weight[m])
                np.add.at(C, idx, (wt[m] * weight[m])[:, None] * img[m].astype(np.float64))
        W = W.reshape(n, h, w)
        with np.errstate(all="ignore"):
            return W > 0, C.reshape(n, h, w, 3) / W[..., None]

    ha, ma = side(a, fwd, t, None if cls is None else cls[0])
    hb, mb = side(b, bwd, 1 - t, None if cls is None else cls[1])
    hole = ~ha & ~hb
    ca = np.where(hole[..., None], a.astype(np.float64), ma)
    cb = np.where(hole[..., None], b.astype(np.float64), mb)
    with np.errstate(all="ignore"):
        both = (1 - t) * ca + t * cb
    value = np.where((ha & ~hb)[..., None], ca, np.where((hb & ~ha)[..., None], cb, both))
    cover = np.where(ha, np.where(hb, 0, 1), np.where(hb, 2, 3)).astype(np.uint8)
    return value, np.where(ha[..., None], ma, np.nan), np.where(hb[..., None], mb, np.nan), cover
