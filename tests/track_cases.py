"""Point tracking restated in numpy float32, operation by operation as include/streamflow_track.h states it, for the tests of
sft_track_advance / sft_draw_tracks to compare against BITWISE; and the makers of their cases.

advance32 is vectorised over the points, advance_scalar walks one point at a time with numpy float32 scalars; draw32 stamps with
array operations, draw_scalar pixel by pixel.  tests/test_track_cases_cpu.py holds each pair to each other; the GPU tests use
advance32 / draw32 alone.  Every float32 operation is written as one numpy operation, so nothing is fused."""
import numpy as np

VISIBLE, OCCLUDED, LOST, PENDING = 0, 1, 2, 3
ALPHA, BETA = 0.01, 0.5
MAX_SEG = 64
F32 = np.float32


def inside(x, y, h, w):
    with np.errstate(invalid="ignore"):
        return (x >= F32(0)) & (x <= F32(w - 1)) & (y >= F32(0)) & (y <= F32(h - 1))


def sample(field, px, py, h, w):
    """field float32 [2, h, w] (any strides), px / py float32 [n] INSIDE positions -> (su, sv) float32 [n]."""
    with np.errstate(all="ignore"):
        fx0, fy0 = np.floor(px), np.floor(py)
        fx, fy = px - fx0, py - fy0
        x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        gx, gy = F32(1) - fx, F32(1) - fy
        out = []
        for c in range(2):
            a = field[c]
            top = gx * a[y0, x0] + fx * a[y0, x1]
            bot = gx * a[y1, x0] + fx * a[y1, x1]
            out.append(gy * top + fy * bot)
    return out[0], out[1]


def initial_state(queries, h, w):
    """([2, P] float32, [P] uint8 all PENDING, start int32 [P]) from rows (t, x, y)."""
    q = np.asarray(queries, F32)
    return np.ascontiguousarray(q[:, 1:].T), np.full(q.shape[0], PENDING, np.uint8), q[:, 0].astype(np.int32)


def grid_state(h, w):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.ravel(), ys.ravel()]).astype(F32), np.full(h * w, PENDING, np.uint8)


def advance32(fwd, bwd=None, state_xy=None, state_status=None, start=None, frame0=0, alpha=ALPHA, beta=BETA, sticky=False):
    """-> (xy float32 [K, 2, P], status uint8 [K, P], counts uint32 [K, 4]).  state_xy None: dense mode."""
    K, _, h, w = fwd.shape
    alpha, beta = F32(alpha), F32(beta)
    if state_xy is None:
        x, y = grid_state(h, w)[0]
        st = np.full(h * w, VISIBLE, np.uint8)
        start = None
    else:
        x, y = state_xy[0].astype(F32).copy(), state_xy[1].astype(F32).copy()
        st = np.where(state_status > PENDING, LOST, state_status).astype(np.uint8)
    P = x.size
    start = np.full(P, -2 ** 31, np.int64) if start is None else start.astype(np.int64)

    def activate(m):
        st[m] = np.where(inside(x[m], y[m], h, w), VISIBLE, LOST)

    if state_xy is not None:
        activate((st == PENDING) & (start <= frame0))
    xy, status, counts = np.empty((K, 2, P), F32), np.empty((K, P), np.uint8), np.zeros((K, 4), np.uint32)
    with np.errstate(all="ignore"):
        for k in range(K):
            f = frame0 + k + 1
            pend = st == PENDING
            active = st <= OCCLUDED
            activate(pend & (start <= f))
            bad = active & ~inside(x, y, h, w)
            st[bad] = LOST
            idx = np.flatnonzero(active & ~bad)
            if idx.size:
                px, py = x[idx], y[idx]
                u, v = sample(fwd[k], px, py, h, w)
                qx, qy = px + u, py + v
                ok = inside(qx, qy, h, w)
                st[idx[~ok]] = LOST
                idx, u, v, qx, qy = idx[ok], u[ok], v[ok], qx[ok], qy[ok]
                x[idx], y[idx] = qx, qy
                if bwd is None:
                    st[idx] = VISIBLE
                elif idx.size:
                    su, sv = sample(bwd[k], qx, qy, h, w)
                    m2 = u * u + v * v
                    dx, dy = u + su, v + sv
                    lhs = dx * dx + dy * dy
                    rhs = alpha * (m2 + (su * su + sv * sv)) + beta
                    vis = lhs <= rhs
                    if sticky:
                        vis &= st[idx] != OCCLUDED
                    st[idx] = np.where(vis, VISIBLE, OCCLUDED)
            xy[k, 0], xy[k, 1], status[k] = x, y, st
            counts[k] = np.bincount(st, minlength=4)[:4]
    return xy, status, counts


def _sample1(field, px, py, h, w):
    fx0, fy0 = np.floor(px), np.floor(py)
    fx, fy = F32(px - fx0), F32(py - fy0)
    x0, y0 = int(fx0), int(fy0)
    x1, y1 = min(x0 + 1, w - 1), min(y0 + 1, h - 1)
    gx, gy = F32(F32(1) - fx), F32(F32(1) - fy)
    out = []
    for c in range(2):
        a = field[c]
        top = F32(F32(gx * a[y0, x0]) + F32(fx * a[y0, x1]))
        bot = F32(F32(gx * a[y1, x0]) + F32(fx * a[y1, x1]))
        out.append(F32(F32(gy * top) + F32(fy * bot)))
    return out


def _inside1(x, y, h, w):
    return bool(x >= F32(0) and x <= F32(w - 1) and y >= F32(0) and y <= F32(h - 1))


def advance_scalar(fwd, bwd=None, state_xy=None, state_status=None, start=None, frame0=0, alpha=ALPHA, beta=BETA, sticky=False):
    """advance32's results, one point at a time (the loop of the kernel's thread)."""
    K, _, h, w = fwd.shape
    alpha, beta = F32(alpha), F32(beta)
    P = h * w if state_xy is None else state_xy.shape[1]
    xy, status = np.empty((K, 2, P), F32), np.empty((K, P), np.uint8)
    with np.errstate(all="ignore"):
        for i in range(P):
            if state_xy is None:
                x, y, st, s0 = F32(i % w), F32(i // w), VISIBLE, -2 ** 31
            else:
                x, y, st = F32(state_xy[0, i]), F32(state_xy[1, i]), int(state_status[i])
                st = LOST if st > PENDING else st
                s0 = -2 ** 31 if start is None else int(start[i])
                if st == PENDING and s0 <= frame0:
                    st = VISIBLE if _inside1(x, y, h, w) else LOST
            for k in range(K):
                f = frame0 + k + 1
                if st == PENDING:
                    if s0 <= f:
                        st = VISIBLE if _inside1(x, y, h, w) else LOST
                elif st <= OCCLUDED:
                    if not _inside1(x, y, h, w):
                        st = LOST
                    else:
                        u, v = _sample1(fwd[k], x, y, h, w)
                        qx, qy = F32(x + u), F32(y + v)
                        if not _inside1(qx, qy, h, w):
                            st = LOST
                        else:
                            x, y = qx, qy
                            if bwd is None:
                                st = VISIBLE
                            else:
                                su, sv = _sample1(bwd[k], qx, qy, h, w)
                                m2 = F32(F32(u * u) + F32(v * v))
                                dx, dy = F32(u + su), F32(v + sv)
                                lhs = F32(F32(dx * dx) + F32(dy * dy))
                                rhs = F32(F32(alpha * F32(m2 + F32(F32(su * su) + F32(sv * sv)))) + beta)
                                vis = bool(lhs <= rhs) and not (sticky and st == OCCLUDED)
                                st = VISIBLE if vis else OCCLUDED
                xy[k, 0, i], xy[k, 1, i], status[k, i] = x, y, st
    counts = np.stack([np.bincount(status[k], minlength=4)[:4] for k in range(K)]).astype(np.uint32)
    return xy, status, counts


# ---- drawing ------------------------------------------------------------------------------------------------------------------------

def drawable(x, y, st, draw_occluded, h, w):
    return bool((st == VISIBLE or (draw_occluded and st == OCCLUDED)) and _inside1(F32(x), F32(y), h, w))


def line_points(cx, cy, nx, ny):
    """The integer line from (cx, cy) to (nx, ny), points s = 1 .. n; [] when n is 0 or above MAX_SEG."""
    dx, dy = nx - cx, ny - cy
    n = max(abs(dx), abs(dy))
    if n < 1 or n > MAX_SEG:
        return []
    sg = lambda d: -1 if d < 0 else 1
    return [(cx + sg(dx) * ((abs(dx) * 2 * s + n) // (2 * n)), cy + sg(dy) * ((abs(dy) * 2 * s + n) // (2 * n))) for s in range(1, n + 1)]


def _centres(j, p, age, first_frame, xy, status, first_row, radius, trail_radius, draw_occluded, h, w):
    """[(cx, cy, r)] discs the sample of age `age` of frame j stamps."""
    N = xy.shape[0]
    r = first_frame + j - age - first_row
    if r < 0 or r >= N or not drawable(xy[r, 0, p], xy[r, 1, p], status[r, p], draw_occluded, h, w):
        return []
    cx, cy = int(np.rint(xy[r, 0, p])), int(np.rint(xy[r, 1, p]))
    if age == 0:
        return [(cx, cy, radius)]
    out = [(cx, cy, trail_radius)]
    if r + 1 < N and drawable(xy[r + 1, 0, p], xy[r + 1, 1, p], status[r + 1, p], draw_occluded, h, w):
        out += [(x, y, trail_radius) for x, y in line_points(cx, cy, int(np.rint(xy[r + 1, 0, p])), int(np.rint(xy[r + 1, 1, p])))]
    return out


def _resolve(frames, keys, trail, palette, alpha_table):
    out = frames.copy()
    hit = keys != 0
    age = trail - (keys >> 20).astype(np.int64)
    point = (keys & 0xFFFFF).astype(np.int64) - 1
    col = palette[point[hit] % palette.shape[0]].astype(np.int64)
    al = alpha_table[age[hit]].astype(np.int64)[:, None]
    out[hit] = ((col * al + frames[hit].astype(np.int64) * (255 - al) + 127) // 255).astype(np.uint8)
    return out


def draw32(frames, first_frame, xy, status, first_row, trail, radius, trail_radius, palette, alpha_table, draw_occluded=False):
    """frames uint8 [n, h, w, 3] -> uint8 [n, h, w, 3] as sft_draw_tracks draws them; discs stamped as arrays."""
    n, h, w, _ = frames.shape
    P = xy.shape[2]
    keys = np.zeros((n, h, w), np.uint32)
    for j in range(n):
        for p in range(P):
            for age in range(trail):
                key = np.uint32(((trail - age) << 20) | (p + 1))
                for cx, cy, r in _centres(j, p, age, first_frame, xy, status, first_row, radius, trail_radius, draw_occluded, h, w):
                    dy, dx = np.mgrid[-r:r + 1, -r:r + 1]
                    m = dx * dx + dy * dy <= r * r
                    xs, ys = cx + dx[m], cy + dy[m]
                    ok = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
                    np.maximum.at(keys[j], (ys[ok], xs[ok]), key)
    return _resolve(frames, keys, trail, palette, alpha_table)


def draw_scalar(frames, first_frame, xy, status, first_row, trail, radius, trail_radius, palette, alpha_table, draw_occluded=False):
    """draw32's bytes, pixel by pixel."""
    n, h, w, _ = frames.shape
    P = xy.shape[2]
    out = frames.copy()
    for j in range(n):
        keys = [[0] * w for _ in range(h)]
        for p in range(P):
            for age in range(trail):
                key = ((trail - age) << 20) | (p + 1)
                for cx, cy, r in _centres(j, p, age, first_frame, xy, status, first_row, radius, trail_radius, draw_occluded, h, w):
                    for dy in range(-r, r + 1):
                        for dx in range(-r, r + 1):
                            x, y = cx + dx, cy + dy
                            if dx * dx + dy * dy <= r * r and 0 <= x < w and 0 <= y < h and key > keys[y][x]:
                                keys[y][x] = key
        for y in range(h):
            for x in range(w):
                key = keys[y][x]
                if key:
                    age, p = trail - (key >> 20), (key & 0xFFFFF) - 1
                    for c in range(3):
                        out[j, y, x, c] = (int(palette[p % len(palette), c]) * int(alpha_table[age]) +
                                           int(frames[j, y, x, c]) * (255 - int(alpha_table[age])) + 127) // 255
    return out


# ---- cases --------------------------------------------------------------------------------------------------------------------------

def smooth_flows(seed, K, h, w, amp=2.0):
    """float32 [K, 2, h, w]: a few sinusoids per plane, about `amp` pixels."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((K, 2, h, w))
    for k in range(K):
        for c in range(2):
            for _ in range(3):
                fx, fy, ph = rng.uniform(0.02, 0.4), rng.uniform(0.02, 0.4), rng.uniform(0, 6.28)
                out[k, c] += rng.uniform(0.2, 1.0) * np.sin(fx * xs + fy * ys + ph)
    return (out * (amp / 1.6)).astype(F32)


def random_queries(seed, P, h, w, n_frames=1):
    """float32 [P, 3]: positions anywhere in the frame (corners and borders among them), start frames in 0 .. n_frames - 1."""
    rng = np.random.default_rng(seed)
    q = np.empty((P, 3), F32)
    q[:, 0] = rng.integers(0, n_frames, P)
    q[:, 1] = rng.uniform(0, w - 1, P) if w > 1 else 0
    q[:, 2] = rng.uniform(0, h - 1, P) if h > 1 else 0
    fixed = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w - 1, (h - 1) / 2), ((w - 1) / 2, h - 1)]   # exactly on x = w - 1 / y = h - 1
    for i, (x, y) in enumerate(fixed[:P]):
        q[i, 1:] = x, y
    return q


SPECIALS = (np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0)


def special_case(seed, K, h, w, P):
    """Smooth flows with NaN, +-Inf, 1e30 and -0.0 scattered in both directions, flows that land a point exactly on the border and
    one ulp beyond it, and queries that hold the same special values: -> (fwd, bwd, queries [P, 3], all starting at frame 0)."""
    rng = np.random.default_rng(seed)
    fwd, bwd = smooth_flows(seed, K, h, w), -smooth_flows(seed + 1, K, h, w)
    for f in (fwd, bwd):
        n = max(1, f.size // 60)
        f.reshape(-1)[rng.integers(0, f.size, n)] = rng.choice(np.array(SPECIALS, F32), n)
    q = random_queries(seed + 2, P, h, w)
    # integer positions read their tap exactly: pixel (0, y) moves to x = w - 1 exactly, pixel (0, y') one ulp beyond
    edge = F32(w - 1)
    if w > 1:
        fwd[0, 0, 0, 0], fwd[0, 1, 0, 0] = edge, 0.0
        if P > 6:
            q[6, 1:] = 0, 0
        if h > 1 and P > 7:
            fwd[0, 0, h - 1, 0], fwd[0, 1, h - 1, 0] = np.nextafter(edge, F32(np.inf)), 0.0
            q[7, 1:] = 0, h - 1
    for i, v in enumerate(SPECIALS):
        if P > 8 + i:
            q[8 + i, 1 + i % 2] = v
    return fwd, bwd, q


def strided(fields, rng_seed=0, row_pad=3, ch_pad=2, field_pad=5, fill=np.nan):
    """A view of a larger float32 buffer that holds `fields` [K, 2, h, w] with row, channel and field strides larger than dense (the
    gaps hold `fill`): -> (buffer 1-d, view)."""
    K, _, h, w = fields.shape
    row = w + row_pad
    ch = h * row + ch_pad
    fs = 2 * ch + field_pad
    buf = np.full(K * fs + 8, fill, F32)
    view = np.lib.stride_tricks.as_strided(buf[4:], (K, 2, h, w), (4 * fs, 4 * ch, 4 * row, 4))
    view[...] = fields
    return buf, view


def draw_case(seed, n_rows, P, h, w):
    """Track rows for drawing: points of every status, discs and lines that cross the frame edge, one segment longer than MAX_SEG."""
    rng = np.random.default_rng(seed)
    xy = np.empty((n_rows, 2, P), F32)
    xy[0, 0], xy[0, 1] = rng.uniform(0, w - 1, P), rng.uniform(0, h - 1, P)
    for r in range(1, n_rows):
        xy[r] = xy[r - 1] + rng.uniform(-6, 6, (2, P)).astype(F32)
    xy[:, 0] = np.clip(xy[:, 0], 0, w - 1)
    xy[:, 1] = np.clip(xy[:, 1], 0, h - 1)
    status = rng.choice(np.array([VISIBLE, VISIBLE, VISIBLE, OCCLUDED, LOST, PENDING], np.uint8), (n_rows, P))
    status[:, 0] = VISIBLE
    xy[:, 0, 0] = np.where(np.arange(n_rows) % 2 == 0, 0.0, w - 1.0)         # point 0 jumps across the frame: too long when w > 65
    xy[:, 1, 0] = h - 1                                                      # ... along the bottom edge (discs clipped)
    if P > 1:
        status[:, 1] = VISIBLE
        xy[:, 0, 1], xy[:, 1, 1] = np.linspace(0, min(w - 1, 40), n_rows), 0.5   # a tie for rintf, on the top edge
    if P > 2:
        xy[0, 0, 2] = np.nan                                                 # never drawable, whatever its status says
        status[0, 2] = VISIBLE
    return xy, status


def small_palette(L=7):
    return (np.arange(L * 3).reshape(L, 3) * 37 % 256).astype(np.uint8)


def write_host_cases(path, cases):
    """The case file of csrc/host/track_host_main.cpp: int32 count, then per case eight int32 (K, h, w, frame0, P, has_bwd, has_start,
    sticky), two float32 (alpha, beta), fwd [K, 2, h, w], bwd when has_bwd, state xy [2, P], state status [P], start [P] when has_start."""
    import struct
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            K, _, h, w = c["fwd"].shape
            P = c["xy"].shape[1]
            f.write(struct.pack("<8i2f", K, h, w, c.get("frame0", 0), P, int(c.get("bwd") is not None), int(c.get("start") is not None),
                                int(c.get("sticky", False)), c.get("alpha", ALPHA), c.get("beta", BETA)))
            f.write(np.ascontiguousarray(c["fwd"], F32).tobytes())
            if c.get("bwd") is not None:
                f.write(np.ascontiguousarray(c["bwd"], F32).tobytes())
            f.write(np.ascontiguousarray(c["xy"], F32).tobytes() + np.ascontiguousarray(c["status"], np.uint8).tobytes())
            if c.get("start") is not None:
                f.write(np.ascontiguousarray(c["start"], np.int32).tobytes())


def read_host_rows(path, cases):
    data, p, out = open(path, "rb").read(), 0, []
    for c in cases:
        K, P = c["fwd"].shape[0], c["xy"].shape[1]
        xy = np.frombuffer(data, F32, K * 2 * P, p).reshape(K, 2, P)
        p += 8 * K * P
        st = np.frombuffer(data, np.uint8, K * P, p).reshape(K, P)
        p += K * P
        out.append((xy, st))
    assert p == len(data)
    return out
