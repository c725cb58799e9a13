"""Seeded cases of the flow-colouring fixture (tests/golden/make_viz_golden.py -> flow_viz.npz), the numpy restatement of the
colour-wheel arithmetic that checks the sf_flow_to_image kernel, and the image criterion, shared by the generator and the tests.

The restatement follows include/streamflow_hip.h (sf_flow_to_image) operation for operation; it is this repository's own code.
Its one deliberate difference from the reference's numpy code is the angle: the fp64 arctangent rounded once to fp32 instead of
the platform's float32 ``arctan2`` (not correctly rounded, differs between libms)."""
import numpy as np

# name -> (H, W); inputs come from field(name), the keyword arguments of the reference call from KWARGS
CASES = {"gauss": (64, 96), "gauss_bgr": (64, 96), "gauss_clip3": (64, 96), "ramp": (55, 128), "px1": (1, 1), "px3x5": (3, 5),
         "px37x61": (37, 61), "big1e4": (32, 48), "zero": (16, 24)}
KWARGS = {"gauss_bgr": {"convert_to_bgr": True}, "gauss_clip3": {"clip_flow": 3.0}}
RAMP_ZERO_ROWS = ((24, 27, -0.0), (27, 31, 0.0))       # rows [a, b) of the ramp with v = -0.0 / +0.0
RAMP_U0_COL = 64


def field(name):
    """float32 [H, W, 2] (the reference's layout) of case `name`."""
    H, W = CASES[name]
    if name.startswith("gauss"):
        return (np.random.default_rng(11).normal(0, 1, (H, W, 2)) * 5).astype(np.float32)
    if name == "ramp":
        u = np.broadcast_to((np.arange(W, dtype=np.float32) - RAMP_U0_COL) * np.float32(0.8), (H, W))
        v = np.broadcast_to(((np.arange(H, dtype=np.float32) - 27) * np.float32(1.5))[:, None], (H, W)).copy()
        for a, b, z in RAMP_ZERO_ROWS:
            v[a:b] = z
        return np.stack([u, v], axis=2).astype(np.float32)
    if name == "zero":
        return np.zeros((H, W, 2), np.float32)
    scale = 1e4 if name == "big1e4" else 5.0
    return (np.random.default_rng(H * 1000 + W).normal(0, 1, (H, W, 2)) * scale).astype(np.float32)


def gaussian_fields(n, H, W, scales, seed):
    """float32 [n, 2, H, W] (the kernel's layout): field i is N(0, 1) * scales[i], smoothed a little along x so that neighbouring
    pixels share wheel segments as real flow does."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, 2, H, W), np.float32)
    for i in range(n):
        g = rng.normal(0, 1, (2, H, W + 2)).astype(np.float32)
        out[i] = (g[:, :, :-2] + g[:, :, 1:-1] + g[:, :, 2:]) * np.float32(scales[i] / 3)
    return out


def make_colorwheel():
    """[55, 3] float64: six linear segments between the pure hues R, Y, G, C, B, M (15, 6, 4, 11, 13 and 6 steps), each step
    floor(255 i / n) up or down.  Written from the description in Baker et al. (ICCV 2007); pinned by the fixture."""
    wheel = []
    # (steps, channel that moves, +1 rising / -1 falling); the two other channels keep the value they have at the segment start
    state = [255.0, 0.0, 0.0]
    for steps, ch, sign in ((15, 1, 1), (6, 0, -1), (4, 2, 1), (11, 1, -1), (13, 0, 1), (6, 2, -1)):
        for i in range(steps):
            ramp = float(np.floor(255 * i / steps))
            row = list(state)
            row[ch] = ramp if sign > 0 else 255.0 - ramp
            wheel.append(row)
        state[ch] = 255.0 if sign > 0 else 0.0
    return np.array(wheel, np.float64)


def radii(flow_hw2, clip_flow=None):
    """fp32 radii [H, W] after the optional clamp, and the mask of pixels with two finite components."""
    flow = np.asarray(flow_hw2, np.float32)
    finite = np.isfinite(flow).all(axis=2)
    flow = np.where(finite[:, :, None], flow, np.float32(0))
    if clip_flow is not None:
        flow = np.where(flow < 0, np.float32(0), flow)                        # by comparison, as np.clip: -0.0 stays -0.0
        flow = np.where(flow > np.float32(clip_flow), np.float32(clip_flow), flow)
    u, v = flow[:, :, 0], flow[:, :, 1]
    return np.sqrt(u * u + v * v), finite, u, v


def rad_max_np(flow_hw2, clip_flow=None):
    rad, finite, _, _ = radii(flow_hw2, clip_flow)
    return np.float32(np.max(np.where(finite, rad, np.float32(0))))


def flow_to_image_np(flow_hw2, clip_flow=None, convert_to_bgr=False, rad_max=None):
    """uint8 [H, W, 3] of a float32 [H, W, 2] field, by the arithmetic contract of sf_flow_to_image."""
    f32, f64 = np.float32, np.float64
    rad, finite, u, v = radii(flow_hw2, clip_flow)
    m = f32(rad_max) if rad_max is not None else f32(np.max(np.where(finite, rad, f32(0))))
    d = f32(m + f32(1e-5))
    un, vn = (u / d).astype(f32), (v / d).astype(f32)
    radn = np.sqrt(un * un + vn * vn).astype(f32)
    angle = np.arctan2(-vn.astype(f64), -un.astype(f64)).astype(f32)          # -x keeps the sign of zero
    a = (angle / f32(np.pi)).astype(f32)
    fk = (((a + f32(1)) / f32(2)) * f32(54)).astype(f32)
    k0 = np.floor(fk).astype(np.int32)
    k1 = np.where(k0 + 1 == 55, 0, k0 + 1)
    f = fk.astype(f64) - k0                      # fp64 from here: numpy's float32 - int32 is float64 (the difference is exact)
    wheel = make_colorwheel()
    img = np.zeros(rad.shape + (3,), np.uint8)
    for c in range(3):
        c0, c1 = wheel[k0, c] / 255.0, wheel[k1, c] / 255.0
        col = (1.0 - f) * c0 + f * c1
        col = np.where(radn <= f32(1), 1.0 - radn.astype(f64) * (1.0 - col), col * 0.75)
        img[:, :, 2 - c if convert_to_bgr else c] = np.where(finite, np.floor(255.0 * col), 0.0).astype(np.uint8)
    return img


def image_mismatch(got, ref):
    """(largest |difference| in levels, number of pixels that differ at all, number of pixels allowed to differ)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.uint8, (got.shape, got.dtype, ref.shape, ref.dtype)
    diff = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    npx = diff.size // 3
    allowed = 1 if npx < 10000 else int(npx * 1e-4)
    return int(diff.max()) if diff.size else 0, int((diff.reshape(-1, 3).max(axis=1) > 0).sum()), allowed


def assert_image_close(got, ref, what=""):
    """The image criterion: at most one level on every channel, and at most 1e-4 of the pixels differ at all (one pixel for
    images under 10 000 pixels).  Prints the figures before it asserts."""
    worst, n, allowed = image_mismatch(got, ref)
    print(f"{what}: max |diff| {worst} level(s), {n} of {np.asarray(ref).size // 3} pixels differ (allowed {allowed})")
    assert worst <= 1 and n <= allowed, (what, worst, n, allowed)
