"""Cases and two independent statements of sf_flow_consistency / sf_warp_frames (include/streamflow_hip.h, "forward-backward
consistency") for tests/test_consistency_cases_cpu.py and tests/test_gpu_flow_consistency.py:

* `make_case`: a seeded generator -- a translation plus small noise as the forward flow, its negative as the backward flow, a band
  of rows of the backward field replaced by a contradicting flow (occluded pixels) and a border strip the translation carries out of
  the frame (outside pixels).  Thin fields (h or w below 8: "degenerate") keep the component along the unit axis at exactly 0.
* `restate32`: the header's expressions operation by operation in numpy float32 (every numpy operation rounds once, as the kernel
  does with contraction off); the kernel must reproduce its classes and bytes BITWISE.
* `formulate64`: an independent float64 formulation through torch.nn.functional.grid_sample(align_corners=True) on the CPU.

This is the project's own code: nothing here is taken from the reference's text."""
import numpy as np
import torch
import torch.nn.functional as F

from streamflow_amd.consistency import ALPHA, BETA                    # the package's constants and row layout: one definition
from streamflow_amd.ops import (FBC_FINITE as FINITE, FBC_LEN as LEN, FBC_OCCLUDED as OCCLUDED, FBC_OUTSIDE as OUTSIDE,
                                FBC_PIXELS as PIXELS, FBC_SUM_FB as SUM_FB, FBC_SUM_MAG as SUM_MAG, FBC_VISIBLE as VISIBLE)

f32 = np.float32


def degenerate(h: int, w: int) -> bool:
    return h < 8 or w < 8


def make_case(seed: int, n: int, h: int, w: int):
    """(fwd, bwd fp32 [n, 2, h, w]; src, ref uint8 [n, h, w, 3]) as numpy arrays."""
    rng = np.random.default_rng(seed)
    fwd = np.zeros((n, 2, h, w), f32)
    bwd = np.zeros((n, 2, h, w), f32)
    for i in range(n):
        sx, sy = (1 if rng.random() < 0.5 else -1), (1 if rng.random() < 0.5 else -1)
        tx = 0.0 if w == 1 else sx * max(1.0, 0.18 * w) * (0.8 + 0.4 * rng.random())
        ty = 0.0 if h == 1 else sy * max(1.0, 0.12 * h) * (0.8 + 0.4 * rng.random())
        fwd[i, 0] = 0.0 if w == 1 else tx + 0.2 * rng.standard_normal((h, w))
        fwd[i, 1] = 0.0 if h == 1 else ty + 0.2 * rng.standard_normal((h, w))
        bwd[i, 0] = 0.0 if w == 1 else -tx + 0.1 * rng.standard_normal((h, w))
        bwd[i, 1] = 0.0 if h == 1 else -ty + 0.1 * rng.standard_normal((h, w))
        # a band of the backward field that contradicts the forward flow: rows (columns for a one-row field)
        if h > 1:
            lo = h // 4 + int(rng.integers(0, max(1, h // 4)))             # (the translation cannot carry the band out of the frame)
            band = (slice(None), slice(lo, lo + max(2, h // 3)), slice(None))
        else:
            lo = int(rng.integers(0, max(1, w // 2)))
            band = (slice(None), slice(None), slice(lo, lo + max(1, w // 4)))
        bwd[i][band] += f32(4.0 + 3.0 * rng.random()) * (1 if rng.random() < 0.5 else -1)
        if h == 1:
            bwd[i, 1] = 0.0
        if w == 1:
            bwd[i, 0] = 0.0
    src = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    ref = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    return fwd, bwd, src, ref


def _targets32(flow):
    """The coordinate rule in float32: (inside, x0, x1, y0, y1, fx, fy), indices clamped to 0 where not inside."""
    n, _, h, w = flow.shape
    u, v = flow[:, 0], flow[:, 1]
    with np.errstate(all="ignore"):
        px = np.arange(w, dtype=f32)[None, None, :] + u
        py = np.arange(h, dtype=f32)[None, :, None] + v
        inside = (px >= f32(0)) & (px <= f32(w - 1)) & (py >= f32(0)) & (py <= f32(h - 1))
        pxs, pys = np.where(inside, px, f32(0)), np.where(inside, py, f32(0))
        fx0, fy0 = np.floor(pxs), np.floor(pys)
        fx, fy = pxs - fx0, pys - fy0
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    return inside, x0, np.minimum(x0 + 1, w - 1), y0, np.minimum(y0 + 1, h - 1), fx.astype(f32), fy.astype(f32)


def _sample32(plane, tg):
    """plane float32 [n, h, w] sampled at the targets, in the header's order of operations."""
    inside, x0, x1, y0, y1, fx, fy = tg
    i = np.arange(plane.shape[0])[:, None, None]
    with np.errstate(all="ignore"):
        gx, gy = f32(1) - fx, f32(1) - fy
        top = gx * plane[i, y0, x0] + fx * plane[i, y0, x1]
        bot = gx * plane[i, y1, x0] + fx * plane[i, y1, x1]
        return gy * top + fy * bot


def restate32(fwd, bwd, alpha=ALPHA, beta=BETA, codes=(0, 1, 2)):
    """(cls uint8 [n, h, w], stats float64 [n, LEN], lhs, rhs float32) of sf_flow_consistency, float32 operation by operation."""
    fwd, bwd = np.asarray(fwd, f32), np.asarray(bwd, f32)
    tg = _targets32(fwd)
    inside = tg[0]
    u, v = fwd[:, 0], fwd[:, 1]
    with np.errstate(all="ignore"):
        bu, bv = _sample32(bwd[:, 0], tg), _sample32(bwd[:, 1], tg)
        dx, dy = u + bu, v + bv
        lhs = dx * dx + dy * dy
        m2 = u * u + v * v
        rhs = f32(alpha) * (m2 + (bu * bu + bv * bv)) + f32(beta)
        vis = inside & (lhs <= rhs)
        occ = inside & ~(lhs <= rhs)
        mag = np.sqrt(m2)
        fin = mag < f32(np.inf)
        fb = np.sqrt(lhs)
    cls = np.where(vis, codes[0], np.where(occ, codes[1], codes[2])).astype(np.uint8)
    n = fwd.shape[0]
    stats = np.zeros((n, LEN), np.float64)
    for i in range(n):
        stats[i] = [inside[i].size, vis[i].sum(), occ[i].sum(), (~inside[i]).sum(), fb[i][vis[i]].astype(np.float64).sum(),
                    mag[i][fin[i]].astype(np.float64).sum(), fin[i].sum()]
    return cls, stats, lhs, rhs


def warp32(src_hwc, flows, cls=None, ref_hwc=None, visible=0):
    """(warped uint8 [n, h, w, 3], stats float64 [n, 2] or None) of sf_warp_frames, float32 operation by operation."""
    flows = np.asarray(flows, f32)
    tg = _targets32(flows)
    inside = tg[0]
    vals = np.stack([_sample32(src_hwc[..., c].astype(f32), tg) for c in range(3)], axis=-1)
    out = np.where(inside[..., None], np.floor(vals + f32(0.5)), f32(0)).astype(np.uint8)
    if cls is None:
        return out, None
    n = flows.shape[0]
    stats = np.zeros((n, 2), np.float64)
    take = inside & (cls == visible)
    for i in range(n):
        d = np.abs(vals[i][take[i]] - ref_hwc[i][take[i]].astype(f32))
        stats[i] = [d.astype(np.float64).sum(), d.size]
    return out, stats


def formulate64(fwd, bwd, src_hwc, alpha=ALPHA, beta=BETA):
    """The independent formulation: float64, bilinear sampling by grid_sample(align_corners=True, padding_mode="border") on the CPU.
    Returns (inside, lhs, rhs, warped values [n, h, w, 3], border distance): all float64 numpy; `border distance` is how far the
    target is from the nearest frame edge (negative outside), for the tests to leave aside targets the float32 sum can round across
    an edge."""
    f = torch.from_numpy(np.asarray(fwd, np.float64))
    b = torch.from_numpy(np.asarray(bwd, np.float64))
    n, _, h, w = f.shape
    xs = torch.arange(w, dtype=torch.float64)[None, None, :] + f[:, 0]
    ys = torch.arange(h, dtype=torch.float64)[None, :, None] + f[:, 1]
    dist = torch.minimum(torch.minimum(xs, (w - 1) - xs), torch.minimum(ys, (h - 1) - ys))
    inside = dist >= 0
    gx = 2 * xs / (w - 1) - 1 if w > 1 else torch.zeros_like(xs)
    gy = 2 * ys / (h - 1) - 1 if h > 1 else torch.zeros_like(ys)
    grid = torch.stack([gx, gy], dim=-1).clamp(-2, 2)
    samp = F.grid_sample(b, grid, mode="bilinear", padding_mode="border", align_corners=True)
    img = torch.from_numpy(np.ascontiguousarray(src_hwc)).permute(0, 3, 1, 2).double()
    vals = F.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True).permute(0, 2, 3, 1)
    lhs = (f[:, 0] + samp[:, 0]) ** 2 + (f[:, 1] + samp[:, 1]) ** 2
    rhs = alpha * (f[:, 0] ** 2 + f[:, 1] ** 2 + samp[:, 0] ** 2 + samp[:, 1] ** 2) + beta
    return inside.numpy(), lhs.numpy(), rhs.numpy(), vals.numpy(), dist.numpy()


def place(t: torch.Tensor, dev, row_pad: int = 0, base: int = 0, fill=float("nan")):
    """Put logical [n, 2, h, w] (or any [..., h, w]) float data into a larger `fill`-poisoned allocation: rows `row_pad` floats
    longer, the view `base` floats into it.  Returns (allocation, view with the logical shape)."""
    shape = list(t.shape)
    wide = shape[:-1] + [shape[-1] + row_pad]
    numel = int(np.prod(wide))
    buf = torch.full((base + numel + 8,), fill, dtype=torch.float32, device=dev)
    view = buf[base:base + numel].view(wide)[..., :shape[-1]]
    view.copy_(t)
    return buf, view
