"""Spring scoring state: the fixed-length fp64 accumulator of ``sf_flow_score`` (layout: include/streamflow_hip.h, SF_SCORE_*), its
host-side twin for flows that live on the host, and the report dictionary (reference evaluate_mf.py:60-102).

Per pixel, in fp32 with every operation rounded on its own (the reference's torch expressions, evaluate_mf.py:63-79):
``e = sqrt((pu - gu)^2 + (pv - gv)^2)``, ``valid = !isnan(gu + gv)``, ``mag = sqrt(gu^2 + gv^2)``.  The device kernel and
:func:`score_host` (numpy float32, whose square root is correctly rounded) compute the same bits and fill the same counters, so
the two paths agree exactly on every count.  Both may differ from the reference's torch-CPU values by one ulp of ``e`` or ``mag``
(torch's float32 CPU square root is not correctly rounded on every host), which matters only for a pixel within one ulp of a
threshold (1, 3, 5, 10, 40).  Means are fp64 sums over counts, where the reference takes a float32 ``np.mean`` of the
concatenated arrays (a few 1e-7 relative apart at millions of pixels).
"""
from __future__ import annotations

from typing import Dict

import numpy as np

# entries of the accumulator (include/streamflow_hip.h)
PIXELS, SUM_EPE, LT1, LT3, LT5, GT1, VALID, SUM_EPE_VALID = range(8)
S0_10, S0_10_GT1, S10_40, S10_40_GT1, S40, S40_GT1 = range(8, 14)
LEN = 14
WS_BYTES = 1024 * LEN * 8                      # SF_SCORE_WS_BYTES


def check_gt(gt_shape, h: int, w: int, step: int) -> None:
    """The ground truth [Hg, Wg, 2] must cover pixel (step (h - 1), step (w - 1)); step is 1 or 2."""
    if step not in (1, 2):
        raise ValueError(f"flow_score: step {step} (1 or 2)")
    if len(gt_shape) != 3 or gt_shape[2] != 2:
        raise ValueError(f"flow_score: ground truth must be [H, W, 2], got {tuple(gt_shape)}")
    if h <= 0 or w <= 0 or gt_shape[0] <= step * (h - 1) or gt_shape[1] <= step * (w - 1):
        raise ValueError(f"flow_score: ground truth {tuple(gt_shape[:2])} does not cover {h} x {w} at step {step}")


def score_host(pred: np.ndarray, gt: np.ndarray, acc: np.ndarray, step: int) -> None:
    """The host path of ``ops.flow_score``: pred float32 [2, h, w], gt float32 [Hg, Wg, 2], acc float64 [LEN] (added to)."""
    pred = np.asarray(pred, dtype=np.float32)
    gt = np.asarray(gt, dtype=np.float32)
    if pred.ndim != 3 or pred.shape[0] != 2:
        raise ValueError(f"flow_score: prediction must be [2, h, w], got {pred.shape}")
    h, w = pred.shape[1:]
    check_gt(gt.shape, h, w, step)
    g = gt[0:step * (h - 1) + 1:step, 0:step * (w - 1) + 1:step]
    pu, pv, gu, gv = pred[0], pred[1], g[..., 0], g[..., 1]
    with np.errstate(invalid="ignore", over="ignore"):             # inf - inf, inf + -inf: NaN, as in the reference
        du, dv = pu - gu, pv - gv
        e = np.sqrt(du * du + dv * dv)
        valid = ~np.isnan(gu + gv)
        mag = np.sqrt(gu * gu + gv * gv)
    gt1 = e > 1
    ev = e[valid]
    mv, gv1 = mag[valid], gt1[valid]
    buckets = (mv < 10, (mv >= 10) & (mv < 40), mv >= 40)
    add = np.zeros(LEN, np.float64)
    add[PIXELS] = e.size
    add[SUM_EPE] = e.astype(np.float64).sum()
    add[LT1], add[LT3], add[LT5] = np.count_nonzero(e < 1), np.count_nonzero(e < 3), np.count_nonzero(e < 5)
    add[GT1] = np.count_nonzero(gt1)
    add[VALID] = ev.size
    add[SUM_EPE_VALID] = ev.astype(np.float64).sum()
    for k, b in enumerate(buckets):
        add[S0_10 + 2 * k] = np.count_nonzero(b)
        add[S0_10_GT1 + 2 * k] = np.count_nonzero(gv1 & b)
    acc += add


def _ratio(a: float, b: float) -> float:
    return float(a / b) if b > 0 else float("nan")            # np.mean of an empty array is NaN


def report(acc) -> Dict[str, float]:
    """The report dictionary of an accumulator (numpy or a torch tensor, on any device)."""
    if hasattr(acc, "detach"):
        acc = acc.detach().cpu().numpy()
    a = np.asarray(acc, dtype=np.float64)
    n = a[PIXELS]
    return {
        "epe": _ratio(a[SUM_EPE], n),
        "1px": _ratio(a[LT1], n), "3px": _ratio(a[LT3], n), "5px": _ratio(a[LT5], n),
        "spring_1px": _ratio(a[GT1], n),
        "spring_1px_s0_10": _ratio(a[S0_10_GT1], a[S0_10]),
        "spring_1px_s10_40": _ratio(a[S10_40_GT1], a[S10_40]),
        "spring_1px_s40": _ratio(a[S40_GT1], a[S40]),
        "epe_valid": _ratio(a[SUM_EPE_VALID], a[VALID]),
        "pixels": int(n), "valid_pixels": int(a[VALID]),
    }
