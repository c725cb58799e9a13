"""Spring scoring state: the fixed-length fp64 accumulator of ``sf_flow_score`` (layout: include/streamflow_hip.h, SF_SCORE_*), its
host-side twin for flows that live on the host, and the report dictionary (reference evaluate_mf.py:60-102).

Per pixel, in fp32 with every operation rounded on its own (the reference's torch expressions, evaluate_mf.py:63-79):
``e = sqrt((pu - gu)^2 + (pv - gv)^2)``, ``valid = !isnan(gu + gv)``, ``mag = sqrt(gu^2 + gv^2)``.  The device kernel and
:func:`score_host` (numpy float32, whose square root is correctly rounded) compute the same bits and fill the same counters, so
the two paths agree exactly on every count.  Both may differ from the reference's torch-CPU values by one ulp of ``e`` or ``mag``
(torch's float32 CPU square root is not correctly rounded on every host), which matters only for a pixel within one ulp of a
threshold (1, 3, 5, 10, 40).  Means are fp64 sums over counts, where the reference takes a float32 ``np.mean`` of the
concatenated arrays (a few 1e-7 relative apart at millions of pixels).

The Sintel / KITTI accumulator of ``sf_flow_score_batch`` (SF_EVAL_*, one row of ``EVAL_LEN`` doubles per scored field) follows the
same rules: :func:`score_host_fields` is its host twin, with ``outlier = valid & (e > 3) & (e / mag > 0.05)`` added to the
expressions above (numpy's float32 division is correctly rounded, as the kernel's is; ``e / 0 = inf`` is an outlier, ``0 / 0`` is
not).  :func:`sintel_from` takes its means as fp64 sums over counts of the summed rows, where the reference takes float32
``np.mean`` of concatenated arrays (evaluate_mf.py:576-586: the same few 1e-7); its returned per-pass value is the mean of
equal-sized per-pair arrays, i.e. 'epe'.  :func:`kitti_from` forms the per-image mean EPE of every row in fp64 (the reference:
float32 ``epe[val].mean()`` per image, then a float64 mean of those) and the F1-all rate from the summed counts (the reference: a
float32 mean of the concatenated 0 / 1 array, exact only below 2^24 ones).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

# entries of the accumulator (include/streamflow_hip.h)
PIXELS, SUM_EPE, LT1, LT3, LT5, GT1, VALID, SUM_EPE_VALID = range(8)
S0_10, S0_10_GT1, S10_40, S10_40_GT1, S40, S40_GT1 = range(8, 14)
LEN = 14
WS_BYTES = 1024 * LEN * 8                      # SF_SCORE_WS_BYTES

# entries of a row of the Sintel / KITTI accumulator (include/streamflow_hip.h, SF_EVAL_*)
EVAL_PIXELS, EVAL_SUM_EPE, EVAL_LT1, EVAL_LT3, EVAL_LT5, EVAL_VALID, EVAL_SUM_EPE_VALID, EVAL_OUTLIER = range(8)
EVAL_OCC, EVAL_SUM_EPE_OCC, EVAL_NOC, EVAL_SUM_EPE_NOC = range(8, 12)
EVAL_LEN = 12
SCORE_BATCH_MAX = 32                           # SF_SCORE_BATCH_MAX: fields one sf_flow_score_batch call takes
GT_KINDS = {"flo": 0, "kitti": 1}              # SF_GT_FLO32, SF_GT_KITTI16


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


def score_host_fields(pred: np.ndarray, gt: np.ndarray, acc_row: np.ndarray, kind: str = "flo", mask: Optional[np.ndarray] = None) -> None:
    """The host twin of ``ops.flow_score_batch`` for ONE field: pred float32 [2, h, w]; gt as its decoder left it -- kind "flo":
    float32 [h, w, 2] (flow_io.read_flo), kind "kitti": the 16-bit samples [h, w, 3] = (u, v, valid) of a flow_occ PNG
    (flow_io.read_png; uint16, or int16 holding the same bits); mask: uint8 [h, w], occluded where 255 (a Sintel occlusions PNG);
    acc_row float64 [EVAL_LEN] (added to)."""
    if kind not in GT_KINDS:
        raise ValueError(f"flow_score_batch: kind {kind!r} ('flo' or 'kitti')")
    pred = np.asarray(pred, dtype=np.float32)
    if pred.ndim != 3 or pred.shape[0] != 2:
        raise ValueError(f"flow_score_batch: prediction must be [2, h, w], got {pred.shape}")
    h, w = pred.shape[1:]
    gt = np.asarray(gt)
    if kind == "flo":
        if gt.shape != (h, w, 2):
            raise ValueError(f"flow_score_batch: 'flo' ground truth must be [{h}, {w}, 2], got {gt.shape}")
        g = gt.astype(np.float32, copy=False)
        gu, gv = g[..., 0], g[..., 1]
        with np.errstate(invalid="ignore", over="ignore"):
            valid = ~np.isnan(gu + gv)
    else:
        if gt.shape != (h, w, 3) or gt.dtype not in (np.uint16, np.int16):
            raise ValueError(f"flow_score_batch: 'kitti' ground truth must be 16-bit [{h}, {w}, 3], got {gt.dtype} {gt.shape}")
        smp = gt.view(np.uint16)
        gu = (smp[..., 0].astype(np.float32) - np.float32(32768.0)) / np.float32(64.0)
        gv = (smp[..., 1].astype(np.float32) - np.float32(32768.0)) / np.float32(64.0)
        valid = smp[..., 2] != 0
    pu, pv = pred[0], pred[1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        du, dv = pu - gu, pv - gv
        e = np.sqrt(du * du + dv * dv)
        mag = np.sqrt(gu * gu + gv * gv)
        outlier = valid & (e > np.float32(3.0)) & ((e / mag) > np.float32(0.05))
    add = np.zeros(EVAL_LEN, np.float64)
    add[EVAL_PIXELS] = e.size
    add[EVAL_SUM_EPE] = e.astype(np.float64).sum()
    add[EVAL_LT1], add[EVAL_LT3], add[EVAL_LT5] = np.count_nonzero(e < 1), np.count_nonzero(e < 3), np.count_nonzero(e < 5)
    add[EVAL_VALID] = np.count_nonzero(valid)
    add[EVAL_SUM_EPE_VALID] = e[valid].astype(np.float64).sum()
    add[EVAL_OUTLIER] = np.count_nonzero(outlier)
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != (h, w) or mask.dtype != np.uint8:
            raise ValueError(f"flow_score_batch: mask must be uint8 [{h}, {w}], got {mask.dtype} {mask.shape}")
        occ = mask == 255
        add[EVAL_OCC], add[EVAL_NOC] = np.count_nonzero(occ), np.count_nonzero(~occ)
        add[EVAL_SUM_EPE_OCC] = e[occ].astype(np.float64).sum()
        add[EVAL_SUM_EPE_NOC] = e[~occ].astype(np.float64).sum()
    acc_row += add


def _rows(acc) -> np.ndarray:
    if hasattr(acc, "detach"):
        acc = acc.detach().cpu().numpy()
    a = np.asarray(acc, dtype=np.float64)
    if a.ndim == 1:
        a = a[None]
    if a.ndim != 2 or a.shape[1] != EVAL_LEN:
        raise ValueError(f"expected accumulator rows [n, {EVAL_LEN}], got {a.shape}")
    return a


def sintel_from(acc) -> Dict[str, float]:
    """The Sintel report of accumulator rows [n, EVAL_LEN] (one per scored pair; numpy or a torch tensor on any device), summed:
    'epe', '1px', '3px', '5px', 'epe_occ', 'epe_noc' (NaN without masks), 'pairs', 'pixels', 'occ_pixels'."""
    rows = _rows(acc)
    a = rows.sum(axis=0)
    n = a[EVAL_PIXELS]
    return {
        "epe": _ratio(a[EVAL_SUM_EPE], n),
        "1px": _ratio(a[EVAL_LT1], n), "3px": _ratio(a[EVAL_LT3], n), "5px": _ratio(a[EVAL_LT5], n),
        "epe_occ": _ratio(a[EVAL_SUM_EPE_OCC], a[EVAL_OCC]), "epe_noc": _ratio(a[EVAL_SUM_EPE_NOC], a[EVAL_NOC]),
        "pairs": int(rows.shape[0]), "pixels": int(n), "occ_pixels": int(a[EVAL_OCC]),
    }


def kitti_from(acc) -> Tuple[float, float]:
    """(EPE, F1-all in percent) of accumulator rows [n, EVAL_LEN], one per image: the mean over the images of each image's mean EPE
    over its valid pixels (NaN as soon as one image has none, as in the reference), and 100 * outliers / valid pixels over all."""
    rows = _rows(acc)
    if rows.shape[0] == 0:
        return float("nan"), float("nan")
    per_image = [_ratio(r[EVAL_SUM_EPE_VALID], r[EVAL_VALID]) for r in rows]
    return float(np.mean(per_image)), 100.0 * _ratio(rows[:, EVAL_OUTLIER].sum(), rows[:, EVAL_VALID].sum())
