"""Yardstick of the Spring scoring tests: a numpy restatement of the reference's validate_spring_mf (evaluate_mf.py:60-102) on
per-pixel arrays, and the case fields the kernel tests score.

`restate(pairs)` takes the scored pairs in order, each (pred float32 [2, h, w], gt float32 [2, h, w] already subsampled), computes
the reference's per-pixel arrays in float32 (every operation rounded on its own, numpy's correctly rounded square root),
concatenates them as the reference does and returns
* 'ref32': the reference's values: np.mean of the float32 EPE array (float32 accumulation) and of the boolean arrays;
* 'f64': the same means with fp64 sums (what the accumulator gives);
* 'counts': the raw counts and fp64 sums, keyed like streamflow_amd.scoring's entries."""
import numpy as np

KEYS = ("epe", "1px", "3px", "5px", "spring_1px", "spring_1px_s0_10", "spring_1px_s10_40", "spring_1px_s40", "epe_valid")


def _mean_or_nan(x):
    return float(np.mean(x)) if x.size else float("nan")


def restate(pairs):
    epe_list, l10, l10_40, l40, lvalid = [], [], [], [], []
    for pred, gt in pairs:
        pred = np.asarray(pred, np.float32)
        gt = np.asarray(gt, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            valid = ~np.isnan(gt[0] + gt[1])
            mag = np.sqrt(gt[0] * gt[0] + gt[1] * gt[1])
            d0, d1 = pred[0] - gt[0], pred[1] - gt[1]
            epe = np.sqrt(d0 * d0 + d1 * d1)
        epe_list.append(epe.reshape(-1))
        l10.append(epe.reshape(-1)[(valid & (mag < 10)).reshape(-1)])
        l10_40.append(epe.reshape(-1)[(valid & (mag >= 10) & (mag < 40)).reshape(-1)])
        l40.append(epe.reshape(-1)[(valid & (mag >= 40)).reshape(-1)])
        lvalid.append(epe.reshape(-1)[valid.reshape(-1)])
    e = np.concatenate(epe_list)
    b10, b10_40, b40, ev = (np.concatenate(x) for x in (l10, l10_40, l40, lvalid))
    ref32 = {"epe": float(np.mean(e)), "1px": float(np.mean(e < 1)), "3px": float(np.mean(e < 3)), "5px": float(np.mean(e < 5)),
             "spring_1px": float(np.mean(e > 1)), "spring_1px_s0_10": _mean_or_nan(b10 > 1),
             "spring_1px_s10_40": _mean_or_nan(b10_40 > 1), "spring_1px_s40": _mean_or_nan(b40 > 1),
             "epe_valid": _mean_or_nan(ev)}
    counts = {"pixels": e.size, "sum_epe": float(e.astype(np.float64).sum()), "lt1": int((e < 1).sum()), "lt3": int((e < 3).sum()),
              "lt5": int((e < 5).sum()), "gt1": int((e > 1).sum()), "valid": ev.size, "sum_epe_valid": float(ev.astype(np.float64).sum()),
              "s0_10": b10.size, "s0_10_gt1": int((b10 > 1).sum()), "s10_40": b10_40.size, "s10_40_gt1": int((b10_40 > 1).sum()),
              "s40": b40.size, "s40_gt1": int((b40 > 1).sum())}

    def r(a, b):
        return a / b if b else float("nan")

    c = counts
    f64 = {"epe": r(c["sum_epe"], c["pixels"]), "1px": r(c["lt1"], c["pixels"]), "3px": r(c["lt3"], c["pixels"]),
           "5px": r(c["lt5"], c["pixels"]), "spring_1px": r(c["gt1"], c["pixels"]), "spring_1px_s0_10": r(c["s0_10_gt1"], c["s0_10"]),
           "spring_1px_s10_40": r(c["s10_40_gt1"], c["s10_40"]), "spring_1px_s40": r(c["s40_gt1"], c["s40"]),
           "epe_valid": r(c["sum_epe_valid"], c["valid"])}
    return {"ref32": ref32, "f64": f64, "counts": counts}


# accumulator entry (streamflow_amd.scoring) of every count above
ENTRY = {"pixels": 0, "sum_epe": 1, "lt1": 2, "lt3": 3, "lt5": 4, "gt1": 5, "valid": 6, "sum_epe_valid": 7, "s0_10": 8,
         "s0_10_gt1": 9, "s10_40": 10, "s10_40_gt1": 11, "s40": 12, "s40_gt1": 13}
SUMS = ("sum_epe", "sum_epe_valid")


def close(a, b, rel):
    """a == b when either is not finite (NaN == NaN here), else |a - b| <= rel |b|."""
    if not (np.isfinite(a) and np.isfinite(b)):
        return (np.isnan(a) and np.isnan(b)) or a == b
    return abs(a - b) <= rel * abs(b)


def assert_acc_matches(acc, want, what=""):
    """acc (numpy fp64 [14]) against restate()['counts']: counts exactly, the two sums within 1e-8 relative.  The bound: two fp64
    sums of at most 2^23 non-negative values, each off by at most n 2^-53 relative, differ by at most 1.9e-9; 5x margin."""
    for k, i in ENTRY.items():
        print(f"{what} {k}: got {acc[i]!r} want {want[k]!r}")
        if k in SUMS:
            assert close(float(acc[i]), want[k], 1e-8), (what, k, acc[i], want[k])
        else:
            assert acc[i] == want[k], (what, k, acc[i], want[k])


def subsample(gt_hw2, step, h, w):
    """gt [Hg, Wg, 2] -> [2, h, w] at gt[step y, step x]: the reference's flow[::2, ::2] (step 2) cropped to the prediction."""
    return np.ascontiguousarray(gt_hw2[0:step * (h - 1) + 1:step, 0:step * (w - 1) + 1:step].transpose(2, 0, 1))


def random_gt(rng, h, w, step, nan_share, decoy=1e6):
    """GT [step h, step w, 2] whose scored pixels have magnitudes spread over the three buckets (< 10, 10 .. 40, >= 40) and a share
    `nan_share` of NaN pixels; every pixel off the step grid holds the decoy value (a wrong subsampling phase fails)."""
    bucket = rng.integers(0, 3, size=(h, w))
    mag = np.array([0.0, 10.0, 40.0])[bucket] + rng.uniform(0, 1, size=(h, w)) * np.array([10.0, 30.0, 40.0])[bucket]
    ang = rng.uniform(-np.pi, np.pi, size=(h, w))
    g = np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1).astype(np.float32)
    if nan_share > 0:
        g[rng.random((h, w)) < nan_share] = np.nan
        if nan_share >= 1:
            g[...] = np.nan
    full = np.full((step * h, step * w, 2), decoy, np.float32)
    full[::step, ::step] = g
    return full
