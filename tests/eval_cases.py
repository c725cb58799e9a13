"""Yardstick of the Sintel / KITTI scoring tests (sf_flow_score_batch, scoring.score_host_fields): a numpy restatement of the
reference's per-pixel expressions (evaluate_mf.py:124-141 validate_kitti_mf, :570-586 validate_sintel_occ_mf) and the case fields
the tests score.

`restate(pred, gt, kind, mask)` decodes the ground truth the way the reference's readers do (KITTI: `(png - 2^15) / 64`, `valid >=
0.5`; occlusion: `astype(uint8) // 255` as bool), computes the per-pixel arrays in float32 (every operation rounded on its own,
numpy's correctly rounded square root and division) and returns the raw counts and fp64 sums of ONE field, keyed like ENTRY."""
import numpy as np

# accumulator entry (streamflow_amd.scoring.EVAL_*) of every count
ENTRY = {"pixels": 0, "sum_epe": 1, "lt1": 2, "lt3": 3, "lt5": 4, "valid": 5, "sum_epe_valid": 6, "outlier": 7,
         "occ": 8, "sum_epe_occ": 9, "noc": 10, "sum_epe_noc": 11}
LEN = 12
SUMS = ("sum_epe", "sum_epe_valid", "sum_epe_occ", "sum_epe_noc")


def decode(gt, kind):
    """(gu, gv, valid) float32 / bool [h, w] of a ground-truth array as read from its file."""
    if kind == "flo":
        g = np.asarray(gt, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            return g[..., 0], g[..., 1], ~np.isnan(g[..., 0] + g[..., 1])
    a = np.asarray(gt).view(np.uint16).astype(np.float32)
    flow = (a[:, :, :2] - 2 ** 15) / 64.0
    return flow[..., 0].astype(np.float32), flow[..., 1].astype(np.float32), a[:, :, 2] >= 0.5


def per_pixel(pred, gt, kind):
    """(e, valid, outlier) of one field, the reference's expressions in float32."""
    gu, gv, valid = decode(gt, kind)
    pred = np.asarray(pred, np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d0, d1 = pred[0] - gu, pred[1] - gv
        epe = np.sqrt(d0 * d0 + d1 * d1)
        mag = np.sqrt(gu * gu + gv * gv)
        out = (epe > np.float32(3.0)) & ((epe / mag) > np.float32(0.05))
    assert epe.dtype == np.float32 and mag.dtype == np.float32
    return epe, valid, out & valid


def restate(pred, gt, kind, mask=None):
    epe, valid, out = per_pixel(pred, gt, kind)
    e64 = epe.astype(np.float64)
    c = {"pixels": epe.size, "sum_epe": float(e64.sum()), "lt1": int((epe < 1).sum()), "lt3": int((epe < 3).sum()),
         "lt5": int((epe < 5).sum()), "valid": int(valid.sum()), "sum_epe_valid": float(e64[valid].sum()), "outlier": int(out.sum()),
         "occ": 0, "sum_epe_occ": 0.0, "noc": 0, "sum_epe_noc": 0.0}
    if mask is not None:
        occ = (np.asarray(mask).astype(np.uint8) // 255).astype(bool)
        c.update(occ=int(occ.sum()), sum_epe_occ=float(e64[occ].sum()), noc=int((~occ).sum()), sum_epe_noc=float(e64[~occ].sum()))
    return c


def close(a, b, rel):
    """a == b when either is not finite (NaN == NaN here), else |a - b| <= rel |b|."""
    if not (np.isfinite(a) and np.isfinite(b)):
        return (np.isnan(a) and np.isnan(b)) or a == b
    return abs(a - b) <= rel * abs(b)


def assert_row_matches(row, want, what=""):
    """One accumulator row (numpy fp64 [12]) against restate(): counts exactly, the fp64 sums within 1e-8 relative -- the bound of
    score_cases.assert_acc_matches (two fp64 sums of at most 2^23 non-negative values differ by at most 1.9e-9 relative; 5x)."""
    for k, i in ENTRY.items():
        if k in SUMS:
            assert close(float(row[i]), want[k], 1e-8), (what, k, row[i], want[k])
        else:
            assert row[i] == want[k], (what, k, row[i], want[k])


def _nx(x, d):
    return np.nextafter(np.float32(x), np.float32(d))


R05 = np.float32(0.05) * np.float32(64.0)                              # 0.05f * 64: exact (a power-of-two scaling)

# (gu, gv, pu, pv, valid sample, mask byte) of the constructed pixels; every gu, gv is a multiple of 1 / 64 (a KITTI code)
_COMMON = (
    # e exactly 1, 3, 5 and one ulp either side (du = pu - 0.5 is exact, dv = 0; 5 is the 3-4-5 triangle)
    [(0.5, 0.25, 1.5, 0.25), (0.5, 0.25, _nx(1.5, np.inf), 0.25), (0.5, 0.25, _nx(1.5, -np.inf), 0.25),
     (0.5, 0.25, 3.5, 0.25), (0.5, 0.25, _nx(3.5, np.inf), 0.25), (0.5, 0.25, _nx(3.5, -np.inf), 0.25),
     (0.5, 0.25, 3.5, 4.25), (0.5, 0.25, _nx(5.5, np.inf), 0.25), (0.5, 0.25, _nx(5.5, -np.inf), 0.25),
     # |gt| = 64, e / |gt| exactly 0.05f (no outlier), one ulp above (outlier), one below
     (0.0, 64.0, R05, 64.0), (0.0, 64.0, _nx(R05, np.inf), 64.0), (0.0, 64.0, _nx(R05, -np.inf), 64.0),
     # |gt| = 0: e = 0 (0 / 0 = NaN: no outlier), e = 4 (4 / 0 = inf: outlier)
     (0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 4.0, 0.0)])
N_COMMON = len(_COMMON)
VALID_SAMPLES = (0, 1, 65535, 1)
MASK_BYTES = (0, 1, 254, 255)


def specials(kind):
    """float32 [k, 4] (gu, gv, pu, pv), uint16 [k] valid samples, uint8 [k] mask bytes.  The valid samples cycle through 0, 1, 65535
    and the mask bytes through 0, 1, 254, 255 with periods 4 and (shifted) 4, so every pixel class above meets more than one of
    each over the fields' shifted placements; the outlier pixels (9 .. 11, 13) are repeated with every valid sample.  Kind "flo"
    appends NaN and infinite ground truth and a NaN prediction."""
    px = list(_COMMON)
    for k in (9, 10, 11, 13, 3, 4):
        px += [_COMMON[k]] * 3
    if kind == "flo":
        inf = np.float32(np.inf)
        px += [(np.nan, 1.0, 0.0, 0.0), (1.0, np.nan, 0.0, 0.0), (inf, 1.0, 0.0, 0.0), (inf, -inf, 0.0, 0.0), (1.0, 2.0, np.nan, 0.0)]
    n = len(px)
    vs = np.array([VALID_SAMPLES[i % 4] for i in range(n)], np.uint16)
    vs[:N_COMMON] = 1
    vs[12] = 0                                                           # an invalid pixel with |gt| = 0
    for j in range(6):                                                   # the repeated pixels: samples 0, 1, 65535 each
        vs[N_COMMON + 3 * j: N_COMMON + 3 * j + 3] = (0, 1, 65535)
    mb = np.array([MASK_BYTES[(i + i // 4) % 4] for i in range(n)], np.uint8)
    return np.array(px, np.float32), vs, mb


def make_field(rng, h, w, kind, shift, with_mask, occ_share=0.3):
    """One case field: (pred float32 [2, h, w], gt as its file holds it, mask uint8 [h, w] or None).  Random ground truth on the
    KITTI code grid (|gt| ~ 28 px, 30 % invalid: NaN for "flo", sample 0 for "kitti"), a prediction 2 px rms off it, and the
    constructed pixels written over the flat positions shift, shift + 1, .. (as many as fit)."""
    g = (np.round(rng.standard_normal((h, w, 2), dtype=np.float32) * 20 * 64) / 64).astype(np.float32)
    invalid = rng.random((h, w)) < 0.3
    pred = (g + rng.standard_normal((h, w, 2), dtype=np.float32) * 2).transpose(2, 0, 1).astype(np.float32).copy()
    sp, vs, mb = specials(kind)
    k = min(len(sp), h * w)
    ys, xs = np.unravel_index((np.arange(k) + shift) % (h * w), (h, w))
    mask = None
    if with_mask:
        mask = np.where(rng.random((h, w)) < occ_share, 255, rng.integers(0, 255, size=(h, w))).astype(np.uint8)
        mask[ys, xs] = mb[:k]
    pred[0, ys, xs], pred[1, ys, xs] = sp[:k, 2], sp[:k, 3]
    if kind == "flo":
        gt = g.copy()
        gt[invalid] = np.nan
        gt[ys, xs, 0], gt[ys, xs, 1] = sp[:k, 0], sp[:k, 1]
    else:
        gt = np.empty((h, w, 3), np.uint16)
        gt[..., :2] = (g * 64 + 32768).astype(np.uint16)
        gt[..., 2] = np.where(invalid, 0, rng.choice(np.array([1, 2, 65535], np.uint16), size=(h, w)))
        gt[ys, xs, 0] = (sp[:k, 0] * 64 + 32768).astype(np.uint16)
        gt[ys, xs, 1] = (sp[:k, 1] * 64 + 32768).astype(np.uint16)
        gt[ys, xs, 2] = vs[:k]
    return pred, gt, mask
