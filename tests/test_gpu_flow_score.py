"""Spring scoring on the GPU: the sf_flow_score kernel (csrc/flow_score.hip, ops.flow_score) against the numpy restatement of the
reference's validate_spring_mf (tests/score_cases.py) -- shapes from 1 x 1 to 1080 x 1920, one to three pairs per accumulator,
predictions as views into padded buffers (unaligned rows take the scalar loads), ground-truth steps 1 and 2, NaN shares of 0, 5 and
100 %, infinities, a NaN prediction, and pixels exactly on (and one ulp either side of) every threshold.

Criterion: every count equal to the restatement's, the two fp64 sums within 1e-8 relative (score_cases.assert_acc_matches gives
the bound), two runs bitwise equal, the accumulator's neighbours in a sentinel-filled buffer untouched, bad arguments refused."""

import numpy as np
import pytest
import torch

from tests import score_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FF4DEADBEEF0001                                       # a NaN payload no computation produces
GUARD = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _guarded_acc(dev):
    from streamflow_amd import scoring
    buf = torch.full((scoring.LEN + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=dev).view(torch.float64)
    acc = buf[GUARD:GUARD + scoring.LEN]
    acc.zero_()
    return buf, acc


def _guards_intact(buf):
    from streamflow_amd import scoring
    raw = buf.view(torch.int64).cpu().numpy()
    return bool((raw[:GUARD] == SENTINEL).all() and (raw[GUARD + scoring.LEN:] == SENTINEL).all())


def _nx(x, d):
    return np.nextafter(np.float32(x), np.float32(d))


def _specials():
    """(gu, gv, pu, pv) of the constructed pixels: infinities, a NaN prediction at a valid pixel, e exactly 1, 3, 5 and |gt| exactly
    10, 40, each with neighbours one ulp above and below."""
    inf = np.float32(np.inf)
    px = [(inf, 1.0, 0.0, 0.0), (-inf, 1.0, 0.0, 0.0), (inf, -inf, 0.0, 0.0), (1.0, 2.0, np.nan, 0.0)]
    for pu in (1.5, 3.5):                                              # e = pu - 0.5 = 1 and 3 (dv = 0)
        px += [(0.5, 0.25, pu, 0.25), (0.5, 0.25, _nx(pu, np.inf), 0.25), (0.5, 0.25, _nx(pu, -np.inf), 0.25)]
    px += [(0.5, 0.25, 3.5, 4.25), (0.5, 0.25, _nx(5.5, np.inf), 0.25), (0.5, 0.25, _nx(5.5, -np.inf), 0.25)]     # e = 5 (3-4-5)
    for gu, gv, m in ((6.0, 8.0, 10.0), (24.0, 32.0, 40.0)):           # |gt| = 10 and 40, and one ulp either side of it
        px += [(gu, gv, 0.0, 0.0), (_nx(m, np.inf), 0.0, 0.0, 0.0), (_nx(m, -np.inf), 0.0, 0.0, 0.0)]
    return np.array(px, np.float32)


def test_specials_sit_on_the_thresholds():
    s = _specials()
    gu, gv, pu, pv = s.T
    e = np.sqrt((pu - gu) * (pu - gu) + (pv - gv) * (pv - gv))
    mag = np.sqrt(gu * gu + gv * gv)
    assert e[4] == 1 and e[5] > 1 and e[6] < 1 and e[7] == 3 and e[8] > 3 and e[9] < 3 and e[10] == 5 and e[11] > 5 and e[12] < 5
    assert mag[13] == 10 and mag[14] > 10 and mag[15] < 10 and mag[16] == 40 and mag[17] > 40 and mag[18] < 40
    assert np.isnan(gu[2] + gv[2]) and np.isinf(e[:3]).all() and np.isnan(e[3])


def _case(h, w, step, nan_share, top, left, npairs, seed):
    """npairs (padded prediction buffer, view offsets, ground truth [step h, step w, 2]) triples."""
    rng = np.random.default_rng(seed)
    out = []
    for p in range(npairs):
        gt = sc.random_gt(rng, h, w, step, nan_share)
        if nan_share < 1:
            sp = _specials()
            k = min(len(sp), h * w)
            ys, xs = np.unravel_index(np.arange(k) + p, (h, w)) if h * w >= k + p else np.unravel_index(np.arange(k), (h, w))
            gt[step * ys, step * xs, 0], gt[step * ys, step * xs, 1] = sp[:k, 0], sp[:k, 1]
        g = sc.subsample(gt, step, h, w)
        pred = (np.nan_to_num(g, nan=0.0, posinf=0.0, neginf=0.0) + rng.normal(0, 2.0, size=(2, h, w))).astype(np.float32)
        if nan_share < 1:
            pred[0, ys, xs], pred[1, ys, xs] = sp[:k, 2], sp[:k, 3]
        wp = w + left + 8 + (-(w + left)) % 4                          # row pitch: a multiple of 4 floats
        buf = np.full((2, h + top + 3, wp), 7e7, np.float32)            # padding that would wreck every score if read
        buf[:, top:top + h, left:left + w] = pred
        out.append((buf, (top, left), gt, pred))
    return out


SHAPES = [(1, 1), (3, 5), (37, 53), (436, 1024), (1080, 1920)]
CASES = [(h, w, step, nan) for (h, w) in SHAPES for step in (1, 2) for nan in (0.0, 0.05, 1.0)]


@pytest.mark.parametrize("h,w,step,nan_share", CASES)
def test_kernel_vs_restatement(dev, h, w, step, nan_share):
    from streamflow_amd import ops, scoring
    i = CASES.index((h, w, step, nan_share))
    top, left, npairs = (3 * i) % 8, (5 * i + 1) % 8, 1 + i % 3
    pairs = _case(h, w, step, nan_share, top, left, npairs, seed=i)
    want = sc.restate([(pred, sc.subsample(gt, step, h, w)) for _, _, gt, pred in pairs])
    dev_pairs = [(torch.from_numpy(buf).to(dev), off, torch.from_numpy(gt).to(dev)) for buf, off, gt, _ in pairs]
    accs = []
    for run in range(2):
        buf, acc = _guarded_acc(dev)
        for b, (t, l), g in dev_pairs:
            ops.flow_score(b[:, t:t + h, l:l + w], g, acc, step)
        torch.cuda.synchronize()
        assert _guards_intact(buf), "sf_flow_score wrote outside the accumulator"
        accs.append(acc.cpu().numpy())
    sc.assert_acc_matches(accs[0], want["counts"], f"{h}x{w} step {step} nan {nan_share} pairs {npairs} offsets {(top, left)}")
    assert accs[0].tobytes() == accs[1].tobytes(), "two runs differ"
    rep = scoring.report(accs[0])
    for k in sc.KEYS:
        assert sc.close(rep[k], want["f64"][k], 1e-8), (k, rep[k], want["f64"][k])
    if nan_share >= 1:
        assert all(np.isnan(rep[k]) for k in ("spring_1px_s0_10", "spring_1px_s10_40", "spring_1px_s40", "epe", "epe_valid"))
    # the host path fills the same counters from the same arithmetic
    host = np.zeros(scoring.LEN)
    for _, _, gt, pred in pairs:
        scoring.score_host(pred, gt, host, step)
    sc.assert_acc_matches(host, want["counts"], "host")


def test_contiguous_and_unaligned_views_agree(dev):
    """The same field through the float4 path (aligned contiguous planes) and the scalar path (odd column offset)."""
    from streamflow_amd import ops, scoring
    (buf, _, gt, pred), = _case(64, 96, 2, 0.05, 0, 0, 1, seed=99)
    g = torch.from_numpy(gt).to(dev)
    a1, a2 = (torch.zeros(scoring.LEN, dtype=torch.float64, device=dev) for _ in range(2))
    ops.flow_score(torch.from_numpy(pred).to(dev), g, a1, 2)
    shifted = torch.zeros(2, 64, 96 + 8, device=dev)
    shifted[:, :, 3:99] = torch.from_numpy(pred).to(dev)
    ops.flow_score(shifted[:, :, 3:99], g, a2, 2)
    assert a1.cpu().numpy().tobytes() == a2.cpu().numpy().tobytes()


def test_bad_arguments(dev):
    from streamflow_amd import _lib, ops, scoring
    lib = _lib.load()
    pred = torch.zeros(2, 4, 6, device=dev)
    gt = torch.zeros(8, 12, 2, device=dev)
    acc = torch.zeros(scoring.LEN, dtype=torch.float64, device=dev)
    ws = torch.empty(scoring.WS_BYTES, dtype=torch.uint8, device=dev)
    s = _lib.stream()

    def call(pred_p=pred.data_ptr(), cs=24, rs=6, gt_p=gt.data_ptr(), gh=8, gw=12, step=2, h=4, w=6, acc_p=acc.data_ptr(),
             ws_p=ws.data_ptr(), wsb=scoring.WS_BYTES):
        return lib.sf_flow_score(pred_p, cs, rs, gt_p, gh, gw, step, h, w, acc_p, ws_p, wsb, s)

    assert call() == 0
    for kw in ({"pred_p": None}, {"gt_p": None}, {"acc_p": None}, {"ws_p": None}, {"h": 0}, {"w": -1}, {"step": 3}, {"step": 0},
               {"gh": 6}, {"gw": 10}, {"step": 1, "gh": 3}, {"h": 1 << 15, "w": 1 << 15, "gh": 1 << 16, "gw": 1 << 16},
               {"wsb": scoring.WS_BYTES - 8}, {"rs": 5}, {"acc_p": acc.data_ptr() + 4}):
        assert call(**kw) == -1, kw                                     # SF_ERR_BAD_ARG
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        ops.flow_score(pred.cpu(), gt, acc, 2)
    with pytest.raises(RuntimeError):
        ops.flow_score(pred, gt, acc.float(), 2)
    with pytest.raises(RuntimeError):
        ops.flow_score(pred.transpose(1, 2), gt, acc, 2)
    with pytest.raises(ValueError):
        ops.flow_score(pred, gt[:6], acc, 2)
    with pytest.raises(ValueError):
        ops.flow_score(pred, gt, acc, 3)
