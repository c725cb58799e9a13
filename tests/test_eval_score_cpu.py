"""The host twin of sf_flow_score_batch (streamflow_amd.scoring.score_host_fields) and the Sintel / KITTI reports on the CPU: against
the numpy restatement of tests/eval_cases.py for both ground-truth kinds, with and without occlusion masks, on fields that carry
pixels exactly on (and one ulp either side of) every threshold; sintel_from / kitti_from on hand-made rows."""
import numpy as np
import pytest

from tests import eval_cases as ec


def test_specials_sit_on_the_thresholds():
    for kind in ("flo", "kitti"):
        sp, vs, mb = ec.specials(kind)
        gu, gv, pu, pv = sp.T
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.sqrt((pu - gu) * (pu - gu) + (pv - gv) * (pv - gv))
            mag = np.sqrt(gu * gu + gv * gv)
            r = e / mag
        assert e.dtype == np.float32 and r.dtype == np.float32
        assert e[0] == 1 and e[1] > 1 and e[2] < 1 and e[3] == 3 and e[4] > 3 and e[5] < 3 and e[6] == 5 and e[7] > 5 and e[8] < 5
        assert np.nextafter(e[0], np.float32(2)) == e[1] and np.nextafter(e[3], np.float32(4)) == e[4]
        # e / |gt| exactly 0.05f is no outlier, one ulp above is one; all three have e > 3
        assert mag[9] == 64 and r[9] == np.float32(0.05) and r[10] > np.float32(0.05) and r[11] < np.float32(0.05)
        assert np.nextafter(r[9], np.float32(1)) == r[10] and (e[9:12] > 3).all()
        assert mag[12] == 0 and e[12] == 0 and np.isnan(r[12]) and mag[13] == 0 and e[13] == 4 and np.isinf(r[13])
        # every ground-truth component is a KITTI code
        fin = np.isfinite(gu) & np.isfinite(gv)
        assert (gu[fin] * 64 == np.round(gu[fin] * 64)).all() and (gv[fin] * 64 == np.round(gv[fin] * 64)).all()
        assert {0, 1, 65535} <= set(vs.tolist()) and {0, 1, 254, 255} <= set(mb.tolist())
        # the outlier-rule pixels meet each valid sample
        for k in (9, 10, 13):
            same = [i for i in range(len(sp)) if (sp[i] == sp[k]).all()]
            assert {0, 1, 65535} <= {int(vs[i]) for i in same}
        if kind == "flo":
            with np.errstate(invalid="ignore"):
                assert np.isnan(gu + gv).sum() == 3
            assert np.isnan(e).sum() >= 3 and np.isinf(e).sum() >= 1


def test_restatement_classifies_the_constructed_pixels():
    """The restatement itself, pixel by pixel, on a field that is nothing but the constructed pixels."""
    sp, vs, mb = ec.specials("kitti")
    n = len(sp)
    pred = np.stack([sp[:, 2], sp[:, 3]]).reshape(2, 1, n)
    gt = np.stack([(sp[:, 0] * 64 + 32768).astype(np.uint16), (sp[:, 1] * 64 + 32768).astype(np.uint16), vs], -1).reshape(1, n, 3)
    e, valid, out = ec.per_pixel(pred, gt, "kitti")
    assert (valid[0] == (vs != 0)).all()
    want_rule = np.zeros(n, bool)
    for i in range(n):
        want_rule[i] = any((sp[i] == sp[k]).all() for k in (4, 6, 7, 8, 10, 13))   # e > 3 and e / |gt| > 0.05f
    assert (out[0] == (want_rule & (vs != 0))).all(), (out[0], want_rule)
    c = ec.restate(pred, gt, "kitti", mb.reshape(1, n))
    assert c["occ"] == int((mb == 255).sum()) and c["noc"] == n - c["occ"] and c["pixels"] == n


@pytest.mark.parametrize("kind", ["flo", "kitti"])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (37, 53), (64, 96)])
def test_score_host_fields_vs_restatement(kind, with_mask, h, w):
    from streamflow_amd import scoring
    rng = np.random.default_rng(h * 1000 + w)
    acc = np.zeros((3, scoring.EVAL_LEN))
    wants = []
    for i in range(3):
        pred, gt, mask = ec.make_field(rng, h, w, kind, 7 * i, with_mask)
        scoring.score_host_fields(pred, gt, acc[i], kind, mask)
        wants.append(ec.restate(pred, gt, kind, mask))
        ec.assert_row_matches(acc[i], wants[i], f"{kind} mask={with_mask} {h}x{w} field {i}")
        if kind == "kitti":                                            # the same bits as int16 (how they travel to the device)
            again = np.zeros(scoring.EVAL_LEN)
            scoring.score_host_fields(pred, gt.view(np.int16), again, kind, mask)
            assert again.tobytes() == acc[i].tobytes()
    if h * w > 100:
        assert len({(w_["lt1"], w_["valid"], w_["outlier"]) for w_ in wants}) == 3, "the fields must differ"
        assert all(w_["outlier"] > 0 and w_["valid"] < w_["pixels"] for w_ in wants)
    if not with_mask:
        assert not acc[:, scoring.EVAL_OCC:].any()
    # a second call adds
    pred, gt, mask = ec.make_field(np.random.default_rng(5), h, w, kind, 0, with_mask)
    one, two = np.zeros(scoring.EVAL_LEN), np.zeros(scoring.EVAL_LEN)
    scoring.score_host_fields(pred, gt, one, kind, mask)
    scoring.score_host_fields(pred, gt, two, kind, mask)
    scoring.score_host_fields(pred, gt, two, kind, mask)
    assert ec.close(two[scoring.EVAL_SUM_EPE], 2 * one[scoring.EVAL_SUM_EPE], 1e-15) and two[scoring.EVAL_PIXELS] == 2 * h * w


def test_kitti_decode_is_the_codecs():
    """The in-kernel decoding expression against flow_io.kitti_decode on every code value."""
    from streamflow_amd import flow_io, scoring
    codes = np.arange(65536, dtype=np.uint16)
    png = np.stack([codes, codes[::-1], (codes % 3 == 0).astype(np.uint16)], -1).reshape(256, 256, 3)
    flow, valid = flow_io.kitti_decode(png)
    gu, gv, v = ec.decode(png, "kitti")
    assert (gu == flow[..., 0]).all() and (gv == flow[..., 1]).all() and (v == (valid >= 0.5)).all()
    row = np.zeros(scoring.EVAL_LEN)
    scoring.score_host_fields(flow.transpose(2, 0, 1), png, row, "kitti")
    assert row[scoring.EVAL_SUM_EPE] == 0 and row[scoring.EVAL_LT1] == 65536 and row[scoring.EVAL_VALID] == (codes % 3 == 0).sum()


def test_score_host_fields_refuses_bad_input():
    from streamflow_amd import scoring
    row = np.zeros(scoring.EVAL_LEN)
    p, g = np.zeros((2, 4, 6), np.float32), np.zeros((4, 6, 2), np.float32)
    for bad in (lambda: scoring.score_host_fields(p, g, row, "spring"), lambda: scoring.score_host_fields(p[0], g, row),
                lambda: scoring.score_host_fields(p, g[:3], row), lambda: scoring.score_host_fields(p, g, row, "kitti"),
                lambda: scoring.score_host_fields(p, np.zeros((4, 6, 3), np.float32), row, "kitti"),
                lambda: scoring.score_host_fields(p, g, row, "flo", np.zeros((4, 6), np.float32)),
                lambda: scoring.score_host_fields(p, g, row, "flo", np.zeros((4, 5), np.uint8))):
        with pytest.raises(ValueError):
            bad()
    assert not row.any()


def test_sintel_from_and_kitti_from():
    from streamflow_amd import scoring as s
    rows = np.zeros((3, s.EVAL_LEN))
    rows[0, [s.EVAL_PIXELS, s.EVAL_SUM_EPE, s.EVAL_LT1, s.EVAL_LT3, s.EVAL_LT5]] = (100, 250.0, 10, 40, 90)
    rows[1, [s.EVAL_PIXELS, s.EVAL_SUM_EPE, s.EVAL_LT1, s.EVAL_LT3, s.EVAL_LT5]] = (100, 50.0, 30, 60, 100)
    rows[2, [s.EVAL_PIXELS, s.EVAL_SUM_EPE, s.EVAL_LT1, s.EVAL_LT3, s.EVAL_LT5]] = (200, 100.0, 40, 100, 110)
    rows[:, s.EVAL_OCC], rows[:, s.EVAL_SUM_EPE_OCC] = (20, 0, 30), (100.0, 0.0, 50.0)
    rows[:, s.EVAL_NOC], rows[:, s.EVAL_SUM_EPE_NOC] = (80, 100, 170), (150.0, 50.0, 50.0)
    rep = s.sintel_from(rows)
    assert rep["pairs"] == 3 and rep["pixels"] == 400 and rep["occ_pixels"] == 50
    assert rep["epe"] == 1.0 and rep["1px"] == 0.2 and rep["3px"] == 0.5 and rep["5px"] == 0.75
    assert rep["epe_occ"] == 3.0 and rep["epe_noc"] == 250.0 / 350
    # no masks: the ratio of an empty set is NaN, as in scoring.report; a single row is accepted as a vector
    rows[:, s.EVAL_OCC:] = 0
    rep = s.sintel_from(rows)
    assert np.isnan(rep["epe_occ"]) and np.isnan(rep["epe_noc"]) and rep["epe"] == 1.0
    assert s.sintel_from(rows[1])["epe"] == 0.5 and s.sintel_from(rows[1])["pairs"] == 1
    assert all(np.isnan(s.sintel_from(np.zeros((1, s.EVAL_LEN)))[k]) for k in ("epe", "1px", "3px", "5px", "epe_occ"))
    # KITTI: the mean of per-image means (NOT the mean over all pixels), outliers over all valid pixels
    rows = np.zeros((2, s.EVAL_LEN))
    rows[0, [s.EVAL_VALID, s.EVAL_SUM_EPE_VALID, s.EVAL_OUTLIER]] = (10, 40.0, 5)
    rows[1, [s.EVAL_VALID, s.EVAL_SUM_EPE_VALID, s.EVAL_OUTLIER]] = (90, 90.0, 5)
    epe, f1 = s.kitti_from(rows)
    assert epe == 2.5 and f1 == 10.0
    rows[1, s.EVAL_VALID] = 0                                            # an image without valid pixels: NaN, as epe[val].mean() is
    epe, f1 = s.kitti_from(rows)
    assert np.isnan(epe) and f1 == 100.0
    assert all(np.isnan(v) for v in s.kitti_from(np.zeros((0, s.EVAL_LEN)))) and all(np.isnan(v) for v in s.kitti_from(np.zeros((1, s.EVAL_LEN))))
    with pytest.raises(ValueError):
        s.sintel_from(np.zeros((2, s.LEN)))
    import torch
    assert s.kitti_from(torch.tensor([[0, 0, 0, 0, 0, 4, 6.0, 1, 0, 0, 0, 0]], dtype=torch.float64)) == (1.5, 25.0)
