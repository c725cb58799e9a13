"""CPU: the numpy restatement of csrc/stabilize.hip (tests/stabilize_cases.py) against independent formulations, the robustness of the
reweighting chain, stabilize.camera_path and the wrappers' argument checks.

Bounds.  Solve formulas against numpy.linalg.solve: 64 * 2^-53 * cond(M) * max |p| (Cholesky's backward error at n <= 4, cond computed
here).  Robustness: the final model moves the frame corners within 0.025 px of the true camera where round 0 (plain least squares)
is off by more than 1 px."""
import numpy as np
import pytest
import torch

from tests import stabilize_cases as sc

SIZES = [(24, 40), (37, 53), (64, 96)]


@pytest.mark.parametrize("kind", [sc.TRANSLATION, sc.SIMILARITY, sc.AFFINE])
@pytest.mark.parametrize("hw", SIZES + [(5, 9)], ids=lambda s: "%dx%d" % s)
def test_restatement_agrees_with_lstsq_and_linalg_solve(hw, kind):
    h, w = hw
    flows, cams = sc.make_fields(3 + h, 2, h, w, noise=0.3, kind=kind)
    cls = sc.make_cls(5, 2, h, w)
    for step in (1, 3):
        wt, xn, yn, u, v = sc.weights32(flows, cls=cls, class_weights=(1.0, 0.25, 0.0), step=step)
        mom, _, _ = sc.moments64(wt, xn, yn, u, v)
        for i in range(2):
            a, c, inv_c2, status, rss = sc.solve64(mom[i], kind)
            assert status == sc.OK
            want = sc.lstsq64(wt[i], xn, yn, u[i], v[i], kind)
            M, rhs = sc.normal_matrix(mom[i], kind)
            cond = np.linalg.cond(M)
            print(f"{hw} kind {kind} step {step}: |a - lstsq| {np.abs(a - want).max():.3g}, cond {cond:.3g}")
            assert np.abs(a - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
            for got, b in zip(sc.unknowns(a, kind), rhs):
                p = np.linalg.solve(M, b)
                assert np.abs(got - p).max() <= 64 * 2.0 ** -53 * cond * np.abs(p).max(), (got, p, cond)
            # rss / S1 against the residuals themselves
            X, Y = np.broadcast_to(xn[None, :], wt[i].shape).astype(np.float64), np.broadcast_to(yn[:, None], wt[i].shape).astype(np.float64)
            ru = u[i] - (a[0] + a[1] * X + a[2] * Y)
            rv = v[i] - (a[3] + a[4] * X + a[5] * Y)
            direct = (wt[i].astype(np.float64) * (ru * ru + rv * rv)).sum() / mom[i, sc.S1]
            assert abs(rss - direct) <= 1e-9 * max(1.0, mom[i, sc.SQQ] / mom[i, sc.S1])
            assert c == max(1.0, 2.0 * np.sqrt(rss)) and inv_c2 == np.float32(1.0 / (c * c))


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "%dx%d" % s)
def test_all_kinds_recover_an_exact_model(hw):
    h, w = hw
    for true_kind in (sc.TRANSLATION, sc.SIMILARITY, sc.AFFINE):
        flows, cams = sc.make_fields(11, 1, h, w, noise=0.0, kind=true_kind)
        for kind in (sc.TRANSLATION, sc.SIMILARITY, sc.AFFINE):
            if kind < true_kind:
                continue                                                 # a smaller model cannot hold a larger motion
            trace = sc.fit(flows, kind, rounds=3)
            err = sc.corner_error(sc.to_pixels(trace[0, -1, sc.T_MODEL:sc.T_MODEL + 6], h, w), cams[0], h, w)
            assert err <= 2e-4, (true_kind, kind, err)                   # the flows are float32 of values up to ~ 10 px
            assert trace[0, -1, sc.T_STATUS] == sc.OK and trace[0, -1, sc.N] == h * w


def test_degenerate_and_empty_inputs_have_statuses():
    for hw, kind, want in (((1, 1), sc.AFFINE, sc.DEGENERATE), ((1, 1), sc.SIMILARITY, sc.DEGENERATE), ((1, 1), sc.TRANSLATION, sc.OK),
                           ((7, 1), sc.AFFINE, sc.DEGENERATE), ((7, 1), sc.SIMILARITY, sc.OK), ((1, 9), sc.AFFINE, sc.DEGENERATE)):
        flows = np.full((1, 2) + hw, 1.5, np.float32)
        trace = sc.fit(flows, kind, rounds=2)
        assert trace[0, -1, sc.T_STATUS] == want, (hw, kind)
        if want == sc.DEGENERATE:
            assert np.array_equal(trace[0, -1, sc.T_MODEL:sc.T_MODEL + 6], [1.5, 0, 0, 1.5, 0, 0])
    flows = np.full((1, 2, 6, 8), np.nan, np.float32)
    trace = sc.fit(flows, sc.AFFINE, rounds=2)
    assert trace[0, -1, sc.T_STATUS] == sc.EMPTY and not trace[0, -1, :sc.T_C].any() and trace[0, -1, sc.T_C] == 1.0
    cls = np.ones((1, 6, 8), np.uint8)                                   # every pixel occluded: weight 0
    trace = sc.fit(np.ones((1, 2, 6, 8), np.float32), sc.AFFINE, rounds=1, cls=cls)
    assert trace[0, 0, sc.T_STATUS] == sc.EMPTY


def test_special_flows_weigh_nothing():
    h, w = 9, 14
    flows, _ = sc.make_fields(2, 1, h, w)
    clean = sc.moments64(*sc.weights32(flows, max_mag=50.0))[0]
    flows[0, 0, 0, :5] = [np.nan, np.inf, -np.inf, 1e30, -1e30]
    flows[0, 1, 1, :5] = [np.nan, np.inf, -np.inf, 1e30, 51.0]
    mom = sc.moments64(*sc.weights32(flows, max_mag=50.0))[0]
    assert np.isfinite(mom).all() and mom[0, sc.N] == h * w - 10 and clean[0, sc.N] == h * w
    model, inv_c2 = np.zeros((1, 6), np.float32), np.array([np.inf], np.float32)        # 0 * inf and x * inf: weight 0, not NaN
    mom = sc.moments64(*sc.weights32(flows, model=model, inv_c2=inv_c2))[0]
    assert np.isfinite(mom).all() and mom[0, sc.N] == 0


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_chain_recovers_the_camera_under_a_moving_quarter(hw):
    h, w = hw
    flow, cam = sc.robust_case(7, h, w)
    trace = sc.fit(flow, sc.AFFINE, rounds=6, kappa=2.0, c_floor=1.0)
    errs = [sc.corner_error(sc.to_pixels(trace[0, r, sc.T_MODEL:sc.T_MODEL + 6], h, w), cam, h, w) for r in range(6)]
    print(f"{hw}: corner error per round {['%.4f' % e for e in errs]}, c {trace[0, :, sc.T_C]}")
    assert errs[0] > 1.0
    assert errs[-1] <= 0.025


def test_camera_path():
    from streamflow_amd import stabilize
    hw = (40, 64)
    eye = np.tile(np.array([[1.0, 0, 0], [0, 1.0, 0]]), (9, 1, 1))
    B, z = stabilize.camera_path(eye, sigma=3.0, zoom="auto", hw=hw)
    assert B.shape == (10, 2, 3) and np.array_equal(B, np.tile(eye[0], (10, 1, 1))) and z == 1.0
    # a constant-velocity translation: nothing to smooth where the window is whole
    n, sigma = 40, 2.0
    vel = eye[:1].repeat(n, axis=0)
    vel[:, :, 2] = (1.5, -0.75)
    B, _ = stabilize.camera_path(vel, sigma=sigma, zoom=1.0, hw=hw)
    r = int(np.ceil(4 * sigma))
    assert np.abs(B[r:n + 1 - r] - eye[0]).max() <= 1e-12
    assert np.abs(B[0] - eye[0]).max() > 0.5                             # at the ends the cut window pulls towards the inside
    # tripod mode: the cumulative product, M_k applied after C_k
    rng = np.random.default_rng(0)
    models = np.stack([sc.camera(k, *hw) for k in range(6)])
    B, _ = stabilize.camera_path(torch.from_numpy(models), sigma=None, zoom=1.0, hw=hw)
    C = np.eye(3)
    assert np.array_equal(B[0], np.eye(3)[:2])
    for k in range(6):
        C = np.vstack([models[k], [0, 0, 1]]) @ C
        assert np.abs(B[k + 1] - C[:2]).max() <= 1e-12
    # jitter about a fixed camera: smoothing maps each frame nearly as tripod mode does
    jit = rng.uniform(-3, 3, (31, 2))
    jit[0] = 0
    steps = eye[:1].repeat(30, axis=0)
    steps[:, :, 2] = jit[1:] - jit[:-1]
    Bs, _ = stabilize.camera_path(steps, sigma=1000.0, zoom=1.0, hw=hw)
    assert np.abs(Bs[:, :, 2] - (jit - jit.mean(0))).max() <= 1e-3 and np.abs(Bs[:, :, :2] - np.eye(2)).max() <= 1e-12
    # zoom: auto is the smallest that keeps every corner inside; fixed zoom scales about the centre
    Bz, z = stabilize.camera_path(steps, sigma=1000.0, zoom="auto", hw=hw, max_zoom=2.0)
    q = np.concatenate([stabilize.corners(hw), np.ones((4, 1))], 1)

    def worst(maps):                                                      # how far outside the worst corner reads (<= 0: inside)
        p = np.einsum("nij,qj->nqi", maps, q)
        return max((-p).max(), (p[..., 0] - (hw[1] - 1)).max(), (p[..., 1] - (hw[0] - 1)).max())

    assert 1.0 < z < 2.0 and worst(Bz) <= 1e-9
    assert worst(stabilize.camera_path(steps, sigma=1000.0, zoom=z * (1 - 1e-6), hw=hw)[0]) > 0
    assert stabilize.camera_path(steps, sigma=1000.0, zoom="auto", hw=hw, max_zoom=1.01)[1] == 1.01          # capped
    B2, _ = stabilize.camera_path(eye, sigma=None, zoom=2.0, hw=hw)
    c = np.array([(hw[1] - 1) / 2, (hw[0] - 1) / 2, 1.0])
    assert np.allclose(B2[3] @ c, c[:2]) and np.allclose(B2[3] @ [0, 0, 1], c[:2] / 2)
    for bad in (dict(sigma=0.0), dict(zoom=0.5), dict(zoom="auto", hw=None), dict(zoom=1.5, hw=None)):
        with pytest.raises(ValueError):
            stabilize.camera_path(eye, **dict(dict(sigma=3.0, zoom=1.0, hw=hw), **bad))


def test_pixel_conversion_matches_the_cases():
    from streamflow_amd import ops
    a = np.random.default_rng(1).standard_normal((3, 6))
    for h, w in ((1, 1), (5, 9), (40, 24)):
        got = ops.motion_to_pixels(torch.from_numpy(a), h, w).numpy()
        for i in range(3):
            assert np.abs(got[i] - sc.to_pixels(a[i], h, w)).max() <= 1e-15 * max(h, w) * np.abs(a[i]).max()
            # the model's displacement at a pixel is the pixel map's
            x, y = 3.0, 2.0
            xs, ys, xn, yn = sc.coords32(h, w)
            s = 2.0 / max(w - 1, h - 1, 1)
            X, Y = (x - (w - 1) / 2) * s, (y - (h - 1) / 2) * s
            want = np.array([x + a[i, 0] + a[i, 1] * X + a[i, 2] * Y, y + a[i, 3] + a[i, 4] * X + a[i, 5] * Y])
            assert np.abs(got[i] @ [x, y, 1.0] - want).max() <= 1e-12


def test_wrappers_refuse_bad_arguments_without_a_gpu():
    from streamflow_amd import ops, stabilize
    flows = torch.zeros(2, 2, 5, 7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.motion_fit(flows)
    for bad in (dict(kind="homography"), dict(rounds=0), dict(rounds=17), dict(rounds=2.0), dict(step=0)):
        with pytest.raises(ValueError):
            ops.motion_fit(flows, **bad)
    frames = torch.zeros(2, 5, 7, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.warp_affine(frames, torch.zeros(2, 2, 3))
    with pytest.raises(ValueError, match="border"):
        ops.warp_affine(frames, torch.zeros(2, 2, 3), border="mirror")
    with pytest.raises(ValueError, match="fill"):
        ops.warp_affine(frames, torch.zeros(2, 2, 3), fill=(0, 0, 256))
    with pytest.raises(RuntimeError, match="no batch"):
        stabilize.MotionSink().models()
