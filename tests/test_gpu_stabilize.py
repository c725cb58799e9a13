"""sf_motion_moments / sf_motion_solve / sf_motion_fit / sf_warp_affine_u8 (csrc/stabilize.hip) through the C ABI with raw strides
and guard bands, and the ops wrappers.

Criteria.  Moments: N exactly; every sum within terms * 2^-52 * sum |term| of numpy's float64 sum of the SAME float64 terms (the
numpy float32 restatement of the weights, tests/stabilize_cases.py; two summation orders of `terms` signed terms differ by at most
(terms - 1) * 2^-53 * sum |term| each); a second call bitwise the first.  Solve: from the device's own moments, within
64 * 2^-53 * cond(M) * max |p| of numpy.linalg.solve (Cholesky's backward error at n <= 4).  rss / S1: within 64 * 2^-53 * (Sqq +
2 |p|.|b| + |p|'|M||p|) / S1 of the float64 value.  The chain: every round's moments and model recomputed on the host from the
device's previous fp32 model and inv_c2 meet the same bounds; on the robustness case (a quarter of the frame moving on its own) the
device's final model sends the frame corners within 0.05 px of the true camera.  Warped bytes and outside counts: BITWISE the
restatement's.  Operands lie in NaN-filled allocations, outputs between sentinel bands; NaN, Inf and huge flows and maps are
ordinary inputs with defined results: nothing here is meant to fault."""
import numpy as np
import pytest
import torch

from tests import consistency_cases as cc
from tests import stabilize_cases as sc
from tests.guarded import GuardedBytes

pytestmark = pytest.mark.gpu

# the last size: five blocks of moments units (18 units of 256 samples, 4 to a block) and three blocks of warp groups, the last partial
SIZES = [(1, 1), (1, 7), (5, 1), (13, 37), (17, 65), (33, 130), (9, 300)]
BAND, SENT = 512, 0x5A
CODES, CLASS_WEIGHTS = (0, 1, 2), (1.0, 0.25, 0.0)
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from streamflow_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Bytes:
    """`size` bytes holding SENT between two bands of BAND sentinel bytes, `shift` bytes off the allocation's alignment."""

    def __init__(self, dev, size, shift=0, data=None):
        self.lo, self.size = BAND + shift, size
        self.buf = torch.full((self.lo + size + BAND,), SENT, dtype=torch.uint8, device=dev)
        if data is not None:
            self.view().copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)))

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo

    def view(self):
        return self.buf[self.lo:self.lo + self.size]

    def bands_intact(self):
        return bool((self.buf[:self.lo] == SENT).all() and (self.buf[self.lo + self.size:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


class Rows:
    """`count` elements of `dtype` holding `start` between two bands of eight sentinel elements."""

    def __init__(self, dev, count, dtype=torch.float64, start=777.25, band=777.25):
        self.band = band
        self.buf = torch.full((8 + count + 8,), band, dtype=dtype, device=dev)
        self.rows = self.buf[8:8 + count]
        self.rows.fill_(start)

    @property
    def ptr(self):
        return self.rows.data_ptr()

    def bands_intact(self):
        return bool((self.buf[:8] == self.band).all() and (self.buf[-8:] == self.band).all())

    def untouched(self):
        return bool((self.buf == self.band).all())


def _bits_equal(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def run_moments(lib, dev, flows, cls, step, model, inv_c2, strided, max_mag=None):
    """sf_motion_moments through the C ABI, twice; returns the rows and asserts every guard and the repeatability."""
    n, _, h, w = flows.shape
    pad, base = (3, 1) if strided else (0, 0)
    fbuf, fv = cc.place(torch.from_numpy(flows), dev, pad, base)
    fsnap = fbuf.clone()
    assert (fv.data_ptr() % 16 != 0) == strided
    cbytes = None if cls is None else Bytes(dev, n * h * w, shift=1 if strided else 0, data=cls)
    mod = None if model is None else Rows(dev, n * 6, torch.float32, band=float("nan"))
    ic2 = None if model is None else Rows(dev, n, torch.float32, band=float("nan"))
    if model is not None:
        mod.rows.copy_(torch.from_numpy(np.asarray(model, np.float32).reshape(-1)))
        ic2.rows.copy_(torch.from_numpy(np.asarray(inv_c2, np.float32).reshape(-1)))
    max_mag = 4.0 * max(h, w) if max_mag is None else max_mag
    got = []
    for _ in range(2):
        out = Rows(dev, n * sc.LEN, start=123.0)                         # WRITTEN, not added to: the start value must vanish
        ws = GuardedBytes(dev, lib.sf_motion_moments_ws_bytes(n, h, w, step), guard=4096)
        st = lib.sf_motion_moments(fv.data_ptr(), fv.stride(0), fv.stride(1), fv.stride(2), n, h, w, None if cls is None else cbytes.ptr,
                                   CODES[0], CODES[1], CODES[2], CLASS_WEIGHTS[0], CLASS_WEIGHTS[1], CLASS_WEIGHTS[2], step, max_mag,
                                   None if model is None else mod.ptr, None if model is None else ic2.ptr, out.ptr, ws.ptr, ws.size,
                                   stream())
        assert st == 0, lib.sf_last_error()
        torch.cuda.synchronize()
        assert out.bands_intact() and ws.guards_unchanged()
        got.append(out.rows.view(n, sc.LEN).cpu().numpy())
    assert _bits_equal(fbuf, fsnap), "the flows were written"
    assert cbytes is None or cbytes.bands_intact()
    assert got[0].tobytes() == got[1].tobytes(), "two calls differ"
    return got[0]


def check_moments(got, want, mag, cnt, tag=""):
    assert np.array_equal(got[:, sc.N], want[:, sc.N]), (tag, got[:, sc.N], want[:, sc.N])
    bound = cnt * 2.0 ** -52 * mag
    err = np.abs(got - want)
    worst = np.argmax(err - bound)
    print(f"{tag}: worst moment error {err.flat[worst]:.3g} against a bound of {bound.flat[worst]:.3g}")
    assert (err <= bound).all(), (tag, got.flat[worst], want.flat[worst], bound.flat[worst])


def model_case(seed, n):
    """A plausible previous model per field (normalised, fp32) and inv_c2: some pixels inside the biweight, some outside."""
    rng = np.random.default_rng(seed)
    model = rng.uniform(-3, 3, (n, 6)).astype(np.float32)
    return model, rng.uniform(0.01, 0.2, n).astype(np.float32)


@pytest.mark.parametrize("robust", [False, True], ids=["plain", "cls+model"])
@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "%dx%d" % s)
def test_moments_match_the_restatement(lib, dev, hw, strided, step, robust):
    h, w = hw
    n = 3
    flows, _ = sc.make_fields(50 + h + w, n, h, w, noise=1.0)
    cls = sc.make_cls(60 + h, n, h, w, CODES) if robust else None
    model, inv_c2 = model_case(70 + w, n) if robust else (None, None)
    got = run_moments(lib, dev, flows, cls, step, model, inv_c2, strided)
    wt = sc.weights32(flows, cls=cls, codes=CODES, class_weights=CLASS_WEIGHTS, step=step, model=model, inv_c2=inv_c2)
    if robust and h * w > 100:
        assert 0 < (wt[0] > 0).sum() < wt[0].size                        # the case has pixels on both sides of the weighting
    check_moments(got, *sc.moments64(*wt), tag=f"{hw} step {step}")


def test_moments_with_many_fields_share_the_blocks(lib, dev):
    """1100 fields: a field's share of the call's blocks is one block, which strides over its four units."""
    n, h, w = 1100, 13, 37
    flows = np.tile(sc.make_fields(5, 4, h, w, noise=1.0)[0], (275, 1, 1, 1))
    flows[:, 0] += np.arange(n, dtype=np.float32)[:, None, None] * np.float32(0.01)
    got = run_moments(lib, dev, flows, None, 1, None, None, False)
    check_moments(got, *sc.moments64(*sc.weights32(flows)), tag="1100 fields")


def test_special_flows_weigh_nothing(lib, dev):
    h, w = 9, 14
    flows, _ = sc.make_fields(2, 2, h, w)
    flows[0, 0, 0, :5] = [np.nan, np.inf, -np.inf, 1e30, -1e30]
    flows[0, 1, 1, :5] = [np.nan, np.inf, -np.inf, 1e30, 51.0]
    flows[1] = np.nan
    for model, inv_c2 in ((None, None), (np.zeros((2, 6), np.float32), np.array([0.001, np.inf], np.float32)),
                          (np.full((2, 6), np.nan, np.float32), np.array([0.001, 0.001], np.float32))):
        got = run_moments(lib, dev, flows, None, 1, model, inv_c2, True, max_mag=50.0)
        want = sc.moments64(*sc.weights32(flows, max_mag=50.0, model=model, inv_c2=inv_c2))
        check_moments(got, *want, tag="special")
        assert np.isfinite(got).all() and not got[1].any()
        assert got[0, sc.N] == (h * w - 10 if model is None or not np.isnan(model).any() else 0)


def solve_on_device(lib, dev, moments, kind, kappa=2.0, c_floor=1.0):
    n = moments.shape[0]
    mom = torch.from_numpy(np.ascontiguousarray(moments)).to(dev)
    m64, m32, c = Rows(dev, n * 6), Rows(dev, n * 6, torch.float32), Rows(dev, n)
    ic2, status = Rows(dev, n, torch.float32), Rows(dev, n, torch.int32, start=-5, band=-9)
    st = lib.sf_motion_solve(mom.data_ptr(), n, kind, kappa, c_floor, m64.ptr, m32.ptr, c.ptr, ic2.ptr, status.ptr, stream())
    assert st == 0, lib.sf_last_error()
    torch.cuda.synchronize()
    assert all(r.bands_intact() for r in (m64, m32, c, ic2, status))
    return (m64.rows.view(n, 6).cpu().numpy(), m32.rows.view(n, 6).cpu().numpy(), c.rows.cpu().numpy(), ic2.rows.cpu().numpy(),
            status.rows.cpu().numpy())


def check_solution(m, a, kind, tag=""):
    """A device model against numpy.linalg.solve on the normal equations of the moments it was solved from."""
    M, rhs = sc.normal_matrix(m, kind)
    cond = np.linalg.cond(M)
    for got, b in zip(sc.unknowns(a, kind), rhs):
        p = np.linalg.solve(M, b)
        err, bound = np.abs(got - p).max(), 64 * EPS * cond * np.abs(p).max()
        print(f"{tag}: model error {err:.3g} against a bound of {bound:.3g} (cond {cond:.3g})")
        assert err <= bound, (tag, got, p)
    if kind == sc.TRANSLATION:
        assert not a[[1, 2, 4, 5]].any()
    if kind == sc.SIMILARITY:
        assert a[1] == a[5] and a[4] == -a[2]


def rss_and_bound(m, a):
    """(rss / S1 in float64 from the moments and a model, the bound on the device's value)."""
    M3 = np.array([[m[sc.S1], m[sc.SX], m[sc.SY]], [m[sc.SX], m[sc.SXX], m[sc.SXY]], [m[sc.SY], m[sc.SXY], m[sc.SYY]]])
    bu, bv = m[[sc.SU, sc.SXU, sc.SYU]], m[[sc.SV, sc.SXV, sc.SYV]]
    pu, pv = a[:3], a[3:]
    rss = max(0.0, m[sc.SQQ] - 2 * (pu @ bu + pv @ bv) + (pu @ M3 @ pu + pv @ M3 @ pv)) / m[sc.S1]
    size = m[sc.SQQ] + 2 * (np.abs(pu) @ np.abs(bu) + np.abs(pv) @ np.abs(bv)) + (np.abs(pu) @ np.abs(M3) @ np.abs(pu)
                                                                                  + np.abs(pv) @ np.abs(M3) @ np.abs(pv))
    return rss, 64 * EPS * size / m[sc.S1]


@pytest.mark.parametrize("kind", [sc.TRANSLATION, sc.SIMILARITY, sc.AFFINE], ids=["translation", "similarity", "affine"])
def test_solve_from_the_devices_own_moments(lib, dev, kind):
    h, w, n = 33, 130, 4
    flows, _ = sc.make_fields(31, n, h, w, noise=0.5)
    moments = run_moments(lib, dev, flows, sc.make_cls(32, n, h, w), 1, None, None, False)
    m64, m32, c, ic2, status = solve_on_device(lib, dev, moments, kind, kappa=1.0, c_floor=1e-6)
    assert (status == sc.OK).all() and np.array_equal(m32, m64.astype(np.float32))
    for i in range(n):
        check_solution(moments[i], m64[i], kind, tag=f"field {i}")
        rss, bound = rss_and_bound(moments[i], m64[i])
        print(f"field {i}: rss / S1 {c[i] * c[i]!r} against {rss!r}, bound {bound:.3g}")
        assert rss > 0.1 and abs(c[i] * c[i] - rss) <= bound             # kappa = 1 and a tiny floor: c = sqrt(rss / S1)
        assert abs(float(ic2[i]) - 1.0 / (c[i] * c[i])) <= 2.0 ** -23 * (1.0 / (c[i] * c[i]))
    # the floor holds, kappa scales
    _, _, c2, ic22, _ = solve_on_device(lib, dev, moments, kind, kappa=2.0, c_floor=100.0)
    assert (c2 == 100.0).all() and (ic22 == np.float32(1e-4)).all()


def test_rank_deficient_inputs_have_statuses(lib, dev):
    for hw, kind, want in (((1, 1), sc.AFFINE, sc.DEGENERATE), ((1, 1), sc.SIMILARITY, sc.DEGENERATE), ((1, 1), sc.TRANSLATION, sc.OK),
                           ((5, 1), sc.AFFINE, sc.DEGENERATE), ((5, 1), sc.SIMILARITY, sc.OK), ((1, 7), sc.AFFINE, sc.DEGENERATE)):
        flows = np.full((2, 2) + hw, 1.5, np.float32)
        flows[1, 1] = -2.0
        moments = run_moments(lib, dev, flows, None, 1, None, None, False)
        m64, _, c, _, status = solve_on_device(lib, dev, moments, kind)
        assert (status == want).all(), (hw, kind, status)
        if want == sc.DEGENERATE:
            assert np.array_equal(m64, [[1.5, 0, 0, 1.5, 0, 0], [1.5, 0, 0, -2.0, 0, 0]]) and (c == 1.0).all()
    # all-zero weights: every pixel occluded (weight 0 here), and a field of NaN
    flows = np.ones((2, 2, 6, 8), np.float32)
    flows[1] = np.nan
    cls = np.full((2, 6, 8), CODES[2], np.uint8)
    cls[1] = CODES[0]
    moments = run_moments(lib, dev, flows, cls, 1, None, None, False)
    assert not moments.any()
    m64, m32, c, ic2, status = solve_on_device(lib, dev, moments, sc.AFFINE)
    assert (status == sc.EMPTY).all() and not m64.any() and not m32.any() and (c == 1.0).all() and (ic2 == 1.0).all()
    nan_rows = np.full((1, sc.LEN), np.nan)
    assert solve_on_device(lib, dev, nan_rows, sc.SIMILARITY)[4][0] == sc.EMPTY


def run_fit(lib, dev, flows, kind, rounds, cls=None, step=1, kappa=2.0, c_floor=1.0, strided=False):
    n, _, h, w = flows.shape
    fbuf, fv = cc.place(torch.from_numpy(flows), dev, *((3, 1) if strided else (0, 0)))
    cbytes = None if cls is None else Bytes(dev, n * h * w, shift=1 if strided else 0, data=cls)
    trace = Rows(dev, n * rounds * sc.TRACE_LEN, start=-1.0)
    ws = GuardedBytes(dev, lib.sf_motion_fit_ws_bytes(n, h, w, step), guard=4096)
    st = lib.sf_motion_fit(fv.data_ptr(), fv.stride(0), fv.stride(1), fv.stride(2), n, h, w, None if cls is None else cbytes.ptr, CODES[0],
                           CODES[1], CODES[2], CLASS_WEIGHTS[0], CLASS_WEIGHTS[1], CLASS_WEIGHTS[2], step, 4.0 * max(h, w), kind, rounds,
                           kappa, c_floor, trace.ptr, ws.ptr, ws.size, stream())
    assert st == 0, lib.sf_last_error()
    torch.cuda.synchronize()
    assert trace.bands_intact() and ws.guards_unchanged()
    return trace.rows.view(n, rounds, sc.TRACE_LEN).cpu().numpy()


@pytest.mark.parametrize("kind", [sc.SIMILARITY, sc.AFFINE], ids=["similarity", "affine"])
@pytest.mark.parametrize("strided,step", [(False, 1), (True, 3)], ids=["contiguous", "strided-step3"])
def test_chain_link_by_link(lib, dev, kind, strided, step):
    """Every round of the trace from the round before it: the weights from the device's fp32 model and inv_c2, the moments from those
    weights, the model and the scale from the device's own moments."""
    h, w, n, rounds, kappa, c_floor = 33, 130, 3, 4, 2.0, 1e-3
    flows = np.concatenate([sc.make_fields(41, n - 1, h, w, noise=0.4)[0], sc.robust_case(9, h, w)[0]])
    cls = sc.make_cls(42, n, h, w)
    trace = run_fit(lib, dev, flows, kind, rounds, cls=cls, step=step, kappa=kappa, c_floor=c_floor, strided=strided)
    model, inv_c2 = None, None
    for r in range(rounds):
        want = sc.moments64(*sc.weights32(flows, cls=cls, codes=CODES, class_weights=CLASS_WEIGHTS, step=step, model=model, inv_c2=inv_c2))
        check_moments(trace[:, r, :sc.LEN], *want, tag=f"round {r}")
        for i in range(n):
            m, a = trace[i, r, :sc.LEN], trace[i, r, sc.T_MODEL:sc.T_MODEL + 6]
            assert trace[i, r, sc.T_STATUS] == sc.OK
            check_solution(m, a, kind, tag=f"round {r} field {i}")
            rss, bound = rss_and_bound(m, a)
            c = trace[i, r, sc.T_C]
            assert kappa * np.sqrt(rss) > 2 * c_floor and abs((c / kappa) ** 2 - rss) <= bound, (r, i, c, rss, bound)      # (above the floor)
            ic2 = trace[i, r, sc.T_INV_C2]
            assert ic2 == np.float64(np.float32(ic2)) and abs(ic2 - 1.0 / (c * c)) <= 2.0 ** -23 / (c * c)
        model, inv_c2 = trace[:, r, sc.T_MODEL:sc.T_MODEL + 6].astype(np.float32), trace[:, r, sc.T_INV_C2].astype(np.float32)
    assert (trace[:, 1:, sc.S1] < trace[:, :1, sc.S1]).all()             # the reweighting took weight away


@pytest.mark.parametrize("hw", [(24, 40), (37, 53), (64, 96)], ids=lambda s: "%dx%d" % s)
def test_chain_recovers_the_camera_under_a_moving_quarter(lib, dev, hw):
    h, w = hw
    flow, cam = sc.robust_case(7, h, w)
    trace = run_fit(lib, dev, flow, sc.AFFINE, 6)
    errs = [sc.corner_error(sc.to_pixels(trace[0, r, sc.T_MODEL:sc.T_MODEL + 6], h, w), cam, h, w) for r in range(6)]
    print(f"{hw}: corner error per round {['%.4f' % e for e in errs]}")
    assert errs[0] > 1.0 and errs[-1] <= 0.05


def _frames(arr_hwc, dev, chw_odd):
    """uint8 [n, h, w, 3] -> (device tensor keeping the allocation alive, ptr, byte strides (frame, row, px, ch))."""
    t = torch.from_numpy(arr_hwc)
    n, h, w, _ = t.shape
    if not chw_odd:
        d = t.contiguous().to(dev)
        return d, d.data_ptr(), (3 * h * w, 3 * w, 3, 1)
    raw = torch.full((3 + t.numel() + 8,), 0xEE, dtype=torch.uint8, device=dev)
    raw[3:3 + t.numel()].copy_(t.permute(0, 3, 1, 2).contiguous().reshape(-1).to(dev))
    return raw, raw.data_ptr() + 3, (3 * h * w, w, 1, h * w)


def warp_maps(h, w):
    """Inverse maps float32 [12, 6]: identity, integer shifts, a sub-pixel shift, a rotation, a 2x zoom, maps that leave the frame
    entirely, NaN / Inf / 1e30 entries."""
    cx, cy = (w - 1) / 2, (h - 1) / 2
    co, si = np.cos(0.3), np.sin(0.3)
    maps = [[1, 0, 0, 0, 1, 0], [1, 0, 2, 0, 1, -1], [1, 0, -3, 0, 1, 1], [1, 0, 0.25, 0, 1, -0.625],
            [co, -si, cx - co * cx + si * cy + 0.3, si, co, cy - si * cx - co * cy - 0.2],
            [0.5, 0, cx / 2, 0, 0.5, cy / 2], [1, 0, 1e4, 0, 1, 0], [1, 0, 0, 0, 1, -(h + 5.0)],
            [np.nan, 0, 0, 0, 1, 0], [1, 0, 0, 0, 1, np.inf], [1, 0, -np.inf, 0, 1, 0], [1e30, 0, 0, 0, -1e30, 0.5]]
    return np.array(maps, np.float32)


def run_warp(lib, dev, src, maps, border, fill, strided):
    n, h, w, _ = src.shape
    skeep, sptr, ss = _frames(src, dev, strided)
    ssnap = skeep.clone()
    mp = Rows(dev, n * 6, torch.float32, band=float("nan"))
    mp.rows.copy_(torch.from_numpy(maps.reshape(-1)))
    out = Bytes(dev, n * h * w * 3, shift=1 if strided else 0)
    counts = Rows(dev, n, torch.int32, start=-5, band=-9)
    ws = GuardedBytes(dev, lib.sf_warp_affine_ws_bytes(n, h, w), guard=4096)
    st = lib.sf_warp_affine_u8(sptr, ss[0], ss[1], ss[2], ss[3], mp.ptr, n, h, w, border, fill[0], fill[1], fill[2], out.ptr, counts.ptr,
                               ws.ptr, ws.size, stream())
    assert st == 0, lib.sf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(skeep, ssnap), "the source was written"
    assert out.bands_intact() and counts.bands_intact() and ws.guards_unchanged()
    return out.view().view(n, h, w, 3).cpu().numpy(), counts.rows.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("border", [sc.CONSTANT, sc.REPLICATE], ids=["constant", "replicate"])
@pytest.mark.parametrize("strided", [False, True], ids=["hwc", "chw-odd"])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "%dx%d" % s)
def test_warp_matches_the_restatement_bitwise(lib, dev, hw, strided, border):
    h, w = hw
    maps = warp_maps(h, w)
    src = np.random.default_rng(80 + h + w).integers(0, 256, size=(len(maps), h, w, 3), dtype=np.uint8)
    fill = (7, 130, 255)
    got, counts = run_warp(lib, dev, src, maps, border, fill, strided)
    want, want_counts = sc.warp_affine32(src, maps, border, fill)
    assert np.array_equal(counts, want_counts), (counts, want_counts)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} bytes differ"
    assert np.array_equal(got[0], src[0]) and counts[0] == 0              # identity
    assert (counts[6:11] == h * w).all()                                 # left the frame entirely, NaN, Inf
    assert (got[8] == fill).all()                                        # NaN: the fill bytes in either mode
    if border == sc.CONSTANT:
        assert (got[6] == fill).all() and (got[7] == fill).all()
    else:
        assert np.array_equal(got[6], np.broadcast_to(src[6][:, -1:], src[6].shape))        # clamped to the last column
        assert np.array_equal(got[7], np.broadcast_to(src[7][:1], src[7].shape))            # clamped to the first row


def test_warp_with_many_frames_shares_the_blocks(lib, dev):
    n, h, w = 1100, 13, 37
    rng = np.random.default_rng(4)
    src = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    maps = np.tile(warp_maps(h, w)[:6], (184, 1))[:n].copy()
    maps[:, 2] += rng.uniform(-2, 2, n).astype(np.float32)
    got, counts = run_warp(lib, dev, src, maps, sc.CONSTANT, (1, 2, 3), False)
    want, want_counts = sc.warp_affine32(src, maps, sc.CONSTANT, (1, 2, 3))
    assert np.array_equal(got, want) and np.array_equal(counts, want_counts)


def test_bad_arguments_write_nothing(lib, dev):
    n, h, w, rounds = 2, 9, 20, 3
    flows = torch.zeros(n, 2, h, w, device=dev)
    src = torch.zeros(n, h, w, 3, dtype=torch.uint8, device=dev)
    maps = torch.zeros(n, 6, device=dev)
    mom, trace, ws = Rows(dev, n * sc.LEN), Rows(dev, n * rounds * sc.TRACE_LEN), Bytes(dev, 1 << 16)
    out, counts = Bytes(dev, n * h * w * 3), Rows(dev, n, torch.int32, start=-9, band=-9)
    m64, m32, c, ic2, status = Rows(dev, n * 6), Rows(dev, n * 6, torch.float32), Rows(dev, n), Rows(dev, n, torch.float32), \
        Rows(dev, n, torch.int32, start=-9, band=-9)
    nan = float("nan")
    ok = dict(flows=flows.data_ptr(), fr=w, ch=h * w, n=n, h=h, w=w, step=1, max_mag=100.0, wv=1.0, model=None, inv_c2=None, mom=mom.ptr,
              ws=ws.ptr, ws_bytes=ws.size, kind=sc.AFFINE, rounds=rounds, kappa=2.0, c_floor=1.0, trace=trace.ptr)

    def moments(**kw):
        a = dict(ok, **kw)
        return lib.sf_motion_moments(a["flows"], 2 * h * w, a["ch"], a["fr"], a["n"], a["h"], a["w"], None, 0, 1, 2, a["wv"], 0.0, 0.0,
                                     a["step"], a["max_mag"], a["model"], a["inv_c2"], a["mom"], a["ws"], a["ws_bytes"], stream())

    def fit(**kw):
        a = dict(ok, **kw)
        return lib.sf_motion_fit(a["flows"], 2 * h * w, a["ch"], a["fr"], a["n"], a["h"], a["w"], None, 0, 1, 2, a["wv"], 0.0, 0.0,
                                 a["step"], a["max_mag"], a["kind"], a["rounds"], a["kappa"], a["c_floor"], a["trace"], a["ws"],
                                 a["ws_bytes"], stream())

    shared = (dict(flows=None), dict(ws=None), dict(n=0), dict(n=65536), dict(h=0), dict(w=0), dict(h=1 << 15, w=1 << 15), dict(fr=w - 1),
              dict(ch=0), dict(flows=flows.data_ptr() + 2), dict(step=0), dict(max_mag=nan), dict(max_mag=-1.0), dict(wv=nan),
              dict(wv=-1.0), dict(wv=float("inf")), dict(ws=ws.ptr + 4))
    for bad in shared + (dict(mom=None), dict(model=maps.data_ptr()), dict(inv_c2=maps.data_ptr()), dict(mom=mom.ptr + 4),
                         dict(ws_bytes=lib.sf_motion_moments_ws_bytes(n, h, w, 1) - 1)):
        assert moments(**bad) == -1, bad
    for bad in shared + (dict(trace=None), dict(kind=3), dict(kind=-1), dict(rounds=0), dict(rounds=17), dict(kappa=nan), dict(kappa=-1.0),
                         dict(c_floor=nan), dict(c_floor=0.0), dict(c_floor=float("inf")), dict(trace=trace.ptr + 4),
                         dict(ws_bytes=lib.sf_motion_fit_ws_bytes(n, h, w, 1) - 1)):
        assert fit(**bad) == -1, bad
    good = torch.zeros(n, sc.LEN, dtype=torch.float64, device=dev)

    def solve(**kw):
        a = dict(dict(mom=good.data_ptr(), n=n, kind=sc.AFFINE, kappa=2.0, c_floor=1.0, m64=m64.ptr, m32=m32.ptr, c=c.ptr, ic2=ic2.ptr,
                      status=status.ptr), **kw)
        return lib.sf_motion_solve(a["mom"], a["n"], a["kind"], a["kappa"], a["c_floor"], a["m64"], a["m32"], a["c"], a["ic2"],
                                   a["status"], stream())

    for bad in (dict(mom=None), dict(m64=None), dict(m32=None), dict(c=None), dict(ic2=None), dict(status=None), dict(n=0), dict(n=65536),
                dict(kind=7), dict(kappa=nan), dict(c_floor=nan), dict(c_floor=-1.0), dict(m64=m64.ptr + 4), dict(m32=m32.ptr + 2)):
        assert solve(**bad) == -1, bad

    def warp(**kw):
        a = dict(dict(src=src.data_ptr(), maps=maps.data_ptr(), n=n, h=h, w=w, border=sc.REPLICATE, out=out.ptr, counts=counts.ptr,
                      ws=ws.ptr, ws_bytes=ws.size, rs=3 * w), **kw)
        return lib.sf_warp_affine_u8(a["src"], 3 * h * w, a["rs"], 3, 1, a["maps"], a["n"], a["h"], a["w"], a["border"], 0, 0, 0, a["out"],
                                     a["counts"], a["ws"], a["ws_bytes"], stream())

    for bad in (dict(src=None), dict(maps=None), dict(out=None), dict(counts=None), dict(ws=None), dict(n=0), dict(n=65536), dict(h=0),
                dict(w=-1), dict(h=1 << 15, w=1 << 15), dict(border=2), dict(rs=-1), dict(maps=maps.data_ptr() + 1),
                dict(counts=counts.ptr + 2), dict(ws_bytes=lib.sf_warp_affine_ws_bytes(n, h, w) - 1)):
        assert warp(**bad) == -1, bad
    for fn, args in ((lib.sf_motion_moments_ws_bytes, (0, h, w, 1)), (lib.sf_motion_moments_ws_bytes, (n, h, w, 0)),
                     (lib.sf_motion_fit_ws_bytes, (n, 1 << 15, 1 << 15, 1)), (lib.sf_warp_affine_ws_bytes, (n, 0, w))):
        assert fn(*args) == -1, args
    torch.cuda.synchronize()
    assert all(r.untouched() for r in (mom, trace, ws, out, counts, m64, m32, c, ic2, status))
    # ... and the good calls do write
    assert moments() == 0 and fit() == 0 and solve() == 0 and warp() == 0
    torch.cuda.synchronize()
    assert float(mom.rows[sc.N]) == h * w and float(trace.rows[sc.N]) == h * w and int(status.rows[0]) == sc.EMPTY
    assert bool((out.view() == 0).all()) and int(counts.rows[0]) == 0


def test_wrappers(dev):
    from streamflow_amd import ops
    n, h, w = 3, 37, 53
    flows = np.concatenate([sc.make_fields(21, n - 1, h, w, noise=0.2, kind=sc.SIMILARITY)[0], sc.robust_case(3, h, w)[0]])
    cls = sc.make_cls(22, n, h, w, (255, 0, 128))
    f = torch.from_numpy(flows).to(dev)
    _, fview = cc.place(f, dev, 3, 1)
    for kind in ("translation", "similarity", "affine"):
        models, info = ops.motion_fit(f, kind=kind)
        assert models.dtype == torch.float64 and tuple(models.shape) == (n, 2, 3) and models.device == dev
        trace = info["trace"].cpu().numpy()
        assert trace.shape == (n, 6, sc.TRACE_LEN) and info["status"].tolist() == [0] * n
        for i in range(n):
            want = sc.to_pixels(trace[i, -1, sc.T_MODEL:sc.T_MODEL + 6], h, w)
            assert np.abs(models[i].cpu().numpy() - want).max() <= 1e-12 * max(h, w)
        assert torch.equal(info["c"], info["trace"][:, -1, sc.T_C])
        share = info["inlier_share"].cpu().numpy()
        assert np.array_equal(share, trace[:, -1, sc.S1] / (h * w)) and (share > 0).all() and (share < 1).all()
        again, _ = ops.motion_fit(fview, kind=kind)
        assert torch.equal(again, models)                                # a view with odd strides: the same bits
    # the restated chain from the same flows ends at the same camera (its fp32 models may differ in the last bit on the way)
    models, info = ops.motion_fit(f, cls=torch.from_numpy(cls).to(dev), kind="affine", rounds=4, step=2, codes=(255, 0, 128),
                                  class_weights=CLASS_WEIGHTS, kappa=2.5, c_floor=0.5)
    want = sc.fit(flows, sc.AFFINE, rounds=4, kappa=2.5, c_floor=0.5, cls=cls, codes=(255, 0, 128), class_weights=CLASS_WEIGHTS, step=2)
    for i in range(n):
        err = sc.corner_error(models[i].cpu().numpy(), sc.to_pixels(want[i, -1, sc.T_MODEL:sc.T_MODEL + 6], h, w), h, w)
        assert err <= 1e-4, (i, err)
    assert ops.motion_fit(f, rounds=1)[1]["inlier_share"].tolist() == [1.0] * n
    # warp_affine: layouts, float64 maps on the host, out=
    maps = warp_maps(h, w)[:6]
    src = np.random.default_rng(5).integers(0, 256, size=(6, h, w, 3), dtype=np.uint8)
    s = torch.from_numpy(src).to(dev)
    for border, code in (("replicate", sc.REPLICATE), ("constant", sc.CONSTANT)):
        want, want_counts = sc.warp_affine32(src, maps, code, (9, 8, 7))
        for frames, cl in ((s, None), (s.permute(0, 3, 1, 2).contiguous(), False), (s.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1), None)):
            got, counts = ops.warp_affine(frames, torch.from_numpy(maps.astype(np.float64)).view(6, 2, 3), border=border, fill=(9, 8, 7),
                                          channels_last=cl)
            assert np.array_equal(got.cpu().numpy(), want) and counts.tolist() == want_counts.tolist()
    held = torch.empty(6, h, w, 3, dtype=torch.uint8, device=dev)
    got, _ = ops.warp_affine(s, torch.from_numpy(maps).to(dev), border="constant", fill=(9, 8, 7), out=held)
    assert got is held and np.array_equal(held.cpu().numpy(), want)
    with pytest.raises(RuntimeError, match="inv_maps"):
        ops.warp_affine(s, torch.zeros(5, 2, 3))
    with pytest.raises(RuntimeError, match="out must"):
        ops.warp_affine(s, torch.zeros(6, 2, 3), out=held[:5])
    with pytest.raises(RuntimeError, match="cls must"):
        ops.motion_fit(f, cls=torch.zeros(n, h, w, device=dev))
    with pytest.raises(ValueError, match="class_weights"):
        ops.motion_fit(f, class_weights=(1.0, -1.0, 0.0))
