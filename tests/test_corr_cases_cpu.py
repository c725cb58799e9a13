"""Pins tests/corr_cases.py, the references, decoders and bounds of tests/test_gpu_corr_kernels.py, without a GPU:

    the float64 pyramid equals oracle.corr_pyramid; the pixel-space lookup equals oracle.corr_lookup within that oracle's documented
        round-trip slack where the oracle is defined (no 1-cell level, in-range coordinates), and both reproduce the reference's golden
        volumes (tests/golden/corr_odd.npz, corr_b2.npz) within the tolerance tests/test_gpu_corr_blocked32.py uses for them;
    every decoder inverts an encoder written here cell by cell from the words of include/streamflow_hip.h; the geometry restatement
        keeps the header's invariants on every grid;
    |model - exact| <= bound / 2 for every case, class and level, and bound <= cap: the cap can hide nothing;
    each wrong kernel of the list, restated as a mutation of the numpy model, is more than TEN bounds off in some element, on the
        smallest grid of the case list that can show it (named per test);
    the case sets, so that a later edit cannot thin them."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import corr_cases as cc

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = cc.cases()
BUILD_CLASSES = ("fp32", "x3", "f16", "b16")


def _case(h, w, **kw):
    return next(c for c in CASES if (c["h"], c["w"]) == (h, w) and all(c[k] == v for k, v in kw.items()))


@functools.lru_cache(maxsize=None)
def _pair(cid, b=0, t=0):
    c = next(c for c in CASES if c["id"] == cid)
    f = cc.features(c)
    return f[b, t], f[b, t + 1]


def _klasses(c):
    """Every arithmetic class the GPU test runs the case with: the blocked fp16 build with frames shared and separate."""
    ks = [cc.klass(n) for n in ("fp32", "x3", "f16")] + [cc.klass("b16", c["D"], c["pairs"], False)]
    if c["pairs"] > 1:
        ks.append(cc.klass("b16", c["D"], c["pairs"], True))
    return ks


# ---- the case sets -----------------------------------------------------------------------------------------------------------------
def test_case_sets():
    assert cc.GRIDS == ((8, 8), (8, 9), (9, 8), (8, 16), (8, 17), (15, 17), (16, 24), (11, 36), (17, 33), (24, 40))
    assert cc.DEPTHS == (1, 8, 24, 40, 64, 256) and cc.IMAGES == ((1, 1), (2, 1), (1, 3), (2, 2))
    assert cc.FAMILIES == ("pyramid", "blocked16", "blocked32")
    assert len(CASES) == 13 and len({c["id"] for c in CASES}) == 13 and len({c["seed"] for c in CASES}) == 13
    # every family runs every case, so coverage per family is coverage of the list
    assert {(c["h"], c["w"]) for c in CASES} == set(cc.GRIDS)
    assert {c["D"] for c in CASES} == set(cc.DEPTHS) and {(c["B"], c["pairs"]) for c in CASES} == set(cc.IMAGES)
    assert {(c["h"], c["w"]) for c in CASES if c["D"] == 256} == set(cc.DEPTH_256_GRIDS) == set(sorted(cc.GRIDS, key=lambda g: g[0] * g[1])[:2])
    odd = lambda c: (c["h"] * c["w"]) % 4 != 0                                   # noqa: E731
    assert {(h, w) for h, w in cc.GRIDS if (h * w) % 4} == {(15, 17), (17, 33)}
    for D in cc.DEPTHS:
        on = [c for c in CASES if c["D"] == D]
        assert len({(c["h"], c["w"]) for c in on}) >= 2 and (D == 256 or any(odd(c) for c in on)), D
    for im in cc.IMAGES:
        on = [c for c in CASES if (c["B"], c["pairs"]) == im]
        assert len({(c["h"], c["w"]) for c in on}) >= 2 and any(odd(c) for c in on), im
    # the edges the grids carry
    N = {g: g[0] * g[1] for g in cc.GRIDS}
    assert N[(8, 8)] == 64 and N[(8, 16)] == 128 and N[(8, 17)] == 136 and N[(15, 17)] == 255 and N[(16, 24)] == 384
    assert (8 >> 3, 8 >> 3) == (1, 1) and 36 % 8 == 4 and 33 == 32 + 1
    assert {n % 32 != 0 for n in N.values()} == {True, False} and {g[1] > 32 for g in cc.GRIDS} == {True, False}


def test_the_four_fold_combinations_of_the_blocked_fp16_build_occur():
    seen = set()
    for c in CASES:
        for shared_frames in ((False, True) if c["pairs"] > 1 else (False,)):
            shared, pa, pb, post = cc.blocked_fold(c["D"], c["pairs"], shared_frames)
            seen.add((shared, post == 1.0 and c["D"] > 1))
            assert abs(pa * pb * post - c["D"] ** -0.5) < 1e-7
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
    assert cc.blocked_fold(256, 3, True) == (True, 0.25, 0.25, 1.0) and cc.blocked_fold(16, 2, True) == (True, 0.5, 0.5, 1.0)
    assert cc.blocked_fold(40, 3, True)[:3] == (True, 1.0, 1.0) and cc.blocked_fold(32, 2, True)[:3] == (True, 1.0, 1.0)
    assert cc.blocked_fold(64, 2, True) == (False, 0.125, 1.0, 1.0) and cc.blocked_fold(256, 3, False) == (False, 0.0625, 1.0, 1.0)
    assert cc.blocked_fold(24, 1, False)[:3] == (False, 1.0, 1.0) and cc.blocked_fold(40, 3, False)[:3] == (False, 1.0, 1.0)


def test_coordinate_sets():
    for h, w in cc.GRIDS:
        fx = cc.fixed_coords(h, w)
        assert tuple(fx) == cc.COORD_NAMES and len({p for p, _ in fx.values()}) == len(fx)
        assert all(y < h and x < w for (y, x), _ in fx.values())
        assert fx["minus_one"][1][0] == -1.0 and fx["last_cell"][1] == (w - 1.0, h - 1.0) and fx["w_minus_1_plus_eps"][1][0] == w - 1 + 2.0 ** -10
        assert fx["level3_outside"][1][0] / 8 - 4 >= (w >> 3) and fx["ys_mod4_3"][1][1] % 4 == 3.75
        assert np.signbit(fx["minus_zero"][1][0]) and fx["large_negative"][1][0] % 1 != 0
        for name, axis, val in (("pos_inf_x", 0, np.inf), ("neg_inf_x", 0, -np.inf), ("pos_inf_y", 1, np.inf), ("neg_inf_y", 1, -np.inf)):
            assert fx[name][1][axis] == val and np.isfinite(fx[name][1][1 - axis])
        assert np.isnan(fx["nan_x"][1][0]) and np.isfinite(fx["nan_x"][1][1]) and np.isnan(fx["nan_y"][1][1]) and np.isfinite(fx["nan_y"][1][0])
    c = _case(8, 9)
    xy = cc.coords(c)
    assert xy.shape == (2, 2, 72) and xy.dtype == np.float32 and np.isnan(xy[:, 0, 4 * 9 + 4]).all() and np.isinf(xy[0, 0, 7 * 9 + 3])


# ---- the reference pinned to what exists ------------------------------------------------------------------------------------------------
def test_pyramid_equals_the_oracle():
    from oracle import streamflow_oracle as orc
    for c in (_case(8, 8), _case(15, 17, D=24), _case(11, 36)):
        h, w = c["h"], c["w"]
        f1, f2 = _pair(c["id"])
        want = orc.corr_pyramid(torch.from_numpy(f1).double().reshape(1, -1, h, w), torch.from_numpy(f2).double().reshape(1, -1, h, w), 4)
        for a, b in zip(cc.pyramid(f1, f2, h, w), want):
            assert a.shape == (h * w,) + tuple(b.shape[2:]) and np.abs(a - b.numpy()[:, 0]).max() < 1e-15


def test_lookup_equals_the_oracle_where_the_oracle_is_defined():
    from oracle import streamflow_oracle as orc
    for c in (_case(16, 24), _case(17, 33, D=8), _case(24, 40)):
        h, w = c["h"], c["w"]
        assert (h >> 3) > 1 and (w >> 3) > 1
        f = cc.features(dict(c, amp=1.0))                                          # unit-normal: the scale of the oracle's documented slack
        lv = [x.astype(np.float32) for x in cc.pyramid(f[0, 0], f[0, 1], h, w)]
        xy = cc.coords(c)[0].copy()
        ident = np.stack(np.meshgrid(np.arange(w), np.arange(h), indexing="xy")).reshape(2, -1).astype(np.float32)
        bad = ~(np.abs(xy) < 1.0e4).all(0)                                       # non-finite and far coordinates: out of the oracle's range
        xy[:, bad] = ident[:, bad]
        want = orc.corr_lookup([torch.from_numpy(x)[:, None] for x in lv], torch.from_numpy(xy).reshape(1, 2, h, w), 4).numpy()
        got, _, _ = cc.lookup([x.astype(np.float64) for x in lv], xy)
        assert np.abs(got - want.reshape(324, -1)).max() < 2e-5 * max(1.0, w / 32)


@pytest.mark.parametrize("tag", ["corr_odd", "corr_b2"])
def test_reference_reproduces_the_golden_volumes(tag):
    from tests import cases
    g = np.load(os.path.join(GOLDEN, tag + ".npz"))
    f1, f2, coords, ident = cases.corr_inputs(tag)
    B, D, h, w = f1.shape
    N = h * w
    for z in range(B):
        lv = cc.pyramid(f1[z].reshape(D, N).numpy(), f2[z].reshape(D, N).numpy(), h, w)
        for l in range(4):
            assert np.abs(lv[l] - g[f"level{l}"][z * N:(z + 1) * N, 0]).max() < 2e-5, (tag, l)
        for xy, key in ((coords, "lookup"), (ident, "lookup_identity")):
            got, _, _ = cc.lookup(lv, xy[z].reshape(2, N).numpy())
            assert np.abs(got - g[key][z].reshape(324, N)).max() < 2e-5, (tag, key)


def test_lookup_rule_at_the_edges():
    """One level-0 map with a single 1 at (y, x) = (2, 3) on an 8 x 8 grid; the other levels zero."""
    m = np.zeros((1, 8, 8))
    m[0, 2, 3] = 1.0
    lv = [m, np.zeros((1, 4, 4)), np.zeros((1, 2, 2)), np.zeros((1, 1, 1))]
    look = lambda x, y: cc.lookup(lv, np.array([[x], [y]], np.float32))            # noqa: E731
    out, asum, dead = look(3.0, 2.0)
    assert out.sum() == 1.0 and not dead[:81].all()                                # integer coordinates: one channel holds the cell
    assert out[4 * 9 + 4, 0] == 1.0 and out[5 * 9 + 4, 0] == 0.0 and out[3 * 9 + 4, 0] == 0.0            # a moves x: x + 1 and x - 1 miss the cell
    out, _, _ = look(2.25, 2.0)                                                    # channel a = 4: x = 2.25 -> 0.25 of the cell to the right
    assert out[4 * 9 + 4, 0] == 0.25 and out[5 * 9 + 4, 0] == 0.75 and out[4 * 9 + 5, 0] == 0.0
    for bad in (np.inf, -np.inf, np.nan, 1.0e6, -1.0e6):
        for xy in ((bad, 2.0), (3.0, bad)):
            out, asum, dead = look(*xy)
            assert not out[:81].any() and dead[:81].all() and np.isfinite(out).all()
    out, _, dead = look(9.9e5, 2.0)
    assert not out.any() and dead.all()
    out, _, _ = look(-0.0, 2.0)
    assert out[(4 + 3) * 9 + 4, 0] == 1.0                                          # -0.0 is 0: a = 7 reaches x = 3
    out, _, _ = look(-1.0, 2.0)
    assert out[8 * 9 + 4, 0] == 1.0
    lv1 = [np.ones((1, 8, 8)), np.ones((1, 4, 4)), np.ones((1, 2, 2)), np.ones((1, 1, 1))]
    out, _, dead = cc.lookup(lv1, np.array([[0.0], [0.0]], np.float32))            # a 1-cell level is defined: the oracle is NaN there
    assert out[3 * 81 + 4 * 9 + 4, 0] == 1.0 and out[3 * 81 + 3 * 9 + 4, 0] == 0.0 and dead[3 * 81 + 2 * 9 + 4, 0] and np.isfinite(out).all()


# ---- decoders and geometry ------------------------------------------------------------------------------------------------------------------
def _encode_rows(cells, dtype, B, pairs, pitch, pair_stride, base, total):
    """Independent of decode_rows: a Python loop over every cell, addressed by the header's sentence."""
    buf = np.full(total, np.nan, dtype)
    n_img, N, hl, wl = cells.shape
    for b in range(B):
        for t in range(pairs):
            for i in range(N):
                start = base + t * pair_stride + (b * N + i) * hl * pitch
                for y in range(hl):
                    for x in range(wl):
                        buf[start + y * pitch + x] = cells[b * pairs + t, i, y, x]
    return buf


@pytest.mark.parametrize("layout", ["dense_f32", "dense_f16", "pitched_f32"])
def test_row_decoders_invert_an_independent_encoder(layout):
    h, w, B, pairs, N = 9, 10, 2, 2, 12                                            # (N need not be h * w for the addressing rule)
    rng = np.random.default_rng(1)
    dtype = np.float16 if layout == "dense_f16" else np.float32
    for l in range(4):
        hl, wl = h >> l, w >> l
        pitch = wl + 3 if layout == "pitched_f32" else wl
        cells = rng.standard_normal((B * pairs, N, hl, wl)).astype(dtype)
        pair_stride, base = B * N * hl * pitch + 5, 3
        raw = _encode_rows(cells, dtype, B, pairs, pitch, pair_stride, base, base + pairs * pair_stride).view(np.uint8)
        dec = {"dense_f32": cc.decode_dense_f32, "dense_f16": cc.decode_dense_f16}.get(layout)
        got = (dec(raw, B, pairs, N, hl, wl, pair_stride, base) if dec else cc.decode_pitched_f32(raw, B, pairs, N, hl, wl, pitch, pair_stride, base))
        assert np.array_equal(got, cells.astype(np.float64))


def _encode_blocked(levels, f32cells, n_img, h, w, img_stride):
    """Cell by cell from the header: record of rec_bytes per source pixel, level l at lvl_off[l], block (by, bx) at (by * nbx + bx) * 128,
    fp16: blocks of 8 x 8, cell at byte ((tx % 8) * 8 + ty % 8) * 2; fp32: blocks of 4 rows x 8 columns, byte ((tx % 8) * 4 + ty % 4) * 4."""
    rows, es = (4, 4) if f32cells else (8, 2)
    nby = [-(-(h >> l) // rows) for l in range(4)]
    nbx = [-(-(w >> l) // 8) for l in range(4)]
    off = [0]
    for l in range(4):
        off.append(off[-1] + nby[l] * nbx[l] * 128)
    rec = off[4]
    raw = np.full(n_img * img_stride, 0xFF, np.uint8)
    for l in range(4):
        v = levels[l].astype(np.float32 if f32cells else np.float16)
        for img in range(n_img):
            for i in range(h * w):
                for ty in range(h >> l):
                    for tx in range(w >> l):
                        at = img * img_stride + i * rec + off[l] + ((ty // rows) * nbx[l] + tx // 8) * 128 + ((tx % 8) * rows + ty % rows) * es
                        raw[at: at + es] = v[img, i, ty, tx: tx + 1].view(np.uint8)
    return raw, rec


@pytest.mark.parametrize("f32cells", [False, True])
def test_blocked_decoders_invert_an_independent_encoder(f32cells):
    h, w, n_img = 9, 17, 2
    rng = np.random.default_rng(2)
    g = cc.blocked_geometry(h, w, f32cells)
    stride = g["src_rows"] * g["rec_bytes"] + 256
    levels = [rng.standard_normal((n_img, h * w, h >> l, w >> l)).astype(np.float16).astype(np.float64) for l in range(4)]
    raw, rec = _encode_blocked(levels, f32cells, n_img, h, w, stride)
    assert rec == g["rec_bytes"]
    for a, b in zip(cc.decode_blocked(raw, f32cells, n_img, h, w, stride), levels):
        assert np.array_equal(a, b)
    mask = cc.blocked_data_mask(n_img, h, w, f32cells, stride)
    assert (raw[~mask] == 0xFF).all() and mask.sum() == n_img * h * w * sum((h >> l) * (w >> l) for l in range(4)) * (4 if f32cells else 2)


@pytest.mark.parametrize("h,w", cc.GRIDS)
def test_geometry_invariants(h, w):
    for f32cells in (False, True):
        g = cc.blocked_geometry(h, w, f32cells)
        rows = 4 if f32cells else 8
        for l in range(4):
            assert (g["nby"][l] - 1) * rows < (h >> l) <= g["nby"][l] * rows and (g["nbx"][l] - 1) * 8 < (w >> l) <= g["nbx"][l] * 8
            end = g["lvl_off"][l] + g["nby"][l] * g["nbx"][l] * 128
            assert end == (g["lvl_off"][l + 1] if l < 3 else g["rec_bytes"])         # ascending, back to back, no overlap
            cb = cc.blocked_cell_bytes(h, w, f32cells, l)
            assert cb.min() >= g["lvl_off"][l] and cb.max() + (4 if f32cells else 2) <= end and len(np.unique(cb)) == cb.size
        assert g["lvl_off"][0] == 0 and g["rec_bytes"] % 128 == 0 and g["src_rows"] % 128 == 0 and 0 <= g["src_rows"] - h * w < 128
        assert cc.blocked_bytes(3, h, w, f32cells) == 3 * g["src_rows"] * g["rec_bytes"]
    assert cc.build_ws_bytes(2, 3, 40, h, w) == 2 * 6 * 64 * h * w * 4 and cc.blocked32_ws_bytes(6, 40, h, w) == cc.build_ws_bytes(2, 3, 40, h, w)
    assert cc.blocked_ws_bytes(6, 40, h, w) == 12 * 32 * (h * w // 8 + 1) * 8 * 16


# ---- rounding models inside half the bound; bounds under the caps -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_models_inside_half_the_bound_and_bounds_under_the_caps(case):
    h, w = case["h"], case["w"]
    pairs = sorted({(0, 0), (case["B"] - 1, case["pairs"] - 1)})
    for b, t in pairs:
        f1, f2 = _pair(case["id"], b, t)
        for K in _klasses(case):
            bound, exact = cc.build_bound(f1, f2, h, w, K)
            mod = cc.model(f1, f2, h, w, K)
            for l in range(4):
                r = float((np.abs(mod[l] - exact[l]) / bound[l]).max())
                assert r <= 0.5, (K, l, r)
                assert (bound[l] <= cc.build_cap(exact[l], K)).all(), (K, l, float((bound[l] / cc.build_cap(exact[l], K)).max()))
        # the lookup on the model's own stored cells: an fp32 evaluation in the kernels' order against the float64 one
        for K in (cc.klass("x3"), cc.klass("f16")):
            cells = cc.model(f1, f2, h, w, K)
            xy = cc.coords(case)[b * case["pairs"] + t]
            ref, asum, dead = cc.lookup(cells, xy)
            assert (cc.lookup_bound(asum) <= cc.CAP_LOOKUP).all() and np.isfinite(ref).all() and not ref[dead].any()
            assert float((np.abs(_lookup32(cells, xy) - ref) / cc.lookup_bound(asum)).max()) <= 0.5


def _lookup32(levels, xy):
    """The lookup with every operation rounded to fp32 (the order of corr_lookup_kernel: four weights, four products, three additions)."""
    f = np.float32
    N = xy.shape[1]
    out = np.zeros((324, N), f)
    pix = np.arange(N)
    for l, m in enumerate(levels):
        hl, wl = m.shape[1:]
        c = xy.astype(f) * f(2.0 ** -l)
        c = np.where((c > f(-1.0e6)) & (c < f(1.0e6)), c, f(-1.0e6)).astype(f)
        c0 = np.floor(c)
        fx, fy = (c[0] - c0[0]).astype(f), (c[1] - c0[1]).astype(f)
        x0, y0 = c0[0].astype(np.int64), c0[1].astype(np.int64)
        P = np.zeros((N, hl + 2, wl + 2), f)
        P[:, 1:-1, 1:-1] = m
        wts = ((f(1) - fx) * (f(1) - fy), fx * (f(1) - fy), (f(1) - fx) * fy, fx * fy)
        for a in range(9):
            for b in range(9):
                acc = None
                for (dy, dx), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), wts):
                    v = P[pix, np.clip(y0 + b - 4 + dy, -1, hl) + 1, np.clip(x0 + a - 4 + dx, -1, wl) + 1] * wt
                    acc = v if acc is None else acc + v
                out[l * 81 + a * 9 + b] = acc
    return out.astype(np.float64)


# ---- wrong kernels ---------------------------------------------------------------------------------------------------------------------------
def _worst(got, exact, bound):
    """Largest |got - exact| / bound; a cell that was never written (NaN) is infinitely far."""
    r = np.abs(got - exact) / bound
    return float(np.where(np.isnan(r), np.inf, r).max())


def _build(case, K, b=0, t=0, wrong=None, f2_pair=None):
    h, w = case["h"], case["w"]
    f1, f2 = _pair(case["id"], b, t)
    if f2_pair is not None:
        f2 = _pair(case["id"], b, f2_pair)[1]
    bound, exact = cc.build_bound(f1, _pair(case["id"], b, t)[1], h, w, K)
    return cc.model(f1, f2, h, w, K, wrong=wrong), exact, bound


def _lookup_mutation(case, wrong):
    cells = cc.model(*_pair(case["id"]), case["h"], case["w"], cc.klass("x3"))
    xy = cc.coords(case)[0]
    ref, asum, _ = cc.lookup(cells, xy)
    return _worst(cc.lookup(cells, xy, wrong=wrong)[0], ref, cc.lookup_bound(asum))


def test_wrong_window_axes_swapped():
    assert _lookup_mutation(_case(8, 8), "swap_ab") > 10               # (8, 8): the smallest grid; any grid shows it


def test_wrong_fourth_tap_dropped():
    assert _lookup_mutation(_case(8, 8), "drop_tap4") > 10             # (8, 8)


def test_wrong_taps_outside_clamped():
    assert _lookup_mutation(_case(8, 8), "clamp") > 10                 # (8, 8)


def test_wrong_ceil_pooling():
    """(8, 9): the smallest grid with an odd size.  Ceil pooling makes level 1 five cells wide: written densely, read back with the
    header's four."""
    c = _case(8, 9)
    K = cc.klass("x3")
    mod, exact, bound = _build(c, K, wrong="ceil_pool")
    assert mod[1].shape[1:] == (4, 5)
    raw = np.ascontiguousarray(mod[1].astype(np.float32)).view(np.uint8).reshape(-1)
    got = cc.decode_dense_f32(raw[: 72 * 4 * 4 * 4], 1, 1, 72, 4, 4)
    assert _worst(got[0], exact[1], bound[1]) > 10


def test_wrong_level2_from_level0_with_a_shifted_origin():
    c = _case(8, 9)                                                    # (8, 9): the smallest grid with a column to shift into
    mod, exact, bound = _build(c, cc.klass("x3"), wrong="shift_l2")
    assert _worst(mod[2], exact[2], bound[2]) > 10 and _worst(mod[1], exact[1], bound[1]) <= 0.5


def test_wrong_scale_one_over_d():
    c = _case(8, 8)                                                    # (8, 8), D = 256 (any D > 1 shows it)
    for name in ("fp32", "x3", "f16"):
        mod, exact, bound = _build(c, cc.klass(name), wrong="inv_d")
        assert _worst(mod[0], exact[0], bound[0]) > 10, name


def test_wrong_pair_index_on_f1_only():
    c = _case(8, 8)                                                    # (8, 8) runs pairs = 3: pair 1 with the f2 of pair 0
    assert c["pairs"] == 3
    mod, exact, bound = _build(c, cc.klass("x3"), t=1, f2_pair=0)
    assert _worst(mod[0], exact[0], bound[0]) > 10


def test_wrong_last_source_of_a_partial_tile_not_written():
    c = _case(8, 9)                                                    # (8, 9): N = 72, the smallest with N % 32 != 0
    assert (c["h"] * c["w"]) % 32 == 8
    mod, exact, bound = _build(c, cc.klass("x3"))
    for l in range(4):
        got = mod[l].copy()
        got[-1] = np.nan                                               # the prefill of the GPU test
        assert _worst(got, exact[l], bound[l]) > 10 and _worst(mod[l], exact[l], bound[l]) <= 0.5


def test_wrong_pad_cells_of_a_pitched_row_read_as_data():
    c = _case(8, 8)                                                    # (8, 8) at the pitch of 32
    mod, exact, bound = _build(c, cc.klass("x3"))
    pitched = np.zeros((64, 8, 32), np.float32)                        # the pad cells of level 0 hold 0 (targets outside the image)
    pitched[:, :, :8] = mod[0]
    raw = pitched.view(np.uint8).reshape(-1)
    right = cc.decode_pitched_f32(raw, 1, 1, 64, 8, 8, 32)[0]
    wrong = cc.decode_dense_f32(raw[: 64 * 64 * 4], 1, 1, 64, 8, 8)[0]
    assert _worst(right, exact[0], bound[0]) <= 0.5 and _worst(wrong, exact[0], bound[0]) > 10


def test_wrong_blocked_cell_order():
    c = _case(8, 8)                                                    # (8, 8): one block per level
    K = cc.klass("b16", c["D"], c["pairs"], False)
    mod, exact, bound = _build(c, K)
    g = cc.blocked_geometry(8, 8, False)
    raw, _ = _encode_blocked([m[None] for m in mod], False, 1, 8, 8, g["src_rows"] * g["rec_bytes"])
    assert _worst(cc.decode_blocked(raw, False, 1, 8, 8)[0][0], exact[0], bound[0]) <= 0.5
    assert _worst(cc.decode_blocked(raw, False, 1, 8, 8, wrong="cell_order")[0][0], exact[0], bound[0]) > 10


def test_wrong_single_product_build_is_beyond_the_cross_layout_limits():
    """(8, 8), D = 256, unit-normal features as tests/test_gpu_corr_kernels.py::test_cross_layout builds them: a blocked fp32 build with
    ONE fp16 product per k instead of the split is more than ten times the 2e-6 (cells) and 2e-5 (looked-up features) away from the
    F16X3 model -- and would be INSIDE both at the AMP scale of the other cases, which is why that test does not use it."""
    c = _case(8, 8)
    for amp, beyond in ((cc.CROSS_AMP, True), (cc.AMP, False)):
        f = cc.features(dict(c, amp=amp))
        right = cc.model(f[0, 0], f[0, 1], 8, 8, cc.klass("x3"))
        wrong = cc.model(f[0, 0], f[0, 1], 8, 8, cc.klass("x1"))
        xy = cc.coords(c)[0]
        dc = max(float(np.abs(a - b).max()) for a, b in zip(right, wrong))
        dl = float(np.abs(cc.lookup(right, xy)[0] - cc.lookup(wrong, xy)[0]).max())
        assert (dc > 10 * cc.CROSS_CELLS and dl > 10 * cc.CROSS_LOOKUP) if beyond else (dc < cc.CROSS_CELLS and dl < cc.CROSS_LOOKUP), (amp, dc, dl)
    # the fp16 rule: a blocked fp16 build with the folded scale applied twice is beyond one fp16 ulp at every cell that is not tiny
    f = cc.features(dict(c, amp=cc.CROSS_AMP))
    K = cc.klass("b16", 256, 3, True)
    dense, good, bad = (cc.model(f[0, 0], f[0, 1], 8, 8, k, wrong=w)[0] for k, w in ((cc.klass("f16"), None), (K, None), (K, "fold_twice")))
    assert (np.abs(dense - good) <= cc.cross_f16_ulp(dense)).all() and (np.abs(dense - bad) > 10 * cc.cross_f16_ulp(dense)).any()


def test_wrong_folded_scale_applied_twice():
    c = _case(8, 8)                                                    # (8, 8), D = 256: folded both shared (1/4, 1/4) and not (1/16)
    for shared in (False, True):
        K = cc.klass("b16", c["D"], c["pairs"], shared)
        assert K["pa"] != 1.0 and K["shared"] == shared
        mod, exact, bound = _build(c, K, wrong="fold_twice")
        assert _worst(mod[0], exact[0], bound[0]) > 10
