"""CPU: what tests/corr_direct_cases.py states -- the direct formulation is the volume's mathematics, the rounding models of both
classes lie inside half the derived bound on every case and coordinate set, the bound stays under the suite's cap, wrong kernels lie
outside it -- and the host side of the volume-free route: the workspace size restated, engine.resolve_corr's truth table and the two
new EngineOptions fields through SF_ENGINE_OPTS."""
import os

import numpy as np
import pytest

from tests import corr_cases as cc
from tests import corr_direct_cases as dc

CASES = dc.cases()
IDS = [c["id"] for c in CASES]


def _ratio(got, ref, k):
    return float((np.abs(got - ref["out"]) / ref["bound"][k]).max())


def test_case_and_coordinate_sets():
    assert [c["id"] for c in CASES] == [c["id"] for c in cc.cases()] and len(CASES) == 13
    for case in CASES:
        h, w, N = case["h"], case["w"], case["h"] * case["w"]
        assert np.array_equal(dc.coords(case, "noise"), cc.coords(case), equal_nan=True)
        u = dc.coords(case, "uniform")
        assert u.shape == (case["B"] * case["pairs"], 2, N) and u[:, 0].min() >= -8 and u[:, 0].max() < w + 8 and u[:, 1].max() < h + 8
        d = dc.coords(case, "dead_tile")[:, :, dc.TILE: 2 * dc.TILE]
        assert (np.isnan(d[:, 0]) | (d[:, 0] > w + 9)).all()
        c = dc.coords(case, "corner")[:, :, : dc.TILE]
        assert (c[:, 0, 5] > w - 2).all() and (np.delete(c[:, 0], 5, axis=1) < 8).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_features_pooled_equal_volume_pooled(case):
    F = cc.features(case)
    for b in range(case["B"]):
        for t in range(case["pairs"]):
            a = dc.feature_pyramid(F[b, t], F[b, t + 1], case["h"], case["w"])
            v = cc.pyramid(F[b, t], F[b, t + 1], case["h"], case["w"])
            for x, y in zip(a, v):
                assert x.shape == y.shape and np.abs(x - y).max() <= 1e-12


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_models_inside_half_the_bound_and_bounds_under_the_cap(case):
    for cs in dc.COORD_SETS:
        ref = dc.reference(case["id"], cs)
        # every tap outside: the reference is exactly zero there (and on a whole tile of dead pixels)
        assert (ref["out"][ref["dead"]] == 0).all()
        if cs == "dead_tile":
            assert ref["dead"][:, :, dc.TILE: 2 * dc.TILE].all()
        for k in dc.KLASSES:
            assert ref["bound"][k].max() < cc.CAP_LOOKUP, (cs, k, ref["bound"][k].max())
            assert _ratio(dc.model_out(ref, k), ref, k) <= 0.5, (cs, k)


def _beyond(wrong=None, lookup_wrong=None, k="f16", sets=("noise",), amp=cc.AMP, model_k=None):
    """The largest error / bound of a wrong kernel over the cases."""
    worst = 0.0
    for case in CASES:
        for cs in sets:
            ref = dc.reference(case["id"], cs, amp)
            worst = max(worst, _ratio(dc.model_out(ref, model_k or k, wrong, lookup_wrong), ref, k))
    return worst


@pytest.mark.parametrize("k", list(dc.KLASSES))
@pytest.mark.parametrize("lookup_wrong", ["swap_ab", "drop_tap4", "clamp"])
def test_wrong_lookups_are_outside_the_bound(lookup_wrong, k):
    assert _beyond(lookup_wrong=lookup_wrong, k=k) > 1.0


@pytest.mark.parametrize("k", list(dc.KLASSES))
@pytest.mark.parametrize("wrong", ["inv_d", "ceil_pool", "stride"])
def test_wrong_cells_are_outside_the_bound(wrong, k):
    assert _beyond(wrong=wrong, k=k) > 1.0


def test_wrong_pooled_features_rounded_at_every_level():
    """One fp16 rounding per level instead of one in all: outside the bound of the fp16 class where nothing averages out (D = 1).  In
    the split class the extra roundings are 2^-9 of these and stay inside (0.6 of the bound at most): not distinguishable there."""
    assert _beyond(wrong="round_each", k="f16") > 1.0
    assert _beyond(wrong="round_each", k="x3") <= 1.0


def test_wrong_single_product_in_the_split_class():
    """One fp16 product per k where the class promises three: beyond the split class's bound at unit-normal features."""
    one = [c for c in CASES if c["id"] == "8x8-D256-B1p3"][0]
    ref = dc.reference(one["id"], "noise", cc.CROSS_AMP)
    assert _ratio(dc.model_out(ref, "f16"), ref, "x3") > 1.0
    assert _ratio(dc.model_out(ref, "x3"), ref, "x3") <= 0.5


# ---- host side ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from streamflow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_ws_bytes_restated(lib):
    for case in CASES:
        for K in dc.KLASSES.values():
            args = (case["B"], case["pairs"], case["D"], case["h"], case["w"], K["precision"])
            assert lib.sf_corr_direct_ws_bytes(*args) == dc.ws_bytes(*args) > 0
    # Sintel's grid, D = 256, fp16 class: 1.33 N D halves per frame and side
    assert lib.sf_corr_direct_ws_bytes(1, 1, 256, 55, 128, cc.F16) == 256 * 2 * (2 * 7040 + 27 * 64 + 13 * 32 + 6 * 16)
    assert lib.sf_corr_direct_ws_bytes(1, 1, 256, 55, 128, cc.FP32) == 0 and lib.sf_corr_direct_ws_bytes(1, 1, 256, 7, 128, cc.F16) == 0


def test_resolve_corr_truth_table():
    from streamflow_amd import ops
    from streamflow_amd.engine import EngineOptions, resolve_corr
    split = (ops.PRECISION_F16X3, ops.PRECISION_F16X2, ops.PRECISION_F16)
    for prec in split + (ops.PRECISION_FP32,):
        for f16 in (False, True):
            for P in (64, 7040, 32640, 129600):
                assert resolve_corr(EngineOptions(), prec, f16, P) == "volume"                     # the defaults: never
                assert resolve_corr(EngineOptions(corr_direct=False, corr_direct_min_px=0), prec, f16, P) == "volume"
    for prec in split:
        for f16 in (False, True):
            assert resolve_corr(EngineOptions(corr_direct=True), prec, f16, 64) == "direct"
            o = EngineOptions(corr_direct_min_px=7040)
            assert [resolve_corr(o, prec, f16, P) for P in (7039, 7040, 32640)] == ["volume", "direct", "direct"]
            assert resolve_corr(EngineOptions(corr_direct=True, corr_direct_min_px=1 << 30), prec, f16, 64) == "direct"
    with pytest.raises(RuntimeError, match="corr_direct"):
        resolve_corr(EngineOptions(corr_direct=True), ops.PRECISION_FP32, False, 7040)
    with pytest.raises(RuntimeError, match="corr_direct"):
        resolve_corr(EngineOptions(corr_direct_min_px=4096), ops.PRECISION_FP32, False, 7040)
    assert resolve_corr(EngineOptions(corr_direct_min_px=4096), ops.PRECISION_FP32, False, 4095) == "volume"


def test_engine_options_from_env(monkeypatch):
    from streamflow_amd.engine import EngineOptions
    assert (EngineOptions().corr_direct, EngineOptions().corr_direct_min_px) == (False, 0)
    monkeypatch.setenv("SF_ENGINE_OPTS", "corr_direct=1,corr_direct_min_px=4096")
    o = EngineOptions.from_env()
    assert o.corr_direct is True and o.corr_direct_min_px == 4096
    assert o == EngineOptions(corr_direct=True, corr_direct_min_px=4096)
    monkeypatch.setenv("SF_ENGINE_OPTS", "corr_direct=0")
    assert EngineOptions.from_env(EngineOptions(corr_direct=True)).corr_direct is False


def test_public_surface_takes_the_route():
    from streamflow_amd import demo, default_args
    assert default_args().corr is None and default_args(corr="direct").corr == "direct"
    assert demo.arg_parser().parse_args(["--frames", "f", "--ckpt", "c", "--corr", "direct"]).corr == "direct"
    assert demo.arg_parser().parse_args(["--frames", "f", "--ckpt", "c"]).corr is None
    with pytest.raises(SystemExit):
        demo.arg_parser().parse_args(["--frames", "f", "--ckpt", "c", "--corr", "rows"])
