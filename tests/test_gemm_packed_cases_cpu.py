"""CPU: the case lists of tests/test_gpu_gemm_packed.py against the library's own dispatch.  sf_gemm_route runs sf_gemm's
validation and dispatch code with every launch site answering instead of launching, so it is safe with dummy pointers; sf_gemm
itself is called here for REFUSED descriptors only (it would launch an accepted one on a machine with a GPU).
  * the route of every case equals the Python restatement in tests/gemm_packed_cases.py (rules that drift apart fail here);
  * the accepted cases reach every kernel branch the GPU file is meant to run;
  * every refusal returns its code and message, from sf_gemm_route and from sf_gemm alike;
  * the float64 reference of the GPU file is sharp: a numpy model of the documented arithmetic stays within half the tolerance,
    models with one documented property wrong exceed twice the tolerance."""
import ctypes
import os

import numpy as np
import pytest

from tests import gemm_packed_cases as pc


@pytest.fixture(scope="module")
def lib():
    from streamflow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def make_gemm(d):
    """SfGemm from the fields of gemm_packed_cases.descriptor()."""
    from streamflow_amd import _lib
    g = _lib.SfGemm()
    names = {n for n, _ in _lib.SfGemm._fields_}
    for k, v in d.items():
        if k in names:
            setattr(g, k, v)
    return g


def lib_route(lib, d):
    """("ok", {field: value}) / ("refused", code, message) from sf_gemm_route."""
    from streamflow_amd import _lib
    r = _lib.SfGemmRoute()
    rc = lib.sf_gemm_route(ctypes.byref(make_gemm(d)), ctypes.byref(r))
    if rc != 0:
        return "refused", rc, lib.sf_last_error().decode()
    assert (r.a_layout, r.b_layout) == (d["a_layout"], d["b_layout"])
    return "ok", {n: getattr(r, n) for n in ("family", "tile_rows", "products", "nks", "res", "msplit", "n_main", "k_splits")}


def test_constants_match_the_binding():
    from streamflow_amd import _lib
    assert (pc.K_MAJOR, pc.SPLIT_F16, pc.F16_K_MAJOR, pc.F16_KOCT) == (_lib.LAYOUT_K_MAJOR, _lib.LAYOUT_SPLIT_F16, _lib.LAYOUT_F16_K_MAJOR,
                                                                     _lib.LAYOUT_F16_KOCT)
    assert (pc.F16X3, pc.F16X2, pc.F16) == (_lib.PRECISION_F16X3, _lib.PRECISION_F16X2, _lib.PRECISION_F16)
    assert (pc.NONE, pc.GELU, pc.RELU, pc.RES, pc.RES_GELU, pc.DW1, pc.AXPY) == (
        _lib.EPI_NONE, _lib.EPI_GELU, _lib.EPI_RELU, _lib.EPI_RES, _lib.EPI_RES_GELU, _lib.EPI_RES_GELU_DW1, _lib.EPI_AXPY)
    assert (pc.AUTO, pc.TILED, pc.BSTAT) == (_lib.ALGO_AUTO, _lib.ALGO_TILED, _lib.ALGO_BSTAT)
    assert (pc.FP32_TILED, pc.SPLIT_TILED, pc.KOCT_DMA, pc.BDIRECT, pc.FAM_BSTAT, pc.FAM_BSTAT_GELU) == (
        _lib.GEMM_FP32_TILED, _lib.GEMM_SPLIT_TILED, _lib.GEMM_KOCT_DMA, _lib.GEMM_BDIRECT, _lib.GEMM_BSTAT, _lib.GEMM_BSTAT_GELU)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "streamflow_hip.h")).read()
    for i, name in enumerate(("FP32_TILED", "SPLIT_TILED", "KOCT_DMA", "BDIRECT", "BSTAT", "BSTAT_GELU")):
        assert "SF_GEMM_FAMILY_%s = %d" % (name, i + 1) in hdr, name
    assert ctypes.sizeof(_lib.SfGemmRoute) == 40


def test_route_query_leaves_out_alone_when_it_refuses_and_needs_out(lib):
    from streamflow_amd import _lib
    c, code, msg = pc.refusals()[0]
    r = _lib.SfGemmRoute()
    r.family = r.nks = 77
    assert lib.sf_gemm_route(ctypes.byref(make_gemm(pc.descriptor(c))), ctypes.byref(r)) == code
    assert (r.family, r.nks) == (77, 77)
    assert lib.sf_gemm_route(ctypes.byref(make_gemm(pc.descriptor(pc.cases()[0]))), None) == pc.BAD_ARG
    assert b"sf_gemm_route" in lib.sf_last_error()
    assert lib.sf_gemm_route(None, ctypes.byref(r)) == pc.BAD_ARG and b"null descriptor" in lib.sf_last_error()
    # an fp32 descriptor: the exact-fp32 tiles
    g = _lib.SfGemm()
    g.A, g.B, g.C, g.M, g.N, g.K, g.batch, g.lda, g.ldb, g.ldc, g.alpha = 4096, 8192, 16384, 300, 5120, 31, 2, 300, 5120, 5120, 1.0
    assert lib.sf_gemm_route(ctypes.byref(g), ctypes.byref(r)) == 0
    assert (r.family, r.products, r.a_layout, r.b_layout, r.k_splits) == (_lib.GEMM_FP32_TILED, 1, 0, 0, 0) and r.tile_rows in (32, 64, 128)


def test_route_equals_the_restatement_for_every_case(lib):
    cases = pc.cases()
    assert len({c["id"] for c in cases}) == len(cases)
    for c in cases:
        d = pc.descriptor(c)
        want, got = pc.route(d), lib_route(lib, d)
        assert want[0] == "ok", (c["id"], want)
        assert got == want, (c["id"], got, want)


def test_accepted_cases_reach_every_branch(lib):
    seen, bstat, gk, msplit, c_forms, forms = set(), set(), set(), set(), set(), set()
    flags = set()
    for c in pc.cases():
        d = pc.descriptor(c)
        kind, r = lib_route(lib, d)
        assert kind == "ok", c["id"]
        fam, pm = r["family"], r["products"]
        seen.add((fam, c["lay"], r["tile_rows"], pm))
        c_forms.add((fam, c["lay"] if fam == pc.SPLIT_TILED else 0, c["c_f16"]))
        forms.add((fam, c["lay"] if fam == pc.SPLIT_TILED else 0, pm, c["c_f16"], c["r"]))
        if fam == pc.FAM_BSTAT:
            bstat.add((r["nks"], r["res"], pm))
        if fam == pc.FAM_BSTAT_GELU:
            gk.add((r["nks"], pm))
        if fam in (pc.FAM_BSTAT, pc.FAM_BSTAT_GELU):
            msplit.add(r["msplit"])
            if r["n_main"] > 0:
                flags.add("n_main")
            assert (r["n_main"] > 0) == (r["msplit"] == 1), c["id"]
            if d["b_group"]:
                flags.add("bstat-group-%d" % c["lay"])
            if d["b_layout"] == pc.F16_K_MAJOR and (d["N"] & 1 or d["ldb"] & 1 or d["strideB"] & 1):
                flags.add("bstat-odd-rows")
            if d["r_f16"] == 2:
                flags.add("bstat-r2-epi%d" % d["epilogue"])
        else:
            if d["b_group"]:
                flags.add("tiled-group-%d" % c["lay"])
            if c["c_f16"] == 2 and fam == pc.SPLIT_TILED:
                assert c["K"] <= 64 or c["K"] > 640 or c["prec"] == "f16x3", c["id"]
            if d["a_k_pad"] in (0, 32):
                flags.add("a_k_pad-%d-fam%d" % (d["a_k_pad"], fam))
        if d["r_group"]:
            flags.add("r_group-fam%d" % fam)
        if d["conv3x3"]:
            flags.add("conv-%d-%s" % (r["tile_rows"], c["prec"]))
        if r["k_splits"] > 1:
            flags.add("splitk-fam%d" % fam)
        if d["lda_h"] > pc.up(d["M"], 128):
            flags.add("lda_h-fam%d" % fam)
    for rows in (32, 64, 128):
        for pm in (1, 2, 3):
            assert (pc.SPLIT_TILED, 8, rows, pm) in seen, ("fp32 planes B", rows, pm)
        for pm in (1, 2):
            assert (pc.SPLIT_TILED, 12, rows, pm) in seen, ("fp16 rows B", rows, pm)
    for pm in (1, 2):
        assert (pc.KOCT_DMA, 13, 128, pm) in seen and (pc.BDIRECT, 13, 128, pm) in seen, pm
        for nks in (8, 16, 24, 32, 40):
            assert (nks, 0, pm) in bstat and (nks, pm) in gk, (nks, pm)
            assert ((nks, 1, pm) in bstat) == (nks <= 24), (nks, pm)
            assert ((nks, 2, pm) in bstat) == (nks <= 32), (nks, pm)
    assert msplit == {1, 2, 3, 4} and "n_main" in flags
    # every output form on every family that takes it (c_f16 = 2 on the register-staged tiles only at K <= 64 or K > 640)
    for fam, lay, cfs in ((pc.SPLIT_TILED, 8, (0, 1, 2, 3)), (pc.SPLIT_TILED, 12, (0, 1, 2, 3)), (pc.KOCT_DMA, 0, (0, 1, 2, 3)),
                            (pc.BDIRECT, 0, (0, 1, 2, 3)), (pc.FAM_BSTAT, 0, (0, 2, 3)), (pc.FAM_BSTAT_GELU, 0, (2,))):
        assert {f for a, b, f in c_forms if (a, b) == (fam, lay)} == set(cfs), (fam, lay)
    # ... and every (family, products, output form, residual format) the library accepts
    assert forms == pc.accepted_forms(), sorted(forms ^ pc.accepted_forms())
    want = {"bstat-group-8", "bstat-group-13", "tiled-group-8", "tiled-group-13", "r_group-fam%d" % pc.FAM_BSTAT,
            "r_group-fam%d" % pc.SPLIT_TILED, "splitk-fam%d" % pc.SPLIT_TILED, "splitk-fam%d" % pc.KOCT_DMA, "bstat-odd-rows",
            "conv-32-f16x3", "conv-64-f16x2", "conv-128-f16",
            "bstat-r2-epi%d" % pc.RES, "bstat-r2-epi%d" % pc.RES_GELU, "bstat-r2-epi%d" % pc.DW1, "bstat-r2-epi%d" % pc.AXPY,
            "lda_h-fam%d" % pc.SPLIT_TILED, "lda_h-fam%d" % pc.KOCT_DMA, "lda_h-fam%d" % pc.BDIRECT, "lda_h-fam%d" % pc.FAM_BSTAT,
            "lda_h-fam%d" % pc.FAM_BSTAT_GELU}
    for a_k_pad in (0, 32):
        want |= {"a_k_pad-%d-fam%d" % (a_k_pad, f) for f in (pc.SPLIT_TILED, pc.KOCT_DMA)}
    want.add("a_k_pad-32-fam%d" % pc.BDIRECT)
    assert want <= flags, sorted(want - flags)
    # the placements: every part-A combination in all three, and the unaligned one really moves something off 16 bytes
    a = [c for c in pc.cases() if c["part"] == "A"]
    assert len(a) % 3 == 0 and all(tuple(c["place"] for c in a[i:i + 3]) == pc.PLACES for i in range(0, len(a), 3))
    for c in a:
        d = pc.descriptor(c)
        if c["place"] == "unaligned" and c["lay"] != 13:
            assert d["B"] & 15, c["id"]
        if c["place"] != "dense":
            assert d["ldb"] > d["N"] and d["ldc"] > d["N"] and d["strideC"] > 0, c["id"]


def test_b_direct_threshold_cases(lib):
    """One tile column below SF_GEMM_BD_MIN_WG the same problem runs on the DMA tile; M = 192 never reaches either."""
    below = [c for c in pc.cases() if c["part"] == "B-below"]
    assert below
    for c in below:
        d = pc.descriptor(c)
        assert lib_route(lib, d)[1]["family"] == pc.KOCT_DMA
        n_wg2 = pc.cdiv(c["N"], 256) * pc.cdiv(c["M"], 128) * c["batch"]
        assert pc.BD_MIN_WG - pc.cdiv(c["M"], 128) * c["batch"] <= n_wg2 < pc.BD_MIN_WG
        up_ = dict(c, N=c["N"] + 256)
        assert lib_route(lib, pc.descriptor(up_))[1]["family"] == pc.BDIRECT
    m192 = [c for c in pc.cases() if c["part"] == "B-m192"]
    assert m192 and all(lib_route(lib, pc.descriptor(c))[1]["family"] == pc.FAM_BSTAT for c in m192)
    for c in (c for c in pc.cases() if c["part"] == "B-bdirect"):
        n_wg2 = pc.cdiv(c["N"], 256) * pc.cdiv(c["M"], 128) * c["batch"]
        assert n_wg2 == pc.BD_MIN_WG and c["N"] % 256, c["id"]                   # exactly at the threshold, ragged last tile


def test_every_refusal_is_pinned(lib):
    refs = pc.refusals()
    assert len({c["id"] for c, _, _ in refs}) == len(refs)
    for c, code, msg in refs:
        d = pc.descriptor(c)
        want = pc.route(d)
        got = lib_route(lib, d)
        assert got[0] == "refused" and got[1] == code and msg in got[2], (c["id"], got)
        assert want[0] == "refused" and want[1] == code and want[2] in got[2], (c["id"], want, got)
        # ... and sf_gemm itself says the same (a refused descriptor never launches)
        rc = lib.sf_gemm(ctypes.byref(make_gemm(d)), None)
        assert rc == code and lib.sf_last_error().decode() == got[2], (c["id"], rc)


def test_each_refusal_is_one_step_from_an_accepted_descriptor(lib):
    """A refusal case without its overrides (and with the base shape where the shape is the fault) is accepted or is refused for the
    property its name carries: the overrides alone must be what turns an accepted descriptor into a refused one."""
    n = 0
    for c, code, msg in pc.refusals():
        if not c["over"]:
            continue
        d = pc.descriptor(dict(c, over={}))
        assert lib_route(lib, d)[0] == "ok", c["id"]
        n += 1
    assert n >= 40


# ---- the reference is sharp -------------------------------------------------------------------------------------------------
def _sharp_inputs(M, K, N, seed):
    import torch
    from streamflow_amd.ops import PackedLinear
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(M, K, generator=g) / K ** 0.5
    X = torch.randn(K, N, generator=g)
    pk = PackedLinear(W, None, "cpu")
    hi = pk.hi.float().permute(1, 0, 2).reshape(pk.lda_h, -1)[:M, :K].numpy()
    lo = pk.lo.float().permute(1, 0, 2).reshape(pk.lda_h, -1)[:M, :K].numpy()
    return W.numpy(), X.numpy(), hi, lo, np.float32(pk.split_scale)


@pytest.mark.parametrize("prec", ["f16x3", "f16x2", "f16"])
def test_reference_is_sharp(prec):
    """The documented arithmetic (include/streamflow_hip.h SF_PRECISION_*): fp16 hi / lo images of split_scale * W, B rounded once to
    fp16 (f16x2, f16) or kept to ~22 bits (f16x3), fp32 accumulation, alpha / split_scale at the end."""
    M, K, N, alpha = 126, 100, 1000, 0.5
    W, X, hi, lo, s = _sharp_inputs(M, K, N, 77)
    tol = pc.TOL[prec]
    X16 = X.astype(np.float16).astype(np.float32)
    # the float64 reference of tests/test_gpu_gemm_packed.py (_operands of tests/test_gpu_gemm_descriptors.py)
    A64 = (W * s).astype(np.float16).astype(np.float64) / s if prec == "f16" else W.astype(np.float64)
    B64 = (X if prec == "f16x3" else X16).astype(np.float64)
    ref = alpha * (A64 @ B64)

    def model(with_lo, b_rounded):
        A = (hi + lo) if with_lo else hi                         # exact in fp32: 22 bits
        acc = A.astype(np.float32) @ (X16 if b_rounded else X)  # fp32 accumulation
        return (np.float32(alpha) / s * acc).astype(np.float64)

    err = lambda y: float(np.abs(y - ref).max())
    faithful = err(model(prec != "f16", prec != "f16x3"))
    assert faithful <= 0.5 * tol, (prec, faithful)
    wrong = {"lo dropped" if prec != "f16" else "lo included": err(model(prec == "f16", prec != "f16x3")),
             "B not rounded" if prec != "f16x3" else "B rounded": err(model(prec != "f16", prec == "f16x3"))}
    for name, e in wrong.items():
        assert e >= 2.0 * tol, (prec, name, e)


def test_fp16_result_tolerance_is_sharp():
    """fp16 results are held to 2^-11 * 1.01 |ref| + 8e-5 (one rounding + the polynomial GELU): a result rounded twice, or with the lo
    product dropped before the rounding, breaks it at some element."""
    M, K, N = 126, 100, 1000
    W, X, hi, lo, s = _sharp_inputs(M, K, N, 78)
    X16 = X.astype(np.float16).astype(np.float32)
    ref = W.astype(np.float64) @ X16.astype(np.float64)
    bound = 2.0 ** -11 * 1.01 * np.abs(ref) + 8e-5
    good = ((hi + lo) @ X16 / s).astype(np.float16).astype(np.float64)
    assert bool((np.abs(good - ref) <= 0.5 * bound + 2.0 ** -12 * np.abs(ref)).all())
    assert bool((np.abs(good - ref) <= bound).all())
    no_lo = (hi @ X16 / s).astype(np.float16).astype(np.float64)
    assert bool((np.abs(no_lo - ref) > 2.0 * bound).any())
