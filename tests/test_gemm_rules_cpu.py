"""CPU: what sf_gemm and sf_splitk_combine must refuse before any launch (dummy, never dereferenced pointers), and that the
case lists of tests/test_gpu_gemm_descriptors.py reach every kernel branch they are meant to."""
import ctypes
import os

import pytest

from tests import gemm_cases as gc


@pytest.fixture(scope="module")
def lib():
    from streamflow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def _desc(prec, **kw):
    from streamflow_amd import _lib
    g = _lib.SfGemm()
    g.A, g.B, g.C = 4096, 8192, 16384
    g.M, g.N, g.K, g.batch = 128, 300, 1000, 1
    g.lda, g.ldb, g.ldc = 1000, 1000, 300
    g.a_layout, g.b_layout = _lib.LAYOUT_K_MINOR, _lib.LAYOUT_K_MINOR
    g.alpha, g.precision = 1.0, prec
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _refused(lib, g, msg):
    rc = lib.sf_gemm(ctypes.byref(g), None)
    err = lib.sf_last_error().decode()
    assert rc != 0 and msg in err, (rc, err)


def test_layout_pairs_refused_where_no_kernel_is_built(lib):
    from streamflow_amd import _lib
    precs = {"fp32": _lib.PRECISION_FP32, "f16x3": _lib.PRECISION_F16X3, "f16x2": _lib.PRECISION_F16X2, "f16": _lib.PRECISION_F16}
    for name, p in precs.items():
        for pair in gc.PAIRS:
            for M in (128, 64, 31):
                msg = gc.refusal(name, pair, M, 300, 1)
                if msg is not None:
                    _refused(lib, _desc(p, M=M, a_layout=pair[0], b_layout=pair[1], lda=1000 if pair[0] else M), msg)


def test_caller_split_k_rules(lib):
    from streamflow_amd import _lib
    for p in (_lib.PRECISION_F16X3, _lib.PRECISION_F16X2, _lib.PRECISION_F16):
        _refused(lib, _desc(p, k_splits=17, split_stride=128 * 300), "k_splits <= 16")
        _refused(lib, _desc(p, k_splits=2, split_stride=128 * 300, bias=4096), "split-K needs SF_EPI_NONE, no bias")
        for epi in range(1, gc.N_EPI):
            _refused(lib, _desc(p, k_splits=3, split_stride=128 * 300, epilogue=epi, R=4096, gamma=4096, dw_w=4096, dw_b=4096),
                     "split-K needs SF_EPI_NONE")
    _refused(lib, _desc(_lib.PRECISION_FP32, k_splits=2, split_stride=128 * 300), "split-K is only built for the split-precision")


def test_splitk_combine_alignment_rules(lib):
    base = dict(partial=4096, split_stride=4096, k_splits=3, part_img_stride=1024, R=8192, r_img_stride=1024, gamma=64,
                out=16384, out_img_stride=1024, n_img=2, floats_per_img=1024)
    for k, v in (("floats_per_img", 1022), ("split_stride", 4098), ("part_img_stride", 1025), ("r_img_stride", 1026),
                 ("out_img_stride", 1027), ("partial", 4100), ("R", 8196), ("out", 16392)):
        a = dict(base, **{k: v})
        rc = lib.sf_splitk_combine(a["partial"], a["split_stride"], a["k_splits"], a["part_img_stride"], a["R"], a["r_img_stride"],
                                   a["gamma"], a["out"], a["out_img_stride"], a["n_img"], a["floats_per_img"], None)
        assert rc != 0 and b"16-byte aligned" in lib.sf_last_error(), k
    for k in ("k_splits", "n_img", "floats_per_img"):
        a = dict(base, **{k: 0})
        rc = lib.sf_splitk_combine(a["partial"], a["split_stride"], a["k_splits"], a["part_img_stride"], a["R"], a["r_img_stride"],
                                   a["gamma"], a["out"], a["out_img_stride"], a["n_img"], a["floats_per_img"], None)
        assert rc != 0 and b"bad args" in lib.sf_last_error(), k


def test_library_split_k_scratch_sizes(lib):
    """sf_gemm_split_ws_floats: positive exactly where the descriptor tests expect a split, zero for grids that fill the chip or
    for short K chains."""
    for M, N, K, batch in gc.AUTO_SPLIT_SHAPES:
        ws = lib.sf_gemm_split_ws_floats(M, N, K, batch)
        assert ws > 0 and ws % (batch * M * N) == 0 and 2 <= ws // (batch * M * N) <= 16, (M, N, K, ws)
    assert lib.sf_gemm_split_ws_floats(64, 196, 8192, 1) == 16 * 64 * 196          # the sr convolutions: the 16-split cap
    assert lib.sf_gemm_split_ws_floats(128, 300, 224, 1) == 0                       # 7 k-tiles: too short to split
    assert lib.sf_gemm_split_ws_floats(256, 128 * 50, 1024, 1) == 0                 # 100 workgroups: the grid is full enough


def test_descriptor_cases_cover_every_branch():
    """Every (precision, layout pair, epilogue) runs or is refused, and every accepted (precision, pair) reaches each tile height
    it has a kernel for (the stored-fp16 B: the 128-row tile only)."""
    cases = [c for _, c in gc.raw_cases()]
    seen = {(c["prec"], c["pair"], c["epi"]) for c in cases if c["refused"] is None}
    refused = {(c["prec"], c["pair"]) for c in cases if c["refused"] is not None}
    tiles = {}
    for c in cases:
        if c["refused"] is None:
            tiles.setdefault((c["prec"], c["pair"]), set()).add(gc.tile_rows(c["prec"], c["M"], c["N"], c["batch"]))
    for prec in gc.PRECS:
        for pair in gc.PAIRS:
            if (prec, pair) in tiles:
                assert all((prec, pair, e) in seen for e in range(gc.N_EPI)), (prec, pair)
                want = {128} if pair[1] == 3 else {32, 64, 128}
                assert tiles[(prec, pair)] == want, (prec, pair, tiles[(prec, pair)])
            else:
                assert (prec, pair) in refused, (prec, pair)
    assert any(c["unaligned"] for c in cases) and any(not c["unaligned"] for c in cases)
    assert {k for k, _, _, _, _, _ in gc.CALLER_SPLIT_CASES} == {2, 3, 4, 16}
    assert any(M * N > 1 << 20 for _, _, M, N, _, _ in gc.CALLER_SPLIT_CASES)
