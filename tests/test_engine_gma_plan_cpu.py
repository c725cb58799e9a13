"""CPU: the decision table of engine.resolve_gma -- which of the five GMA forms (matrix, chunked, recompute, stored, hybrid) a plan
runs, for which images, and with which split-K.  The function calls the library's host sizing functions only, no device.  Cases are
(images, pixels); default EngineOptions and an available v projection unless a case says otherwise."""
import os
from dataclasses import replace

import pytest

from streamflow_amd import ops
from streamflow_amd.engine import EngineOptions, resolve_gma

SPLIT, FP32 = ops.PRECISION_F16X3, ops.PRECISION_FP32
FUSED_MODES = ("flash", "stored", "hybrid")


@pytest.fixture(scope="module", autouse=True)
def lib():
    from streamflow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def resolve(mode, n, P, precision=SPLIT, products=1, project_ok=True, **opts):
    return resolve_gma(mode, precision, products, EngineOptions(**opts), n, P, project_ok)


@pytest.mark.parametrize("n, P", [(4, 384), (2, 357), (3, 32400)])
def test_flash_with_split_logits_stores_the_weights_at_every_grid(n, P):
    g = resolve("flash", n, P, products=3)
    assert (g.form, g.n_store, g.auto_stored, g.attn_rows) == ("stored", n, True, 1)


FLASH_ONE_PRODUCT = [((4, 384), "recompute"), ((18, 7040), "recompute"), ((2, 16380), "recompute"),
                     ((2, 16384), "stored"), ((3, 32400), "stored")]


@pytest.mark.parametrize("grid, form", FLASH_ONE_PRODUCT)
def test_flash_with_one_product_stores_from_stored_auto_px_on(grid, form):
    n, P = grid
    g = resolve("flash", n, P)
    assert (g.form, g.n_store, g.auto_stored) == (form, n if form == "stored" else 0, form == "stored")
    assert g == resolve("flash", n, P, precision=ops.PRECISION_F16X2)         # every split precision decides alike
    off = resolve("flash", n, P, stored_auto_px=0)
    assert (off.form, off.n_store, off.auto_stored) == ("recompute", 0, False)


def test_stored_mode_and_flash_stats():
    g = resolve("stored", 4, 384)
    assert (g.form, g.n_store, g.auto_stored) == ("stored", 4, False)
    g = resolve("stored", 4, 384, flash_stats=False)
    assert (g.form, g.n_store, g.auto_stored) == ("recompute", 0, False)


@pytest.mark.parametrize("grid, form, n_store", [((18, 7040), "hybrid", 9), ((6, 7040), "recompute", 0), ((3, 7040), "recompute", 0),
                                                 ((4, 384), "hybrid", 2), ((2, 357), "hybrid", 1)])
def test_hybrid_splits_the_batch_where_neither_half_needs_the_key_split(grid, form, n_store):
    g = resolve("hybrid", *grid)
    assert (g.form, g.n_store, g.auto_stored, g.project_v) == (form, n_store, False, True)


@pytest.mark.parametrize("grid", [(4, 384), (2, 357)])
@pytest.mark.parametrize("how", ["not available", "project_v=0"])
def test_hybrid_without_the_projection_recomputes(grid, how):
    g = (resolve("hybrid", *grid, project_ok=False) if how == "not available" else resolve("hybrid", *grid, project_v=False))
    assert (g.form, g.n_store, g.project_v, g.auto_stored) == ("recompute", 0, False, False)


@pytest.mark.parametrize("precision, grid, form, rows", [
    (SPLIT, (4, 384), "matrix", 384), (SPLIT, (2, 16380), "matrix", 16380),
    (SPLIT, (2, 16384), "recompute", 1),                          # P * P == 2^28 does not fit
    (SPLIT, (3, 32400), "recompute", 1),
    (FP32, (4, 384), "matrix", 384), (FP32, (2, 16384), "chunked", 16383), (FP32, (3, 32400), "chunked", 8285)])
def test_auto(precision, grid, form, rows):
    g = resolve("auto", *grid, precision=precision)
    assert (g.form, g.attn_rows, g.n_store, g.auto_stored) == (form, rows, 0, False)
    assert g.attn_f16 == (precision == SPLIT and form == "matrix")


def test_matrix_mode_chunks_what_does_not_fit_and_what_attn_chunk_rows_forces():
    g = resolve("matrix", 3, 32400)
    assert (g.form, g.attn_rows, g.attn_f16) == ("chunked", 8285, True)
    for mode in ("matrix", "auto"):
        g = resolve(mode, 4, 384, attn_chunk_rows=100)
        assert (g.form, g.attn_rows) == ("chunked", 100)


@pytest.mark.parametrize("mode", FUSED_MODES)
def test_fused_modes_refuse_exact_fp32(mode):
    with pytest.raises(RuntimeError, match=f"gma_mode='{mode}' needs a split precision"):
        resolve(mode, 4, 384, precision=FP32)


def test_k_splits():
    assert resolve("matrix", 4, 384).k_splits == 3
    assert resolve("matrix", 4, 384, precision=FP32).k_splits == 1
    assert resolve("matrix", 2, 357).k_splits == 1                          # P % 4 != 0
    assert resolve("matrix", 4, 384, attn_k_splits=9).k_splits == 4
    assert resolve("matrix", 4, 384, attn_k_splits=1).k_splits == 1


def test_the_form_is_a_function_of_its_arguments_only():
    o = EngineOptions()
    a = resolve_gma("hybrid", SPLIT, 1, o, 18, 7040, True)
    assert a == resolve_gma("hybrid", SPLIT, 1, replace(o, split_solo=0, parallel_branches=False), 18, 7040, True)
    assert hash(a) == hash(resolve_gma("hybrid", SPLIT, 1, o, 18, 7040, True))


SWEEP_P = (16384, 32400, 46000, 46400, 57600, 92160)


def test_the_library_accepts_every_image_the_plan_stores(lib):
    """attn.hip refuses a single image whose stored weights reach 4 GiB (sf_gma_stored_image_ok), whatever the total: whenever a
    plan stores anything, the exported rule accepts its grid -- and a grid it refuses resolves to the recompute form.  (2, 57600)
    is 13.3 GB in all, under every total limit, and 6.6 GB per image: the stored form it used to get raised in the setup."""
    assert [bool(lib.sf_gma_stored_image_ok(P)) for P in SWEEP_P] == [True, True, True, False, False, False]
    assert not lib.sf_gma_stored_image_ok(0) and not lib.sf_gma_stored_image_ok(-5) and lib.sf_gma_stored_image_ok(1)
    for P in (46208, 46209):                                                    # Ppad = 46208 is the last padded size under the limit
        Ppad = -(-P // 128) * 128
        assert bool(lib.sf_gma_stored_image_ok(P)) == (Ppad * Ppad * 2 + 3 * (Ppad // 32) * 4096 < 1 << 32) == (P == 46208)
    seen = set()
    for P in SWEEP_P:
        for n in (1, 2, 3):
            for mode in FUSED_MODES:
                for products in (1, 3):
                    g = resolve(mode, n, P, products=products)
                    if g.n_store > 0:
                        assert lib.sf_gma_stored_image_ok(P), (mode, n, P, products, g)
                        assert ops.gma_stored_p_bytes(g.n_store, P) <= 64 << 30
                    else:
                        assert (g.form, g.auto_stored) == ("recompute", False)
                    if not lib.sf_gma_stored_image_ok(P):
                        assert (g.form, g.n_store, g.auto_stored) == ("recompute", 0, False), (mode, n, P, products)
                        seen.add((n, P))
    assert ops.gma_stored_p_bytes(2, 57600) <= 16 << 30 and (2, 57600) in seen
    assert resolve("flash", 2, 46000).form == "stored" and resolve("stored", 1, 46000).n_store == 1     # still stored below the limit
