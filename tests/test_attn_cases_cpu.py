"""Pins tests/attn_cases.py, the references and bounds of tests/test_gpu_attn_kernels.py, without a GPU:

    exact equals the oracle (oracle/streamflow_oracle.py gma_attention + gma_aggregate, oracle/twins_oracle.py _attend and
        locally_grouped_attn) to float64 round-off;
    |model - exact| <= bound / 2 on every element of every case and class: the documented roundings alone stay inside the bound
        with margin (measured: GMA at most 0.19, encoder cores at most 0.40 -- the hi + lo class, whose dropped lo * lo product is a
        2^-22 relative logit error beside the 2^-20 the bound grants);
    wrong kernels, restated in numpy, exceed the bound at least tenfold on some element of a case aimed at them;
    the case sets, so that a later edit cannot thin them.

One wrong kernel of the issue's list cannot be told from a right one by ANY bound of this form -- the row sum taken over the
unrounded weights (test_unrounded_row_sum_is_inside_the_bound_by_construction): with r_j the rounding error of weight j, that kernel
is off by sum_j r_j v_j / sum w to first order, and the bound's weight term sum_j e_j (|v_j| + |o|) / sum w, e_j >= |r_j|, grants
exactly that.  Nothing on the GPU pins it either: the recompute form with statistics and the stored-weights form take 1 / row sum from
the same statistics pass (attn.hip:238, :413, :416, :725) and stay bitwise equal whichever sum that pass takes, and the online form
differs from them inside the bound.  The choice of sum is a property no test of this kind can see."""
import numpy as np
import pytest
import torch

from tests import attn_cases as ac


def _ratio(model, exact, bound):
    return float(np.max(np.abs(model - exact) / bound))


# ---- the case sets ---------------------------------------------------------------------------------------------------------------------
def test_case_sets():
    assert ac.GMA_P == (1, 63, 64, 65, 127, 128, 129, 193, 385, 512, 513, 641) and ac.GMA_N == (1, 3)
    assert ac.GMA_FAMILIES == ("randn", "sharp", "dominant", "flat", "gamma0") and ac.GMA_PRODUCTS == (1, 2, 3)
    cases = ac.gma_cases()
    assert len(cases) == 60 and len({c["id"] for c in cases}) == 60 and len({c["seed"] for c in cases}) == 60
    assert {(c["P"], c["family"]) for c in cases} == {(P, f) for P in ac.GMA_P for f in ac.GMA_FAMILIES}
    # both sides of the key-split predicate at the smallest split grid; its last key tile empty, the one before with one key
    assert (ac.GMA_SPLIT_P, ac.GMA_SPLIT_N) == (385, (95, 96))
    assert ac.use_key_split(95, 385) and not ac.use_key_split(96, 385) and not ac.use_key_split(1, 384) and ac.use_key_split(1, 385)
    assert all(ac.use_key_split(1, P) == ac.use_key_split(3, P) for P in ac.GMA_P)       # a batch and its images: the same decision
    assert {P for P in ac.GMA_P if ac.use_key_split(3, P)} == {385, 512, 513, 641}
    assert {P for P in ac.GMA_P if 1 <= P % 128 <= 64} == {1, 63, 64, 129, 385, 513, 641}  # a last 64-key tile without a key
    assert ac.WIN_WS == (2, 3, 4, 5, 6, 7) and ac.WIN_HEADS == (4, 8) and ac.WIN_N == (1, 3)
    assert ac.win_grids(7) == ((1, 1), (7, 7), (8, 13), (1, 22)) and len(ac.win_cases()) == 24
    assert ac.WIN_CLASSES == ("fp32", "x3", "x1", "koct") and ac.OUT_MODES == ("out", "koct", "both")
    assert ac.SUB_N == (1, 31, 32, 33, 127, 128, 129, 255, 256, 257) and ac.SUB_M == (1, 31, 32, 33, 63, 64, 65, 97)
    sub = ac.sub_cases()
    assert len(sub) == 17 and {c["heads"] for c in sub} == {1, 4, 8}
    assert {c["N"] for c in sub if c["M"] == 97} == set(ac.SUB_N) and {c["M"] for c in sub if c["N"] == 129} == set(ac.SUB_M)
    assert ac.SUB_CLASSES == ("fp32", "x3", "x1")


def test_workspace_size_restated():
    # one image at Ppad = 128: five 32 KB planes, 128 statistics pairs, the header; the partial buffers only when split
    assert ac.gma_ws_bytes(1, 1) == 5 * 32768 + 1024 + 16
    assert ac.gma_ws_bytes(95, 385) == 95 * (5 * 131072 + 4096 + 16) + 2 * 95 * 128 * 512 * 4
    assert ac.gma_ws_bytes(96, 385) == 96 * (5 * 131072 + 4096 + 16)


def test_roundings():
    assert ac.f16(2.0 ** -24) == 2.0 ** -24 and ac.f16(2.0 ** -25 * 1.01) == 2.0 ** -24 and ac.f16(2.0 ** -25) == 0.0   # subnormals kept, ties to even
    assert ac.f16(1.0 + 2.0 ** -11) == 1.0 and ac.f16(1.0 + 3 * 2.0 ** -11) == 1.0 + 2.0 ** -9
    hi, lo = ac._parts(np.array([1.0 + 2.0 ** -12, 0.1]), "split")
    assert hi[0] == 1.0 and lo[0] == 2.0 ** -12 and abs(hi[1] + lo[1] - 0.1) <= 2.0 ** -21 * 0.1
    assert ac.ulp32(1.0) == 2.0 ** -23 and ac.ulp32(-3.0) == 2.0 ** -22


# ---- exact == the oracle -----------------------------------------------------------------------------------------------------------------
def test_gma_exact_equals_the_oracle():
    from oracle import streamflow_oracle as so
    g = torch.Generator().manual_seed(11)
    B, h, w = 2, 5, 13
    inps = torch.randn(B, 128, h, w, generator=g, dtype=torch.float64)
    fmap = torch.randn(B, 128, h, w, generator=g, dtype=torch.float64)
    w_qk = torch.randn(256, 128, 1, 1, generator=g, dtype=torch.float64) * 0.2
    w_v = torch.randn(128, 128, 1, 1, generator=g, dtype=torch.float64) * 0.1
    gamma = torch.tensor([0.61], dtype=torch.float64)
    want = so.gma_aggregate(so.gma_attention(inps, w_qk), fmap, w_v, gamma).reshape(B, 128, h * w).numpy()
    qk = torch.einsum("oc,bcp->bop", w_qk[:, :, 0, 0], inps.reshape(B, 128, -1)).numpy()
    v = torch.einsum("oc,bcp->bop", w_v[:, :, 0, 0], fmap.reshape(B, 128, -1)).numpy()
    exact, _, _ = ac.gma_reference(qk, v, fmap.reshape(B, 128, -1).numpy(), 0.61, products=(1,))
    assert np.max(np.abs(exact - want)) <= 1e-13 * np.max(np.abs(want))


@pytest.mark.parametrize("ws,H,W,heads", [(7, 8, 13, 4), (3, 4, 5, 8), (2, 1, 7, 4)])
def test_window_exact_equals_the_oracle(ws, H, W, heads):
    from oracle import twins_oracle as tw
    g = torch.Generator().manual_seed(12)
    C, B = heads * 32, 2
    x = torch.randn(B, H * W, C, generator=g, dtype=torch.float64)
    Wq = torch.randn(3 * C, C, generator=g, dtype=torch.float64) * 0.1
    b = torch.randn(3 * C, generator=g, dtype=torch.float64)
    p = {"a.qkv.weight": Wq, "a.qkv.bias": b, "a.proj.weight": torch.eye(C, dtype=torch.float64)}
    want = tw.locally_grouped_attn(x, (H, W), p, "a", heads, ws).permute(0, 2, 1).numpy()          # [B][C][N]
    qkv = (x @ Wq.t() + b).permute(0, 2, 1).numpy()
    exact, _, _ = ac.window_reference(qkv, b.numpy(), heads, H, W, ws, ["fp32"])
    assert np.max(np.abs(exact - want)) <= 1e-13 * np.max(np.abs(want))


def test_subsample_exact_equals_the_oracle():
    from oracle import twins_oracle as tw
    n, heads, N, M = 2, 4, 33, 97
    q, kv = ac.subsample_inputs(n, heads, N, M, 13)
    C = heads * 32
    t = lambda a, L: torch.from_numpy(a.astype(np.float64)).view(n, heads, 32, L).transpose(-1, -2)      # noqa: E731
    want = tw._attend(t(q, N), t(kv[:, :C], M), t(kv[:, C:], M), 32 ** -0.5).transpose(-1, -2).reshape(n, C, N).numpy()
    exact, _, _ = ac.subsample_reference(q, kv, heads, ["fp32"])
    assert np.max(np.abs(exact - want)) <= 1e-13 * np.max(np.abs(want))


# ---- the reference alone stays inside the bound, with margin --------------------------------------------------------------------------------
@pytest.mark.parametrize("P", ac.GMA_P)
def test_gma_model_is_inside_half_the_bound(P):
    for c in ac.gma_cases():
        if c["P"] != P:
            continue
        qk, v, mf = ac.gma_inputs(P, 3, c["family"], c["seed"])
        exact, bound, model = ac.gma_reference(qk, v, mf, ac.gma_gamma(c["family"]))
        for p in ac.GMA_PRODUCTS:
            assert np.all(bound[p] > 0) and np.all(np.isfinite(bound[p]))
            assert np.all(np.abs(model[p] - exact) <= 0.5 * bound[p]), (c["id"], p, _ratio(model[p], exact, bound[p]))
        if c["family"] == "gamma0":
            assert np.array_equal(exact, mf.astype(np.float64))


def test_gma_split_images_model_is_inside_half_the_bound():
    qk, v, mf = ac.gma_split_inputs()
    assert qk.shape == (ac.GMA_SPLIT_BASE, 256, ac.GMA_SPLIT_P)
    exact, bound, model = ac.gma_reference(qk, v, mf, ac.GMA_GAMMA)
    for p in ac.GMA_PRODUCTS:
        assert np.all(np.abs(model[p] - exact) <= 0.5 * bound[p])


def test_dominant_family_is_what_it_says():
    """For every third query one key 16 to 22 log2 units above all others: the rest of the row in fp16's subnormal range."""
    P = 641
    qk, v, mf = ac.gma_inputs(P, 3, "dominant", 1)
    for z in range(3):
        l = (qk[z, :128].astype(np.float64).T * (ac.GMA_SCALE * ac.LOG2E)) @ qk[z, 128:].astype(np.float64)
        top2 = np.sort(l[0::3], axis=1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
        assert gap.min() >= 14.0 and gap.max() <= 24.0 and np.all(np.argmax(l[0::3], axis=1) == (P - 1 if z == 0 else P // 3))
        w = np.exp2(l[0::3] - l[0::3].max(1, keepdims=True))
        sub = (w < 2.0 ** -14) & (w >= 2.0 ** -25)
        assert sub.sum(1).min() >= 0.9 * (P - 1)


@pytest.mark.parametrize("ws", ac.WIN_WS)
def test_window_model_is_inside_half_the_bound(ws):
    for c in ac.win_cases():
        if c["ws"] != ws:
            continue
        for heads in ac.WIN_HEADS:
            for koct in (False, True):
                qkv, bias = ac.window_inputs(3, heads, c["H"], c["W"], c["seed"] + heads, koct)
                classes = ["koct"] if koct else ["fp32", "x3", "x1"]
                exact, bound, model = ac.window_reference(qkv, bias, heads, c["H"], c["W"], ws, classes)
                for k in classes:
                    assert np.all(np.abs(model[k] - exact) <= 0.5 * bound[k]), (c["id"], heads, k, _ratio(model[k], exact, bound[k]))


def test_subsample_model_is_inside_half_the_bound():
    for c in ac.sub_cases():
        q, kv = ac.subsample_inputs(3, c["heads"], c["N"], c["M"], c["seed"])
        exact, bound, model = ac.subsample_reference(q, kv, c["heads"], list(ac.SUB_CLASSES))
        for k in ac.SUB_CLASSES:
            assert np.all(np.abs(model[k] - exact) <= 0.5 * bound[k]), (c["id"], k, _ratio(model[k], exact, bound[k]))


# ---- wrong kernels are outside it ------------------------------------------------------------------------------------------------------------
GMA_WRONG = [
    # (wrong kernel, P, family, products it must show at)
    ("pad_key", 385, "flat", (1, 2, 3)),                    # key < P -> key <= P: the zero key of the padding, logit 0, takes the -19 rows
    ("pad_key", 65, "flat", (1, 2, 3)),
    ("drop_last_tile", 385, "randn", (2, 3)),               # (one key of 385: below ten bounds of the one-product class)
    ("drop_last_tile", 641, "dominant", (1, 2, 3)),         # image 0's dominant key is the last one
    ("drop_second_partial", 385, "randn", (1, 2, 3)),
    ("drop_second_partial", 641, "sharp", (1, 2, 3)),
    ("ftz", 641, "dominant", (1, 2, 3)),                    # weights below 2^-14 flushed: the tail IS the result
    ("no_log2e", 385, "randn", (1, 2, 3)),
    ("no_log2e", 65, "sharp", (1, 2, 3)),
    ("mf_neighbour", 65, "randn", (1, 2, 3)),
    ("mf_neighbour", 385, "gamma0", (1, 2, 3)),
]


@pytest.mark.parametrize("wrong,P,family,products", GMA_WRONG, ids=[f"{w}-P{P}-{f}" for w, P, f, _ in GMA_WRONG])
def test_wrong_gma_kernels_exceed_ten_bounds(wrong, P, family, products):
    seed = next(c["seed"] for c in ac.gma_cases() if c["P"] == P and c["family"] == family)
    qk, v, mf = ac.gma_inputs(P, 3, family, seed)
    gamma = ac.gma_gamma(family)
    exact, bound, model = ac.gma_reference(qk, v, mf, gamma, products=products)
    _, _, bad = ac.gma_reference(qk, v, mf, gamma, products=products, wrong=wrong)
    for p in products:
        assert _ratio(model[p], exact, bound[p]) <= 0.5
        assert _ratio(bad[p], exact, bound[p]) >= 10.0, (wrong, p, _ratio(bad[p], exact, bound[p]))


def test_ignored_k_lo_exceeds_ten_bounds():
    qk, v, mf = ac.gma_klo_inputs()
    exact, bound, model = ac.gma_reference(qk, v, mf, ac.GMA_GAMMA, products=(3,))
    _, _, bad = ac.gma_reference(qk, v, mf, ac.GMA_GAMMA, products=(3,), wrong="no_klo")
    assert _ratio(model[3], exact, bound[3]) <= 0.5
    assert _ratio(bad[3], exact, bound[3]) >= 10.0, _ratio(bad[3], exact, bound[3])


def test_unrounded_row_sum_is_inside_the_bound_by_construction():
    """See the module docstring: no case can show this wrong kernel outside the bound; its distance from the right model is what the
    bound's weight term grants.  Pinned so that the statement stays checked: at the peaked rows of the dominant family and at rows
    of identical logits it stays below the bound, and it does differ from the right model (the restatement is not a no-op)."""
    for P, family in ((641, "dominant"), (385, "flat"), (129, "sharp")):
        qk, v, mf = ac.gma_inputs(P, 3, family, 77)
        exact, bound, model = ac.gma_reference(qk, v, mf, ac.GMA_GAMMA)
        _, _, bad = ac.gma_reference(qk, v, mf, ac.GMA_GAMMA, wrong="rowsum_unrounded")
        for p in ac.GMA_PRODUCTS:
            assert np.any(bad[p] != model[p])
            assert _ratio(bad[p], exact, bound[p]) <= 1.0


@pytest.mark.parametrize("ws,H,W", [(7, 8, 13), (2, 1, 7), (5, 1, 1), (4, 5, 7)])
def test_wrong_window_kernels_exceed_ten_bounds(ws, H, W):
    for koct in (False, True):
        classes = ["koct"] if koct else ["fp32", "x3", "x1"]
        qkv, bias = ac.window_inputs(3, 8, H, W, 21, koct)
        exact, bound, _ = ac.window_reference(qkv, bias, 8, H, W, ws, classes)
        for wrong in ("pad_zero", "heads_v"):
            _, _, bad = ac.window_reference(qkv, bias, 8, H, W, ws, classes, wrong=wrong)
            for k in classes:
                assert _ratio(bad[k], exact, bound[k]) >= 10.0, (wrong, k)
                if wrong == "heads_v":                             # heads 0..3 are right, heads 4..7 are not
                    assert np.all(np.abs(bad[k][:, :128] - exact[:, :128]) <= 0.5 * bound[k][:, :128])


def test_wrong_subsample_heads_exceed_ten_bounds():
    q, kv = ac.subsample_inputs(3, 8, 129, 97, 22)
    exact, bound, _ = ac.subsample_reference(q, kv, 8, list(ac.SUB_CLASSES))
    _, _, bad = ac.subsample_reference(q, kv, 8, list(ac.SUB_CLASSES), wrong="heads_v")
    for k in ac.SUB_CLASSES:
        assert _ratio(bad[k], exact, bound[k]) >= 10.0


def test_project_v_inputs_are_exact_in_fp32():
    """Every partial sum of (w_hi + w_lo) x is a multiple of 2^-9 below 2^15: exact in fp32 in any order, and alpha a power of two."""
    x, w_hi, w_lo, alpha = ac.project_v_inputs(65, 2, 5)
    assert np.array_equal(ac.f16(x), x) and np.array_equal(ac.f16(w_hi), w_hi) and np.array_equal(ac.f16(w_lo), w_lo)
    worst = 128 * (np.abs(w_hi).max() + np.abs(w_lo).max()) * np.abs(x).max()
    assert worst < 2.0 ** 15 and np.all(np.mod(x * 64, 1) == 0) and np.all(np.mod(w_lo * 8, 1) == 0) and alpha == 2.0 ** -4
    v = alpha * np.einsum("dc,ncp->ndp", w_hi + w_lo, x)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
