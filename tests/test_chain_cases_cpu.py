"""CPU: the case lists of tests/test_gpu_chain_descriptors.py (tests/chain_cases.py) cover what they claim, every placement honours
the entry points' alignment rules, and the float64 restatements that file compares the kernels with -- held here, with the
parameter draws -- are the reference's arithmetic: with their fp16 roundings switched off and exact fp32 weights they reproduce
the oracle's skblock / temporal_block / upsample_flow (oracle/streamflow_oracle.py, itself pinned against the reference's goldens
in tests/test_oracle_golden.py) within the tolerance that file uses for the same function.  No GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import chain_cases as cc


# ---- float64 restatements (all arguments float64; round16 = the fp16 hand-overs the kernels make and the references model) -------
def _r16(t, on):
    return t.half().double() if on else t


def _lin(W, b, x):
    y = torch.einsum("mk,nkp->nmp", W, x)
    return y if b is None else y + b[None, :, None]


def ref_pair(W1, b1, W2, b2, x, mode, gelu_out=False, dw_w=None, dw_b=None, resid=None, round16=True):
    """sf_ffn_pair (update.py:14-16, 30-32): x [n, K1, P].  mode 0: y = W2 gelu(W1 x + b1) + b2 (gelu'ed with gelu_out);
    mode 1: x1 = gelu(resid + y), gelu(x1 + dw_w x1 + dw_b), resid = x unless given (the fp32 residual planes)."""
    y = _lin(W2, b2, _r16(F.gelu(_lin(W1, b1, x)), round16))
    if mode == 0:
        return F.gelu(y) if gelu_out else y
    x1 = F.gelu((x if resid is None else resid) + y)
    return F.gelu(x1 + (dw_w[None, :, None] * x1 + dw_b[None, :, None]))


def ref_tail(Wp_res, bp, W0, b0, W2, b2, x, gelu_out=False, round16=True):
    """sf_sk_tail (update.py:35-36): x4 = gelu((pw + I) x3 + bp); y = ffn2(x4).  Wp_res = pw + I."""
    x4 = _r16(F.gelu(_lin(Wp_res, bp, x)), round16)
    y = _lin(W2, b2, _r16(F.gelu(_lin(W0, b0, x4)), round16))
    return F.gelu(y) if gelu_out else y


def ref_temporal(x, p, Wq, Wp, W1, W2):
    """sf_temporal_block (update.py:459-484 -> timm Block): tokens x [B, TT, C, P] -> the same shape.  The kernel's five internal
    fp16 hand-overs are not modelled (tests/test_gpu_temporal_block.py: the tolerance there is theirs)."""
    C = x.shape[2]
    d = lambda k: p[k].double()
    t = x.permute(0, 3, 1, 2)                                  # [B, P, TT, C]
    h = F.layer_norm(t, (C,), d("ln1_w"), d("ln1_b"), 1e-5)
    qkv = h @ Wq.t()
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    a = torch.softmax((q * C ** -0.5) @ k.transpose(-1, -2), dim=-1)
    t = t + (a @ v) @ Wp.t() + d("proj_b")
    h = F.layer_norm(t, (C,), d("ln2_w"), d("ln2_b"), 1e-5)
    t = t + F.gelu(h @ W1.t() + d("fc1_b")) @ W2.t() + d("fc2_b")
    return t.permute(0, 2, 3, 1)


def ref_upsample(flow, mask):
    """streamflow.py:82-93 in float64: flow [n, 2, h, w], mask [n, 576, h, w]; F.unfold pads with zeros."""
    n, _, h, w = flow.shape
    m = torch.softmax(mask.view(n, 1, 9, 8, 8, h, w), dim=2)
    up = F.unfold(8 * flow, [3, 3], padding=1).view(n, 2, 9, 1, 1, h, w)
    return torch.sum(m * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(n, 2, 8 * h, 8 * w)


def ref_mask_upsample(W, b, x, flow):
    """sf_mask_upsample: mask = 0.25 (W x + b) (update.py:758,777), then the convex upsampling.  x [n, 256, h w], flow [n, 2, h, w]."""
    n, _, h, w = flow.shape
    return ref_upsample(flow, (0.25 * _lin(W, b, x)).view(n, -1, h, w))


# ---- parameter draws (the distributions of the kernels' own test files: their bounds belong to them) -------------------------------
def lo_heavy(W, sign=1.0):
    """W moved so that split_scale * W sits 0.45 fp16 ulp ABOVE (sign = -1: below; a tensor: per row) its round-to-nearest fp16
    value, every element of a row the same way: the `lo` half of PackedLinear's split is as large as it can be without changing
    `hi`, and over inputs of one sign the dropped halves add up instead of cancelling."""
    s = 2.0 ** min(14, max(-14, -math.floor(math.log2(float(W.abs().max())))))          # PackedLinear.split_scale
    h = (W * s).half()
    ulp = torch.from_numpy(np.spacing(np.abs(h.numpy())).astype(np.float32))
    return (h.float() + sign * 0.45 * ulp) / s


def weff(A, single):
    """The weights a launch multiplies: hi alone (one product) or hi + lo (two), float64, of a streamflow_amd.ops.PackedLinear."""
    hi = A.hi.float().permute(1, 0, 2).reshape(A.lda_h, -1)[: A.M, : A.K].double().cpu()
    lo = A.lo.float().permute(1, 0, 2).reshape(A.lda_h, -1)[: A.M, : A.K].double().cpu()
    return (hi if single else hi + lo) / A.split_scale


def draw_weights(kernel, shape, heavy=False):
    """{name: fp32 tensor} of one kernel shape, seeded by the shape.  heavy: part C's weights (lo_heavy) and parameters that keep
    every layer's input of one sign on average (positive LayerNorm biases, a positive mean in the v rows of qkv)."""
    g = torch.Generator().manual_seed(7 * shape[0] + shape[-1] + (100000 if heavy else 0))
    r = lambda *s: torch.randn(*s, generator=g)
    hv = lo_heavy if heavy else (lambda W: W)
    if kernel == "ffn_pair":
        K1, H, M2 = shape
        return {"first": hv(r(H, K1) / K1 ** 0.5), "b1": r(H) * 0.2, "second": hv(r(M2, H) / H ** 0.5 * 1.7), "b2": r(M2) * 0.2,
                "dw_w": r(M2) * 0.5, "dw_b": r(M2) * 0.1}
    if kernel == "sk_tail":
        C, H, M2 = shape
        return {"pw": hv(r(C, C) / C ** 0.5 * 0.7 + torch.eye(C)), "b_pw": r(C) * 0.2, "ffn2_0": hv(r(H, C) / C ** 0.5), "b0": r(H) * 0.2,
                "ffn2_2": hv(r(M2, H) / H ** 0.5 * 1.7), "b2": r(M2) * 0.2}
    if kernel == "temporal_block":
        C, H = shape
        qkv, fc2 = r(3 * C, C) / C ** 0.5 * 1.5, None
        if heavy:
            qkv[2 * C:] += 0.03
        p = {"qkv": hv(qkv), "proj": hv(r(C, C) / C ** 0.5), "proj_b": r(C) * 0.2, "fc1": hv(r(H, C) / C ** 0.5), "fc1_b": r(H) * 0.2,
             "fc2": r(C, H) / H ** 0.5, "fc2_b": r(C) * 0.2, "ln1_w": 1 + 0.3 * r(C), "ln1_b": 0.2 * r(C), "ln2_w": 1 + 0.3 * r(C),
             "ln2_b": 0.2 * r(C)}
        if heavy:                                                # one sign on average into every layer, and through fc2 to the output
            p["fc2"] = lo_heavy(p["fc2"] + 0.03)
            for k in ("ln1_b", "ln2_b", "fc1_b"):
                p[k] += 1.0
        return p
    K, M = shape
    W = r(M, K) / 16 * 3
    if heavy:                                                    # (a shift common to a sub-pixel's nine logits leaves its softmax alone:
        k9 = torch.arange(M) // 64                               # the neighbours k = row / 64 move in alternating directions)
        W = lo_heavy(W, (1.0 - 2.0 * (k9 % 2)).view(M, 1))
    return {"mask2": W, "b": r(M)}


def pack(kernel, w, pm, device):
    """(PackedLinear per layer in cc.layers_of(kernel) order, the kernel's stream packer) with the layers' `single` flags set."""
    from streamflow_amd import ops
    names = cc.layers_of(kernel)
    bias = {"first": "b1", "second": "b2", "pw": "b_pw", "ffn2_0": "b0", "ffn2_2": "b2", "qkv": None, "proj": "proj_b", "fc1": "fc1_b",
            "fc2": "fc2_b", "mask2": "b"}
    L = [ops.PackedLinear(w[n].view(*w[n].shape, 1, 1), None if bias[n] is None else w[bias[n]], device) for n in names]
    pms = pm if isinstance(pm, tuple) else (pm,) * len(L)
    for A, k in zip(L, pms):
        A.single = k == 1
    P = {"ffn_pair": ops.PackedPair, "sk_tail": ops.PackedTail, "temporal_block": ops.PackedTemporal, "mask_upsample": ops.PackedMask}
    return L, P[kernel](*L)


def draw_input(c, heavy=False):
    """The activations of a case: {x [n, K, P] fp32 (+ flow [n, 2, h, w])}, n = batch (x TT for the temporal block)."""
    g = torch.Generator().manual_seed(c["seed"])
    k = c["kernel"]
    P = c["N"] if "N" in c else c["hw"][0] * c["hw"][1]
    n = c["batch"] * c.get("TT", 1)
    K = c["shape"][0]
    x = torch.randn(n, K, P, generator=g) * (1.5 if k == "temporal_block" else 1.0)
    if k == "mask_upsample":
        return {"x": torch.relu(x), "flow": torch.randn(c["batch"], 2, *c["hw"], generator=g) * 5}
    if heavy and k != "temporal_block":                        # (LayerNorm removes a mean: the temporal block's sign comes from ln*_b)
        x = x + 0.75
    return {"x": x}


def gelu_out_of(c):
    return (c["kernel"] == "ffn_pair" and c["shape"][2] == 256) or (c["kernel"] == "sk_tail" and c["shape"][2] == 64)


def reference(c, w, Wd, inp, resid=None):
    """float64 result of a case: Wd = {layer: float64 weights} (weff of the packed layers on the GPU side, exact weights here), inp
    = draw_input() (x already what the kernel reads: fp16-rounded by the caller where the operand is fp16)."""
    k, d = c["kernel"], (lambda n: w[n].double())
    x = inp["x"].double()
    if k == "ffn_pair":
        return ref_pair(Wd["first"], d("b1"), Wd["second"], d("b2"), x, c["mode"], gelu_out_of(c), d("dw_w"), d("dw_b"), resid)
    if k == "sk_tail":
        return ref_tail(Wd["pw"], d("b_pw"), Wd["ffn2_0"], d("b0"), Wd["ffn2_2"], d("b2"), x, gelu_out_of(c))
    if k == "temporal_block":
        B, TT = c["batch"], c["TT"]
        C, P = x.shape[1], x.shape[2]
        return ref_temporal(x.view(B, TT, C, P), w, Wd["qkv"], Wd["proj"], Wd["fc1"], Wd["fc2"]).reshape(B * TT, C, P)
    return ref_mask_upsample(Wd["mask2"], d("b"), x, inp["flow"].double())


def class_weights(L, names, pms, flip=None):
    """{layer: weff} for the product counts pms, layer `flip` (an index) taken in the OTHER class."""
    return {n: weff(A, (k == 1) != (i == flip)) for i, (n, A, k) in enumerate(zip(names, L, pms))}


def rms(t):
    return float((t.double() ** 2).mean().sqrt())


# ---- 1 - 5: coverage -------------------------------------------------------------------------------------------------------------
def _keys(cases, kernel):
    return {(c["shape"], c.get("mode"), c["pm"], c.get("TT")) for c in cases if c["kernel"] == kernel}


def test_every_built_shape_and_product_combination_is_listed():
    from streamflow_amd import ops
    A, B = cc.part_a(), [c for _, g in cc.part_b() for c in g]
    for mode in (0, 1):
        listed = {(s[0], s[2]) for s, m in cc.pair_shapes() if m == mode}
        assert listed == ops.PAIR_SHAPES[mode], (mode, listed ^ ops.PAIR_SHAPES[mode])
    for part in (A, B):
        for shape, mode in cc.pair_shapes():
            assert any(c["kernel"] == "ffn_pair" and c["shape"] == shape and c["mode"] == mode for c in part), (shape, mode)
    for shape, mode in cc.pair_shapes():
        for pm in [(1, 1), (2, 1), (2, 2)]:
            assert (shape, mode, pm, None) in _keys(A + B, "ffn_pair"), (shape, mode, pm)
            assert (shape, mode, pm, None) in _keys(cc.part_c(), "ffn_pair"), (shape, mode, pm)
        assert (shape, mode, (2, 2), None) in _keys(B, "ffn_pair")                 # B: the largest product count
    assert cc.PAIR_PM == [(1, 1), (2, 1), (2, 2)]
    from tests.test_gpu_sk_tail import SHAPES
    assert cc.TAIL_SHAPES == SHAPES
    for shape in SHAPES:
        for pm in (1, 2):
            assert (shape, None, pm, None) in _keys(A, "sk_tail") and (shape, None, pm, None) in _keys(cc.part_c(), "sk_tail")
        assert (shape, None, 2, None) in _keys(B, "sk_tail")
    for TT in (1, 2, 3):
        for pm in (1, 2):
            assert (cc.TEMPORAL_SHAPE, None, pm, TT) in _keys(A, "temporal_block")
            assert (cc.TEMPORAL_SHAPE, None, pm, TT) in _keys(cc.part_c(), "temporal_block")
        assert (cc.TEMPORAL_SHAPE, None, 2, TT) in _keys(B, "temporal_block")
    for pm in (1, 2):
        assert (cc.MASK_SHAPE, None, pm, None) in _keys(A, "mask_upsample") and (cc.MASK_SHAPE, None, pm, None) in _keys(cc.part_c(), "mask_upsample")
    ids = [c["id"] for c in A + B + cc.part_c()]
    assert len(ids) == len(set(ids))
    for c in A + B + cc.part_c():
        assert {"kernel", "shape", "pm", "batch", "placement", "seed"} <= set(c) and ("N" in c) != ("hw" in c), c


def test_part_a_sizes_and_special_forms():
    A = cc.part_a()
    assert all(c["batch"] == 3 and c["placement"] in ("aligned", "unaligned") for c in A)
    for k, N in (("ffn_pair", 132), ("sk_tail", 132), ("temporal_block", 68)):
        assert {c["N"] for c in A if c["kernel"] == k} == {N}
        assert N % 8 == 4 and all(N > wg and N % wg for wg in cc.WORKGROUP[k])                  # ragged, more than one workgroup
    assert {c["hw"] for c in A if c["kernel"] == "mask_upsample"} == {(4, 17), (9, 15)}
    grouped = {(c["shape"][0], c["mode"]) for c in A if c.get("x_group") == 128 and not c.get("r32")}
    assert grouped == {(K1, m) for K1 in (384, 256, 128) for m in (0, 1)}
    assert {c["shape"][0] for c in A if c.get("r32")} == set(cc.R32_K1) and all(c["mode"] == 1 for c in A if c.get("r32"))
    for k in ("ffn_pair", "sk_tail", "temporal_block", "mask_upsample"):                         # both classes per kernel and shape
        for shape in {c["shape"] for c in A if c["kernel"] == k}:
            assert {c["placement"] for c in A if c["kernel"] == k and c["shape"] == shape} == {"aligned", "unaligned"}, (k, shape)


def test_part_b_sizes_sit_on_the_tile_edges():
    """Relative to each kernel's own widths: one pixel, one short of / one past a wave, one past a workgroup (of either size for
    sf_ffn_pair), a middle size that is no multiple of 4, and more than two workgroups."""
    B = cc.part_b()
    want = {"sk_tail": [1, 31, 33, 100, 128, 129, 260], "ffn_pair": [1, 15, 17, 68, 127, 129, 260], "temporal_block": [1, 15, 17, 65, 132]}
    for k, sizes in want.items():
        wave, wgs = cc.WAVE[k], cc.WORKGROUP[k]
        assert {1, wave - 1, wave + 1} <= set(sizes) and any(N == wg + 1 for N in sizes for wg in wgs)
        assert any(N % 4 for N in sizes if N > wave) and max(sizes) > 2 * min(wgs)
        for gid, cs in B:
            if cs[0]["kernel"] == k:
                assert sorted({c["N"] for c in cs}) == sizes, gid
                assert {(c["N"], c["batch"]) for c in cs} == {(N, b) for N in sizes for b in (1, 3)}, gid
                assert all(c["placement"] == "contiguous" and c["pm"] == cc.largest_pm(k, c["shape"]) for c in cs)
        for big, small in cc.B_PREFIX[k]:
            assert big in sizes and small in sizes and small < big
    assert cc.B_PREFIX["sk_tail"] == [(129, 33), (260, 129)] and cc.B_PREFIX["ffn_pair"] == [(129, 17), (260, 129)]
    hws = [cs[0]["hw"] for _, cs in B if cs[0]["kernel"] == "mask_upsample"]
    assert hws == [(1, 1), (1, 5), (5, 1), (5, 13), (2, 34), (9, 15)]
    assert any(h == 1 for h, w in hws) and any(w == 1 for h, w in hws) and any(h * w > 64 and (h * w) % 64 for h, w in hws)
    assert {c["TT"] for _, cs in B for c in cs if c["kernel"] == "temporal_block"} == {1, 2, 3}


def test_part_c_and_d_sizes():
    C = cc.part_c()
    assert all(c["batch"] == 2 and (c.get("N") == 260 or c["hw"][0] * c["hw"][1] == 260) for c in C)
    assert cc.D_HW == (47, 156) and (47 * 156) % 64 == 36 and cc.D_BATCH == 3 and cc.D_REPEATS == 5


# ---- 6: placements honour the entry points' requirements -------------------------------------------------------------------------
def test_placements_honour_the_entry_points():
    for c in cc.part_a():
        for i, (field, layout, rows, group, tight) in enumerate(cc.operands(c)):
            cols = cc.cols_of(c, field)
            for placement in ("contiguous", c["placement"]):
                off, ld, stride, gs = cc.place(layout, placement, rows, cols, c["seed"] + i, group, tight)
                what = (c["id"], field, placement, off, ld, stride, gs)
                assert (off * cc.ELEM[layout]) % cc.BASE_ALIGN[layout] == 0, what
                if layout == "koct":
                    assert stride % 8 == 0 and gs % 8 == 0, what
                    assert (not group) or (group % 32 == 0 and rows % group == 0), what
                if placement == "contiguous":
                    assert off == 0 and ld == cols, what
                    continue
                assert off > 0, what
                if tight:
                    assert (ld, stride) == (cols, rows * cols), what
                    continue
                assert ld > cols, what
                per_row = 8 if layout == "koct" else 1
                grows = -(-(group or rows) // per_row)
                gspan = grows * ld * per_row
                if group:
                    assert gs > gspan and stride > (rows // group - 1) * gs + gspan, what
                else:
                    assert stride > gspan, what
                if placement == "unaligned":
                    assert ld in (cols + 1, cols + 3) and (layout != "rows16" or ld % 2 == 1), what
                    assert off * cc.ELEM[layout] == cc.BASE_ALIGN[layout], what                # the smallest the alignment allows
                else:
                    assert (ld * (16 if layout == "koct" else cc.ELEM[layout])) % 16 == 0, what


# ---- the restatements against the oracle, roundings off --------------------------------------------------------------------------
def _close(a, b, atol, rtol):
    """tests/test_oracle_golden.py::close."""
    err = (a - b).abs()
    assert bool((err <= atol + rtol * b.abs()).all()), f"max err {float(err.max()):.3e}"


def test_pair_depthwise_tail_restate_the_oracle_skblock():
    """ffn1 pair (mode 1: residual, GELU, depthwise 1x1, GELU), the depthwise K x K step, then the tail = orc.skblock with
    k_conv = (1, 3); tolerance of test_oracle_golden.py::test_skblocks."""
    from oracle import streamflow_oracle as orc
    g = torch.Generator().manual_seed(3)
    n, h, wd = 2, 5, 7
    for C, H, M2 in ((128, 192, 64), (256, 384, 126)):
        w1 = draw_weights("ffn_pair", (C, H, C))
        w2 = draw_weights("sk_tail", (C, H, M2))
        dwk, dwkb = torch.randn(C, 1, 3, 3, generator=g).double() * 0.2, torch.randn(C, generator=g).double() * 0.1
        x = torch.randn(n, C, h, wd, generator=g).double()
        d = lambda t: t.double()
        x2 = ref_pair(d(w1["first"]), d(w1["b1"]), d(w1["second"]), d(w1["b2"]), x.view(n, C, -1), 1, False, d(w1["dw_w"]), d(w1["dw_b"]),
                      round16=False).view(n, C, h, wd)
        x3 = F.gelu(x2 + F.conv2d(x2, dwk, dwkb, padding=1, groups=C))
        got = ref_tail(d(w2["pw"]), d(w2["b_pw"]), d(w2["ffn2_0"]), d(w2["b0"]), d(w2["ffn2_2"]), d(w2["b2"]), x3.view(n, C, -1),
                       round16=False).view(n, M2, h, wd)
        P = {"b.ffn1.0.weight": d(w1["first"]).view(H, C, 1, 1), "b.ffn1.0.bias": d(w1["b1"]), "b.ffn1.2.weight": d(w1["second"]).view(C, H, 1, 1),
             "b.ffn1.2.bias": d(w1["b2"]), "b.conv_list.0.weight": d(w1["dw_w"]).view(C, 1, 1, 1), "b.conv_list.0.bias": d(w1["dw_b"]),
             "b.conv_list.1.weight": dwk, "b.conv_list.1.bias": dwkb, "b.pw.weight": (d(w2["pw"]) - torch.eye(C).double()).view(C, C, 1, 1),
             "b.pw.bias": d(w2["b_pw"]), "b.ffn2.0.weight": d(w2["ffn2_0"]).view(H, C, 1, 1), "b.ffn2.0.bias": d(w2["b0"]),
             "b.ffn2.2.weight": d(w2["ffn2_2"]).view(M2, H, 1, 1), "b.ffn2.2.bias": d(w2["b2"])}
        _close(got, orc.skblock(x, P, "b", (1, 3)), 2e-5, 1e-5)
        # mode 0 of the pair is the ffn2 of the same block
        y0 = ref_pair(d(w2["ffn2_0"]), d(w2["b0"]), d(w2["ffn2_2"]), d(w2["b2"]),
                      F.gelu(_lin(d(w2["pw"]), d(w2["b_pw"]), x3.view(n, C, -1))), 0, round16=False).view(n, M2, h, wd)
        _close(y0, got, 2e-5, 1e-5)


def test_temporal_restates_the_oracle_temporal_block():
    """Tolerance of test_oracle_golden.py::test_update_block for the temporal tokens."""
    from oracle import streamflow_oracle as orc
    C, H = cc.TEMPORAL_SHAPE
    p = draw_weights("temporal_block", (C, H))
    for TT in (1, 2, 3):
        B, P = 2, 9
        x = torch.randn(B, TT, C, P, generator=torch.Generator().manual_seed(TT)).double() * 1.5
        got = ref_temporal(x, p, *(p[k].double() for k in ("qkv", "proj", "fc1", "fc2")))
        pre = "tb"
        params = {pre + ".norm1.weight": p["ln1_w"], pre + ".norm1.bias": p["ln1_b"], pre + ".norm2.weight": p["ln2_w"], pre + ".norm2.bias": p["ln2_b"],
                  pre + ".attn.qkv.weight": p["qkv"], pre + ".attn.proj.weight": p["proj"], pre + ".attn.proj.bias": p["proj_b"],
                  pre + ".mlp.fc1.weight": p["fc1"], pre + ".mlp.fc1.bias": p["fc1_b"], pre + ".mlp.fc2.weight": p["fc2"], pre + ".mlp.fc2.bias": p["fc2_b"]}
        params = {k: v.double() for k, v in params.items()}
        tok = x.permute(0, 3, 1, 2).reshape(B * P, TT, C)
        ref = orc.temporal_block(tok, params, pre).reshape(B, P, TT, C).permute(0, 2, 3, 1)
        _close(got, ref, 3e-5, 1e-5)


def test_mask_upsample_restates_the_oracle_upsample_flow():
    """orc.upsample_flow of the float64 mask; tolerance of test_oracle_golden.py::test_upsample.  One-row and one-column grids too."""
    from oracle import streamflow_oracle as orc
    w = draw_weights("mask_upsample", cc.MASK_SHAPE)
    for hw in cc.B_HW:
        c = dict(kernel="mask_upsample", shape=cc.MASK_SHAPE, batch=2, hw=hw, seed=hw[0] * 100 + hw[1])
        inp = draw_input(c)
        x, flow = inp["x"].double(), inp["flow"].double()
        got = ref_mask_upsample(w["mask2"].double(), w["b"].double(), x, flow)
        mask = (0.25 * _lin(w["mask2"].double(), w["b"].double(), x)).view(2, 576, *hw)
        _close(got, orc.upsample_flow(flow, mask), 5e-6, 0.0)


# ---- part C: the two references of a case differ, and by much more than fp32 accumulation could blur -------------------------------
def test_lo_heavy_weights_have_large_lo_halves():
    from streamflow_amd import ops
    W = lo_heavy(torch.randn(64, 96, generator=torch.Generator().manual_seed(1)) / 10)
    A = ops.PackedLinear(W.view(64, 96, 1, 1), None, "cpu")
    hi = A.hi.float().permute(1, 0, 2).reshape(A.lda_h, -1)[:64, :96]
    lo = A.lo.float().permute(1, 0, 2).reshape(A.lda_h, -1)[:64, :96]
    ulp = torch.from_numpy(np.spacing(np.abs(hi.half().numpy())).astype(np.float32))
    frac = lo / ulp
    # (all but a few elements: a lo in fp16's subnormals is a multiple of 2^-24, and a negative power of two has half the spacing
    # towards zero, so that 0.45 of the upper one rounds to the next value)
    assert float(((frac > 0.44) & (frac < 0.46)).float().mean()) > 0.98 and float(frac.abs().max()) <= 0.5, (float(frac.min()), float(frac.max()))


@pytest.mark.parametrize("case", cc.part_c(), ids=[c["id"] for c in cc.part_c()])
def test_part_c_references_differ(case):
    """rms(ref_right - ref_wrong) for every flipped layer against the WORST case of an fp32 accumulation: a sum of K terms rounds
    each partial sum by at most 2^-24 of the result's scale, K 2^-24 if every rounding falls the same way (K = the kernel's longest
    contraction, <= 576: 3.4e-5).  Demanded: twice that, so that no summation order can move a result from one reference to the
    other."""
    c = dict(case, batch=1, **({"N": 64} if "N" in case else {"hw": (8, 8)}))      # (the class signal is per pixel: a small draw suffices)
    k = c["kernel"]
    w = draw_weights(k, c["shape"], heavy=True)
    L, _ = pack(k, w, c["pm"], "cpu")
    names = cc.layers_of(k)
    pms = c["pm"] if isinstance(c["pm"], tuple) else (c["pm"],) * len(L)
    inp = draw_input(c, heavy=True)
    inp = dict(inp, x=inp["x"].half().float())
    right = reference(c, w, class_weights(L, names, pms), inp)
    kmax = max(A.K for A in L)
    floor = 2 * kmax * 2.0 ** -24 * max(1.0, float(right.abs().max()))
    for i, n in enumerate(names):
        wrong = reference(c, w, class_weights(L, names, pms, flip=i), inp)
        assert rms(right - wrong) > floor, (c["id"], n, rms(right - wrong), floor)
