"""CPU: the restatements, draws and case lists of tests/test_gpu_glue_kernels.py (tests/glue_cases.py).

1. Each restatement below -- written once, evaluated in float64 (the reference) and in torch float32 (the yardstick of the
   tolerance rule) -- reproduces the oracle's function of the same name within the tolerance tests/test_oracle_golden.py uses for
   it; the attention as the attention step of test_chain_cases_cpu.ref_temporal / orc.temporal_block.
2. The case lists cover the edges they were written for: asserted as sets, so that an edit that drops one fails here.
3. Teeth: a plausible wrong kernel, restated, is at least 10 tolerances away from the reference on a listed case (outputs that
   are compared exactly: differs at all).  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import glue_cases as gc
from tests.test_chain_cases_cpu import _close, draw_weights, ref_temporal, ref_upsample

F64, F32 = torch.float64, torch.float32


# ---- the tolerance rule -----------------------------------------------------------------------------------------------------------
# caps: the bound the suite already holds the same entry point to at the same input scale (tests/test_gpu_fuzz.py,
# tests/test_gpu_parity.py)
CAP = {("layernorm", "golden"): 2e-5, ("temporal_attn", 1): 2e-5, ("bilinear", None): 5e-6}


def tol_of(r32, r64, cap=None):
    """4 x the error of the float32 evaluation + 4 ulps (fp32) of the largest output, at most `cap`."""
    r64 = r64.double()
    t = 4.0 * float((r32.double() - r64).abs().max()) + 4.0 * 2.0 ** -24 * float(r64.abs().max())
    return min(t, cap) if cap is not None else t


def koct_close(a16, b32):
    """tests/test_gpu_fuzz.py: an fp16 k-octet copy against the fp32 output of the same call."""
    a, b = a16.float(), b32.float()
    return bool(((a - b).abs() <= 2.0 ** -11 * 1.01 * b.abs() + 1e-6).all())


# ---- restatements: every argument in the dtype to evaluate in -----------------------------------------------------------------------
def ref_attn(qkv, B, TT, C, scale=None, over="u"):
    """qkv [B TT][3C][P] (rows q | k | v) -> [B TT][C][P]: softmax_u(q_t . k_u / sqrt(C)) v_u per pixel (update.py:466-474)."""
    P = qkv.shape[-1]
    t = qkv.reshape(B, TT, 3, C, P)
    s = torch.einsum("btcp,bucp->bptu", t[:, :, 0], t[:, :, 1]) * (C ** -0.5 if scale is None else scale)
    a = torch.softmax(s, dim=-1 if over == "u" else -2)
    return torch.einsum("bptu,bucp->btcp", a, t[:, :, 2]).reshape(B * TT, C, P)


def ref_layernorm(x, gamma, beta, eps):
    """x [n][C][P], normalised over C per (image, pixel)."""
    return F.layer_norm(x.permute(0, 2, 1), (x.shape[1],), gamma, beta, eps).permute(0, 2, 1)


def ref_bilinear(img, coords, rounding=torch.floor):
    """utils.py:65-79 (F.grid_sample bilinear / zeros / align_corners) in pixel coordinates: img [M][C][Hi][Wi], coords
    [M][Ho][Wo][2] (x, y) -> [M][C][Ho][Wo].  A tap outside the image is zero; a non-finite coordinate samples zero."""
    M, C, Hi, Wi = img.shape
    x, y = coords[..., 0], coords[..., 1]
    ok = torch.isfinite(x) & torch.isfinite(y)
    x, y = torch.where(ok, x, torch.full_like(x, -8.0)), torch.where(ok, y, torch.full_like(y, -8.0))
    x0, y0 = rounding(x), rounding(y)
    fx, fy = (x - x0).unsqueeze(1), (y - y0).unsqueeze(1)
    x0, y0 = x0.long(), y0.long()
    flat = img.reshape(M, C, Hi * Wi)

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < Wi) & (yy >= 0) & (yy < Hi)
        idx = (yy.clamp(0, Hi - 1) * Wi + xx.clamp(0, Wi - 1)).reshape(M, 1, -1).expand(M, C, -1)
        return torch.gather(flat, 2, idx).reshape(M, C, *xx.shape[1:]) * inside.unsqueeze(1).to(img.dtype)

    return (tap(y0, x0) * ((1 - fx) * (1 - fy)) + tap(y0, x0 + 1) * (fx * (1 - fy)) + tap(y0 + 1, x0) * ((1 - fx) * fy)
            + tap(y0 + 1, x0 + 1) * (fx * fy))


def ref_bilinear_mask(coords, Hi, Wi, strict=True):
    """utils.py:69-70, 75-77 in the float32 the reference computes it in: normalised coordinates strictly inside (-1, 1)."""
    assert coords.dtype == F32
    gx = 2 * coords[..., 0] / (Wi - 1) - 1
    gy = 2 * coords[..., 1] / (Hi - 1) - 1
    m = ((gx > -1) & (gy > -1) & (gx < 1) & (gy < 1)) if strict else ((gx >= -1) & (gy >= -1) & (gx <= 1) & (gy <= 1))
    return m.to(F32).unsqueeze(-1)


def ref_context_split(cnets, hdim):
    """streamflow.py:119-122: cnets [n][2 hdim][P] -> tanh(first half), relu(second half)."""
    return torch.tanh(cnets[:, :hdim]), torch.relu(cnets[:, hdim:])


def ref_grid(n, h, w, dtype=F32):
    """utils.py:82-85 as [n][2][h w]: channel 0 = x, channel 1 = y."""
    p = torch.arange(h * w)
    return torch.stack([p % w, p // w]).to(dtype)[None].expand(n, 2, h * w).contiguous()


def ref_flow_update(coords1, delta, n, h, w):
    """streamflow.py:133,138: (coords1 + delta, coords1 + delta - grid), float32: adds and a subtraction, nothing to contract."""
    c = coords1 if delta is None else coords1 + delta
    return c, c - ref_grid(n, h, w, coords1.dtype)


def ref_dwconv(x, w, b):
    """timm PosConv: x + depthwise3x3(x) + b; x [n][C][H][W], w [C][9]."""
    C = x.shape[1]
    return x + F.conv2d(x, w.view(C, 1, 3, 3), b, padding=1, groups=C)


# ---- wrong kernels (teeth) --------------------------------------------------------------------------------------------------------
def wrong_layernorm_onepass(x, gamma, beta, eps):
    """float32, var = E[x^2] - mean^2 in one pass."""
    x = x.float()
    mean = x.mean(1, keepdim=True)
    var = ((x * x).mean(1, keepdim=True) - mean * mean).clamp(min=0)
    return ((x - mean) / torch.sqrt(var + eps) * gamma.float()[None, :, None] + beta.float()[None, :, None]).double()


def wrong_upsample_transposed(flow, mask):
    n, _, h, w = flow.shape
    perm = [(k % 3) * 3 + k // 3 for k in range(9)]
    return ref_upsample(flow, mask.view(n, 9, 64, h, w)[:, perm].reshape(n, 576, h, w))


def wrong_pack_truncate(x):
    """fp32 -> fp16 by dropping the low bits (towards zero) where round-to-nearest-even is wanted."""
    a = x.contiguous().numpy().view(np.uint32) & np.uint32(0xFFFFE000)
    return torch.from_numpy(a.view(np.float32).copy()).half()               # (exact in fp16 for the normal range it is used on)


# ---- draws (float32; what the GPU file feeds the kernels) ---------------------------------------------------------------------------
def _gen(c, salt=0):
    return torch.Generator().manual_seed(c["seed"] * 16 + salt)


def draw_attn(c, gain):
    g = _gen(c, gain)
    qkv = torch.randn(c["B"] * c["TT"], 3 * c["C"], c["P"], generator=g)
    qkv[:, :2 * c["C"]] *= gain
    return qkv


def draw_ln(c, cls):
    g = _gen(c, gc.LN_CLASSES.index(cls))
    n, C, P = c["n"], c["C"], c["P"]
    x = torch.randn(n, C, P, generator=g)
    x = {"golden": x * 2 + 0.3, "mean100": x + 100, "tiny": x * 1e-3, "constcol": x * 2 + 0.3}[cls]
    if cls == "constcol":
        x[:, :, P // 2] = gc.LN_CONST
    return x, torch.randn(C, generator=g), torch.randn(C, generator=g)


def draw_up(c, cls):
    g = _gen(c, gc.UP_CLASSES.index(cls))
    n, h, w = c["nhw"]
    flow = torch.randn(n, 2, h, w, generator=g) * (100 if cls == "sharp" else 3)
    if cls == "equal":
        mask = (torch.randn(n, 1, 64, h, w, generator=g) * 2).expand(n, 9, 64, h, w).reshape(n, 576, h, w).contiguous()
    elif cls == "onehot":
        hot = torch.randint(0, 9, (n, 1, 64, h, w), generator=g)
        mask = torch.full((n, 9, 64, h, w), -80.0).scatter_(1, hot, 80.0).reshape(n, 576, h, w)
    else:
        mask = torch.randn(n, 576, h, w, generator=g) * (30 if cls == "sharp" else 2)
    return flow, mask


def draw_bs(c):
    g = _gen(c)
    M, C, Hi, Wi = c["img"]
    Ho, Wo = gc.BS_POINTS
    img = torch.randn(M, C, Hi, Wi, generator=g)
    crd = torch.rand(M, Ho, Wo, 2, generator=g) * torch.tensor([Wi - 1.0, Hi - 1.0])
    fixed = torch.tensor(gc.bs_fixed_coords(Hi, Wi))
    crd.view(M, Ho * Wo, 2)[:, :len(fixed)] = fixed
    return img, crd


def draw_cs(c):
    g = _gen(c)
    n, hd, P = c["n"], c["hdim"], c["P"]
    x = torch.randn(n, 2 * hd, P, generator=g) * 3
    for z in range(n):                                     # saturated tanh, a clipped and a kept large value, -0.0 into the ReLU
        x[z, 0, 0] = gc.CS_SATURATED[z % 2]
        x[z, hd, 0] = (gc.CS_SATURATED[1], gc.CS_SATURATED[0], -0.0)[z % 3]
    return x


def draw_fu(c):
    g = _gen(c)
    n, h, w = c["nhw"]
    coords = ref_grid(n, h, w) + torch.randn(n, 2, h * w, generator=g) * 2
    coords[0, 0, 0] += gc.FU_FAR[0]
    coords[-1, 1, -1] += gc.FU_FAR[1]
    return coords, torch.randn(n, 2, h * w, generator=g)


def draw_pk(c):
    g = _gen(c)
    x = torch.randn(c["n"], c["rows"], c["P"], generator=g) * 3
    flat = x.view(-1)
    step = max(1, flat.numel() // len(gc.PK_SPECIAL))
    for i, v in enumerate(gc.PK_SPECIAL):
        if i * step < flat.numel():
            flat[i * step] = v
    return x


def draw_dw(c, C, n):
    g = _gen(c, C)
    H, W = c["hw"]
    return torch.randn(n, C, H, W, generator=g), torch.randn(C, 9, generator=g) * 0.3, torch.randn(C, generator=g) * 0.2


# ---- 1: the restatements against the oracle -----------------------------------------------------------------------------------------
def test_attention_restates_the_attention_step_of_the_temporal_block():
    """A temporal block whose LayerNorm 1 is the plain normalisation, whose proj is the identity and whose MLP ends in zeros is
    x + attention(qkv(LN x)): against ref_temporal and orc.temporal_block at the tolerance of test_update_block's temporal tokens."""
    from oracle import streamflow_oracle as orc
    C, H = 128, 256
    p = {k: v.double() for k, v in draw_weights("temporal_block", (C, H)).items()}
    p.update(ln1_w=torch.ones(C, dtype=F64), ln1_b=torch.zeros(C, dtype=F64), proj=torch.eye(C, dtype=F64), proj_b=torch.zeros(C, dtype=F64),
             fc2=torch.zeros(C, H, dtype=F64), fc2_b=torch.zeros(C, dtype=F64))
    for TT in gc.ATTN_TT:
        B, P = 2, 5
        x = torch.randn(B, TT, C, P, generator=torch.Generator().manual_seed(TT)).double() * 1.5
        h = F.layer_norm(x.permute(0, 1, 3, 2), (C,), None, None, 1e-5)                      # [B, TT, P, C]
        qkv = (h @ p["qkv"].t()).permute(0, 1, 3, 2).reshape(B * TT, 3 * C, P)
        got = x + ref_attn(qkv, B, TT, C).view(B, TT, C, P)
        _close(got, ref_temporal(x, p, p["qkv"], p["proj"], p["fc1"], p["fc2"]), 3e-5, 1e-5)
        pre = "tb"
        names = {"norm1.weight": "ln1_w", "norm1.bias": "ln1_b", "norm2.weight": "ln2_w", "norm2.bias": "ln2_b", "attn.qkv.weight": "qkv",
                 "attn.proj.weight": "proj", "attn.proj.bias": "proj_b", "mlp.fc1.weight": "fc1", "mlp.fc1.bias": "fc1_b",
                 "mlp.fc2.weight": "fc2", "mlp.fc2.bias": "fc2_b"}
        params = {pre + "." + k: p[v] for k, v in names.items()}
        tok = x.permute(0, 3, 1, 2).reshape(B * P, TT, C)
        _close(got, orc.temporal_block(tok, params, pre).reshape(B, P, TT, C).permute(0, 2, 3, 1), 3e-5, 1e-5)


def test_layernorm_restates_the_oracle_layer_norm():
    from oracle import streamflow_oracle as orc
    c = dict(seed=1, n=2, C=96, P=7)
    for cls in gc.LN_CLASSES:
        for eps in gc.LN_EPS:
            x, g, b = (t.double() for t in draw_ln(c, cls))
            _close(ref_layernorm(x, g, b, eps), orc.layer_norm(x.permute(0, 2, 1), g, b, eps).permute(0, 2, 1), 3e-5, 1e-5)


def test_upsample_restatement_on_these_shapes_and_classes():
    from oracle import streamflow_oracle as orc
    for c in gc.up_cases():
        for cls in gc.UP_CLASSES:
            flow, mask = (t.double() for t in draw_up(c, cls))
            _close(ref_upsample(flow, mask), orc.upsample_flow(flow, mask), 5e-6, 0.0)


def test_bilinear_restates_the_oracle_bilinear_sampler():
    """Finite coordinates inside and up to 1.5 pixels outside; tolerance of test_oracle_golden.py::test_bilinear_sampler.  (The
    oracle normalises by Hi - 1: no one-row image here.)"""
    from oracle import streamflow_oracle as orc
    g = torch.Generator().manual_seed(5)
    for M, C, Hi, Wi in ((1, 1, 2, 2), (3, 5, 6, 7), (2, 3, 5, 8)):
        img = torch.randn(M, C, Hi, Wi, generator=g).double()
        crd = torch.rand(M, 6, 11, 2, generator=g).double() * torch.tensor([Wi + 2.0, Hi + 2.0]) - 1.5
        crd[:, 0, :4] = torch.tensor([[0.0, 0.0], [Wi - 1.0, Hi - 1.0], [-1.0, 0.5], [0.5, float(Hi)]], dtype=F64)
        _close(ref_bilinear(img, crd), orc.bilinear_sampler(img, crd), 2e-6, 0.0)
        out, mask = orc.bilinear_sampler(img.float(), crd.float(), mask=True)
        assert torch.equal(ref_bilinear_mask(crd.float(), Hi, Wi), mask.float().view(M, 6, 11, 1))


def test_grid_is_the_oracle_coords_grid():
    from oracle import streamflow_oracle as orc
    for n, h, w in gc.FU_SHAPES:
        assert torch.equal(ref_grid(n, h, w), orc.coords_grid(n, h, w).view(n, 2, h * w))


# ---- 2: coverage ------------------------------------------------------------------------------------------------------------------
def test_case_lists_cover_the_edges():
    ids = [c["id"] for c in gc.all_cases()]
    assert len(ids) == len(set(ids)) and {c["kernel"] for c in gc.all_cases()} == set(gc.KERNELS)
    assert gc.BATCHES == (1, 3)
    # attention: every TT the switch instantiates at every C; the pixel edges of the 64-pixel workgroup at both ends of TT
    A = {(c["TT"], c["C"], c["P"]) for c in gc.attn_cases()}
    assert all(c["B"] == 3 for c in gc.attn_cases())
    assert {(TT, C, 65) for TT in range(1, 8) for C in (4, 36, 32, 128)} <= A
    assert {(TT, C, P) for TT in (1, 3, 7) for C in (36, 128) for P in (1, 63, 64, 65, 130)} <= A
    assert (36 // 4) % 4 != 0 and 4 // 4 == 1 and 32 // 4 == 8                    # the unroll-by-4 remainder, one channel, one octet a wave
    assert gc.ATTN_GAINS == (1, 4) and gc.ATTN_ENTRIES == ("f32", "f16in")
    assert gc.attn_forms(128) == gc.attn_forms(32) == ("out", "koct", "both") and gc.attn_forms(36) == gc.attn_forms(4) == ("out",)
    assert gc.ATTN_TT_REFUSED == 8 and gc.ATTN_KOCT_C_REFUSED == 36
    # LayerNorm: the three dispatch branches, both sides of 64 (split kernel) and 256 (generic), one pixel
    L = {(c["C"], c["P"]) for c in gc.ln_cases()}
    assert L == {(C, P) for C in (128, 256, 96, 324, 1) for P in (1, 63, 64, 65, 257)} and all(c["n"] == 3 for c in gc.ln_cases())
    assert gc.LN_EPS == (1e-5, 1e-6) and gc.LN_CLASSES == ("golden", "mean100", "tiny", "constcol")
    assert gc.ln_forms(128) == gc.ln_forms(256) == ("y", "koct", "both") and gc.ln_forms(96) == gc.ln_forms(324) == gc.ln_forms(1) == ("y",)
    assert gc.LN_KOCT_C_REFUSED == 96
    c = float(np.float32(gc.LN_CONST))                                             # (the constant column's sums are exact in fp32)
    assert c == gc.LN_CONST and all(float(np.float32(c * k)) == c * k for k in range(1, 325))
    # upsampling: one pixel, w < / == / > one segment, a partial segment behind two full ones, h = 1
    assert gc.UP_SHAPES == ((1, 1, 1), (2, 2, 31), (1, 3, 32), (2, 3, 33), (1, 2, 65))
    ws = {w for _, _, w in gc.UP_SHAPES}
    assert {gc.UP_SEG - 1, gc.UP_SEG, gc.UP_SEG + 1, 2 * gc.UP_SEG + 1} <= ws and any(h == 1 for _, h, _ in gc.UP_SHAPES)
    assert gc.UP_CLASSES == ("golden", "sharp", "equal", "onehot")
    # bilinear sampler
    assert gc.BS_IMAGES == ((1, 1, 2, 2), (3, 5, 6, 7), (2, 1, 1, 9)) and gc.BS_POINTS[0] * gc.BS_POINTS[1] == 300 > 256
    for _, _, Hi, Wi in gc.BS_IMAGES:
        pts = gc.bs_fixed_coords(Hi, Wi)
        assert {(0.0, 0.0), (Wi - 1.0, 0.0), (0.0, Hi - 1.0), (Wi - 1.0, Hi - 1.0)} <= set(pts[:4])
        xs, ys = [x for x, _ in pts], [y for _, y in pts]
        assert -0.5 in xs and Wi - 0.5 in xs and -1.0 in ys and float(Hi) in ys and 1e7 in xs and -1e7 in xs and gc.INF in xs
        assert any(x != x for x in xs) and any(y != y for y in ys) and len(pts) <= 300
        for x, y in pts[gc.BS_ZERO]:                                               # these sample zero: non-finite, or no tap inside
            assert not (abs(x) < 1e6 and abs(y) < 1e6) or x <= -1 or x >= Wi or y <= -1 or y >= Hi, (x, y)
    # context split, flow update, pack
    assert {(c["hdim"], c["P"]) for c in gc.cs_cases()} == {(a, b) for a in (1, 128) for b in (1, 257)} and all(c["n"] == 3 for c in gc.cs_cases())
    assert gc.CS_SATURATED == (20.0, -20.0)
    assert gc.FU_SHAPES == ((1, 1, 1), (3, 9, 20), (2, 3, 257)) and gc.FU_DESTS == ("a", "b", "ab", "koct")
    assert gc.FU_KOCT_ROWS == (126, 7, 0) and any(r % 8 == 7 for r in gc.FU_KOCT_ROWS) and gc.FU_KOCT_IMAGE_ROWS == 128
    assert gc.FU_FAR == (3000.0, -3000.0)
    assert {(c["rows"], c["P"]) for c in gc.pk_cases()} == {(r, P) for r in (1, 7, 8, 9, 126, 324) for P in (1, 255, 256, 257)}
    assert all(c["n"] == 3 for c in gc.pk_cases())
    sp = torch.tensor(gc.PK_SPECIAL)
    h = sp.half()
    assert bool(torch.isinf(h).any()) and bool(((h != 0) & (h.abs() < 2.0 ** -14)).any())          # overflow, fp16 subnormals
    assert h[4].item() == 1.0 and h[5].item() == 1.0 + 2.0 ** -9                                    # ties go to even: down, up
    # depthwise 3x3: one pixel, one vec4, both kernels past one workgroup (1024 pixels vec4, 256 scalar)
    assert gc.DW_SHAPES == ((1, 1), (1, 4), (3, 4), (5, 9), (9, 31), (5, 260)) and gc.DW_C == (1, 3) and gc.DW_N == (1, 2)
    assert any(W % 4 == 0 and H * W > 1024 for H, W in gc.DW_SHAPES) and any(W % 4 and H * W > 256 for H, W in gc.DW_SHAPES)


def test_placements_honour_the_entry_points():
    for layout in gc.ELEM:
        for rows, cols in ((1, 1), (7, 5), (324, 257)):
            assert gc.place(layout, rows, cols, False) == (0, -(-rows // 8) * cols * 8 if layout == "koct" else rows * cols)
            for strided in (True, False):
                for k in (0, 1):
                    off, stride = gc.place(layout, rows, cols, True, strided, k)
                    span = gc.place(layout, rows, cols, False)[1]
                    assert off > 0 and (off * gc.ELEM[layout]) % gc.BASE_ALIGN[layout] == 0
                    assert (stride > span and (stride - span) % gc.STRIDE_MULT[layout] == 0) if strided else (stride == span)
                    assert layout != "koct" or stride % 8 == 0
    # an "f32" placement of a W % 4 == 0 image has a stride that is no multiple of 4 floats: sf_dwconv3x3_res takes its scalar kernel
    for H, W in gc.DW_SHAPES:
        if W % 4 == 0:
            assert all(gc.place("f32", 3 * H, W, True, True, k)[1] % 4 for k in (0, 1))
            assert all(gc.place("f32x4", 3 * H, W, True, True, k)[1] % 4 == 0 for k in (0, 1))
    assert gc.place("koct", 9, 5, True, True, 1)[1] % 8 == 0


# ---- 3: teeth ---------------------------------------------------------------------------------------------------------------------
def _ratio(wrong, r64, tol):
    return float((wrong.double() - r64).abs().max()) / tol


def test_teeth_layernorm_one_pass_variance():
    best = 0.0
    for c in gc.ln_cases():
        for eps in gc.LN_EPS:
            x, g, b = draw_ln(c, "mean100")
            r64 = ref_layernorm(x.double(), g.double(), b.double(), eps)
            tol = tol_of(ref_layernorm(x, g, b, eps), r64)
            best = max(best, _ratio(wrong_layernorm_onepass(x, g, b, eps), r64, tol))
    assert best >= 10, best


def test_teeth_attention_scale_and_softmax_axis():
    for wrong in (dict(scale=1.0 / 128), dict(over="t")):
        best = 0.0
        for c in gc.attn_cases():
            if c["C"] != 128 or c["TT"] == 1:
                continue
            for gain in gc.ATTN_GAINS:
                q = draw_attn(c, gain)
                r64 = ref_attn(q.double(), c["B"], c["TT"], c["C"])
                tol = tol_of(ref_attn(q, c["B"], c["TT"], c["C"]), r64, CAP.get(("temporal_attn", gain)))
                best = max(best, _ratio(ref_attn(q.double(), c["B"], c["TT"], c["C"], **wrong), r64, tol))
        assert best >= 10, (wrong, best)


def test_teeth_upsample_neighbour_order_and_factor():
    for c in gc.up_cases():
        if c["nhw"] == (1, 1, 1):
            continue                                       # (one pixel: its 8 neighbours are zero padding either way round)
        flow, mask = draw_up(c, "golden")
        r64 = ref_upsample(flow.double(), mask.double())
        tol = tol_of(ref_upsample(flow, mask), r64)
        assert _ratio(wrong_upsample_transposed(flow.double(), mask.double()), r64, tol) >= 10, c["id"]
        assert _ratio(ref_upsample(flow.double() / 8, mask.double()), r64, tol) >= 10, c["id"]
    flow, mask = draw_up(gc.up_cases()[0], "golden")                                # the factor shows at one pixel too
    r64 = ref_upsample(flow.double(), mask.double())
    assert _ratio(ref_upsample(flow.double() / 8, mask.double()), r64, tol_of(ref_upsample(flow, mask), r64)) >= 10


def test_teeth_bilinear_rounding_and_mask_bounds():
    for c in gc.bs_cases():
        img, crd = draw_bs(c)
        r64 = ref_bilinear(img.double(), crd.double())
        tol = tol_of(ref_bilinear(img, crd), r64, CAP[("bilinear", None)])
        assert _ratio(ref_bilinear(img.double(), crd.double(), rounding=torch.round), r64, tol) >= 10, c["id"]
        _, _, Hi, Wi = c["img"]
        if Hi > 1:
            m = ref_bilinear_mask(crd, Hi, Wi)
            assert not torch.equal(m, ref_bilinear_mask(crd, Hi, Wi, strict=False)), c["id"]
            assert m.view(c["img"][0], -1)[:, :4].sum() == 0 and 0 < m.sum() < m.numel()        # 0 at exactly x = 0 and x = Wi - 1
        assert bool((r64.view(*r64.shape[:2], -1)[:, :, gc.BS_ZERO] == 0).all())              # out of range, non-finite: zero


def test_teeth_pack_truncation():
    hit = 0
    for c in gc.pk_cases():
        x = draw_pk(c)
        ok = torch.isfinite(x.half()) & (x.abs() >= 2.0 ** -14)                    # (the bit trick is a truncation for fp16 normals)
        hit += int((wrong_pack_truncate(x)[ok].view(torch.int16) != x.half()[ok].view(torch.int16)).any())
    assert hit == len(gc.pk_cases()) - 1                   # (all but rows = 1, P = 1: its three values are +-7e4 and 1e-7)


def test_exact_restatements_behave_as_the_gpu_file_assumes():
    """TT = 1: the attention is v (float32 evaluation included); flow_update without delta leaves the coordinates alone."""
    c = next(c for c in gc.attn_cases() if c["TT"] == 1 and c["C"] == 128)
    q = draw_attn(c, 4)
    assert torch.equal(ref_attn(q, c["B"], 1, 128), q[:, 256:])
    c = gc.fu_cases()[1]
    coords, delta = draw_fu(c)
    assert ref_flow_update(coords, None, *c["nhw"])[0] is coords
    assert float(ref_flow_update(coords, delta, *c["nhw"])[1].abs().max()) > 2900
    for cs in gc.cs_cases():
        t, r = ref_context_split(draw_cs(cs).double(), cs["hdim"])
        assert float(t.abs().max()) > 1 - 1e-15 and bool((r >= 0).all())           # tanh saturates at +-20
