"""Cases, float64 unit references, class emulation, wrong variants and bounds of tests/test_gpu_update_stages.py: what
HotPathEngine._setup and ._iteration compose (streamflow_amd/engine.py), unit by unit.  Pure CPU torch; tests/test_update_cases_cpu.py
pins what is here.  The conventions are those of tests/twins_cases.py (dev, r16, split_weight, MARGIN, SEPARATION).

Taps.  `_Plan.taps()` hands out fp32 clones of the plan's buffers after a forward: after forward(iters=0) what the setup wrote (nets0,
inps, qk, volume), after forward(iters=1, flow_init=...) what ONE iteration wrote.  A unit's reference is the oracle's own function
(oracle/streamflow_oracle.py) in float64 on the GPU's PREVIOUS taps: errors do not accumulate and a failure names its unit.  Within
the iteration nets is overwritten in place and flow_update rewrites the flow rows of mf: the hidden state before the iteration is the
nets0 tap of the iters=0 call on the same inputs, the flow and the coordinates before it are fp32(grid + flow_init) - grid (pre_state).
The reference takes the weights as packed (effective_params): (hi + lo) / scale, hi / scale for a single-product layer, a '<block>.dw'
of the single-depthwise set and everything under precision='f16', and pw_res - I where the route folds the pw residual.

Units (UNITS): context qk volume lookup convf1 convf2 convc1 convc2 conv temporal gma gru flow_head flow_update mask0 mask_up, and from
the all_masks=True call mask2 and upsample (the mask as a tensor of its own).

Yardsticks, both (rms, max) of a difference to that float64 reference over the unit's tap:
    e32    the oracle's unit in float32 (torch CPU) on the same input;
    e_cls  the unit in float64 with a round to fp16 wherever the code documents one (emulate_unit): every GEMM activation operand in
           F16X2 / F16 (ops.gemm), the stored hand-over tensors of the route (SkRoute.x2 / x3 as fp16 rows, the k-octet-only
           tensors corr, f128, cor256, cat256), fp16(x2) into the depthwise layer, the temporal block's fp16 hand-overs
           (csrc/temporal.hip), q / k / v and the softmax weights per flash_qk_products (tests/attn_cases.py CLASSES gma1 / gma3,
           restated for whole grids in gma_model and pinned to it on the CPU), the fp16 matrix of the materialised form, fp16
           features and fp16 cells of corr_dtype='f16' (tests/corr_cases.py class 'b16' / 'f16', restated in corr16 and pinned).
           The SK blocks compose tests/test_chain_cases_cpu.py's ref_pair / ref_tail.
Bounds (bound()): fp32 and f16x3  3 e32 (rms) and 3 e32 (max); f16x2 and f16  2 e_cls (rms) and 4 e_cls (max) -- twins_cases.MARGIN.
The global aggregation keeps its softmax weights (and, fused, v) in fp16 in EVERY split class (presets.py: 'only the softmax weights
and v enter the second contraction in fp16'): its yardstick is e_cls with the reduced margin wherever facts()['gma'] rounds anything,
e32 with margin 3 only where nothing is rounded (precision='fp32').  UNIT_MARGIN holds the raised margins, each with its reason.
Units that round nothing (flow_update, the ReLU half of context) are compared exactly.

Wrong variants of the reference (run_unit(wrong=...)): 'a' mfg and mft swapped in the GRU's concat, 'b' the flow rows of mf taken
after the update, 'c' mask alpha 0.25 dropped, 'd' the GMA scale 128^-0.5 dropped, 'e' the lookup of pair t at pair t + 1's
coordinates, 'f' convc1 without its final GELU, 'g' the flow head fed pair-major images instead of the (T C) grouping."""
import functools

import torch
import torch.nn.functional as F

from oracle import streamflow_oracle as orc
from streamflow_amd import presets, synthetic as syn
from tests import test_chain_cases_cpu as chain
from tests.twins_cases import MARGIN, SEPARATION, dev, r16, split_weight  # noqa: F401  (one set of conventions)

HDIM, D = 128, 256
# name -> (clips, T, h, w)
CASES = {"S": (2, 3, 16, 24), "R": (1, 4, 17, 21), "F": (3, 4, 48, 68)}
CONFIGS = ("fp32", "fp32_class", "config2_fp16", "config2_mixed", "f16", "f16x3_matrix")
PRESETS = ("fp32_class", "config2_fp16", "config2_mixed")
CLASS_OF = {"fp32": "fp32", "fp32_class": "f16x3", "config2_fp16": "f16x2", "config2_mixed": "f16x2", "f16": "f16", "f16x3_matrix": "f16x3"}
REDUCED = ("f16x2", "f16")
SETUP_UNITS = ("context", "qk", "volume")
ITER_UNITS = ("lookup", "convf1", "convf2", "convc1", "convc2", "conv", "temporal", "gma", "gru", "flow_head", "flow_update", "mask0",
              "mask_up")
MASK_UNITS = ("mask2", "upsample")                            # from the all_masks=True call: the mask materialised
UNITS = SETUP_UNITS + ITER_UNITS + MASK_UNITS
SK_UNITS = {"convf2": ("update_block.encoder.convf2", syn.K_CONV), "convc1": ("update_block.encoder.convc1", syn.K_CONV),
            "convc2": ("update_block.encoder.convc2", syn.K_CONV), "conv": ("update_block.encoder.conv", syn.K_CONV),
            "gru": ("update_block.gru", syn.GRU_CONV), "flow_head": ("update_block.flow_head", syn.K_CONV)}
EXACT_UNITS = ("flow_update",)
# no class separation to assert: no contraction -- and mask_up, whose tap is the upsampled flow: the fp32 arithmetic on 8 x flow is
# within a factor 30 of what fp16 operands of mask.2 move (3 e32 does not fit under 0.1 e_cls); mask.2 is separated as unit mask2
NO_GEMM = ("context", "lookup", "flow_update", "upsample", "mask_up")
WRONG = {"a": "gru", "b": "gru", "c": "mask_up", "d": "gma", "e": "lookup", "f": "convc1", "g": "flow_head"}
PARAM_SEED, FEATURE_SEED, FLOW_SEED = 57, 58, 59
# (unit, class) -> (rms, max): margins raised after measurement, each 3 times a CPU model of its reason (the models: end of this file;
# their ratios to e32: tests/test_update_cases_cpu.py::test_models_of_the_raised_margins).
# mask0: a bare K = 9 * 128 = 1152 convolution + ReLU, no residual.  The GEMM adds the K products of an output in ONE fp32 chain, the
#   CPU's float32 convolution in interleaved partial sums: single_chain_mask0 alone is 2.73 e32 in rms and 4.1 - 4.3 in max (measured
#   on the GPU: 2.73 and 4.3 - 5.4 in fp32, 2.03 and 3.2 - 3.8 in f16x3, whose three products per k go into the same chain).
# convf1 in f16x3: a bare K = 2 layer on the flow.  split8() cuts an activation towards zero twice, to within 2^-20 |x|; with two terms
#   and no residual nothing dilutes that: the unit on split8_image(flow) alone is 2.45 - 2.6 e32 in rms, 4.3 - 4.7 in max.
UNIT_MARGIN = {("mask0", "fp32"): (8.2, 12.9), ("mask0", "f16x3"): (8.2, 12.9), ("convf1", "f16x3"): (7.8, 14.0)}
TB = "update_block.transformer_block.transformer_block"
ENGINE_KW = {"fp32": dict(precision="fp32"), "f16": dict(precision="f16"), "f16x3_matrix": dict(precision="f16x3", gma_mode="matrix")}


def engine_kwargs(cfg):
    return dict(ENGINE_KW[cfg]) if cfg in ENGINE_KW else presets.engine_kwargs(cfg)


def fills(c):
    """engine.resolve_skblock's `fills` for the chains case c runs: half-batch chains when the clip count is even."""
    B, T, h, w = CASES[c]
    chains = 2 if B % 2 == 0 else 1
    return (B // chains) * (T - 1) * h * w >= 4 * 7040


@functools.lru_cache(maxsize=None)
def params(T):
    return syn.make_params(PARAM_SEED, T)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """(fmaps [B, T, D, h, w], cnets [B, T - 1, 256, h, w], flow_init: T - 1 tensors [B, 2, h, w] of about 2 px), fp32."""
    B, T, h, w = CASES[c]
    f, cn = syn.make_features(FEATURE_SEED, B, T, h, w)
    return f, cn, [syn.randn(FLOW_SEED, f"update_stages.{c}.{i}", (B, 2, h, w), 2.0) for i in range(T - 1)]


def pre_state(c):
    """(coords, flow) [n, 2, h, w] fp32 as HotPathEngine._begin leaves them: fp32(grid + flow_init) and that minus the grid."""
    B, T, h, w = CASES[c]
    grid = orc.coords_grid(B * (T - 1), h, w)
    coords = grid + torch.stack(inputs(c)[2], dim=1).reshape(B * (T - 1), 2, h, w)
    return coords, coords - grid


def images_of(c):
    """Image indices whose float64 references are evaluated: all, in case F those of the first and the last clip (whole clips)."""
    B, T, h, w = CASES[c]
    clips = range(B) if c != "F" else (0, B - 1)
    return [b * (T - 1) + t for b in clips for t in range(T - 1)]


# ---- what a configuration does at a case (engine.py, restated; asserted against the plan on the GPU) ---------------------------------
def facts(cfg, c):
    """dict: cls, reduced, hand (fp16 hand-overs, k-octet copies, fold: reduced and P % 4 == 0), corr16 (fp16 volume cells), lookup16
    (the features leave the lookup as fp16 k-octets only), gma (form and what it rounds), singles (layer names)."""
    B, T, h, w = CASES[c]
    P = h * w
    cls = CLASS_OF[cfg]
    kw = engine_kwargs(cfg)
    reduced = cls in REDUCED
    hand = reduced and P % 4 == 0
    corr16 = kw.get("corr_dtype", "f32") == "f16"
    mode = kw.get("gma_mode", "auto")
    if cls == "fp32":
        gma = dict(form="matrix", q16=False, k16=False, w16=None, v16=False)
    elif mode in ("auto", "matrix"):
        # materialised (every case here: P * P < 2^28).  The matrix is kept in fp16 at even P; at odd P it stays fp32 and attn @ v
        # takes it as its B operand: rounded to fp16 on load under F16, split by split8() under F16X3 -- softmax weights of about 1 / P
        # have their lo halves among fp16's subnormals, so the pair holds them to 2^-24 ABSOLUTE, 2^-16 of a weight at P = 357
        w16 = "norm" if (P % 2 == 0 or cls == "f16") else "split8"
        gma = dict(form="matrix", q16=cls == "f16", k16=cls == "f16", w16=w16, v16=cls == "f16")
    else:                                                     # fused: flash_qk_products 3 (q, k hi + lo) or 1 (fp16)
        one = kw["flash_qk_products"] == 1
        gma = dict(form="flash", q16=one, k16=one, w16="exp2", v16=True)
    return dict(cfg=cfg, cls=cls, reduced=reduced, hand=hand, corr16=corr16, lookup16=corr16 and hand, gma=gma,
                singles=tuple(kw.get("single_layers") or ()), T=T, B=B, h=h, w=w)


def gma_rounds(f):
    g = f["gma"]
    return bool(g["q16"] or g["k16"] or g["w16"] or g["v16"])


# ---- the weights as packed ---------------------------------------------------------------------------------------------------------
def layer_key(name):
    """engine.HotPathWeights.layers() name -> reference state-dict key of the weight."""
    plain = {"to_qk": "att.to_qk.weight", "convf1": "update_block.encoder.convf1.weight", "to_v": "update_block.aggregator.to_v.weight",
             "qkv": TB + ".attn.qkv.weight", "proj": TB + ".attn.proj.weight", "fc1": TB + ".mlp.fc1.weight", "fc2": TB + ".mlp.fc2.weight",
             "mask0": "update_block.mask.0.weight", "mask2": "update_block.mask.2.weight"}
    if name in plain:
        return plain[name]
    blk, lay = name.split(".")
    return f"{SK_UNITS[blk][0]}.{lay[:4]}.{lay[5]}.weight" if lay != "pw" else f"{SK_UNITS[blk][0]}.pw.weight"


def layer_names():
    from streamflow_amd.engine import HotPathWeights as H
    return list(H.PLAIN_LAYERS) + [f"{b}.{l}" for b in H.SK_BLOCKS for l in H.SK_LAYERS]


@functools.lru_cache(maxsize=None)
def _effective(T, cls, singles, fold):
    p = params(T)
    out = {k: t.double() for k, t in p.items()}
    if cls == "fp32":
        return out
    one = lambda n: cls == "f16" or n in singles              # noqa: E731
    for n in layer_names():
        k = layer_key(n)
        hi, lo, s = split_weight(p[k])
        out[k] = (hi if one(n) else hi + lo) / s
        if fold and n.endswith(".pw"):                        # SKBlockWeights.pw_res: the residual folded, then split
            w = p[k]
            eye = torch.eye(w.shape[0]).reshape(w.shape[0], w.shape[0], 1, 1)
            hi, lo, s = split_weight(w + eye)
            res = (hi if one(n) else hi + lo) / s
            out[k.replace(".pw.", ".pw_res.")] = res
            out[k] = res - eye.double()
    for blk, (prefix, _) in SK_UNITS.items():
        if cls == "f16" or (blk + ".dw") in singles:          # the K x K depthwise weights as one fp16 value (no pre-scale)
            out[prefix + ".conv_list.1.weight"] = r16(p[prefix + ".conv_list.1.weight"])
    return out


def effective_params(cfg, c):
    """float64 parameters as configuration cfg multiplies them at case c (module docstring)."""
    f = facts(cfg, c)
    return _effective(f["T"], f["cls"], f["singles"], f["hand"])


# ---- the units, from the oracle's own functions ---------------------------------------------------------------------------------------
def dwconv(x, w, b, padding, groups):
    """F.conv2d for a depthwise K x K layer.  torch's float64 depthwise convolution takes 2.8 s for one layer of case F; in float64
    and K >= 7 the same sums are formed through an FFT (the linear convolution with the flipped kernel, cropped), which agrees with
    it to 1e-13 of the largest value (tests/test_update_cases_cpu.py) -- six orders below the fp32 yardstick."""
    k = w.shape[-1]
    if x.dtype != torch.float64 or groups != x.shape[1] or w.shape[1] != 1 or k < 7:
        return F.conv2d(x, w, b, padding=padding, groups=groups)
    h, wd = x.shape[-2:]
    size = (h + k - 1, wd + k - 1)
    y = torch.fft.irfft2(torch.fft.rfft2(x, s=size) * torch.fft.rfft2(torch.flip(w[:, 0], (-2, -1)), s=size)[None], s=size)
    o = k - 1 - padding
    y = y[..., o:o + h, o:o + wd]
    return y if b is None else y + b[None, :, None, None]


class _OracleF:
    """torch.nn.functional as the oracle sees it while an SK block runs: conv2d sends depthwise layers through dwconv."""

    def __getattr__(self, name):
        return getattr(F, name)

    @staticmethod
    def conv2d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        if groups > 1 and stride == 1 and dilation == 1:
            return dwconv(x, w, b, padding, groups)
        return F.conv2d(x, w, b, stride, padding, dilation, groups)


def _skblock(x, p, prefix, k_conv):
    """orc.skblock, its depthwise layers through dwconv."""
    keep, orc.F = orc.F, _OracleF()
    try:
        return orc.skblock(x, p, prefix, k_conv)
    finally:
        orc.F = keep


def _lookup(levels, coords):
    """orc.corr_lookup without its final .float(): levels [n * P, 1, hl, wl] per level, coords [n, 2, h, w]."""
    n, _, h, w = coords.shape
    pts = coords.permute(0, 2, 3, 1).reshape(n * h * w, 1, 1, 2)
    d = torch.linspace(-4, 4, 9, dtype=coords.dtype)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).view(1, 9, 9, 2)
    outs = [orc.bilinear_sampler(vol, pts / 2 ** l + delta).reshape(n, h, w, 81) for l, vol in enumerate(levels)]
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def _tokens(x, B):
    n, C, h, w = x.shape
    return x.reshape(B, n // B, C, h * w).permute(0, 3, 1, 2).reshape(B * h * w, n // B, C)


def _untokens(tok, B, h, w):
    S, Tn, C = tok.shape
    return tok.reshape(B, h * w, Tn, C).permute(0, 2, 3, 1).reshape(B * Tn, C, h, w)


def _eye_qk(dtype):
    return torch.eye(2 * HDIM, dtype=dtype).reshape(2 * HDIM, 2 * HDIM, 1, 1)


def run_unit(unit, x, p, Pn, wrong=None):
    """One unit in the dtype of x and p.  x: dict of the unit's inputs, images [n, C, h, w] with n a multiple of the Pn pairs of
    a clip (whole clips); p: parameters under the reference's keys.  Returns {tap name: tensor}."""
    assert wrong is None or WRONG[wrong] == unit
    u = "update_block"
    if unit == "context":
        cn = x["cnets"]
        return {"nets0": torch.tanh(cn[:, :HDIM]), "inps": torch.relu(cn[:, HDIM:])}
    if unit == "qk":
        return {"qk": F.conv2d(x["inps"], p["att.to_qk.weight"])}
    if unit == "volume":                                      # x: f1, f2 [n, D, h, w] -> four levels [n, P, hl, wl]
        n, _, h, w = x["f1"].shape
        return {"volume": [lv.reshape(n, h * w, *lv.shape[-2:]) for lv in orc.corr_pyramid(x["f1"], x["f2"])]}
    if unit == "lookup":
        coords = x["coords"]
        if wrong == "e":                                      # pair t at pair t + 1's coordinates (cyclic within the clip)
            n = coords.shape[0]
            coords = coords.reshape(n // Pn, Pn, *coords.shape[1:]).roll(-1, dims=1).reshape(coords.shape)
        return {"corr": _lookup([lv.reshape(-1, 1, *lv.shape[-2:]) for lv in x["volume"]], coords)}
    if unit == "convf1":
        return {"f128": F.conv2d(x["flow"], p[u + ".encoder.convf1.weight"], p[u + ".encoder.convf1.bias"])}
    if unit in ("convf2", "convc1", "convc2", "conv"):
        y = _skblock(x["x"], p, *SK_UNITS[unit])
        if unit == "convc1" and wrong != "f":
            y = orc.gelu(y)
        return {{"convf2": "cat256.flo", "convc1": "cor256", "convc2": "cat256.cor", "conv": "mf"}[unit]: y}
    if unit == "temporal":
        n, _, h, w = x["mf"].shape
        return {"mft": _untokens(orc.temporal_block(_tokens(x["mf"], n // Pn), p, TB), n // Pn, h, w)}
    if unit == "gma":
        qk = x["qk"]
        if wrong == "d":
            qk = torch.cat([qk[:, :HDIM] * HDIM ** 0.5, qk[:, HDIM:]], dim=1)
        attn = orc.gma_attention(qk, _eye_qk(qk.dtype))       # (the q k products of the GPU's own qk tap: an identity to_qk)
        return {"mfg": orc.gma_aggregate(attn, x["mf"], p[u + ".aggregator.to_v.weight"], p[u + ".aggregator.gamma"])}
    if unit == "gru":
        parts = [x["nets"], x["inps"], x["mf"], x["mfg"], x["mft"]]
        if wrong == "a":
            parts[3], parts[4] = parts[4], parts[3]
        return {"nets": _skblock(torch.cat(parts, dim=1), p, *SK_UNITS["gru"])}
    if unit == "flow_head":
        nets = x["nets"]
        n, C, h, w = nets.shape
        if wrong == "g":                                      # image = pair * clips + clip
            nets = nets.reshape(Pn, n // Pn, C, h, w).transpose(0, 1).reshape(n, C, h, w)
        return {"delta": _skblock(nets.reshape(n // Pn, Pn * C, h, w), p, *SK_UNITS["flow_head"]).reshape(n, 2, h, w)}
    if unit == "flow_update":
        n, _, h, w = x["coords"].shape
        coords1 = x["coords"] + x["delta"]
        return {"coords1": coords1, "flow": coords1 - orc.coords_grid(n, h, w).to(coords1.dtype)}
    if unit == "mask0":
        return {"m256": torch.relu(F.conv2d(x["nets"], p[u + ".mask.0.weight"], p[u + ".mask.0.bias"], padding=1))}
    if unit in ("mask2", "mask_up"):
        m = F.conv2d(x["m256"], p[u + ".mask.2.weight"], p[u + ".mask.2.bias"])
        m = m if wrong == "c" else 0.25 * m
        return {"mask": m} if unit == "mask2" else {"up": orc.upsample_flow(x["flow"], m)}
    if unit == "upsample":
        return {"up": orc.upsample_flow(x["flow"], x["mask"])}
    raise KeyError(unit)


# ---- class emulation -----------------------------------------------------------------------------------------------------------------
def corr16(f1, f2):
    """fp16 features, one product per k, fp16 cells (tests/corr_cases.py classes 'b16' / 'f16' without the fp32 accumulation steps):
    f1, f2 [n, D, h, w] float64 -> four levels [n, P, hl, wl]."""
    n, _, h, w = f1.shape
    lv = run_unit("volume", dict(f1=r16(f1), f2=r16(f2)), None, 1)["volume"]
    return [r16(v) for v in lv]


def gma_model(qk, v, mf, gamma, g, scale=HDIM ** -0.5):
    """mf + gamma * attn v with the roundings g = facts()['gma'] names; qk [n, 256, P], v, mf [n, 128, P], float64.
    'flash' is tests/attn_cases.py's model of CLASSES gma1 / gma3 for whole grids: q times fp32(scale log2 e) in fp32, fp16 q and k
    at one product, weights fp16(exp2(l - max)) normalised by the sum of the ROUNDED weights, v fp16.  'matrix': logits at the GEMM's
    class (fp16 q, k under F16), the normalised fp32 softmax rounded to fp16 where the matrix is kept in fp16, v fp16 under F16."""
    rq = r16 if g["q16"] else (lambda t: t)
    rk = r16 if g["k16"] else (lambda t: t)
    rv = r16 if g["v16"] else (lambda t: t)
    q, k = qk[:, :HDIM], qk[:, HDIM:]
    if g["form"] == "flash":
        qs = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.44269504088896340736, dtype=torch.float32))
        l = torch.einsum("ndi,ndj->nij", rq((q.float() * qs).double() if g["q16"] or g["w16"] else q * qs), rk(k))
        wgt = torch.exp2(l - l.max(dim=2, keepdim=True).values)
        if g["w16"]:
            wgt = r16(wgt)
        a = wgt / wgt.sum(dim=2, keepdim=True)
    else:
        a = torch.softmax(scale * torch.einsum("ndi,ndj->nij", rq(q), rk(k)), dim=2)
        if g["w16"]:
            a = split8_image(a.float()) if g["w16"] == "split8" else r16(a)
    return mf + gamma * torch.einsum("nij,ndj->ndi", a, rv(v))


def _lin4(x, w, b=None):
    return F.conv2d(x, w.reshape(w.shape[0], -1, 1, 1), b)


def _emulate_sk(unit, x, pe, f, rounding):
    """An SK block as resolve_skblock routes it: the front half is ref_pair (mode 1), the back half ref_tail where the route folds
    (x3 handed over as fp16 rows through pw_res), else the pw GEMM with its fp32 residual and ref_pair (mode 0)."""
    prefix, k_conv = SK_UNITS[unit]
    rnd = r16 if rounding else (lambda t: t)
    hand = f["hand"]                                          # (the folded data flow also with rounding=False: pinned to the oracle)
    g = lambda nm: pe[f"{prefix}.{nm}"]                                   # noqa: E731
    W = lambda nm: g(nm + ".weight").reshape(g(nm + ".weight").shape[0], -1)      # noqa: E731
    n, C, h, w = x.shape
    flat = x.reshape(n, C, h * w)
    x2 = chain.ref_pair(W("ffn1.0"), g("ffn1.0.bias"), W("ffn1.2"), g("ffn1.2.bias"), rnd(flat), 1, dw_w=g("conv_list.0.weight").reshape(-1),
                        dw_b=g("conv_list.0.bias"), resid=flat, round16=rounding)
    if hand and rounding:
        x2 = r16(x2)                                          # SkRoute.x2 == 'f16': stored as fp16 rows, the depthwise layer's residual too
    x2 = x2.reshape(n, C, h, w)
    k = k_conv[1]
    x3 = F.gelu(x2 + dwconv(rnd(x2), g("conv_list.1.weight"), g("conv_list.1.bias"), k // 2, C)).reshape(n, C, h * w)
    final = unit == "convc1"
    if hand:
        res = pe.get(prefix + ".pw_res.weight")               # (absent in the weights of a class that never folds: W + I unsplit)
        Wres = W("pw") + torch.eye(C, dtype=torch.float64) if res is None else res.reshape(C, C)
        y = chain.ref_tail(Wres, g("pw.bias"), W("ffn2.0"), g("ffn2.0.bias"), W("ffn2.2"), g("ffn2.2.bias"), rnd(x3), gelu_out=final,
                           round16=rounding)
    else:
        x4 = F.gelu(x3 + chain._lin(W("pw"), g("pw.bias"), rnd(x3)))
        y = chain.ref_pair(W("ffn2.0"), g("ffn2.0.bias"), W("ffn2.2"), g("ffn2.2.bias"), rnd(x4), 0, gelu_out=final, round16=rounding)
    return y.reshape(n, -1, h, w)


def _emulate_temporal(mf, pe, f, Pn, rounding):
    """csrc/temporal.hip in one launch (k-octet copies present): input AND residual are fp16(mf); LN1, q / k / v, the softmax weights,
    the attention output, LN2 and the MLP's hidden tensor enter their products as fp16.  Seven launches (fp32 planes): the GEMM
    operands alone (LN1, attention output, LN2, hidden); the attention core is fp32."""
    rnd = r16 if rounding else (lambda t: t)
    fused = f["hand"] and rounding
    core = r16 if fused else (lambda t: t)
    g = lambda nm: pe[f"{TB}.{nm}"]                            # noqa: E731
    n, C, h, w = mf.shape
    B = n // Pn
    x = _tokens(core(mf), B)
    y = rnd(orc.layer_norm(x, g("norm1.weight"), g("norm1.bias")))
    qkv = core(y @ g("attn.qkv.weight").t())
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    a = core(torch.softmax((q * C ** -0.5) @ k.transpose(1, 2), dim=-1))
    x = x + rnd(a @ v) @ g("attn.proj.weight").t() + g("attn.proj.bias")
    y = rnd(orc.layer_norm(x, g("norm2.weight"), g("norm2.bias")))
    y = rnd(orc.gelu(y @ g("mlp.fc1.weight").t() + g("mlp.fc1.bias")))
    return _untokens(x + y @ g("mlp.fc2.weight").t() + g("mlp.fc2.bias"), B, h, w)


def emulate_unit(unit, x, pe, f, rounding=True):
    """The unit in float64 with the roundings of facts f (module docstring); rounding=False: none -- must then be run_unit."""
    u, Pn = "update_block", f["T"] - 1
    rnd = r16 if (rounding and f["reduced"]) else (lambda t: t)
    out16 = r16 if (rounding and f["hand"]) else (lambda t: t)            # the k-octet-only tensors of the motion encoder
    x = {k: ([t.double() for t in v] if isinstance(v, list) else v.double()) for k, v in x.items()}
    if unit in ("context", "flow_update", "upsample"):
        return run_unit(unit, x, pe, Pn)
    if unit == "qk":
        return run_unit(unit, dict(inps=rnd(x["inps"])), pe, Pn)
    if unit == "volume":
        return {"volume": corr16(x["f1"], x["f2"])} if (rounding and f["corr16"]) else run_unit(unit, x, pe, Pn)
    if unit == "lookup":
        y = run_unit(unit, x, pe, Pn)["corr"]
        return {"corr": r16(y) if (rounding and f["lookup16"]) else y}
    if unit == "convf1":
        return {"f128": out16(run_unit(unit, dict(flow=rnd(x["flow"])), pe, Pn)["f128"])}
    if unit in SK_UNITS:
        if unit == "gru":
            inp = torch.cat([x["nets"], x["inps"], x["mf"], x["mfg"], x["mft"]], dim=1)
        elif unit == "flow_head":
            n, C, h, w = x["nets"].shape
            inp = x["nets"].reshape(n // Pn, Pn * C, h, w)
        else:
            inp = x["x"]
        y = _emulate_sk(unit, inp, pe, f, rounding and f["reduced"])
        name = {"convf2": "cat256.flo", "convc1": "cor256", "convc2": "cat256.cor", "conv": "mf", "gru": "nets", "flow_head": "delta"}[unit]
        if unit in ("convf2", "convc1", "convc2"):
            y = out16(y)
        return {name: y.reshape(-1, 2, *y.shape[-2:]) if unit == "flow_head" else y}
    if unit == "temporal":
        return {"mft": _emulate_temporal(x["mf"], pe, f, Pn, rounding and f["reduced"])}
    if unit == "gma":
        if not rounding:
            return run_unit(unit, x, pe, Pn)
        n, C, h, w = x["mf"].shape
        v = _lin4(rnd(x["mf"]), pe[u + ".aggregator.to_v.weight"])
        y = gma_model(x["qk"].reshape(n, 2 * HDIM, h * w), v.reshape(n, C, h * w), x["mf"].reshape(n, C, h * w),
                      pe[u + ".aggregator.gamma"], f["gma"])
        return {"mfg": y.reshape(n, C, h, w)}
    if unit == "mask0":
        return run_unit(unit, dict(nets=rnd(x["nets"])), pe, Pn)
    if unit in ("mask2", "mask_up"):
        return run_unit(unit, dict(x, m256=rnd(x["m256"])), pe, Pn)
    raise KeyError(unit)


# ---- yardsticks and bounds -------------------------------------------------------------------------------------------------------------
def _flat(d):
    """{tap: tensor or list of tensors} -> one flat float64 vector per tap."""
    return {k: (torch.cat([t.double().reshape(-1) for t in v]) if isinstance(v, list) else v.double().reshape(-1)) for k, v in d.items()}


def dev_taps(got, want):
    """{tap: (rms, max)}."""
    a, b = _flat(got), _flat(want)
    return {k: dev(a[k], b[k]) for k in b}


def yard_kind(unit, f):
    """'exact', 'e32' (margin 3: the unit rounds nothing below fp32 in this configuration) or 'e_cls' (it does: the reduced margin)."""
    if unit in EXACT_UNITS:
        return "exact"
    if unit == "gma":
        return "e_cls" if gma_rounds(f) else "e32"
    if unit in ("context", "upsample") or (unit == "volume" and not f["corr16"]) or (unit == "lookup" and not f["lookup16"]):
        return "e32"                                          # (fp32 volumes are built from three split products in every class)
    return "e_cls" if f["reduced"] else "e32"


def bound(unit, f, e32, e_cls):
    kind = yard_kind(unit, f)
    m = MARGIN["f16x2"] if kind == "e_cls" else UNIT_MARGIN.get((unit, f["cls"]), MARGIN["fp32"])
    y = e_cls if kind == "e_cls" else e32
    return m[0] * y[0], m[1] * y[1]


def reduced_facts(f):
    """The F16X2 form of the same case with the same weights, for the class separation of the fp32 classes."""
    g = dict(form="flash", q16=True, k16=True, w16="exp2", v16=True)
    return dict(f, cls="f16x2", reduced=True, hand=(f["h"] * f["w"]) % 4 == 0, corr16=True, lookup16=False, gma=g)


def yardsticks(unit, x, cfg, c, separation=False):
    """For one unit on the fp32 inputs x: dict(ref={tap: float64 reference with the configuration's weights}, e32={tap: (rms, max)},
    e_cls={tap: ...} (the configuration's own class emulation), sep={tap: ...} (e_cls of F16X2, on request))."""
    f = facts(cfg, c)
    Pn = f["T"] - 1
    pe = effective_params(cfg, c)
    x64 = {k: ([t.double() for t in v] if isinstance(v, list) else v.double()) for k, v in x.items()}
    ref = run_unit(unit, x64, pe, Pn)
    p32 = {k: t.float() for k, t in pe.items()}
    x32 = {k: ([t.float() for t in v] if isinstance(v, list) else v.float()) for k, v in x.items()}
    out = dict(ref=ref, e32=dev_taps(run_unit(unit, x32, p32, Pn), ref))
    if yard_kind(unit, f) != "e_cls":
        out["e_cls"] = out["e32"]                             # nothing is rounded: the yardstick is e32
    else:
        out["e_cls"] = dev_taps(emulate_unit(unit, x, pe, f), ref)
    if separation:
        out["sep"] = dev_taps(emulate_unit(unit, x, pe, reduced_facts(f)), ref)
    return out


# ---- a unit's inputs from a set of taps; the whole chain on the CPU ------------------------------------------------------------------
OUTPUTS = {"context": ("nets0", "inps"), "qk": ("qk",), "volume": ("volume",), "lookup": ("corr",), "convf1": ("f128",),
           "convf2": ("cat256.flo",), "convc1": ("cor256",), "convc2": ("cat256.cor",), "conv": ("mf",), "temporal": ("mft",),
           "gma": ("mfg",), "gru": ("nets",), "flow_head": ("delta",), "flow_update": ("coords1", "flow"), "mask0": ("m256",),
           "mask_up": ("up",), "mask2": ("mask",), "upsample": ("up",)}


def tap_of(t, name):
    if name == "cat256.cor":
        return t["cat256"][:, :192]
    if name == "cat256.flo":
        return t["cat256"][:, 192:]
    return t[name]


def unit_inputs(unit, t, wrong=None):
    """The inputs of a unit out of taps t (GPU taps, or oracle_taps): also 'cnets', 'f1', 'f2' (the data, image-major) and 'coords0',
    'flow0' (pre_state).  mf as the iteration's consumers read it: rows 0 .. 125 of the tap and the flow BEFORE the update."""
    mf = lambda: torch.cat([t["mf"], t["flow" if wrong == "b" else "flow0"]], dim=1)          # noqa: E731
    if unit == "context":
        return dict(cnets=t["cnets"])
    if unit == "volume":
        return dict(f1=t["f1"], f2=t["f2"])
    if unit == "lookup":
        return dict(volume=t["volume"], coords=t["coords0"])
    if unit == "gru":
        return dict(nets=t["nets0"], inps=t["inps"], mf=mf(), mfg=t["mfg"], mft=t["mft"])
    if unit == "gma":
        return dict(qk=t["qk"], mf=mf())
    if unit == "temporal":
        return dict(mf=mf())
    if unit == "flow_update":
        return dict(coords=t["coords0"], delta=t["delta"])
    if unit in ("mask_up", "mask2"):
        return dict(m256=t["m256"], flow=t["flow"])
    if unit == "upsample":
        return dict(flow=t["flow"], mask=t["mask"])
    return {"qk": dict(inps=t.get("inps")), "convf1": dict(flow=t["flow0"]), "convf2": dict(x=t.get("f128")), "convc1": dict(x=t.get("corr")),
            "convc2": dict(x=t.get("cor256")), "conv": dict(x=t.get("cat256")), "flow_head": dict(nets=t.get("nets")),
            "mask0": dict(nets=t.get("nets"))}[unit]


def data_taps(c, imgs=None):
    """cnets, f1, f2 [n, ., h, w] (image = clip * pairs + pair) and the state before the iteration, fp32; imgs: those images only."""
    B, T, h, w = CASES[c]
    n = B * (T - 1)
    fm, cn, _ = inputs(c)
    coords, flow = pre_state(c)
    t = dict(cnets=cn.reshape(n, 2 * HDIM, h, w), f1=fm[:, :-1].reshape(n, D, h, w), f2=fm[:, 1:].reshape(n, D, h, w), coords0=coords,
             flow0=flow)
    return t if imgs is None else {k: v[imgs] for k, v in t.items()}


def oracle_taps(c, p, dtype=torch.float64):
    """Every unit on the taps before it, no GPU: the taps dict of one iteration in `dtype` with parameters p."""
    Pn = CASES[c][1] - 1
    t = {k: v.to(dtype) for k, v in data_taps(c).items()}
    for u in UNITS:
        if u == "mask2":
            continue                                          # (mask_up holds the same layer; 'upsample' below needs the tensor)
        if u == "upsample":
            t["mask"] = run_unit("mask2", unit_inputs("mask2", t), p, Pn)["mask"]
        out = run_unit(u, unit_inputs(u, t), p, Pn)
        if u in ("convf2", "convc2"):
            t.setdefault("cat256.parts", {})[u] = next(iter(out.values()))
            if len(t["cat256.parts"]) == 2:
                t["cat256"] = torch.cat([t["cat256.parts"]["convc2"], t["cat256.parts"]["convf2"]], dim=1)
            continue
        t.update(out)
    del t["cat256.parts"]
    return t


# ---- CPU models of the raised margins (UNIT_MARGIN) ------------------------------------------------------------------------------------
def split8_image(x):
    """hi + lo of csrc/split_operand.h split8() (tests/dwconv_cases.py restates it bit by bit): what a three-product GEMM multiplies in
    place of an fp32 activation -- cut towards zero twice, within 2^-20 |x|, and within 2^-24 ABSOLUTE where lo is an fp16 subnormal."""
    from tests.dwconv_cases import split8
    hi, lo = split8(x.double().numpy())
    return torch.from_numpy(hi + lo)


def single_chain_mask0(nets, p):
    """mask.0 (3 x 3, K = 9 * 128 = 1152, ReLU) with the K products of an output added one after the other into ONE fp32 accumulator
    (one rounding per step, as a fused multiply-add chain), in the packed order k = (ky * 3 + kx) * 128 + c.  nets fp32 [n, 128, h, w]."""
    n, C, h, w = nets.shape
    cols = F.unfold(nets.float(), 3, padding=1).reshape(n, C, 9, h * w).permute(0, 2, 1, 3).reshape(n, 9 * C, h * w)
    wt = p["update_block.mask.0.weight"].float().permute(0, 2, 3, 1).reshape(-1, 9 * C)
    acc = torch.zeros(n, wt.shape[0], h * w, dtype=torch.float32)
    for k in range(9 * C):
        acc = (acc.double() + wt[None, :, k, None].double() * cols[:, None, k, :].double()).float()
    acc = (acc.double() + p["update_block.mask.0.bias"].double()[None, :, None]).float()
    return torch.relu(acc).reshape(n, -1, h, w)
