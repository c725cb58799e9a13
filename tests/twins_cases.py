"""Cases, float64 unit references, class emulation, wrong variants and bounds of tests/test_gpu_twins_stages.py: the Twins_CSC encoder
(streamflow_amd/encoders.py) unit by unit.  Pure CPU torch / numpy; tests/test_twins_cases_cpu.py pins what is here.

Units.  `Twins_CSC.forward(..., taps=d)` stores the fp32 token planes [B, E_i, gh_i, gw_i] after each of the eight steps
embed0, block0.0, peg0, block0.1, embed1, block1.0, peg1, block1.1.  A unit's reference is the oracle's own function (patch_embed,
block, pos_conv of oracle/twins_oracle.py) in float64 on the PREVIOUS tap (the images for embed0): errors do not accumulate and a
failure names its unit.  In the split classes the reference takes the weights as packed (effective_params: (hi + lo) / scale, hi
alone in F16), so the weight split is not charged to the kernels.

Yardsticks, both (rms, max) of a difference to that float64 reference over the whole tap:
    e32    the oracle's unit in float32 (torch CPU) on the same input;
    e_cls  the class emulation: the unit in float64 with a round to fp16 wherever the code documents one -- every GEMM activation
           operand (ops.py: PRECISION_F16X2 / _F16), the hand-over tensors (the same roundings, stored), q / k / v and the softmax
           weights of the matrix-core attention (tests/attn_cases.py: class 'koct' behind a k-octet qkv, 'x1' behind fp32 planes,
           'fp32' for exact_attention), and in F16 the weights' hi image.  The positional conv rounds nothing in any class:
           its e_cls is e32.
Bounds (bound()): fp32 and f16x3  3 e32 (rms) and 3 e32 (max): a different summation order and nothing else;
                  f16x2 and f16   2 e_cls (rms) and 4 e_cls (max): roundings inside the cores that the emulation may not model
                                  and fp32 accumulation; the max of rounding noise is heavy-tailed.
UNIT_MARGIN holds the units whose margin was raised after measurement, each with its reason.

Wrong variants of the reference (run_unit(wrong=...)): 'a' pad tokens left out of the window softmax, 'b' frames attended one by
one instead of stacked along the height, 'c' the sr convolution's remainder zero-padded instead of dropped, 'd' eps 1e-5 in the
blocks' LayerNorms.  tests/test_twins_cases_cpu.py asserts that the bounds above tell each of them from the right reference."""
import contextlib
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import twins_oracle as two
from streamflow_amd import synthetic as syn
from tests import attn_cases as ac

CASES = ((1, 4, 32, 64), (2, 3, 40, 72), (1, 2, 56, 112), (2, 4, 24, 40))            # B, T, H, W
# per case: hand-over taken in the reduced classes, the two token grids, keys of the sub-sampled attention per stage
CASE_FACTS = {(1, 4, 32, 64): (True, ((32, 16), (16, 8)), (8, 8)), (2, 3, 40, 72): (False, ((30, 18), (15, 9)), (6, 6)),
              (1, 2, 56, 112): (True, ((28, 28), (14, 14)), (9, 9)), (2, 4, 24, 40): (True, ((24, 10), (12, 5)), (3, 3))}
CLASSES = ("fp32", "f16x3", "f16x2", "f16")
REDUCED = ("f16x2", "f16")
UNITS = ("embed0", "block0.0", "peg0", "block0.1", "embed1", "block1.0", "peg1", "block1.1")
ATTENTION_UNITS = ("block0.0", "block0.1", "block1.0", "block1.1")
WRONG = ("a", "b", "c", "d")
PARAM_SEED = 91
MARGIN = {"fp32": (3.0, 3.0), "f16x3": (3.0, 3.0), "f16x2": (2.0, 4.0), "f16": (2.0, 4.0)}     # (rms, max) times the yardstick
# (unit, class) -> (rms, max): raised margins.
# embed1 in fp32: the exact-fp32 GEMM sums the 2 x 2 conv's K = 512 products of an output in ONE fp32 chain (32x32x2 MFMA steps on one
# accumulator), the CPU's float32 GEMM in interleaved partial sums, and the unit is a bare conv + LayerNorm: no residual dilutes it.
# A CPU model of that single chain (tests/test_twins_cases_cpu.py::test_single_chain_model_of_embed1) sits at 2.4 e32 rms and
# 2.8 - 3.7 e32 max by itself; the margin 3 for "another order" goes on top of that: 3 x 2.4 and 3 x 3.7.
UNIT_MARGIN = {("embed1", "fp32"): (7.2, 11.0)}
SEPARATION = 0.1                                              # fp32 / f16x3 deviations are at most this times e_cls of F16X2


def case_id(c):
    return "x".join(str(v) for v in c)


def handover(c):
    """encoders.py: the reduced classes hand fp16 k-octet planes between kernels only when this holds."""
    return (c[1] * c[2] * c[3]) % 256 == 0


def params():
    return syn.make_twins_params(PARAM_SEED)


def images(c):
    """Normalised frames [B, T, 3, H, W] in (-1, 1), fp32."""
    return torch.tanh(syn.randn(PARAM_SEED + 1, "twins_stages." + case_id(c), (c[0], c[1], 3, c[2], c[3])))


def previous(unit):
    """The tap a unit reads (None: the images)."""
    i = UNITS.index(unit)
    return UNITS[i - 1] if i else None


def _parse(unit):
    if unit.startswith("embed"):
        return "embed", int(unit[5]), None
    if unit.startswith("peg"):
        return "peg", int(unit[3]), None
    return "block", int(unit[5]), int(unit[7])


def _tokens(planes):
    B, E, gh, gw = planes.shape
    return planes.reshape(B, E, gh * gw).permute(0, 2, 1), (gh, gw)


def _planes(tok, size):
    return tok.permute(0, 2, 1).reshape(tok.shape[0], tok.shape[2], *size).contiguous()


def _frames(planes, T):
    """Token planes [B, E, T*h, w] -> the reference's 'b t c h w'."""
    B, E, gh, gw = planes.shape
    return planes.reshape(B, E, T, gh // T, gw).permute(0, 2, 1, 3, 4)


def output_view(last_tap, T):
    """The documented output [B, T, 256, H/8, W/8] of the last tap."""
    return _frames(last_tap, T).contiguous()


# ---- wrong variants ----------------------------------------------------------------------------------------------------------------
def _lga_without_pad_keys(x, size, p, prefix, heads, ws=two.WINDOW):
    """two.locally_grouped_attn with the pad tokens masked out of every softmax (variant a)."""
    B, N, C = x.shape
    H, W = size
    hd = C // heads
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    g = F.pad(x.reshape(B, H, W, C), (0, 0, 0, pad_r, 0, pad_b))
    Hp, Wp = H + pad_b, W + pad_r
    nh, nw = Hp // ws, Wp // ws
    real = torch.zeros(Hp, Wp, dtype=torch.bool)
    real[:H, :W] = True
    real = real.reshape(nh, ws, nw, ws).permute(0, 2, 1, 3).reshape(nh * nw, ws * ws)
    win = g.reshape(B, nh, ws, nw, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, nh * nw, ws * ws, C)
    qkv = two._linear(win, p, prefix + ".qkv").reshape(B, nh * nw, ws * ws, 3, heads, hd).permute(3, 0, 1, 4, 2, 5)
    logits = (qkv[0] * hd ** -0.5) @ qkv[1].transpose(-2, -1)
    logits = logits.masked_fill(~real[None, :, None, None, :], float("-inf"))
    o = torch.softmax(logits, dim=-1) @ qkv[2]
    o = o.permute(0, 1, 3, 2, 4).reshape(B, nh, nw, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    return two._linear(o[:, :H, :W, :].reshape(B, N, C), p, prefix + ".proj")


def _gsa_zero_padded(x, size, p, prefix, heads, sr):
    """two.global_subsample_attn with the grid zero-padded to a multiple of sr before the sr convolution (variant c)."""
    B, N, C = x.shape
    H, W = size
    hd = C // heads
    q = two._linear(x, p, prefix + ".q").reshape(B, N, heads, hd).permute(0, 2, 1, 3)
    g = F.pad(x.permute(0, 2, 1).reshape(B, C, H, W), (0, (sr - W % sr) % sr, 0, (sr - H % sr) % sr))
    s = F.conv2d(g, p[prefix + ".sr.weight"], p[prefix + ".sr.bias"], stride=sr).reshape(B, C, -1).permute(0, 2, 1)
    s = two._ln(s, p[prefix + ".norm.weight"], p[prefix + ".norm.bias"], two.LN_EPS)
    kv = two._linear(s, p, prefix + ".kv").reshape(B, -1, 2, heads, hd).permute(2, 0, 3, 1, 4)
    o = two._attend(q, kv[0], kv[1], hd ** -0.5).permute(0, 2, 1, 3).reshape(B, N, C)
    return two._linear(o, p, prefix + ".proj")


@contextlib.contextmanager
def _oracle_with(wrong):
    """The oracle module with one of its parts replaced (a, c, d); restored on exit."""
    swap = {"a": ("locally_grouped_attn", _lga_without_pad_keys), "c": ("global_subsample_attn", _gsa_zero_padded),
            "d": ("BLOCK_LN_EPS", 1e-5)}.get(wrong)
    if swap is None:
        yield
        return
    keep = getattr(two, swap[0])
    setattr(two, swap[0], swap[1])
    try:
        yield
    finally:
        setattr(two, swap[0], keep)


# ---- the units, from the oracle's own functions --------------------------------------------------------------------------------------
def run_unit(unit, inp, p, T, wrong=None):
    """One unit in the dtype of `inp` and `p`.  inp: the images [B, T, 3, H, W] for embed0, else the previous tap [B, E, gh, gw].
    Returns the unit's tap [B, E, gh, gw]."""
    assert wrong is None or wrong in WRONG
    kind, i, j = _parse(unit)
    if kind == "embed":
        tok, size = two.patch_embed(inp if i == 0 else _frames(inp, T), p, f"svt.patch_embeds.{i}", two.PATCH[i])
        return _planes(tok, size)
    tok, size = _tokens(inp)
    if kind == "peg":
        return _planes(two.pos_conv(tok, size, p, f"svt.pos_block.{i}"), size)
    B, N, E = tok.shape
    if wrong == "b":                                          # every frame a grid of its own
        tok, sz = tok.reshape(B * T, N // T, E), (size[0] // T, size[1])
    else:
        sz = size
    with _oracle_with(wrong):
        tok = two.block(tok, sz, p, f"svt.blocks.{i}.{j}", two.NUM_HEADS[i], two.SR_RATIOS[i], local=(j == 0))
    return _planes(tok.reshape(B, N, E), size)


def chain(x, p, T):
    """Every unit on the previous unit's result (no GPU): {unit: tap} in the dtype of x and p."""
    taps, cur = {}, x
    for u in UNITS:
        cur = taps[u] = run_unit(u, cur, p, T)
    return taps


# ---- the weights as packed -------------------------------------------------------------------------------------------------------------
def is_gemm_weight(key, t):
    return key.endswith(".weight") and t.dim() >= 2 and "pos_block" not in key


def split_weight(w):
    """ops.PackedLinear restated: (hi, lo, scale) with scale * w = hi + lo + residue, hi and lo fp16 (returned as float64)."""
    w2 = w.detach().float().reshape(w.shape[0], -1)
    wmax = float(w2.abs().max())
    s = 2.0 ** min(14, max(-14, -math.floor(math.log2(wmax)))) if wmax > 0 else 1.0
    wm = w2 * s
    hi = wm.to(torch.float16)
    lo = (wm - hi.float()).to(torch.float16)
    return hi.double().reshape(w.shape), lo.double().reshape(w.shape), s


@functools.lru_cache(maxsize=None)
def _effective(cls):
    out = {}
    for k, t in params().items():
        if cls != "fp32" and is_gemm_weight(k, t):
            hi, lo, s = split_weight(t)
            out[k] = (hi if cls == "f16" else hi + lo) / s
        else:
            out[k] = t.double()
    return out


def effective_params(cls):
    """float64 parameters as class `cls` multiplies them: fp32 as drawn; (hi + lo) / scale in f16x3 and f16x2; hi / scale in f16."""
    return _effective(cls)


# ---- class emulation -----------------------------------------------------------------------------------------------------------------
def r16(x):
    """fp32 -> fp16 -> float64, as a kernel rounds a value it holds in fp32."""
    return x.float().to(torch.float16).double()


def _chan(tok):
    """[B, N, C] tokens -> the kernels' channel-major planes [B][C][N], numpy."""
    return tok.permute(0, 2, 1).contiguous().numpy()


def emulate_unit(unit, inp, pe, T, hand, exact_attention=False, rounding=True):
    """The unit in float64 with the reduced classes' roundings (module docstring).  pe: effective_params of the class; hand: the
    hand-over is taken; rounding=False: no rounding anywhere and the exact attention -- must then be the oracle's unit."""
    rnd = r16 if rounding else (lambda t: t)
    inp = inp.double()
    kind, i, j = _parse(unit)
    if kind == "embed":
        return run_unit(unit, rnd(inp), pe, T)                # the im2col columns are the GEMM's activation operand
    if kind == "peg":
        return run_unit(unit, inp, pe, T)
    pre, heads = f"svt.blocks.{i}.{j}", two.NUM_HEADS[i]
    x, (H, W) = _tokens(inp)
    B, N, C = x.shape
    y = two._ln(x, pe[pre + ".norm1.weight"], pe[pre + ".norm1.bias"], two.BLOCK_LN_EPS)
    core = "fp32" if exact_attention else None
    if j == 0:
        qkv = two._linear(rnd(y), pe, pre + ".attn.qkv")
        if core is None:
            core = "koct" if hand else "x1"
            if hand:
                qkv = rnd(qkv)                                # the qkv GEMM stores fp16 k-octets
        exact, _, model = ac.window_reference(_chan(qkv), pe[pre + ".attn.qkv.bias"].numpy(), heads, H, W, two.WINDOW, (core,))
    else:
        core = core or "x1"
        q = two._linear(rnd(y), pe, pre + ".attn.q")
        g = rnd(y).permute(0, 2, 1).reshape(B, C, H, W)
        sr = two.SR_RATIOS[i]
        s = F.conv2d(g, pe[pre + ".attn.sr.weight"], pe[pre + ".attn.sr.bias"], stride=sr).reshape(B, C, -1).permute(0, 2, 1)
        s = two._ln(s, pe[pre + ".attn.norm.weight"], pe[pre + ".attn.norm.bias"], two.LN_EPS)
        kv = two._linear(rnd(s), pe, pre + ".attn.kv")
        exact, _, model = ac.subsample_reference(_chan(q), _chan(kv), heads, (core,))
    o = torch.from_numpy(np.ascontiguousarray(model[core] if rounding else exact)).permute(0, 2, 1)
    x = x + two._linear(rnd(o), pe, pre + ".attn.proj")
    y = two._ln(x, pe[pre + ".norm2.weight"], pe[pre + ".norm2.bias"], two.BLOCK_LN_EPS)
    x = x + two._linear(rnd(F.gelu(two._linear(rnd(y), pe, pre + ".mlp.fc1"))), pe, pre + ".mlp.fc2")
    return _planes(x, (H, W))


# ---- yardsticks and bounds -------------------------------------------------------------------------------------------------------------
def dev(a, b):
    """(rms, max) of a - b, float64."""
    d = (a.double() - b.double()).reshape(-1)
    return float(d.pow(2).mean().sqrt()), float(d.abs().max())


def bound(unit, cls, e32, e_cls):
    """(rms, max) bound of class `cls` from the yardsticks; e_cls: that of `cls` itself (ignored in the fp32 classes)."""
    m = UNIT_MARGIN.get((unit, cls), MARGIN[cls])
    y = e_cls if cls in REDUCED else e32
    return m[0] * y[0], m[1] * y[1]


def yardsticks(unit, inp, T, hand, classes=REDUCED, exact_attention=False):
    """For one unit on the fp32 input `inp`: dict(ref={class: float64 reference with that class's weights}, e32=(rms, max),
    e_cls={class: (rms, max)}) -- ref for every class, e_cls for `classes` (of REDUCED)."""
    d = inp.double()
    ref = {"fp32": run_unit(unit, d, effective_params("fp32"), T), "f16x3": run_unit(unit, d, effective_params("f16x3"), T)}
    ref["f16x2"] = ref["f16x3"]                               # the same hi + lo weights
    e32 = dev(run_unit(unit, inp.float(), params(), T), ref["fp32"])
    e_cls = {}
    for c in classes:
        if c == "f16":
            ref["f16"] = run_unit(unit, d, effective_params("f16"), T)
        e_cls[c] = e32 if unit.startswith("peg") else dev(emulate_unit(unit, d, effective_params(c), T, hand, exact_attention), ref[c])
    return dict(ref=ref, e32=e32, e_cls=e_cls)
