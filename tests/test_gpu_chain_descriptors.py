"""The four fused chain kernels -- sf_ffn_pair, sf_sk_tail, sf_temporal_block, sf_mask_upsample -- through RAW descriptors (-m gpu):
the _lib.Sf* structs filled here, not by the ops wrappers (which only ever set ld = P, tight strides and offset 0).

A. Placement.  Every shape x product combination at one ragged size, twice on the same data: contiguous, then pitched (every ld
   beyond the extent), gapped (every image and group stride beyond its span) and off the allocation's start, in two classes
   (tests/chain_cases.py::place).  Operands sit in NaN (columns [N, ld), gaps, the bytes before the base; rows at or past K of a
   partial last k-octet hold 1000.0: the format wants them finite, not zero), outputs in a finite sentinel.  The placed result
   is BITWISE the contiguous one (the kernels dispatch on shape and product count alone, pixels are independent columns), nothing
   outside any view changes, and the contiguous result meets the float64 bound of the kernel's own test file.
   Rows at or past M2 of a k-octet output's last octet: with c16_partial / y16_partial = 1 they keep the sentinel; with 0 they are
   written and hold 0.0 (the accumulators of zero weight rows start at a zero bias; gelu(0) = 0): asserted finite, and zero.
B. Tile edges, contiguous: sizes around each kernel's wave and workgroup widths, most of them no multiple of 4 (the C ABI takes any
   N > 0 and computes them correctly, so ops.ffn_pair_ok / sk_tail_ok no longer refuse P % 4 != 0: the wrapper test below, and the
   sentence in include/streamflow_hip.h), batches 1 and 3: the float64 bound, every
   cell of a NaN-filled output written, the first N' pixels of a run at N bitwise the run at N', image z of a batch bitwise
   the run on image z alone.
C. Product class.  With weights whose `lo` halves are as large as fp16 allows (test_chain_cases_cpu.py::lo_heavy) a result must be
   nearer (rms) to the float64 reference of ITS product counts than to the one with any single layer's class flipped: a launch
   that lost its `lo` fragments, or multiplied them where it should not, is the other class.  No tolerance.  The ratios
   rms(got - right) / rms(got - wrong) are printed; worst per kernel on an MI355X:
       sf_ffn_pair 0.107 (128 -> 192 -> 128, mode 1, (2, 2), first layer), sf_sk_tail 0.103 (384 -> 576 -> 6, pm 2, pw),
       sf_temporal_block 0.282 (TT = 3, pm 2, fc2; its five internal fp16 hand-overs are not modelled: rms 1.3e-3 to the right
       reference), sf_mask_upsample 0.0001 (1.8e-6 against 1.6e-2).
D. Five launches of sf_mask_upsample at the KITTI grid (47 x 156: a 36-pixel last tile) beside a busy stream: bit-identical, guard
   band intact (csrc/mask_upsample.hip records a store hazard in the last workgroups).
The float64 references, parameter draws and their CPU cross-check against the oracle: tests/test_chain_cases_cpu.py."""
import ctypes as Ct
import functools

import pytest
import torch

from tests import chain_cases as cc
from tests import test_chain_cases_cpu as ref
from tests.guarded import SENTINEL, Guarded

pytestmark = pytest.mark.gpu
NAN = float("nan")
DEVICE = "cuda:0"
TAIL = 64                                                     # guard elements behind the last image of every buffer


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _packed(kernel, shape, pm, heavy=False):
    """(weights, PackedLinear layers, weight stream, the other parameters on the device) -- packed once per module."""
    dv = torch.device(DEVICE)
    w = ref.draw_weights(kernel, shape, heavy)
    L, pk = ref.pack(kernel, w, pm, dv)
    st = pk.stream(*pm) if kernel == "ffn_pair" else pk.stream(pm)
    extra = {k: v.to(dv).contiguous() for k, v in w.items() if k in ("dw_w", "dw_b", "ln1_w", "ln1_b", "ln2_w", "ln2_b")}
    return w, L, st, extra


def _built(c):
    if c["kernel"] == "sk_tail":
        from streamflow_amd import _lib
        if int(_lib.load().sf_sk_tail_frags(*c["shape"], c["pm"])) == 0:
            assert (c["shape"], c["pm"]) == cc.TAIL_UNBUILT        # the one combination that is not built (tests/test_gpu_sk_tail.py)
            pytest.skip("256 -> H -> 192 with single-product weights is not built")


def _guard(dev, c, field, placement, batch, fill, rows=None):
    table = {f: (i, lay, r, g, t) for i, (f, lay, r, g, t) in enumerate(cc.operands(c))}
    i, layout, r0, group, tight = table[field]
    rows = rows or r0
    cols = cc.cols_of(c, field)
    off, ld, stride, gs = cc.place(layout, placement, rows, cols, c["seed"] + i, group, tight)
    dtype = torch.float32 if layout.startswith("f32") else torch.float16
    return Guarded(dev, batch, rows, cols, off, ld, stride, fill, dtype, group=group, group_stride=gs, koct=layout == "koct", tail=TAIL)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _call(fn, g, what):
    from streamflow_amd import _lib
    status = fn(Ct.byref(g), _lib.stream())
    torch.cuda.synchronize()
    assert status == 0, f"{what}: refused ({status}): {_lib.load().sf_last_error().decode(errors='replace')}"


def variants(c):
    """Output requests of a case: where the struct offers fp32 planes and a k-octet copy, both together and each alone."""
    k = c["kernel"]
    if k == "ffn_pair":
        return ["C+C16", "C", "C16"] if c["mode"] == 0 else ["C16"]
    return ["out"] if k == "mask_upsample" else ["Y+Y16", "Y", "Y16"]


def run(dev, c, inp, placement, variant, fill=SENTINEL, heavy=False):
    """One launch of case c on inp (test_chain_cases_cpu.draw_input: x [images, K, P] fp32, rounded to fp16 here where the operand
    is fp16) at a placement.  Returns (operands, outputs): {field: Guarded}; an output's view is its first M2 rows, or all rows of
    its octets when the launch writes them (`partial` = 0 with M2 % 8)."""
    from streamflow_amd import _lib, ops
    lib = _lib.load()
    k, pm = c["kernel"], c["pm"]
    w, L, st, extra = _packed(k, c["shape"], pm, heavy)
    x = inp["x"]
    n = x.shape[0]
    ins, outs = {}, {}
    if k == "ffn_pair":
        K1, H, M2 = c["shape"]
        Ka = (K1 + 7) // 8 * 8
        xp = torch.cat([x, torch.full((n, Ka - K1, x.shape[2]), 1000.0)], dim=1) if Ka > K1 else x
        X = ins["X"] = _guard(dev, c, "X", placement, n, NAN, rows=Ka).put(xp)
        g = _lib.SfFfnPair()
        g.X, g.strideX, g.ldx = X.ptr, X.stride, X.ld
        g.x_group, g.x_group_stride = c.get("x_group", 0), X.group_stride
        g.wstream, g.wstream_bytes = st.data_ptr(), st.numel() * 2
        g.bias1, g.bias2 = ops._bias_ptr(L[0]), ops._bias_ptr(L[1])
        g.alpha1, g.alpha2 = 1.0 / L[0].split_scale, 1.0 / L[1].split_scale
        g.N, g.batch, g.K1, g.H, g.M2 = c["N"], n, K1, H, M2
        g.pm1, g.pm2, g.mode, g.gelu_out = pm[0], pm[1], c["mode"], int(ref.gelu_out_of(c))
        if c["mode"] == 1:
            g.dw_w, g.dw_b = extra["dw_w"].data_ptr(), extra["dw_b"].data_ptr()
            Y = outs["C16"] = _guard(dev, c, "C16", placement, n, fill)
            g.C16, g.strideC16, g.ldc16 = Y.ptr, Y.stride, Y.ld
            if c.get("r32"):
                R = ins["R32"] = _guard(dev, c, "R32", placement, n, NAN).put(x)
                g.R32, g.strideR32, g.ldr32, g.r32_group_stride = R.ptr, R.stride, R.ld, R.group_stride
        else:
            if "C16" in variant:
                g.c16_partial = 1 if (variant == "C+C16" and M2 % 8) else 0
                Y = outs["C16"] = _guard(dev, c, "C16", placement, n, fill, rows=M2 if g.c16_partial else (M2 + 7) // 8 * 8)
                g.C16, g.strideC16, g.ldc16 = Y.ptr, Y.stride, Y.ld
            if variant != "C16":
                Y = outs["C"] = _guard(dev, c, "C", placement, n, fill)
                g.C, g.strideC, g.ldc = Y.ptr, Y.stride, Y.ld
        _call(lib.sf_ffn_pair, g, c["id"])
    elif k == "sk_tail":
        C, H, M2 = c["shape"]
        X = ins["X"] = _guard(dev, c, "X", placement, n, NAN).put(x)
        g = _lib.SfSkTail()
        g.X, g.strideX, g.ldx = X.ptr, X.stride, X.ld
        g.wstream, g.wstream_bytes = st.data_ptr(), st.numel() * 2
        g.bias1, g.bias2, g.bias3 = (ops._bias_ptr(A) for A in L)
        g.alpha1, g.alpha2, g.alpha3 = (1.0 / A.split_scale for A in L)
        g.N, g.batch, g.C, g.H, g.M2, g.pm, g.gelu_out = c["N"], n, C, H, M2, pm, int(ref.gelu_out_of(c))
        if "Y16" in variant:
            g.y16_partial = 1 if (variant == "Y+Y16" and M2 % 8) else 0
            Y = outs["Y16"] = _guard(dev, c, "Y16", placement, n, fill, rows=M2 if g.y16_partial else (M2 + 7) // 8 * 8)
            g.Y16, g.strideY16, g.ldy16 = Y.ptr, Y.stride, Y.ld
        if variant != "Y16":
            Y = outs["Y"] = _guard(dev, c, "Y", placement, n, fill)
            g.Y, g.strideY, g.ldy = Y.ptr, Y.stride, Y.ld
        _call(lib.sf_sk_tail, g, c["id"])
    elif k == "temporal_block":
        X = ins["X16"] = _guard(dev, c, "X16", placement, n, NAN).put(x)
        g = _lib.SfTemporalBlock()
        g.X16, g.strideX, g.ldx = X.ptr, X.stride, X.ld
        g.wstream, g.wstream_bytes = st.data_ptr(), st.numel() * 2
        g.ln1_w, g.ln1_b, g.ln2_w, g.ln2_b = (extra[q].data_ptr() for q in ("ln1_w", "ln1_b", "ln2_w", "ln2_b"))
        g.bias_proj, g.bias_fc1, g.bias_fc2 = ops._bias_ptr(L[1]), ops._bias_ptr(L[2]), ops._bias_ptr(L[3])
        g.alpha_qkv, g.alpha_proj, g.alpha_fc1, g.alpha_fc2 = (1.0 / A.split_scale for A in L)
        g.ss_proj, g.ss_fc2, g.eps, g.scale = L[1].split_scale, L[3].split_scale, 1e-5, 128 ** -0.5
        g.N, g.B, g.TT, g.C, g.H, g.pm = c["N"], n // c["TT"], c["TT"], 128, 256, pm
        if "Y16" in variant:
            Y = outs["Y16"] = _guard(dev, c, "Y16", placement, n, fill)
            g.Y16, g.strideY16, g.ldy16 = Y.ptr, Y.stride, Y.ld
        if variant != "Y16":
            Y = outs["Y"] = _guard(dev, c, "Y", placement, n, fill)
            g.Y, g.strideY, g.ldy = Y.ptr, Y.stride, Y.ld
        _call(lib.sf_temporal_block, g, c["id"])
    else:
        h, wd = c["hw"]
        X = ins["X16"] = _guard(dev, c, "X16", placement, n, NAN).put(x)
        Fl = ins["flow"] = _guard(dev, c, "flow", placement, n, NAN).put(inp["flow"].reshape(n, 2 * h, wd))
        O = outs["out"] = _guard(dev, c, "out", placement, n, fill)
        g = _lib.SfMaskUpsample()
        g.X16, g.strideX, g.ldx = X.ptr, X.stride, X.ld
        g.wstream, g.wstream_bytes = st.data_ptr(), st.numel() * 2
        g.bias, g.flow, g.out = ops._bias_ptr(L[0]), Fl.ptr, O.ptr
        g.n_img, g.h, g.w, g.K, g.M, g.pm, g.alpha = n, h, wd, 256, 576, pm, 0.25 / L[0].split_scale
        _call(lib.sf_mask_upsample, g, c["id"])
    return ins, outs


def logical(c, outs):
    """{field: the [images][M2][N] part of an output} (an output's view may include the pad rows of its last octet)."""
    M2 = {"ffn_pair": c["shape"][-1], "sk_tail": c["shape"][-1], "temporal_block": 128}.get(c["kernel"])
    return {f: (G.region()[:, :M2] if M2 else G.region()) for f, G in outs.items()}


def reference64(c, inp, heavy=False, flip=None):
    """float64 over the values the launch multiplies: fp16-rounded activations (the fp32 residual of the R32 form as it is), the
    layers' effective weights for the case's product counts (layer `flip` in the other class)."""
    w, L, _, _ = _packed(c["kernel"], c["shape"], c["pm"], heavy)
    names = cc.layers_of(c["kernel"])
    pms = c["pm"] if isinstance(c["pm"], tuple) else (c["pm"],) * len(L)
    resid = inp["x"].double() if c.get("r32") else None
    return ref.reference(c, w, ref.class_weights(L, names, pms, flip), dict(inp, x=inp["x"].half().float()), resid)


def check_bound(c, variant, res, r64):
    """The float64 bound of the kernel's own test file (tests/test_gpu_ffn_pair.py, test_gpu_sk_tail.py, test_gpu_temporal_block.py,
    test_gpu_mask_upsample.py), expression by expression; res = logical(outs)."""
    k = c["kernel"]
    got = {f: t.double().cpu() for f, t in res.items()}
    for f, t in got.items():
        assert bool(torch.isfinite(t).all()), (c["id"], variant, f, "a cell was not written, or a NaN of the padding was read")
    scale = max(1.0, r64.abs().max().item())
    if k == "ffn_pair" and c["mode"] == 1:
        err = (got["C16"] - r64).abs()
        assert bool((err <= 2.0 ** -10 * r64.abs() + 3e-3).all()), (c["id"], err.max().item())
        return
    if k == "mask_upsample":
        err = (got["out"].view_as(r64) - r64).abs().max().item()
        assert err <= 2e-4 * scale, (c["id"], err)
        return
    f32, f16 = ("C", "C16") if k == "ffn_pair" else ("Y", "Y16")
    tol = {"ffn_pair": 2e-3, "sk_tail": 3e-3, "temporal_block": 4e-3}[k]
    if f32 in got:
        err = (got[f32] - r64).abs().max().item()
        print(f"{c['id']} {variant}: max abs err vs float64 = {err:.2e} (scale {scale:.1f})")
        assert (err < tol * scale) if k != "temporal_block" else (err <= tol * scale), (c["id"], variant, err, scale)
        if k == "temporal_block":
            assert ref.rms(got[f32] - r64) <= 6e-4 * scale, (c["id"], variant, ref.rms(got[f32] - r64))
        if f16 in got:                                         # the k-octet copy is the fp16 rounding of the fp32 result
            assert torch.equal(res[f16].float(), res[f32].half().float()), (c["id"], variant)
    elif k != "temporal_block":                                # k-octet planes alone
        err = (got[f16] - r64).abs()
        assert bool((err <= 2.0 ** -10 * r64.abs() + tol * scale).all()), (c["id"], variant, err.max().item())


def pad_rows_finite(c, outs):
    for f, G in outs.items():
        M2 = c["shape"][2] if c["kernel"] in ("ffn_pair", "sk_tail") else None
        if M2 and G.shape[1] > M2:
            pad = G.region()[:, M2:].float()
            assert bool(torch.isfinite(pad).all()) and bool((pad == 0).all()), (c["id"], f, "pad rows of the last octet")


# ---- A ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.part_a(), ids=[c["id"] for c in cc.part_a()])
def test_placement_is_invisible(dev, case):
    c = case
    _built(c)
    inp = ref.draw_input(c)
    r64 = reference64(c, inp)
    y16_alone = None
    for variant in variants(c):
        ins1, outs1 = run(dev, c, inp, "contiguous", variant)
        ins2, outs2 = run(dev, c, inp, c["placement"], variant)
        for which, (ins, outs) in (("contiguous", (ins1, outs1)), (c["placement"], (ins2, outs2))):
            for f, G in list(ins.items()) + list(outs.items()):
                assert G.outside_unchanged(), (c["id"], variant, which, f, "an element outside the view changed")
            pad_rows_finite(c, outs)
        for f in outs1:
            assert _same(outs1[f].region(), outs2[f].region()), (c["id"], variant, f, "the placed result is not bitwise the contiguous one")
        res = logical(c, outs1)
        check_bound(c, variant, res, r64)
        if c["kernel"] == "temporal_block":                    # (its k-octet copy has no bound of its own: alone == beside the planes)
            if variant == "Y+Y16":
                y16_alone = res["Y16"].clone()
            elif variant == "Y16":
                assert _same(res["Y16"], y16_alone), (c["id"], "Y16 alone differs from Y16 beside Y")


# ---- B ---------------------------------------------------------------------------------------------------------------------------
def _slice(c, inp, N=None, clip=None):
    """The first N pixels and / or clip `clip` (its TT images) of a draw."""
    x = inp["x"]
    tt = c.get("TT", 1)
    if clip is not None:
        x = x[clip * tt:(clip + 1) * tt]
    out = {"x": (x[:, :, :N] if N is not None else x).contiguous()}
    if "flow" in inp:
        out["flow"] = inp["flow"][clip:clip + 1] if clip is not None else inp["flow"]
    return out


@pytest.mark.parametrize("group", [g for _, g in cc.part_b()], ids=[i for i, _ in cc.part_b()])
def test_tile_edges(dev, group):
    c0 = group[0]
    k = c0["kernel"]
    variant = variants(c0)[0]
    sizes = sorted({c["N"] for c in group}) if "N" in c0 else [None]
    assert {c["batch"] for c in group} == {1, 3}
    full = ref.draw_input(dict(c0, batch=3, **({"N": sizes[-1]} if sizes[0] else {})))
    kept = {}
    for N in sizes:
        c3 = next(c for c in group if c.get("N") == N and c["batch"] == 3)
        c1 = next(c for c in group if c.get("N") == N and c["batch"] == 1)
        inp = _slice(c3, full, N)
        ins, outs = run(dev, c3, inp, "contiguous", variant, fill=NAN)
        res = logical(c3, outs)
        check_bound(c3, variant, res, reference64(c3, inp))                    # (finite everywhere: every cell written)
        for f, G in list(ins.items()) + list(outs.items()):
            assert G.outside_unchanged(), (c3["id"], f)
        for z in range(3):                                                     # image (clip) z alone
            _, o1 = run(dev, c1, _slice(c1, inp, None, z), "contiguous", variant, fill=NAN)
            tt = c1.get("TT", 1)
            for f, t in logical(c1, o1).items():
                assert _same(t, res[f][z * tt:(z + 1) * tt]), (c1["id"], f, z, "an image of a batch differs from the same image alone")
        kept[N] = {f: t.clone() for f, t in res.items()}
    for big, small in cc.B_PREFIX.get(k, []):
        for f in kept[big]:
            assert _same(kept[big][f][:, :, :small], kept[small][f]), (c0["id"], f, big, small, "a prefix of the pixels depends on N")


def test_ops_wrappers_admit_pixel_counts_that_are_no_multiple_of_4(dev):
    """ops.ffn_pair_ok / sk_tail_ok used to refuse P % 4 != 0 although the entry points take any N: through the wrappers at P = 133."""
    from streamflow_amd import ops
    from streamflow_amd.ops import Planes
    cx = ops.Ctx(precision=ops.PRECISION_F16X2)
    P, n = 133, 2
    for mode, shape in ((0, (128, 192, 64)), (1, (128, 192, 128))):
        c = dict(kernel="ffn_pair", shape=shape, pm=(2, 2), batch=n, N=P, mode=mode, placement="contiguous", seed=5000 + mode, id=f"ops-pair-m{mode}")
        inp = ref.draw_input(c)
        _, L, _, extra = _packed("ffn_pair", shape, (2, 2))
        pair = ops.PackedPair(L[0], L[1])
        K1, _, M2 = shape
        X = Planes(torch.zeros(n * K1 * P // 2 + 8, device=dev), 0, K1 * P, n, K1, P, f16=True, koct=True)
        ops.pack_koct(Planes.of(inp["x"].to(dev).contiguous()), X)
        assert ops.ffn_pair_ok(pair, X, mode, cx)
        if mode == 0:
            y = torch.full((n, M2, P), NAN, device=dev)
            ops.ffn_pair(pair, X, Planes.of(y), 0, gelu_out=ref.gelu_out_of(c), cx=cx)
            res = {"C": y}
        else:
            Y = Planes(torch.full((n * M2 * P // 2 + 8,), NAN, device=dev), 0, M2 * P, n, M2, P, f16=True)
            ops.ffn_pair(pair, X, Y, 1, dw_w=extra["dw_w"], dw_b=extra["dw_b"], cx=cx)
            res = {"C16": Y.tensor()}
        torch.cuda.synchronize()
        check_bound(c, "C" if mode == 0 else "C16", res, reference64(c, inp))
    shape = (128, 192, 64)
    c = dict(kernel="sk_tail", shape=shape, pm=2, batch=n, N=P, placement="contiguous", seed=5002, id="ops-tail")
    inp = ref.draw_input(c)
    _, L, _, _ = _packed("sk_tail", shape, 2)
    tail = ops.PackedTail(*L)
    h16 = inp["x"].half().to(dev).contiguous()
    X = Planes(h16.view(-1).view(torch.float32), 0, shape[0] * P, n, shape[0], P, f16=True)
    y = torch.full((n, shape[2], P), NAN, device=dev)
    assert ops.sk_tail_ok(tail, X, Planes.of(y), cx)
    ops.sk_tail(tail, X, Planes.of(y), gelu_out=ref.gelu_out_of(c), cx=cx)
    torch.cuda.synchronize()
    check_bound(c, "Y", {"Y": y}, reference64(c, inp))


# ---- C ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.part_c(), ids=[c["id"] for c in cc.part_c()])
def test_result_belongs_to_its_product_class(dev, case):
    c = case
    _built(c)
    inp = ref.draw_input(c, heavy=True)
    variant = {"ffn_pair": "C" if c.get("mode") == 0 else "C16", "mask_upsample": "out"}.get(c["kernel"], "Y")
    _, outs = run(dev, c, inp, "contiguous", variant, fill=NAN, heavy=True)
    (f, got), = logical(c, outs).items()
    fp16_out = got.dtype == torch.float16
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all())
    model = (lambda t: t.half().double()) if fp16_out else (lambda t: t)       # (fp16 rows out: both references rounded like the result)
    right = ref.rms(got - model(reference64(c, inp, heavy=True)).view_as(got))
    for i, name in enumerate(cc.layers_of(c["kernel"])):
        wrong = ref.rms(got - model(reference64(c, inp, heavy=True, flip=i)).view_as(got))
        print(f"CLASS {c['kernel']} {c['id']} flip {name}: rms right {right:.3e} wrong {wrong:.3e} ratio {right / wrong:.3f}")
        assert right < wrong, (c["id"], name, right, wrong)


# ---- D ---------------------------------------------------------------------------------------------------------------------------
def test_mask_upsample_repeats_bit_identically_beside_a_busy_stream(dev):
    c = dict(kernel="mask_upsample", shape=cc.MASK_SHAPE, pm=2, batch=cc.D_BATCH, hw=cc.D_HW, placement="aligned", seed=4000, id="D")
    inp = ref.draw_input(c)
    side = torch.cuda.Stream(device=dev)
    junk = torch.empty(64 << 20, device=dev)
    first = None
    for rep in range(cc.D_REPEATS):
        with torch.cuda.stream(side):
            junk.normal_()
        ins, outs = run(dev, c, inp, "aligned", "out")
        O = outs["out"]
        assert O.outside_unchanged(), (rep, "guard band")
        assert all(G.outside_unchanged() for G in ins.values())
        cur = O.region().clone()
        assert bool(torch.isfinite(cur).all()), rep
        first = cur if first is None else first
        assert _same(cur, first), (rep, int((cur != first).sum()))
    torch.cuda.synchronize()
    check_bound(c, "out", {"out": first}, reference64(c, inp))
