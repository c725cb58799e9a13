"""The per-pixel kernels between the GEMMs and the fused chains -- sf_temporal_attn / sf_temporal_attn_f16in, sf_layernorm_cm,
sf_upsample_flow, sf_bilinear_sampler, sf_context_split, sf_flow_update, sf_pack_koct, sf_dwconv3x3_res -- through the C ABI
(-m gpu): raw pointers and strides handed to streamflow_amd._lib.load(), not the ops wrappers (which only ever pass tight strides
and offset 0), at the smallest shapes at which their index arithmetic can go wrong (tests/glue_cases.py).

Every operand and output sits in a guard-banded buffer (tests/guarded.py): operands in NaN, arithmetic outputs in NaN, copied /
rounded outputs in a finite sentinel.  Every case asserts: status 0; every element of every output view written; nothing outside
any view changed, inputs included; the run off the allocation's start, with image strides beyond the span where the entry point
takes strides (the base aligned where include/streamflow_hip.h demands it), BITWISE equal to the contiguous one; image z of a
batch bitwise the run on image z alone; and the numerical bound:

    tol = 4 * max|ref32 - ref64| + 4 * 2^-24 * max|ref64|

ref64 / ref32 = the kernel's restatement (tests/test_glue_cases_cpu.py) evaluated for that case in float64 / torch float32: two
fp32 summation orders have errors of the same size, not the same value, and the second term keeps the bound off zero where
float32 is exact.  Capped by the bound the suite already has for the entry point at the same input scale (test_glue_cases_cpu.CAP).
An fp16 k-octet copy is held to test_gpu_fuzz.py's rule against the fp32 output of the same call; the copy alone is bitwise the
copy beside the planes.  A rule of this file's own, for a call that asks for the copy alone (no fp32 output to compare with): one
fp16 rounding of a value within tol of ref64, |copy - ref64| <= 2^-11 * 1.01 * |ref64| + 1e-6 + tol (_koct_alone_bound).
Outputs that are no arithmetic (sf_flow_update, sf_pack_koct, the ReLU half of sf_context_split, the sampler's mask) are compared
exactly.  test_glue_cases_cpu.py shows that these bounds tell a wrong kernel from a right one.

err / tol is printed per case ("GLUE ..."); worst per kernel on an MI355X:
    sf_temporal_attn 0.798 (TT = 7, C = 36, P = 1, gain 4: 2.8e-6 against 3.5e-6), sf_temporal_attn_f16in 0.874 (TT = 3, C = 128,
    P = 1, gain 4: 1.75e-6 against 2.0e-6), sf_upsample_flow 0.373 (2 x 3 x 33, golden scales: 2.7e-5 against 7.3e-5),
    sf_bilinear_sampler 0.163 (3 x 5 x 6 x 7), sf_context_split 0.213 (tanh, hdim 128, P = 257), sf_dwconv3x3_res 0.180 (5 x 260,
    C = 3); sf_flow_update and sf_pack_koct are exact.
    sf_layernorm_cm 0.477 (the generic kernel, C = 324, P = 65, randn * 2 + 0.3: 3.2e-6 against 6.7e-6); its split kernels
    (C = 128 / 256) 0.466 (C = 256, P = 64, randn + 100: 8.3e-5 against 1.8e-4).  The generic kernel with a plain running sum
    for the mean had 2.135 (C = 96, P = 1, randn + 100: 1.16e-4 against 5.4e-5; C = 324, P = 1: 2.14e-4 against 1.06e-4); with
    the corrected two-pass mean it has 0.193 there (1.0e-5 against 5.3e-5)."""
import numpy as np
import pytest
import torch

from tests import glue_cases as gc
from tests import test_glue_cases_cpu as ref
from tests.guarded import SENTINEL, Guarded

pytestmark = pytest.mark.gpu
NAN = float("nan")
TAIL = 64                                                     # guard elements behind the last image of every buffer
SF_ERR_UNSUPPORTED = -2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _ids(cases):
    return [c["id"] for c in cases]


def _lib():
    from streamflow_amd import _lib as L
    return L


def _buf(dev, shape, layout, placed, fill, strided=True, k=0, data=None):
    """A guard-banded [batch][rows][cols] view (ld = cols) at the placement of glue_cases.place; data: put into it."""
    batch, rows, cols = shape
    off, stride = gc.place(layout, rows, cols, placed, strided, k)
    dtype = torch.float32 if layout.startswith("f32") else torch.float16
    G = Guarded(dev, batch, rows, cols, off, cols, stride, fill, dtype, koct=layout == "koct", tail=TAIL)
    assert (G.ptr % gc.BASE_ALIGN[layout]) == 0
    return G if data is None else G.put(data.reshape(shape))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b.to(a.device))))


def _go(fn, *args):
    status = fn(*args, _lib().stream())
    torch.cuda.synchronize()
    return status


def _ok(status, what):
    assert status == 0, f"{what}: refused ({status}): {_lib().load().sf_last_error().decode(errors='replace')}"


def _intact(what, *groups):
    for grp in groups:
        for f, G in grp.items():
            assert G.outside_unchanged(), (what, f, "an element outside the view changed")


def _untouched(G):
    """The whole buffer, view included, is bitwise what it was."""
    before = getattr(G, "snap", None)
    return _same(G.buf, before if before is not None else torch.full_like(G.buf, G.fill))


def _written(what, outs):
    for f, G in outs.items():
        assert bool(torch.isfinite(G.region().float()).all()), (what, f, "a cell was not written, or a NaN of the padding was read")


def _same_runs(what, a, b, why):
    assert a.keys() == b.keys()
    for f in a:
        assert _same(a[f].region(), b[f].region()), (what, f, why)


def _bound(kernel, what, got, r64, tol):
    err = float((got.double().cpu().reshape(r64.shape) - r64).abs().max())
    print(f"GLUE {kernel} {what}: err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert err <= tol, (kernel, what, err, tol)


def _koct_alone_bound(what, got16, r64, tol):
    """The k-octet copy with no fp32 output beside it: one fp16 rounding (test_gpu_fuzz.py's rule) of a value within tol of r64."""
    err = (got16.double().cpu().reshape(r64.shape) - r64).abs()
    assert bool((err <= 2.0 ** -11 * 1.01 * r64.abs() + 1e-6 + tol).all()), (what, float(err.max()))


def _opt(G):
    return (G.ptr, G.stride) if G is not None else (None, 0)


# ---- sf_temporal_attn, sf_temporal_attn_f16in --------------------------------------------------------------------------------------
def run_attn(dev, qkv, B, TT, C, entry, form, placed):
    """qkv [B TT][3C][P] (tight: the entry points take no strides).  Returns (status, ins, outs)."""
    lib = _lib().load()
    n, _, P = qkv.shape
    ins = {"qkv": _buf(dev, qkv.shape, "rows16" if entry == "f16in" else "f32", placed, NAN, strided=False, data=qkv)}
    outs = {}
    if form != "koct":
        outs["out"] = _buf(dev, (n, C, P), "f32", placed, NAN, strided=False)
    if form != "out":
        outs["koct"] = _buf(dev, (n, C, P), "koct", placed, NAN, strided=False)
    fn = lib.sf_temporal_attn_f16in if entry == "f16in" else lib.sf_temporal_attn
    st = _go(fn, ins["qkv"].ptr, _opt(outs.get("out"))[0], _opt(outs.get("koct"))[0], B, TT, C, P)
    return st, ins, outs


@pytest.mark.parametrize("case", gc.attn_cases(), ids=_ids(gc.attn_cases()))
def test_temporal_attn(dev, case):
    c = case
    B, TT, C, P = c["B"], c["TT"], c["C"], c["P"]
    forms = gc.attn_forms(C)
    for gain in gc.ATTN_GAINS:
        q32 = ref.draw_attn(c, gain)
        q16 = q32.half().float()                                              # the values the f16 entry point reads
        for entry in gc.ATTN_ENTRIES:
            q = q16 if entry == "f16in" else q32
            what = f"{c['id']} gain{gain} {entry}"
            r64 = ref.ref_attn(q.double(), B, TT, C)
            tol = ref.tol_of(ref.ref_attn(q, B, TT, C), r64, ref.CAP.get(("temporal_attn", gain)))
            kept = {}
            for form in forms:
                st1, ins1, outs1 = run_attn(dev, q, B, TT, C, entry, form, False)
                st2, ins2, outs2 = run_attn(dev, q, B, TT, C, entry, form, True)
                _ok(st1, what), _ok(st2, what)
                _written((what, form), outs1), _written((what, form), outs2)
                _intact((what, form), ins1, outs1, ins2, outs2)
                _same_runs((what, form), outs1, outs2, "the run off the allocation's start is not bitwise the contiguous one")
                res = kept[form] = {f: G.region().clone() for f, G in outs1.items()}
                if "out" in res:
                    _bound("sf_temporal_attn" + ("_f16in" if entry == "f16in" else ""), f"{what} {form}", res["out"], r64, tol)
                    if TT == 1 and entry == "f32":
                        assert _same(res["out"].cpu(), q[:, 2 * C:]), (what, "one token: the output is v")
                    if "koct" in res:
                        assert ref.koct_close(res["koct"], res["out"]), (what, form)
                        assert _same(res["koct"], kept["koct"]["koct"]), (what, "the k-octet copy alone differs from the copy beside out")
                else:
                    _koct_alone_bound((what, form), res["koct"], r64, tol)
            last = forms[-1]
            for z in range(B):                                                # clip z alone
                st, i1, o1 = run_attn(dev, q[z * TT:(z + 1) * TT], 1, TT, C, entry, last, False)
                _ok(st, what), _intact((what, z), i1, o1)
                for f, G in o1.items():
                    assert _same(G.region(), kept[last][f][z * TT:(z + 1) * TT]), (what, f, z, "a clip of a batch differs from the clip alone")
            if entry == "f16in":                                              # the fp32 entry point fed the same values
                st, _, of = run_attn(dev, q, B, TT, C, "f32", "out", False)
                _ok(st, what)
                d = float((of["out"].region() - kept["out"]["out"]).abs().max())
                assert d < 2e-6, (what, d)


def test_temporal_attn_refusals_write_nothing(dev):
    g = torch.Generator().manual_seed(9)
    C, P = gc.ATTN_KOCT_C_REFUSED, 65
    q = torch.randn(2 * 3, 3 * C, P, generator=g)
    for entry in gc.ATTN_ENTRIES:
        for form in ("koct", "both"):                                         # the k-octet copy needs C % 32 == 0
            st, ins, outs = run_attn(dev, q, 2, 3, C, entry, form, False)
            assert st != 0 and all(_untouched(G) for G in list(ins.values()) + list(outs.values())), (entry, form, st)
        TT = gc.ATTN_TT_REFUSED
        q8 = torch.randn(TT, 3 * 32, P, generator=g)
        for form in gc.attn_forms(32):
            st, ins, outs = run_attn(dev, q8, 1, TT, 32, entry, form, False)
            assert st == SF_ERR_UNSUPPORTED and all(_untouched(G) for G in list(ins.values()) + list(outs.values())), (entry, form, st)


# ---- sf_layernorm_cm -----------------------------------------------------------------------------------------------------------------
def run_ln(dev, x, gam, bet, eps, form, placed):
    lib = _lib().load()
    n, C, P = x.shape
    ins = {"x": _buf(dev, x.shape, "f32", placed, NAN, k=0, data=x), "gamma": _buf(dev, (1, 1, C), "f32", placed, NAN, strided=False, data=gam),
           "beta": _buf(dev, (1, 1, C), "f32", placed, NAN, strided=False, data=bet)}
    outs = {}
    if form != "koct":
        outs["y"] = _buf(dev, (n, C, P), "f32", placed, NAN, k=1)
    if form != "y":
        outs["koct"] = _buf(dev, (n, C, P), "koct", placed, NAN, k=2)
    st = _go(lib.sf_layernorm_cm, ins["x"].ptr, ins["x"].stride, ins["gamma"].ptr, ins["beta"].ptr, *_opt(outs.get("y")),
             *_opt(outs.get("koct")), n, C, P, eps)
    return st, ins, outs


@pytest.mark.parametrize("case", gc.ln_cases(), ids=_ids(gc.ln_cases()))
def test_layernorm_cm(dev, case):
    c = case
    n, C, P = c["n"], c["C"], c["P"]
    forms = gc.ln_forms(C)
    for cls in gc.LN_CLASSES:
        x, gam, bet = ref.draw_ln(c, cls)
        for eps in gc.LN_EPS:
            e32 = float(np.float32(eps))                                      # the float the entry point receives
            what = f"{c['id']} {cls} eps{eps:g}"
            r64 = ref.ref_layernorm(x.double(), gam.double(), bet.double(), e32)
            tol = ref.tol_of(ref.ref_layernorm(x, gam, bet, e32), r64, ref.CAP.get(("layernorm", cls)))
            kept = {}
            for form in forms:
                st1, ins1, outs1 = run_ln(dev, x, gam, bet, eps, form, False)
                st2, ins2, outs2 = run_ln(dev, x, gam, bet, eps, form, True)
                _ok(st1, what), _ok(st2, what)
                _written((what, form), outs1), _written((what, form), outs2)
                _intact((what, form), ins1, outs1, ins2, outs2)
                _same_runs((what, form), outs1, outs2, "the gapped / offset run is not bitwise the contiguous one")
                res = kept[form] = {f: G.region().clone() for f, G in outs1.items()}
                if "y" in res:
                    _bound("sf_layernorm_cm", f"{what} {form}", res["y"], r64, tol)
                    if cls == "constcol":                                     # variance 0: beta
                        col = res["y"][:, :, P // 2].double().cpu()
                        assert float((col - bet.double()[None]).abs().max()) <= tol, what
                    if "koct" in res:
                        assert ref.koct_close(res["koct"], res["y"]), (what, form)
                        assert _same(res["koct"], kept["koct"]["koct"]), (what, "the k-octet copy alone differs from the copy beside y")
                else:
                    _koct_alone_bound((what, form), res["koct"], r64, tol)
            last = forms[-1]
            for z in range(n):
                st, i1, o1 = run_ln(dev, x[z:z + 1], gam, bet, eps, last, False)
                _ok(st, what), _intact((what, z), i1, o1)
                for f, G in o1.items():
                    assert _same(G.region(), kept[last][f][z:z + 1]), (what, f, z, "an image of a batch differs from the image alone")


def test_layernorm_cm_refuses_a_koct_output_at_c96(dev):
    C = gc.LN_KOCT_C_REFUSED
    g = torch.Generator().manual_seed(10)
    x, gam, bet = torch.randn(2, C, 65, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)
    for form in ("koct", "both"):
        st, ins, outs = run_ln(dev, x, gam, bet, 1e-5, form, False)
        assert st != 0 and all(_untouched(G) for G in list(ins.values()) + list(outs.values())), (form, st)


# ---- sf_upsample_flow ----------------------------------------------------------------------------------------------------------------
def run_up(dev, flow, mask, placed):
    lib = _lib().load()
    n, _, h, w = flow.shape
    ins = {"flow": _buf(dev, (n, 2 * h, w), "f32", placed, NAN, strided=False, data=flow),
           "mask": _buf(dev, (n, 576 * h, w), "f32", placed, NAN, strided=False, data=mask)}
    outs = {"out": _buf(dev, (n, 16 * h, 8 * w), "f32", placed, NAN, strided=False)}
    st = _go(lib.sf_upsample_flow, ins["flow"].ptr, ins["mask"].ptr, outs["out"].ptr, n, h, w)
    return st, ins, outs


@pytest.mark.parametrize("case", gc.up_cases(), ids=_ids(gc.up_cases()))
def test_upsample_flow(dev, case):
    c = case
    n, h, w = c["nhw"]
    for cls in gc.UP_CLASSES:
        what = f"{c['id']} {cls}"
        flow, mask = ref.draw_up(c, cls)
        r64 = ref.ref_upsample(flow.double(), mask.double())
        tol = ref.tol_of(ref.ref_upsample(flow, mask), r64)
        st1, ins1, outs1 = run_up(dev, flow, mask, False)
        st2, ins2, outs2 = run_up(dev, flow, mask, True)
        _ok(st1, what), _ok(st2, what)
        _written(what, outs1), _written(what, outs2)
        _intact(what, ins1, outs1, ins2, outs2)
        _same_runs(what, outs1, outs2, "the run off the allocation's start is not bitwise the contiguous one")
        got = outs1["out"].region().clone()
        _bound("sf_upsample_flow", what, got, r64, tol)
        for z in range(n if n > 1 else 0):
            st, i1, o1 = run_up(dev, flow[z:z + 1], mask[z:z + 1], False)
            _ok(st, what), _intact((what, z), i1, o1)
            assert _same(o1["out"].region(), got[z:z + 1]), (what, z, "an image of a batch differs from the image alone")


# ---- sf_bilinear_sampler -------------------------------------------------------------------------------------------------------------
def run_bs(dev, img, crd, placed, want_mask=True):
    lib = _lib().load()
    M, C, Hi, Wi = img.shape
    _, Ho, Wo, _ = crd.shape
    ins = {"img": _buf(dev, (M, C * Hi, Wi), "f32", placed, NAN, strided=False, data=img),
           "coords": _buf(dev, (M, Ho, Wo * 2), "f32", placed, NAN, strided=False, data=crd)}
    outs = {"out": _buf(dev, (M, C * Ho, Wo), "f32", placed, NAN, strided=False)}
    if want_mask:
        outs["mask"] = _buf(dev, (M, Ho, Wo), "f32", placed, NAN, strided=False)
    st = _go(lib.sf_bilinear_sampler, ins["img"].ptr, ins["coords"].ptr, outs["out"].ptr, _opt(outs.get("mask"))[0], M, C, Hi, Wi, Ho, Wo)
    return st, ins, outs


@pytest.mark.parametrize("case", gc.bs_cases(), ids=_ids(gc.bs_cases()))
def test_bilinear_sampler(dev, case):
    c = case
    M, C, Hi, Wi = c["img"]
    Ho, Wo = gc.BS_POINTS
    what = c["id"]
    img, crd = ref.draw_bs(c)
    r64 = ref.ref_bilinear(img.double(), crd.double())
    tol = ref.tol_of(ref.ref_bilinear(img, crd), r64, ref.CAP[("bilinear", None)])
    st1, ins1, outs1 = run_bs(dev, img, crd, False)
    st2, ins2, outs2 = run_bs(dev, img, crd, True)
    st3, ins3, outs3 = run_bs(dev, img, crd, False, want_mask=False)
    _ok(st1, what), _ok(st2, what), _ok(st3, what)
    _written(what, outs1), _written(what, outs2), _written(what, outs3)
    _intact(what, ins1, outs1, ins2, outs2, ins3, outs3)
    _same_runs(what, outs1, outs2, "the run off the allocation's start is not bitwise the contiguous one")
    assert _same(outs3["out"].region(), outs1["out"].region()), (what, "out depends on whether the mask is asked for")
    got = outs1["out"].region().clone()
    _bound("sf_bilinear_sampler", what, got, r64, tol)
    zero = got.view(M, C, Ho * Wo)[:, :, gc.BS_ZERO]
    assert bool((zero == 0).all()), (what, "an out-of-range or non-finite coordinate does not sample zero")
    mask = outs1["mask"].region().clone()
    assert bool(((mask == 0) | (mask == 1)).all()), what
    if Hi > 1:      # (Hi = 1: the reference's rule divides by Hi - 1 = 0 -- its mask is then 0 at y = 0 (NaN) and unspecified in spirit: not asserted)
        assert _same(mask.cpu().view(M, Ho, Wo, 1), ref.ref_bilinear_mask(crd, Hi, Wi)), (what, "mask")
    for z in range(M if M > 1 else 0):
        st, i1, o1 = run_bs(dev, img[z:z + 1], crd[z:z + 1], False)
        _ok(st, what), _intact((what, z), i1, o1)
        assert _same(o1["out"].region(), got[z:z + 1]) and _same(o1["mask"].region(), mask[z:z + 1]), (what, z)


# ---- sf_context_split ----------------------------------------------------------------------------------------------------------------
def run_cs(dev, x, hdim, placed):
    lib = _lib().load()
    n, _, P = x.shape
    ins = {"cnets": _buf(dev, x.shape, "f32", placed, NAN, strided=False, data=x)}
    outs = {"nets": _buf(dev, (n, hdim, P), "f32", placed, NAN, k=0), "inps": _buf(dev, (n, hdim, P), "f32", placed, NAN, k=1)}
    st = _go(lib.sf_context_split, ins["cnets"].ptr, outs["nets"].ptr, outs["nets"].stride, outs["inps"].ptr, outs["inps"].stride, n, hdim, P)
    return st, ins, outs


@pytest.mark.parametrize("case", gc.cs_cases(), ids=_ids(gc.cs_cases()))
def test_context_split(dev, case):
    c = case
    n, hdim = c["n"], c["hdim"]
    what = c["id"]
    x = ref.draw_cs(c)
    t64, _ = ref.ref_context_split(x.double(), hdim)
    t32, relu = ref.ref_context_split(x, hdim)
    st1, ins1, outs1 = run_cs(dev, x, hdim, False)
    st2, ins2, outs2 = run_cs(dev, x, hdim, True)
    _ok(st1, what), _ok(st2, what)
    assert outs2["nets"].stride != outs2["inps"].stride
    _written(what, outs1), _written(what, outs2)
    _intact(what, ins1, outs1, ins2, outs2)
    _same_runs(what, outs1, outs2, "the gapped / offset run is not bitwise the contiguous one")
    nets, inps = outs1["nets"].region().clone(), outs1["inps"].region().clone()
    _bound("sf_context_split", what + " tanh", nets, t64, ref.tol_of(t32, t64))
    assert bool((inps.cpu() == relu).all()), (what, "the ReLU half")          # by value: -0.0 == 0.0
    for z in range(n):
        st, i1, o1 = run_cs(dev, x[z:z + 1], hdim, False)
        _ok(st, what), _intact((what, z), i1, o1)
        assert _same(o1["nets"].region(), nets[z:z + 1]) and _same(o1["inps"].region(), inps[z:z + 1]), (what, z)


# ---- sf_flow_update ------------------------------------------------------------------------------------------------------------------
def run_fu(dev, coords, delta, dest, row, nhw, placed):
    """dest: "a" / "b" / "ab" (fp32 destinations) or "koct" (rows `row`, `row + 1` of a 128-row k-octet image).  coords1 is updated
    in place: ins["coords1"] holds the result."""
    lib = _lib().load()
    n, h, w = nhw
    P = h * w
    ins = {"coords1": _buf(dev, (n, 2, P), "f32", placed, NAN, strided=False, data=coords)}
    if delta is not None:
        ins["delta"] = _buf(dev, (n, 2, P), "f32", placed, NAN, strided=False, data=delta)
    outs = {}
    if "a" in dest:
        outs["a"] = _buf(dev, (n, 2, P), "f32", placed, NAN, k=0)
    if "b" in dest:
        outs["b"] = _buf(dev, (n, 2, P), "f32", placed, NAN, k=1)
    if dest == "koct":
        outs["koct"] = _buf(dev, (n, gc.FU_KOCT_IMAGE_ROWS, P), "koct", placed, SENTINEL, k=2)
    st = _go(lib.sf_flow_update, ins["coords1"].ptr, _opt(ins.get("delta"))[0], *_opt(outs.get("a")), *_opt(outs.get("b")),
             *_opt(outs.get("koct")), row, n, h, w)
    return st, ins, outs


def _check_fu(what, coords, delta, ins, outs, row, nhw):
    """Everything exact: fp32 adds and a subtraction."""
    want_c, want_f = ref.ref_flow_update(coords, delta, *nhw)
    if delta is None:
        assert _untouched(ins["coords1"]), (what, "coords1 changed without a delta")
    else:
        assert _same(ins["coords1"].region().cpu(), want_c), (what, "coords1 + delta")
        assert _untouched(ins["delta"]), what
    assert ins["coords1"].outside_unchanged(), what
    for f in ("a", "b"):
        if f in outs:
            assert _same(outs[f].region().cpu(), want_f), (what, f)
            assert outs[f].outside_unchanged(), (what, f)
    if "koct" in outs:
        K = outs["koct"]
        img = K.region().cpu()
        assert _same(img[:, row:row + 2], want_f.half()), (what, "the two k-octet rows")
        rest = torch.cat([img[:, :row], img[:, row + 2:]], dim=1)
        assert _same(rest, torch.full_like(rest, SENTINEL)), (what, "another row of the k-octet image was written")
        assert K.outside_unchanged(), (what, "koct")


@pytest.mark.parametrize("case", gc.fu_cases(), ids=_ids(gc.fu_cases()))
def test_flow_update(dev, case):
    c = case
    nhw = c["nhw"]
    n = nhw[0]
    coords, delta_t = ref.draw_fu(c)
    for delta in (delta_t, None):
        for dest in gc.FU_DESTS:
            for row in (gc.FU_KOCT_ROWS if dest == "koct" else (0,)):
                what = f"{c['id']} {'delta' if delta is not None else 'nodelta'} {dest} row{row}"
                st1, ins1, outs1 = run_fu(dev, coords, delta, dest, row, nhw, False)
                st2, ins2, outs2 = run_fu(dev, coords, delta, dest, row, nhw, True)
                _ok(st1, what), _ok(st2, what)
                if dest == "ab":
                    assert outs2["a"].stride != outs2["b"].stride
                _check_fu(what, coords, delta, ins1, outs1, row, nhw)
                _check_fu(what + " placed", coords, delta, ins2, outs2, row, nhw)
                _same_runs(what, outs1, outs2, "the gapped / offset run is not bitwise the contiguous one")
                assert _same(ins1["coords1"].region(), ins2["coords1"].region()), what
                if dest in ("ab", "koct") and n > 1:
                    for z in range(n):
                        dz = None if delta is None else delta[z:z + 1]
                        st, i1, o1 = run_fu(dev, coords[z:z + 1], dz, dest, row, (1,) + nhw[1:], False)
                        _ok(st, what)
                        assert _same(i1["coords1"].region(), ins1["coords1"].region()[z:z + 1]), (what, z)
                        for f, G in o1.items():
                            assert G.outside_unchanged() and _same(G.region(), outs1[f].region()[z:z + 1]), (what, f, z)


# ---- sf_pack_koct --------------------------------------------------------------------------------------------------------------------
def run_pk(dev, x, placed):
    lib = _lib().load()
    n, rows, P = x.shape
    ins = {"x": _buf(dev, x.shape, "f32", placed, NAN, k=0, data=x)}
    outs = {"y": _buf(dev, (n, rows, P), "koct", placed, SENTINEL, k=1)}
    st = _go(lib.sf_pack_koct, ins["x"].ptr, ins["x"].stride, n, rows, P, outs["y"].ptr, outs["y"].stride)
    return st, ins, outs


def _pad_rows_keep_the_sentinel(Y, rows, P):
    """Rows [rows, next multiple of 8) of every image's last octet (outside the view: outside_unchanged() covers them; said again)."""
    pad = np.arange(rows, -(-rows // 8) * 8)
    if pad.size == 0:
        return True
    z = np.arange(Y.shape[0])[:, None, None]
    idx = Y.off + z * Y.stride + ((pad[None, :, None] // 8) * P + np.arange(P)[None, None, :]) * 8 + pad[None, :, None] % 8
    got = Y.buf[torch.from_numpy(idx.reshape(-1)).to(Y.buf.device)]
    return _same(got, torch.full_like(got, SENTINEL))


@pytest.mark.parametrize("case", gc.pk_cases(), ids=_ids(gc.pk_cases()))
def test_pack_koct(dev, case):
    c = case
    n, rows, P = c["n"], c["rows"], c["P"]
    what = c["id"]
    x = ref.draw_pk(c)
    want = x.half()                                                           # round to nearest even; 7e4 -> inf, 1e-7 -> a subnormal
    st1, ins1, outs1 = run_pk(dev, x, False)
    st2, ins2, outs2 = run_pk(dev, x, True)
    _ok(st1, what), _ok(st2, what)
    assert ins2["x"].stride > rows * P and outs2["y"].stride > -(-rows // 8) * 8 * P
    for outs in (outs1, outs2):
        assert _same(outs["y"].region().cpu(), want), (what, "not x rounded to fp16 (every row written)")
        assert _pad_rows_keep_the_sentinel(outs["y"], rows, P), (what, "a row past `rows` in the last octet was written")
    _intact(what, ins1, outs1, ins2, outs2)
    _same_runs(what, outs1, outs2, "the gapped / offset run is not bitwise the contiguous one")
    for z in range(n):
        st, i1, o1 = run_pk(dev, x[z:z + 1], False)
        _ok(st, what), _intact((what, z), i1, o1)
        assert _same(o1["y"].region(), outs1["y"].region()[z:z + 1]), (what, z)


# ---- sf_dwconv3x3_res ----------------------------------------------------------------------------------------------------------------
def run_dw(dev, x, w, b, layout, placed):
    """layout "f32x4": bases and strides at which the entry point takes its vec4 kernel when W % 4 == 0; "f32": the scalar kernel."""
    lib = _lib().load()
    n, C, H, W = x.shape
    ins = {"x": _buf(dev, (n, C * H, W), layout, placed, NAN, k=0, data=x), "w": _buf(dev, (1, 1, C * 9), "f32", placed, NAN, strided=False, data=w),
           "b": _buf(dev, (1, 1, C), "f32", placed, NAN, strided=False, data=b)}
    outs = {"y": _buf(dev, (n, C * H, W), layout, placed, NAN, k=1)}
    st = _go(lib.sf_dwconv3x3_res, ins["x"].ptr, ins["x"].stride, ins["w"].ptr, ins["b"].ptr, outs["y"].ptr, outs["y"].stride, n, C, H, W)
    return st, ins, outs


@pytest.mark.parametrize("case", gc.dw_cases(), ids=_ids(gc.dw_cases()))
def test_dwconv3x3_res(dev, case):
    c = case
    H, W = c["hw"]
    n = gc.DW_N[-1]
    for C in gc.DW_C:
        what = f"{c['id']} C{C}"
        x, w, b = ref.draw_dw(c, C, n)
        r64 = ref.ref_dwconv(x.double(), w.double(), b.double())
        tol = ref.tol_of(ref.ref_dwconv(x, w, b), r64)
        vec = "f32x4" if W % 4 == 0 else "f32"
        st1, ins1, outs1 = run_dw(dev, x, w, b, vec, False)
        st2, ins2, outs2 = run_dw(dev, x, w, b, vec, True)
        _ok(st1, what), _ok(st2, what)
        _written(what, outs1), _written(what, outs2)
        _intact(what, ins1, outs1, ins2, outs2)
        _same_runs(what, outs1, outs2, "the gapped / offset run is not bitwise the contiguous one")
        got = outs1["y"].region().clone()
        _bound("sf_dwconv3x3_res", what, got, r64, tol)
        if W % 4 == 0:                                                        # image strides that are no multiple of 4 floats: the scalar kernel
            st3, ins3, outs3 = run_dw(dev, x, w, b, "f32", True)
            _ok(st3, what), _written(what, outs3), _intact(what, ins3, outs3)
            assert ins3["x"].stride % 4 and outs3["y"].stride % 4
            assert _same(outs3["y"].region(), got), (what, "the scalar kernel and the vec4 kernel differ (same taps in the same order)")
        for z in range(n):
            st, i1, o1 = run_dw(dev, x[z:z + 1], w, b, vec, False)
            _ok(st, what), _intact((what, z), i1, o1)
            assert _same(o1["y"].region(), got[z:z + 1]), (what, z, "an image of a batch differs from the image alone")
