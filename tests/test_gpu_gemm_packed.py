"""sf_gemm with packed weights (a_layout = SF_LAYOUT_SPLIT_F16: the form that ships) through raw descriptors against float64
(-m gpu): the register-staged tiles, the k-octet DMA tile, the B-direct 128 x 256 kernel and the activation-stationary family.

Every case (tests/gemm_packed_cases.py; its coverage is proven on the CPU by tests/test_gemm_packed_cases_cpu.py) checks
  placement: operands sit in NaN-filled allocations -- the weight planes too: a read past [K pad][lda_h] that reaches a result
             shows -- and outputs in sentinel-filled ones with ld > N, gaps between images and bases off the allocation; everything
             outside [z][m < M][n < N] comes back bitwise unchanged (c_f16 = 2 may write the rows up to the end of the last octet,
             finite values; c_f16 = 3 may not), and no operand is written;
  value:     against the float64 product of the values the arithmetic class multiplies (_operands / _weights_eff), TOL[prec] for
             fp32 results and one fp16 rounding (2^-11 * 1.01 |ref| + 8e-5) for fp16 results;
  route:     sf_gemm_route on the very descriptor that runs names the kernel family (and instantiation) the case is there for."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_packed_cases as pc
from tests.guarded import SENTINEL, Placed, _bits
from tests.test_gpu_gemm_bstat import _weights_eff
from tests.test_gpu_gemm_descriptors import TOL, _operands, _ref

pytestmark = pytest.mark.gpu

FIN = 1000.0            # rows past K / M in the last octet of a k-octet operand: finite (they meet zero weights), not NaN


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    return torch.device("cuda:0")


class Weights:
    """PackedLinear's hi / lo planes re-cut to what the case states -- k extent = K rounded up to a_k_pad (32 for a_k_pad = 0), lda_h
    rows per k-octet plane -- in the middle of an fp16-NaN allocation.  Rows [M padded to 128, lda_h) hold NaN as well: no kernel
    has any business there."""

    def __init__(self, dev, W, bias, M, K, a_k_pad, lda_h, conv=False):
        from streamflow_amd.ops import PackedLinear
        self.pk = PackedLinear(W, bias, dev, conv3x3=conv)
        kp = pc.up(K, a_k_pad if a_k_pad else 32)
        mp = pc.up(M, 128)
        assert self.pk.hi.shape[0] * 8 >= kp and self.pk.hi.shape[1] == mp and lda_h >= mp
        guard = 4096                                                       # halves: 8 KB of NaN on either side
        self.bufs, self.ptrs = [], []
        for src in (self.pk.hi, self.pk.lo):
            buf = torch.full((2 * guard + kp // 8 * lda_h * 8,), float("nan"), dtype=torch.float16, device=dev)
            planes = buf[guard: guard + kp // 8 * lda_h * 8].view(kp // 8, lda_h, 8)
            planes[:, :mp] = src[: kp // 8]
            self.bufs.append((buf, buf.clone()))
            self.ptrs.append(buf.data_ptr() + 2 * guard)

    def untouched(self):
        return all(torch.equal(_bits(b), _bits(s)) for b, s in self.bufs)


def _data(c):
    """The problem's values on the host: W [M][K] in the kernel's k order, X [batch][rows of B][N] as stored, Bmat [batch][K][N] as
    multiplied, bias, residual, depthwise scale / shift, gamma."""
    g = torch.Generator().manual_seed(c["seed"])
    M, N, K, batch = c["M"], c["N"], c["K"], c["batch"]
    conv = c.get("conv")
    if conv:
        cin = K // 9
        W4 = torch.randn(M, cin, 3, 3, generator=g) / K ** 0.5
        W = W4.permute(0, 2, 3, 1).reshape(M, K)                            # k = (ky * 3 + kx) * Cin + c
    else:
        W4 = W = torch.randn(M, K, generator=g) / K ** 0.5
    bias = torch.randn(M, generator=g) * 0.1 if c.get("bias", True) else None
    X = torch.randn(batch, K // 9 if conv else K, N, generator=g)
    if c["lay"] != 8:
        X = X.half().float()                                                # the stored halves ARE the operand
    if conv:
        h, w = conv
        cols = F.unfold(X.view(batch, -1, h, w), 3, padding=1)              # [batch][c * 9 + tap][N]
        Bmat = cols.view(batch, -1, 9, N).permute(0, 2, 1, 3).reshape(batch, K, N)
    else:
        Bmat = X
    R = torch.randn(batch, M, N, generator=g)
    if c["r"] == 2:
        R = R.half().float()
    dw_w, dw_b = torch.randn(M, generator=g) * 0.5, torch.randn(M, generator=g) * 0.1
    return dict(W=W, W4=W4, bias=bias, X=X, Bmat=Bmat, R=R, dw_w=dw_w, dw_b=dw_b, gamma=0.37)


def _placed(dev, geo, fill, tail_fill=None, batch=1):
    kind, rows, cols, off, ld, stride, group, gs = geo
    return Placed(dev, kind, batch, rows, cols, off, ld, stride, group, gs, fill, tail_fill)


def _route(d):
    from streamflow_amd import _lib
    from tests.test_gemm_packed_cases_cpu import lib_route
    return lib_route(_lib.load(), d)


class Run:
    """One case on the GPU: buffers at the case's placement, the route of the real descriptor, the launch, every check."""

    def __init__(self, dev, c, data=None):
        from streamflow_amd import _lib
        self.c, self.dev = c, dev
        self.data = dt = data or _data(c)
        self.d = d = pc.descriptor(c)
        geo, batch = d.pop("_geo"), c["batch"]
        self.wt = Weights(dev, dt["W4"], dt["bias"], c["M"], c["K"], d["a_k_pad"], d["lda_h"], conv=bool(c.get("conv")))
        nan = float("nan")
        self.B = _placed(dev, geo["B"], nan, FIN, batch).put(dt["X"])
        self.C = _placed(dev, geo["C"], SENTINEL, None, batch)
        self.C16 = _placed(dev, geo["C16"], SENTINEL, None, batch) if "C16" in geo else None
        self.R = _placed(dev, geo["R"], nan, FIN, batch).put(dt["R"]) if "R" in geo else None
        self.small = {k: dt[k].to(dev) for k in ("dw_w", "dw_b")}
        self.small["gamma"] = torch.tensor([dt["gamma"]], device=dev)
        self.small["bias"] = self.wt.pk.bias_split
        real = dict(A_hi=self.wt.ptrs[0], A_lo=self.wt.ptrs[1], B=self.B.ptr, C=self.C.ptr)
        if self.C16 is not None:
            real["C16"] = self.C16.ptr
        if self.R is not None:
            real.update(R=self.R.ptr, dw_w=self.small["dw_w"].data_ptr(), dw_b=self.small["dw_b"].data_ptr(),
                        gamma=self.small["gamma"].data_ptr())
        real["bias"] = self.small["bias"].data_ptr() if dt["bias"] is not None else 0
        self.ws = None
        if d.get("split_ws"):
            self.ws = torch.full((d["split_ws_floats"] + 1024,), nan, device=dev)
            real["split_ws"] = self.ws.data_ptr()
        for k, v in real.items():                        # the real buffers sit where the case says: same alignment within 16 bytes
            if k in ("B", "C", "C16", "R", "A_hi", "A_lo"):
                assert v % 16 == d[k] % 16, (c["id"], k)
        d.update(real)
        d["alpha"] = c.get("alpha", 0.5) / self.wt.pk.split_scale
        # route: the library's own dispatch on THIS descriptor == the restatement == a kernel of the family the case is listed for
        self.route = _route(d)
        assert self.route == pc.route(d), (c["id"], self.route, pc.route(d))
        assert self.route[0] == "ok", (c["id"], self.route)
        self.prec_ctx = {"f16x3": _lib.PRECISION_F16X3, "f16x2": _lib.PRECISION_F16X2, "f16": _lib.PRECISION_F16}[c["prec"]]

    def launch(self):
        from streamflow_amd import ops
        kw = {k: v for k, v in self.d.items() if k != "precision" and not (k in ("bias", "R", "split_ws") and not v)}
        ops.gemm_raw(ops.Ctx(self.prec_ctx), **kw)
        torch.cuda.synchronize()
        return self

    def reference(self):
        c, dt = self.c, self.data
        s = self.wt.pk.split_scale
        ref = _ref(c["prec"], None, dt["Bmat"], c["epi"], c.get("alpha", 0.5), dt["bias"], dt["R"] if c["r"] else None, dt["dw_w"], dt["dw_b"],
                   dt["gamma"], b_f16=c["lay"] != 8, packed=(dt["W"], s))
        if not c.get("conv"):
            # the same product from the planes the kernel was handed (_weights_eff): the packer and _operands agree to the split error
            A = _weights_eff(self.wt.pk, c["M"], c["K"], c["prec"] == "f16")
            A0 = _operands(c["prec"], None, dt["Bmat"], True, packed=(dt["W"], s))[0][0]
            assert (A - A0).abs().max().item() <= 2.0 ** -21 * dt["W"].abs().max().item()
        return ref

    def check(self, ref=None):
        c = self.c
        what = c["id"]
        ref = self.reference() if ref is None else ref
        out = {}
        if c["c_f16"] in (0, 3):
            assert self.C.outside_unchanged(), f"{what}: fp32 store outside [z][m < M][n < N]"
            got = self.C.region().double().cpu()
            assert bool(torch.isfinite(got).all()), f"{what}: non-finite fp32 results"
            err = (got - ref).abs().max().item()
            print(f"{what}: fp32 max error {err:.3e} (tolerance {TOL[c['prec']]:.1e})")
            assert err <= TOL[c["prec"]], f"{what}: max error {err:.3e} > {TOL[c['prec']]:.1e}"
            out["C"] = self.C.region().clone()
        if c["c_f16"] != 0:
            H = self.C if c["c_f16"] != 3 else self.C16
            assert H.outside_unchanged(tail_free=c["c_f16"] == 2), f"{what}: fp16 store outside [z][m < M][n < N]"
            if c["c_f16"] == 2 and H.tail_idx is not None:
                assert bool(torch.isfinite(H.tail()).all()), f"{what}: non-finite rows past M in the last octet"
            got = H.region().double().cpu()
            assert bool(torch.isfinite(got).all()), f"{what}: non-finite fp16 results"
            err = (got - ref).abs()
            bound = 2.0 ** -11 * 1.01 * ref.abs() + 8e-5
            print(f"{what}: fp16 max error / bound {(err / bound).max().item():.3f}")
            assert bool((err <= bound).all()), f"{what}: fp16 result off by {(err / bound).max().item():.2f} bounds"
            out["H"] = H.region().clone()
        assert self.wt.untouched() and self.B.untouched() and (self.R is None or self.R.untouched()), f"{what}: an operand was written"
        if self.ws is not None:
            n = self.d["split_ws_floats"]
            assert bool(torch.isfinite(self.ws[:n]).any()) and bool(torch.isnan(self.ws[n:]).all()), f"{what}: split_ws use"
        return out


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


# ---- A. placement: pitched / dense / unaligned, bitwise the same results ----------------------------------------------------
_A = [c for c in pc.cases() if c["part"] == "A"]
_A_TRIPLES = [_A[i:i + 3] for i in range(0, len(_A), 3)]


@pytest.mark.parametrize("triple", _A_TRIPLES, ids=[t[0]["id"].replace("-pitched", "") for t in _A_TRIPLES])
def test_placements_vs_float64_and_each_other(dev, triple):
    data, ref, outs = _data(triple[0]), None, []
    for c in triple:
        assert c["seed"] == triple[0]["seed"]
        run = Run(dev, c, data).launch()
        ref = run.reference() if ref is None else ref
        outs.append(run.check(ref))
    assert _same(outs[0], outs[1]), "dense != pitched"
    assert _same(outs[0], outs[2]), "unaligned != pitched"


# ---- B. edges ---------------------------------------------------------------------------------------------------------------
_B = [c for c in pc.cases() if c["part"].startswith("B-") and c["part"] != "B-prefix"]


@pytest.mark.parametrize("case", _B, ids=[c["id"] for c in _B])
def test_edges_vs_float64(dev, case):
    run = Run(dev, case).launch()
    run.check()
    fam = run.route[1]["family"]
    want = {"B-bstat": (pc.FAM_BSTAT, pc.FAM_BSTAT_GELU), "B-nks": (pc.FAM_BSTAT, pc.FAM_BSTAT_GELU), "B-msplit": (pc.FAM_BSTAT, pc.FAM_BSTAT_GELU),
            "B-m192": (pc.FAM_BSTAT,), "B-bdirect": (pc.BDIRECT,), "B-below": (pc.KOCT_DMA,), "B-tiledc2": (pc.SPLIT_TILED, pc.KOCT_DMA),
            "B-tile": (pc.SPLIT_TILED,), "B-conv": (pc.SPLIT_TILED,), "B-splitk": (pc.SPLIT_TILED, pc.KOCT_DMA)}.get(case["part"])
    if want is not None:
        assert fam in want, (case["id"], fam)
    if case["part"] == "B-splitk":
        assert run.route[1]["k_splits"] > 1


_PREFIX = [c for c in pc.cases() if c["part"] == "B-prefix"]
_PAIRS = [_PREFIX[i:i + 2] for i in range(0, len(_PREFIX), 2)]


@pytest.mark.parametrize("pair", _PAIRS, ids=[p[0]["id"] for p in _PAIRS])
def test_bstat_pixel_prefix_is_bitwise_the_smaller_run(dev, pair):
    """A wave owns its pixels' whole K: the first `small` pixels of the run at `big` are bitwise the run at `small`."""
    big, small = pair
    assert (big["N"], small["N"]) == big["pair"] == small["pair"]
    db = _data(big)
    ds = dict(db, X=db["X"][:, :, : small["N"]].contiguous(), Bmat=db["Bmat"][:, :, : small["N"]].contiguous(),
              R=db["R"][:, :, : small["N"]].contiguous())
    ob = Run(dev, big, db).launch().check()
    os_ = Run(dev, small, ds).launch().check()
    assert ob.keys() == os_.keys()
    for k in ob:
        assert torch.equal(_bits(ob[k][:, :, : small["N"]].contiguous()), _bits(os_[k])), k


# ---- C. determinism ---------------------------------------------------------------------------------------------------------
_C = [c for c in pc.cases() if c["part"] == "C"]


@pytest.mark.parametrize("case", _C, ids=[c["id"] for c in _C])
def test_five_runs_are_bitwise_equal(dev, case):
    run = Run(dev, case)
    first = run.launch().check()
    for rep in range(4):
        run.C.buf.copy_(run.C.snap)
        if run.C16 is not None:
            run.C16.buf.copy_(run.C16.snap)
        run.launch()
        now = {}
        if case["c_f16"] in (0, 3):
            now["C"] = run.C.region()
        if case["c_f16"] != 0:
            now["H"] = (run.C if case["c_f16"] != 3 else run.C16).region()
        assert _same(first, now), (case["id"], rep)
