"""sf_gemm through raw descriptors, the two split-K forms and sf_softmax_rows against float64 (-m gpu).

Every operand sits inside a larger allocation whose padding (ld beyond the extent, rows past K, rows past M / N) holds NaN, so
a read of it that reaches a stored result shows up; every output sits inside a buffer of a finite sentinel with ldc > N and an
image stride beyond M * ldc, and everything outside [z][m < M][n < N] must come back bitwise unchanged.  The float64 reference
multiplies the values the arithmetic class multiplies (_operands): fp32 / f16x3 the operands as given, f16x2 (and f16 with an
fp32 A) the B operand rounded to fp16, f16 with packed weights both rounded, a stored-fp16 B its halves.  Case lists and the
dispatcher rules they cover: tests/gemm_cases.py."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_cases as gc
from tests.guarded import SENTINEL, Guarded, _operand, _output

pytestmark = pytest.mark.gpu

TOL = {"fp32": 3e-5, "f16x3": 3e-5, "f16x2": 5e-5, "f16": 5e-5}
SPLIT_PRECS = ("f16x3", "f16x2", "f16")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _prec(name):
    from streamflow_amd import ops
    return {"fp32": ops.PRECISION_FP32, "f16x3": ops.PRECISION_F16X3, "f16x2": ops.PRECISION_F16X2, "f16": ops.PRECISION_F16}[name]


def _epilogue(epi, v, R, dw_w, dw_b, gamma):
    from streamflow_amd import ops
    if epi == ops.EPI_GELU:
        return F.gelu(v)                         # exact (erf) form
    if epi == ops.EPI_RELU:
        return torch.relu(v)
    if epi == ops.EPI_RES:
        return R + v
    if epi == ops.EPI_RES_GELU:
        return F.gelu(R + v)
    if epi == ops.EPI_RES_GELU_DW1:
        t = F.gelu(R + v)
        return F.gelu(t + dw_w[None, :, None] * t + dw_b[None, :, None])
    if epi == ops.EPI_AXPY:
        return R + gamma * v
    return v


def _operands(prec, A, B, b_f16=False, packed=None):
    """float64 [batch][M][K] and [batch][K][N] of the values the arithmetic class multiplies.  A: fp32 values, or None with
    `packed` = (W [M][K] fp32, PackedLinear.split_scale s): f16 multiplies the fp16 rounding of s * W, undone by 1 / s."""
    if packed is not None:
        W, s = packed
        A = ((W * s).half().double() / s) if prec == "f16" else W.double()
        A = A[None]
    else:
        A = A.double()
    if not b_f16 and prec in ("f16x2", "f16"):
        B = B.half()
    return A, B.double()


def _ref(prec, A, B, epi, alpha, bias, R, dw_w, dw_b, gamma, b_f16=False, packed=None):
    A64, B64 = _operands(prec, A, B, b_f16, packed)
    v = torch.matmul(A64, B64)
    if bias is not None:
        v = v + bias.double()[None, :, None]
    v = alpha * v
    return _epilogue(epi, v, None if R is None else R.double(), dw_w.double(), dw_b.double(), gamma)


def _residual_inputs(g, M):
    return torch.randn(M, generator=g) * 0.5, torch.randn(M, generator=g) * 0.1, 0.37


def _check(C, ref, tol, what):
    assert C.outside_unchanged(), f"{what}: store outside [z][m < M][n < N]"
    got = C.region().double().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite results"
    err = (got - ref).abs().max().item()
    assert err <= tol, f"{what}: max error {err:.3e} > {tol:.1e}"
    return got


# ---- A. raw descriptors: every precision x layout pair x epilogue, guard bands and poison -------------------------------------
@pytest.mark.parametrize("case", [c for _, c in gc.raw_cases()], ids=[i for i, _ in gc.raw_cases()])
def test_raw_descriptor_vs_float64(dev, case):
    from streamflow_amd import ops
    prec, (alay, blay), epi = case["prec"], case["pair"], case["epi"]
    M, N, K, batch, alpha = case["M"], case["N"], case["K"], case["batch"], case["alpha"]
    rng = np.random.default_rng(case["seed"])
    g = torch.Generator().manual_seed(case["seed"])
    A = torch.randn(batch, M, K, generator=g) / K ** 0.5                   # logical [z][m][k]
    B = torch.randn(batch, K, N, generator=g)                              # logical [z][k][n]
    b16 = blay == ops.LAYOUT_F16_K_MINOR
    if b16:
        B = B.half()
    bias = torch.randn(M, generator=g) * 0.1 if case["bias"] else None
    Rv = torch.randn(batch, M, N, generator=g)
    dw_w, dw_b, gam = _residual_inputs(g, M)
    un = case["unaligned"]
    GA = _operand(dev, rng, A if alay == ops.LAYOUT_K_MINOR else A.transpose(1, 2), un)
    GB = _operand(dev, rng, B if blay == ops.LAYOUT_K_MAJOR else B.transpose(1, 2), un, torch.float16 if b16 else torch.float32)
    GR = _output(dev, rng, batch, M, N, un, fill=float("nan")).put(Rv)
    gamma = torch.tensor([gam], device=dev)
    dwd, dbd = dw_w.to(dev), dw_b.to(dev)
    biasd = None if bias is None else bias.to(dev)

    def run(p, C):
        ops.gemm_raw(ops.Ctx(_prec(p)), A=GA.ptr, B=GB.ptr, C=C.ptr, bias=None if biasd is None else biasd.data_ptr(),
                     R=GR.ptr, dw_w=dwd.data_ptr(), dw_b=dbd.data_ptr(), gamma=gamma.data_ptr(), M=M, N=N, K=K, batch=batch,
                     lda=GA.ld, ldb=GB.ld, ldc=C.ld, ldr=GR.ld, strideA=GA.stride, strideB=GB.stride, strideC=C.stride,
                     strideR=GR.stride, a_layout=alay, b_layout=blay, alpha=alpha, epilogue=epi)
        torch.cuda.synchronize()
        return C

    C = _output(dev, rng, batch, M, N, un)
    if case["refused"] is not None:
        with pytest.raises(RuntimeError, match=re.escape(case["refused"])):
            run(prec, C)
        assert bool((C.buf == SENTINEL).all()), "a refused descriptor wrote a result"
        return
    run(prec, C)
    ref = _ref(prec, A, B, epi, alpha, bias, Rv, dw_w, dw_b, gam, b_f16=b16)
    got = _check(C, ref, TOL[prec], case)
    assert GA.outside_unchanged() and GB.outside_unchanged() and GR.outside_unchanged(), "an operand was written"
    if prec == "f16":
        # with an fp32 A operand the one-product mode IS the two-product kernel (gemm_split.hip: an fp32 A is split on the fly)
        C2 = run("f16x2", _output(dev, rng, batch, M, N, un))
        assert torch.equal(C2.region().cpu().view(torch.int32), got.float().view(torch.int32)), "f16 != f16x2 with an fp32 A"


def test_a_padded_operand_vs_float64(dev):
    """a_padded = 1 promises A zero padded to [K up to 32][M up to 128]: the fp32 kernel loads the pad unconditionally.
    Real zeros there (what PackedLinear.wt holds); the result must not depend on the promise beyond it."""
    from streamflow_amd import ops
    g = torch.Generator().manual_seed(91)
    M, N, K, batch = 100, 301, 45, 2
    Wt = torch.randn(M, K, generator=g) / K ** 0.5
    X = torch.randn(batch, K, N, generator=g)
    lda = 128
    Apad = torch.zeros(1, 64, lda)
    Apad[0, :K, :M] = Wt.t()
    rng = np.random.default_rng(91)
    GA = Guarded(dev, 1, 64, lda, 0, lda, 64 * lda, 0.0).put(Apad)
    GB = _operand(dev, rng, X, False)
    for a_padded in (1, 0):
        C = _output(dev, rng, batch, M, N, False)
        ops.gemm_raw(ops.Ctx(ops.PRECISION_FP32), A=GA.ptr, B=GB.ptr, C=C.ptr, M=M, N=N, K=K, batch=batch, lda=lda, ldb=GB.ld,
                     ldc=C.ld, strideA=0, strideB=GB.stride, strideC=C.stride, a_layout=0, b_layout=0, alpha=0.75,
                     a_padded=a_padded)
        torch.cuda.synchronize()
        _check(C, 0.75 * torch.matmul(Wt.double()[None], X.double()), TOL["fp32"], ("a_padded", a_padded))


# ---- C. split-K chosen by the library (SfGemm.split_ws) --------------------------------------------------------------------
def _packed_case(dev, prec, epi, M, N, K, batch, seed, r_group):
    from streamflow_amd import ops
    from streamflow_amd.ops import PackedLinear
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    W = torch.randn(M, K, generator=g) / K ** 0.5
    bias = torch.randn(M, generator=g) * 0.1
    X = torch.randn(batch, K, N, generator=g)
    Rv = torch.randn(batch, M, N, generator=g)
    dw_w, dw_b, gam = _residual_inputs(g, M)
    pk = PackedLinear(W, bias, dev)
    GB = _operand(dev, rng, X, False)
    GR = _output(dev, rng, batch, M, N, False, fill=float("nan"), group=r_group).put(Rv)
    gamma, dwd, dbd = torch.tensor([gam], device=dev), dw_w.to(dev), dw_b.to(dev)
    alpha = 0.5

    def run(ws=None, ws_floats=0):
        C = _output(dev, rng, batch, M, N, False)
        kw = dict(split_ws=ws.data_ptr(), split_ws_floats=ws_floats) if ws is not None else {}
        ops.gemm_raw(ops.Ctx(_prec(prec)), B=GB.ptr, C=C.ptr, bias=pk.bias_split.data_ptr(), R=GR.ptr, dw_w=dwd.data_ptr(),
                     dw_b=dbd.data_ptr(), gamma=gamma.data_ptr(), M=M, N=N, K=K, batch=batch, ldb=GB.ld, ldc=C.ld, ldr=GR.ld,
                     strideB=GB.stride, strideC=C.stride, strideR=GR.stride, r_group=r_group, r_group_stride=GR.group_stride,
                     a_layout=ops.LAYOUT_SPLIT_F16, b_layout=ops.LAYOUT_K_MAJOR, A_hi=pk.hi.data_ptr(), A_lo=pk.lo.data_ptr(),
                     lda_h=pk.lda_h, a_k_pad=pk.k_pad, alpha=alpha / pk.split_scale, epilogue=epi, **kw)
        torch.cuda.synchronize()
        return C

    ref = _ref(prec, None, X, epi, alpha, bias, Rv, dw_w, dw_b, gam, packed=(W, pk.split_scale))
    return run, ref, (GB, GR)


@pytest.mark.parametrize("epi", range(gc.N_EPI))
@pytest.mark.parametrize("prec", SPLIT_PRECS)
def test_library_split_k_vs_float64(dev, prec, epi):
    """The split_ws path: auto_splits, partial slabs in the scratch, splitk_epilogue_kernel<EPI> (bias, alpha, grouped residual).
    Against float64, against the unsplit call (summation order only), bitwise run to run, and bitwise the unsplit result when
    the scratch is one float short."""
    from streamflow_amd import ops
    pi = SPLIT_PRECS.index(prec)
    M, N, K, batch = gc.AUTO_SPLIT_SHAPES[(epi + pi) % len(gc.AUTO_SPLIT_SHAPES)]
    need = ops.gemm_split_ws_floats(M, N, K, batch, cx=ops.Ctx(_prec(prec)))
    assert need > 0 and need % (batch * M * N) == 0, need
    grouped = epi in (ops.EPI_RES, ops.EPI_RES_GELU, ops.EPI_RES_GELU_DW1, ops.EPI_AXPY) and (epi + pi) % 2 == 0
    run, ref, operands = _packed_case(dev, prec, epi, M, N, K, batch, 8000 + 10 * pi + epi, 32 if grouped else 0)
    guard = 4096
    ws = torch.full((need + guard,), float("nan"), device=dev)
    C1 = run(ws, need)
    assert bool(torch.isfinite(ws[:need]).any()), "the scratch was not used: the dispatcher did not split"
    assert bool(torch.isnan(ws[need:]).all()), "write past split_ws_floats"
    got = _check(C1, ref, TOL[prec], (prec, epi, M, N, K))
    C2 = run(ws, need)
    assert torch.equal(C2.region().view(torch.int32), C1.region().view(torch.int32)), "split-K is not deterministic"
    C0 = run()
    plain = _check(C0, ref, TOL[prec], (prec, epi, "unsplit"))
    assert (got - plain).abs().max().item() <= TOL[prec]
    ws.fill_(float("nan"))
    C3 = run(ws, need - 1)                                   # too small: the dispatcher must not split
    assert torch.equal(C3.region().view(torch.int32), C0.region().view(torch.int32)), "short scratch changed the result"
    assert bool(torch.isnan(ws).all()), "a scratch shorter than ks * slab was written"
    for o in operands:
        assert o.outside_unchanged()


def test_library_split_k_not_taken(dev):
    """Problems the dispatcher must not split although the shape would: fp16 output (c_f16), the implicit 3x3 convolution and
    problems routed to the activation-stationary kernel.  Passing the scratch changes nothing, bitwise, and never writes it."""
    from dataclasses import replace
    from streamflow_amd import ops
    from streamflow_amd.ops import PackedLinear, Planes
    g = torch.Generator().manual_seed(95)

    def both(prec, M, N, K, batch, call):
        need = ops.gemm_split_ws_floats(M, N, K, batch, cx=ops.Ctx(_prec(prec)))
        assert need > 0, (M, N, K, batch)
        ws = torch.full((need,), float("nan"), device=dev)
        y0 = call(ops.Ctx(_prec(prec)))
        y1 = call(ops.Ctx(_prec(prec), split_ws=ws))
        torch.cuda.synchronize()
        assert torch.equal(y0.view(torch.int16 if y0.dtype == torch.float16 else torch.int32),
                           y1.view(torch.int16 if y1.dtype == torch.float16 else torch.int32)), (prec, M, N, K)
        assert bool(torch.isnan(ws).all()), ("scratch written", prec, M, N, K)
        return y0

    # c_f16 = 1: fp16 rows out
    M, N, K = 128, 300, 1024
    pk = PackedLinear(torch.randn(M, K, generator=g) / K ** 0.5, torch.randn(M, generator=g) * 0.1, dev)
    X = Planes.of(torch.randn(1, K, N, generator=g).to(dev))

    def f16_out(cx):
        ybuf = torch.zeros(M * N // 2, device=dev)
        ops.gemm(pk, X, Planes(ybuf, 0, M * N, 1, M, N, f16=True), ops.EPI_GELU, cx=cx)
        return ybuf.view(torch.float16).clone()

    both("f16x2", M, N, K, 1, f16_out)
    # conv3x3: K = 9 * 128
    cin, cout, h, w = 128, 64, 14, 14
    pc = PackedLinear(torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5, torch.randn(cout, generator=g) * 0.1, dev,
                      conv3x3=True)
    Xc = Planes.of(torch.randn(1, cin, h * w, generator=g).to(dev))

    def conv(cx):
        y = torch.empty(1, cout, h * w, device=dev)
        ops.gemm(pc, Xc, Planes.of(y), ops.EPI_RELU, hw=(h, w), cx=cx)
        return y

    both("f16x3", cout, h * w, 9 * cin, 1, conv)
    # activation-stationary: f16x2, fp16 k-octet B, M = 64 <= 96, 64 < K <= 640
    M, N, K = 64, 300, 512
    pb = PackedLinear(torch.randn(M, K, generator=g) / K ** 0.5, None, dev)
    Xp = Planes.of(torch.randn(1, K, N, generator=g).to(dev))
    sh = ops.new_shadow(Xp, dev)
    ops.pack_koct(Xp, sh)
    Xs = replace(Xp, shadow=sh)

    def bstat(cx):
        y = torch.empty(1, M, N, device=dev)
        ops.gemm(pb, Xs, Planes.of(y), ops.EPI_NONE, cx=cx)
        return y

    both("f16x2", M, N, K, 1, bstat)


# ---- D. split-K chosen by the caller + sf_splitk_combine -----------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(gc.CALLER_SPLIT_CASES)))
def test_caller_split_k_and_combine_vs_float64(dev, ci):
    """k_splits slabs of attn @ v (engine.py matrix-mode GMA), K not a whole number of k-tiles, then out = R + gamma * sum."""
    from streamflow_amd import ops
    from streamflow_amd.ops import Planes
    ks, (alay, blay), M, N, K, n = gc.CALLER_SPLIT_CASES[ci]
    prec = SPLIT_PRECS[ci % 3]
    g = torch.Generator().manual_seed(9000 + ci)
    rng = np.random.default_rng(9000 + ci)
    A = torch.randn(n, M, K, generator=g) / K ** 0.5
    b16 = blay == ops.LAYOUT_F16_K_MINOR
    B = torch.randn(n, K, N, generator=g)
    if b16:
        B = B.half()
    Rv = torch.randn(n, M, N, generator=g)
    gam = -0.61
    GA = _operand(dev, rng, A, ci % 2 == 1)
    GB = _operand(dev, rng, B.transpose(1, 2), ci % 2 == 1, torch.float16 if b16 else torch.float32)
    slab = n * M * N
    guard = 1024
    part = torch.full((ks * slab + guard,), float("nan"), device=dev)
    ops.gemm_raw(ops.Ctx(_prec(prec)), A=GA.ptr, B=GB.ptr, C=part.data_ptr(), M=M, N=N, K=K, batch=n, lda=GA.ld, ldb=GB.ld,
                 ldc=N, strideA=GA.stride, strideB=GB.stride, strideC=M * N, a_layout=alay, b_layout=blay, alpha=1.0,
                 epilogue=ops.EPI_NONE, k_splits=ks, split_stride=slab)
    torch.cuda.synchronize()
    assert bool(torch.isnan(part[ks * slab:]).all()), "write past the last slab"
    slabs = part[: ks * slab].view(ks, n, M, N)
    assert bool(torch.isfinite(slabs).all()), "a slab element was not written (empty K slices must write zeros)"
    A64, B64 = _operands(prec, A, B, b16)
    prod = torch.matmul(A64, B64)
    err = (slabs.double().sum(0).cpu() - prod).abs().max().item()
    assert err <= TOL[prec], (ks, M, N, K, prec, err)
    # combine: R and out as planes inside larger buffers (image strides beyond M * N)
    stride = M * N + 4 * int(rng.integers(1, 9))
    GR = Guarded(dev, n, M, N, 4, N, stride, float("nan")).put(Rv)
    GO = Guarded(dev, n, M, N, 8, N, stride + 8, SENTINEL)
    gamma = torch.tensor([gam], device=dev)
    ops.splitk_combine(part, slab, ks, M * N, Planes(GR.buf, GR.off, GR.stride, n, M, N), gamma,
                       Planes(GO.buf, GO.off, GO.stride, n, M, N))
    torch.cuda.synchronize()
    _check(GO, Rv.double() + gam * prod, TOL[prec], ("combine", ks, M, N, K, prec))
    assert GR.outside_unchanged() and GA.outside_unchanged() and GB.outside_unchanged()


# ---- E. sf_softmax_rows -------------------------------------------------------------------------------------------------
def _softmax_rows_input(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * torch.tensor([1.0, 10.0, 30.0])[torch.arange(rows) % 3][:, None]
    x[0] = torch.linspace(-80.0, 80.0, cols)[torch.randperm(cols, generator=g)]     # spread +-80
    if rows > 2:
        x[2] = 3.7                                                                   # constant row
    return x


@pytest.mark.parametrize("out16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 8191, 8192, 8193, 32768, 32769, 40000])
def test_softmax_rows_vs_float64(dev, cols, out16):
    """<256> up to 8192 columns, <1024> up to 32768, the three-pass long kernel beyond; in place or fp16 out."""
    from streamflow_amd import ops
    for rows in (1, 3, 300):
        x = _softmax_rows_input(rows, cols, 17 * cols + rows)
        x64 = x.double()
        ref = torch.softmax(x64, dim=1)
        guard = 64
        buf = torch.full((rows * cols + guard,), SENTINEL, device=dev)
        buf[: rows * cols] = x.view(-1).to(dev)
        o16 = torch.full((rows * cols + guard,), 7.0, dtype=torch.float16, device=dev) if out16 else None
        ops.softmax_rows(buf, rows, cols, out16=o16)
        torch.cuda.synchronize()
        assert bool((buf[rows * cols:] == SENTINEL).all()), "write past the last row"
        if out16:
            assert bool((o16[rows * cols:] == 7.0).all()), "fp16 write past the last row"
            got = o16[: rows * cols].view(rows, cols).cpu()
            r16 = ref.half()
            ulp = torch.from_numpy(np.spacing(r16.numpy().astype(np.float16)).astype(np.float64))
            err = (got.double() - r16.double()).abs()
            assert bool((err <= ulp).all()), (rows, cols, (err / ulp).max().item())
        else:
            got = buf[: rows * cols].view(rows, cols).cpu()
            d = (x64 - x64.max(dim=1, keepdim=True).values).abs()
            err = (got.double() - ref).abs()
            # ~1e-6 relative, plus the fp32 rounding of (x - max) that the exponent amplifies (2^-24 |x - max|)
            bound = (2e-6 + 2.0 ** -23 * d) * ref + 1e-37
            assert bool((err <= bound).all()), (rows, cols, (err / (ref + 1e-30)).max().item())
            assert (got.double().sum(1) - 1.0).abs().max().item() <= 1e-5
        if rows == 3:
            for r in range(rows):                            # a batch of rows == the same rows one at a time, bitwise
                b1 = x[r].to(dev).clone()
                s16 = torch.empty(cols, dtype=torch.float16, device=dev) if out16 else None
                ops.softmax_rows(b1, 1, cols, out16=s16)
                one = (s16 if out16 else b1).cpu()
                row = got[r]
                assert torch.equal(one.view(torch.int16 if out16 else torch.int32), row.view(torch.int16 if out16 else torch.int32)), r


def test_gma_attention_1024_kernel_vs_float64(dev):
    """The public gma.Attention at 96 x 96 (P = 9216: the <1024> softmax kernel), heads = 1, sampled query rows."""
    from streamflow_amd import gma
    torch.manual_seed(5)
    att = gma.Attention(dim=128, heads=1, dim_head=128)
    h = w = 96
    P = h * w
    fmap = torch.randn(1, 128, h, w)
    out = att.to(dev)(fmap.to(dev))
    torch.cuda.synchronize()
    assert out.shape == (1, 1, P, P)
    Wqk = att.to_qk.weight.detach().cpu().double().view(256, 128)
    qk = Wqk @ fmap.double().view(128, P)
    rows = torch.from_numpy(np.random.default_rng(5).choice(P, 48, replace=False))
    logits = att.scale * qk[:128, rows].t() @ qk[128:]
    ref = torch.softmax(logits, dim=1)
    got = out[0, 0, rows.to(dev)].double().cpu()
    rel = ((got - ref).abs() / ref).max().item()
    assert rel <= 1e-4, rel
    assert (got.sum(1) - 1.0).abs().max().item() <= 1e-5
