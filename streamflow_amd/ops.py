"""Tensor-level wrappers over the C ABI (streamflow_amd/_lib.py).

Internal data layout: every activation is a set of *channel-major planes* ``[n_img][rows][P]``
(P = h*w contiguous, i.e. NCHW) living inside a flat fp32 device buffer; a :class:`Planes`
object is a (pointer, image stride, rows) view of it, so concatenations (``torch.cat`` in the
reference) are just kernels writing into row slices of a wider buffer.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass, replace
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import (EPI_AXPY, EPI_GELU, EPI_NONE, EPI_RELU, EPI_RES, EPI_RES_GELU, EPI_RES_GELU_DW1,  # noqa: F401
                   LAYOUT_K_MAJOR, LAYOUT_K_MINOR, LAYOUT_SPLIT_F16, LAYOUT_F16_K_MINOR, PRECISION_F16, PRECISION_F16X2, PRECISION_F16X3,
                   PRECISION_FP32,
                   SfGemm)

# Arithmetic mode of every GEMM-shaped op (sf_gemm, corr build):
#   PRECISION_FP32  exact fp32 on v_mfma_f32_32x32x2_f32
#   PRECISION_F16X3 split precision (x = hi + lo in fp16, 3 MFMAs per product, fp32 accumulate; ~2^-22 relative)
#   PRECISION_F16X2 weights split hi + lo, activations rounded once to fp16 (2 MFMAs per product; 2^-11 relative on
#                   the activations: ~1e-4 px EPE on the flows)
#   PRECISION_F16   weights AND activations rounded once to fp16 (1 MFMA per product, fp32 accumulation): the reference's
#                   deployed arithmetic class (fp16 autocast), opt-in
PRECISION = PRECISION_F16X3
_PRECISION_NAMES = {"fp32": PRECISION_FP32, "f16x3": PRECISION_F16X3, "f16x2": PRECISION_F16X2, "f16": PRECISION_F16}


def set_precision(mode) -> int:
    """mode: 'fp32' | 'f16x3' | 'f16x2' (or the integer constants).  Returns the previous mode."""
    global PRECISION
    prev = PRECISION
    PRECISION = _PRECISION_NAMES[mode] if isinstance(mode, str) else int(mode)
    if PRECISION not in (PRECISION_FP32, PRECISION_F16X3, PRECISION_F16X2, PRECISION_F16):
        PRECISION = prev
        raise RuntimeError(f"unknown precision {mode}")
    return prev


def precision_name() -> str:
    return {v: k for k, v in _PRECISION_NAMES.items()}[PRECISION]


@dataclass(frozen=True)
class Ctx:
    """Everything a launch depends on besides its operands -- passed explicitly (`cx=`) by the engine and the encoder, so
    that two engines with different presets can be driven from two threads (there is no process-wide launch
    state; the module-level PRECISION below is only the DEFAULT of calls that do not pass a context, like a default dtype).
    precision: PRECISION_*.  split_ws: scratch that lets sf_gemm split K for small grids (None: never).
    shadows / shadow_fused: use and maintain Planes.shadow; producers write the k-octet copy in their own epilogue.
    flash_stats: the fused GMA kernel uses the softmax statistics stored once per clip.
    hidden_f16 / hidden_koct / pw_fold / x2_f16: hand-over formats inside an SK block (engine.run_skblock)."""
    precision: int
    split_ws: Optional[torch.Tensor] = None
    shadows: bool = True
    shadow_fused: bool = True
    flash_stats: bool = True
    hidden_f16: bool = True
    hidden_koct: bool = True
    pw_fold: bool = True
    x2_f16: bool = True
    ffn_pairs: bool = True      # an SK block's ffn1 / ffn2 as ONE launch where sf_ffn_pair has the shape (csrc/ffn_pair.hip)
    head_pairs: bool = False    # ... also the flow head's (grouped view, fp32 residual)
    sk_tail: bool = True        # an SK block's pw -> ffn2.0 -> ffn2.2 as ONE launch where sf_sk_tail has the shape (csrc/sk_tail.hip)
    sk_tail_all: bool = False   # ... also where it does not pay (the flow head's shape, small launches)

    def no_split(self) -> "Ctx":
        """The same context without the split-K scratch (ONE buffer: only one stream may use it at a time)."""
        return self if self.split_ws is None else replace(self, split_ws=None)


def _cx(cx: Optional["Ctx"]) -> "Ctx":
    return cx if cx is not None else Ctx(PRECISION)


class Profiler:
    """Per-launch HIP-event timing on the stream the kernels are launched on (torch's current stream).
    Used by bench.py's instrumented pass: every wrapped op records (name, algorithmic flops, algorithmic
    bytes, start event, end event)."""

    def __init__(self):
        self.records = []

    def launch(self, name, flops, nbytes, fn, products=1.0):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        self.records.append((name, float(flops), float(nbytes), s, e, float(flops) * float(products)))

    def summary(self):
        """per name: launches, ms, algorithmic flops and bytes, and mfma_flops = flops x MFMA products per algorithmic
        product (3 / 2 / 1 in f16x3 / f16x2 / f16 or a single-product layer; fp32 MFMA counts as 1)."""
        torch.cuda.synchronize()
        out = {}
        for name, fl, by, s, e, mf in self.records:
            d = out.setdefault(name, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0, "mfma_flops": 0.0})
            d["launches"] += 1
            d["ms"] += s.elapsed_time(e)
            d["flops"] += fl
            d["bytes"] += by
            d["mfma_flops"] += mf
        return out


# SF_DEBUG_RANGE=1: before every contraction that rounds / splits an fp32 operand to fp16, check max |x| < 65504 (the fp16
# range: above it `hi` saturates silently) -- a host-side, synchronising debug aid; raises RuntimeError
DEBUG_RANGE = os.environ.get("SF_DEBUG_RANGE", "0") == "1"
F16_MAX = 65504.0


def _check_range(X: "Planes", what: str) -> None:
    if X.f16 or X.group:
        return
    m = float(X.tensor().abs().max())
    if not (m < F16_MAX):
        raise RuntimeError(f"SF_DEBUG_RANGE: {what}: max |activation| = {m:.4g} does not fit fp16 (65504): the split-precision "
                           "modes would saturate it silently; run this layer with precision='fp32'")


PROFILER: Optional[Profiler] = None
PROFILE_SHAPES = False      # tag GEMM launches with their shape in the profiler (bench.py --gemm-shapes)


def _launch(name: str, flops: float, nbytes: float, fn, products: float = 1.0) -> None:
    if PROFILER is None:
        fn()
    else:
        PROFILER.launch(name, flops, nbytes, fn, products)


def _products(prec: int) -> float:
    return {PRECISION_FP32: 1.0, PRECISION_F16X3: 3.0, PRECISION_F16X2: 2.0, PRECISION_F16: 1.0}[prec]


def on_tensor_device(fn):
    """Run `fn` with the device of its first tensor / Planes / torch.device argument current.  The C ABI enqueues on
    the stream it is given and `_lib.stream()` is the CURRENT device's stream, so a launch on tensors of another GPU
    would otherwise mix a device-0 stream with device-1 pointers."""
    import functools

    def _device(a):
        if isinstance(a, torch.Tensor):
            return a.device if a.is_cuda else None
        if isinstance(a, Planes):
            return a.base.device
        if isinstance(a, BlockedVolume):
            return a.buf.device
        if isinstance(a, torch.device):
            return a if a.type == "cuda" else None
        if isinstance(a, (list, tuple)) and a:
            return _device(a[0])
        return None

    @functools.wraps(fn)
    def wrapped(*args, **kw):
        for a in list(args) + list(kw.values()):
            d = _device(a)
            if d is not None:
                with torch.cuda.device(d):
                    return fn(*args, **kw)
        return fn(*args, **kw)

    return wrapped


def _dev_check(t: torch.Tensor) -> None:
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError("streamflow_amd ops need contiguous float32 tensors on the GPU "
                           f"(got device={t.device}, dtype={t.dtype}, contiguous={t.is_contiguous()}); "
                           "there is no CPU fallback")


@dataclass(frozen=True)
class Planes:
    """View of channel-major planes [n_img][rows][P] inside ``base`` (a flat fp32 device tensor)."""
    base: torch.Tensor
    off: int            # float offset of (img 0, row 0)
    img_stride: int     # floats between consecutive images
    n_img: int
    rows: int
    P: int
    group: int = 0          # rows per group for '(B T) C -> B (T C)' views (0 = plain)
    group_stride: int = 0
    f16: bool = False       # the planes hold IEEE fp16 values (img_stride then counts halves; `off` stays in floats of
                            # the underlying fp32 allocation): GEMM-to-GEMM hand-over in the f16x2 mode (SfGemm.c_f16)
    koct: bool = False      # (with f16) k-octet planes [ceil(rows/8)][P][8] instead of rows [rows][P]: the consumer GEMM's
                            # LDS image, moved there by DMA (SF_LAYOUT_F16_KOCT / c_f16 = 2)
    shadow: Optional["Planes"] = None   # fp16 k-octet COPY of these fp32 planes, kept current by every producer (f16x2 mode):
                                        # a GEMM on the DMA-fed tile reads it as its B operand, everything else (residuals,
                                        # element-wise kernels) keeps reading the fp32 planes

    @staticmethod
    def of(t: torch.Tensor) -> "Planes":
        """Wrap a contiguous [n, C, h, w] or [n, C, P] tensor."""
        _dev_check(t)
        n, c = t.shape[0], t.shape[1]
        p = t.numel() // (n * c)
        return Planes(t, 0, c * p, n, c, p)

    @property
    def ptr(self) -> int:
        return self.base.data_ptr() + 4 * self.off

    def slice(self, r0: int, r1: int, unshadowed: bool = False) -> "Planes":
        """Rows r0 .. r1-1.  A slice of shadowed planes that does not start on an octet cannot carry the k-octet copy along:
        the caller must say so (`unshadowed=True`) and keep that copy current itself -- a producer writing through such a
        slice would otherwise leave the parent's copy stale without any error."""
        assert 0 <= r0 < r1 <= self.rows and self.group == 0
        if self.f16:                                # k-octet planes: whole octets only
            assert self.koct and r0 % 8 == 0 and self.shadow is None
            return replace(self, off=self.off + (r0 // 8) * self.P * 4, rows=r1 - r0)
        if self.shadow is not None and r0 % 8 != 0 and not unshadowed:
            raise RuntimeError(f"Planes.slice({r0}, {r1}): shadowed planes can only be sliced at octet boundaries "
                               "(pass unshadowed=True and maintain the k-octet copy explicitly)")
        sh = self.shadow.slice(r0, r1) if (self.shadow is not None and r0 % 8 == 0) else None
        return replace(self, off=self.off + r0 * self.P, rows=r1 - r0, shadow=sh)

    def tensor(self) -> torch.Tensor:
        """Materialise as a [n_img, rows, P] torch view (only for contiguous-row, ungrouped views)."""
        assert self.group == 0
        if self.f16 and self.koct:                     # logical [n_img, rows, P] copy out of the octet planes (tests only)
            h = self.base.view(torch.float16)
            oc = (self.rows + 7) // 8
            t = torch.as_strided(h, (self.n_img, oc, self.P, 8), (self.img_stride, self.P * 8, 8, 1),
                                 2 * (self.base.storage_offset() + self.off))
            return t.permute(0, 1, 3, 2).reshape(self.n_img, oc * 8, self.P)[:, : self.rows]
        if self.f16:
            h = self.base.view(torch.float16)
            return torch.as_strided(h, (self.n_img, self.rows, self.P), (self.img_stride, self.P, 1),
                                    2 * (self.base.storage_offset() + self.off))
        return torch.as_strided(self.base, (self.n_img, self.rows, self.P), (self.img_stride, self.P, 1),
                                self.base.storage_offset() + self.off)


class Workspace:
    """Bump allocator over one flat device buffer; `take` hands out contiguous [n_img][rows][P] planes."""

    def __init__(self, floats: int, device):
        self.buf = torch.empty(int(floats), dtype=torch.float32, device=device)
        self.top = 0

    def take(self, n_img: int, rows: int, P: int) -> Planes:
        size = n_img * rows * P
        start = (self.top + 63) // 64 * 64          # 256-byte aligned
        if start + size > self.buf.numel():
            raise RuntimeError("workspace exhausted")
        self.top = start + size
        return Planes(self.buf, start, rows * P, n_img, rows, P)

    def take_flat(self, floats: int) -> torch.Tensor:
        start = (self.top + 63) // 64 * 64
        if start + floats > self.buf.numel():
            raise RuntimeError("workspace exhausted")
        self.top = start + floats
        return self.buf[start:start + floats]


class PackedLinear:
    """A 1x1-conv / Linear weight [Cout, Cin(,1,1)] repacked K-major ([Cin][Cout padded to 4]) for sf_gemm."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor], device, conv3x3: bool = False):
        # single: in the f16x2 mode this layer's weights enter the products as their round-to-nearest fp16 `hi` image alone
        # (ONE MFMA per product instead of two, no `lo` plane read): set per layer by HotPathEngine(single_layers=...)
        self.single = False
        w = weight.detach().to(device=device, dtype=torch.float32)
        if conv3x3:                                   # [Cout, Cin, 3, 3] -> k = (ky*3+kx)*Cin + c
            cout = w.shape[0]
            w2 = w.permute(2, 3, 1, 0).reshape(-1, cout)
        else:
            w2 = w.reshape(w.shape[0], -1).t()
        self.K, self.M = w2.shape
        self.lda = (self.M + 127) // 128 * 128            # zero padded to [K up to 32][M up to 128] (a_padded)
        wt = torch.zeros((self.K + 31) // 32 * 32, self.lda, dtype=torch.float32, device=device)
        wt[: self.K, : self.M] = w2
        self.wt = wt.contiguous()
        self.bias = None if bias is None else bias.detach().to(device=device, dtype=torch.float32).contiguous()
        self.conv3x3 = conv3x3
        # split-precision image: w = hi + lo (fp16 each) in k-octet planes [K padded to 32 / 8][M padded to 128][8], zero
        # padded (SF_LAYOUT_SPLIT_F16): 16 bytes = one MFMA operand octet of one output row.
        # The tensor is first scaled by a power of two so that max|w| lands in [1, 2): fp16 keeps 11 bits only for
        # |x| >= 6.1e-5, so the lo part of an unscaled small weight (|w| < 0.12) would fall into fp16 subnormals
        # (absolute spacing 6e-8) and a layer whose weights are all ~1e-3 would keep ~15 bits instead of ~21.  The
        # scale is exact (power of two) and is undone in the epilogue: alpha' = alpha / s, bias' = bias * s.
        # (K padded to 128: the tiled kernels read K rounded up to 32, the activation-stationary one whole weight stages)
        mp, kp = (self.M + 127) // 128 * 128, (self.K + 127) // 128 * 128
        self.k_pad = 128
        wmax = float(w2.abs().max()) if w2.numel() else 0.0
        if not torch.isfinite(torch.tensor(wmax)):
            raise RuntimeError("PackedLinear: non-finite weight")
        self.split_scale = 2.0 ** min(14, max(-14, -math.floor(math.log2(wmax)))) if wmax > 0 else 1.0
        wm = torch.zeros(mp, kp, dtype=torch.float32, device=device)
        wm[: self.M, : self.K] = w2.t() * self.split_scale
        hi = wm.to(torch.float16)
        lo = (wm - hi.float()).to(torch.float16)
        self.hi = hi.view(mp, kp // 8, 8).permute(1, 0, 2).contiguous()
        self.lo = lo.view(mp, kp // 8, 8).permute(1, 0, 2).contiguous()
        self.lda_h = mp
        self.bias_split = None if self.bias is None else (self.bias * self.split_scale).contiguous()
        # achieved split accuracy relative to the largest weight (reported, used by tests)
        self.split_error = float(((hi.float() + lo.float()) - wm).abs().max() / max(wmax * self.split_scale, 1e-30))


def _bias_ptr(A: "PackedLinear") -> Optional[int]:
    """Device address of a layer's pre-scaled bias (None: no bias)."""
    return None if A.bias_split is None else A.bias_split.data_ptr()


def _shared_products(layers, cx: "Ctx") -> Optional[int]:
    """MFMA products per weight where a kernel takes ONE value for all its layers: 1 (fp16 weights) or 2 (hi + lo); a layer set that
    mixes the two keeps the unfused launches (None)."""
    if cx.precision == PRECISION_F16 or all(l.single for l in layers):
        return 1
    return 2 if not any(l.single for l in layers) else None


class _PackedStream:
    """What the weight streams of the fused chain kernels share (csrc/weight_ring.h is their consumer): one stream per product
    count(s), built on first use and kept; never inside a graph capture; (hi, lo) fp16 images of split_scale * W.  A subclass adds
    its fragment order (`stream`) and which stream a context asks for (`prebuild`)."""

    def __init__(self):
        self._streams = {}

    @staticmethod
    def _split(A: "PackedLinear", rows: int, cols: int):
        """(hi, lo) fp16 images of split_scale * W, zero-padded to [rows, cols] (the same rounding as PackedLinear.hi / .lo)."""
        w = torch.zeros(rows, cols, dtype=torch.float32, device=A.wt.device)
        w[: A.M, : A.K] = A.wt[: A.K, : A.M].t() * A.split_scale
        hi = w.to(torch.float16)
        return hi, (w - hi.float()).to(torch.float16)

    def _cached(self, key, pack) -> torch.Tensor:
        """The stream of `key`, packed by pack() on first use.  A forward enqueues on several streams and may be a graph capture: a
        stream built inside one would be read by another before it exists, so the first use must come earlier (prebuild)."""
        st = self._streams.get(key)
        if st is None:
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{type(self).__name__}.stream: weight stream requested for the first time inside a graph capture; "
                                   "build it before (HotPathEngine does at construction)")
            st = self._streams[key] = pack()
        return st


class PackedPair(_PackedStream):
    """The two 1x1 convolutions of an SK block's FFN (update.py:14-16: conv -> GELU -> conv) as ONE weight stream for
    sf_ffn_pair (csrc/ffn_pair.hip): 1-KB MFMA fragments in consumption order, built per (products of layer 1, products of
    layer 2) on first use.  `first` / `second` are the layers' PackedLinear objects (their `single` flags, scales and biases
    are the source of truth: the pair computes exactly what the two sf_gemm launches compute)."""

    S = 16                                               # fragments per stage (csrc/ffn_pair.hip)

    def __init__(self, first: "PackedLinear", second: "PackedLinear"):
        assert first.M == second.K and not first.conv3x3 and not second.conv3x3
        super().__init__()
        self.first, self.second = first, second
        self.K1, self.H, self.M2 = first.K, first.M, second.M

    def products(self, cx: "Ctx"):
        one = cx.precision == PRECISION_F16
        return (1 if (one or self.first.single) else 2), (1 if (one or self.second.single) else 2)

    def prebuild(self, cx: "Ctx") -> None:
        if (self.K1, self.M2) in PAIR_SHAPES[0] | PAIR_SHAPES[1]:
            self.stream(*self.products(cx))

    def stream(self, pm1: int, pm2: int) -> torch.Tensor:
        return self._cached((pm1, pm2), lambda: self._pack(pm1, pm2))

    def _pack(self, pm1: int, pm2: int) -> torch.Tensor:
        nk1, nt2, hp = (self.K1 + 31) // 32, (self.M2 + 15) // 16, (self.H + 31) // 32
        fpad = int(_lib.load().sf_ffn_pair_frags(self.K1, self.M2, pm1, pm2))
        h1, l1 = self._split(self.first, hp * 32, nk1 * 32)
        h2, l2 = self._split(self.second, nt2 * 16, hp * 32)
        dev = h1.device
        # layer 1: fragment (m, u, s, plane) = rows 32 m + 16 u .. + 15, k 32 s .. + 31; lane (row, kq) holds k = 8 kq .. + 7
        planes1 = [l1, h1] if pm1 == 2 else [h1]
        f1 = torch.stack([w.view(hp, 2, 16, nk1, 4, 8) for w in planes1], dim=0)          # [plane, m, u, row, s, kq, i]
        f1 = f1.permute(1, 2, 4, 0, 5, 3, 6).reshape(hp, 2 * nk1 * pm1, 64 * 8)          # [m][(u, s, plane)][(kq, row), i]
        # layer 2: fragment (m, t, plane) = rows 16 t .. + 15, hidden rows 32 m .. + 31 in the order the layer-1 accumulators
        # hold them: k = 8 kq + i  <->  4 kq + i (i < 4) | 16 + 4 kq + i - 4 (i >= 4)
        kq = torch.arange(4, device=dev).view(4, 1)
        i = torch.arange(8, device=dev).view(1, 8)
        perm = torch.where(i < 4, 4 * kq + i, 16 + 4 * kq + i - 4).reshape(-1)             # [32] hidden row of (kq, i)
        planes2 = [l2, h2] if pm2 == 2 else [h2]
        f2 = torch.stack([w.view(nt2, 16, hp, 32)[..., perm].reshape(nt2, 16, hp, 4, 8) for w in planes2], dim=0)
        f2 = f2.permute(3, 1, 0, 4, 2, 5).reshape(hp, nt2 * pm2, 64 * 8)                  # [m][(t, plane)][(kq, row), i]
        pad = torch.zeros(hp, fpad - f1.shape[1] - f2.shape[1], 64 * 8, dtype=torch.float16, device=dev)
        st = torch.cat([f1, f2, pad], dim=1).contiguous().view(-1)
        assert st.numel() * 2 == hp * fpad * 1024
        return st


class PackedTail(_PackedStream):
    """The back half of an SK block -- pw (residual folded: W + I), ffn2.0, ffn2.2 (update.py:35-36, :14-16) -- as ONE weight stream for
    sf_sk_tail (csrc/sk_tail.hip): 1-KB fragments of 32 rows x 16 k in consumption order, units padded to 16-fragment stages (layout:
    include/streamflow_hip.h).  The PackedLinear objects stay the source of truth (rounding, power-of-two scales, biases, `single`)."""

    S = 16

    def __init__(self, pw_res: "PackedLinear", f0: "PackedLinear", f2: "PackedLinear"):
        assert pw_res.M == pw_res.K == f0.K and f0.M == f2.K and not (pw_res.conv3x3 or f0.conv3x3 or f2.conv3x3)
        super().__init__()
        self.layers = (pw_res, f0, f2)
        self.C, self.H, self.M2 = pw_res.K, f0.M, f2.M

    def products(self, cx: "Ctx") -> Optional[int]:
        return _shared_products(self.layers, cx)

    def built(self, pm: Optional[int]) -> bool:
        return pm is not None and int(_lib.load().sf_sk_tail_frags(self.C, self.H, self.M2, pm)) > 0

    def prebuild(self, cx: "Ctx") -> None:
        pm = self.products(cx)
        if self.built(pm):
            self.stream(pm)

    def stream(self, pm: int) -> torch.Tensor:
        return self._cached(pm, lambda: self._pack(pm))

    def _pack(self, pm: int) -> torch.Tensor:
        nc, nh, nm = (self.C + 31) // 32, self.H // 32, (self.M2 + 31) // 32
        ks = 2 * nc
        stage, group, one = C.c_int(0), C.c_int(0), C.c_int(0)
        total = int(_lib.load().sf_sk_tail_layout(self.C, self.H, self.M2, pm, C.byref(stage), C.byref(group), C.byref(one)))
        assert total > 0 and (stage.value, group.value, one.value) == (self.S, 1, 0)   # every tile a unit of its own, padded to a stage
        w1, w2, w3 = (self._split(l, r, c) for l, (r, c) in zip(self.layers, ((nc * 32, nc * 32), (nh * 32, nc * 32), (nm * 32, nh * 32))))
        dev = w1[0].device
        khalf = torch.arange(2, device=dev).view(2, 1)
        i = torch.arange(8, device=dev).view(1, 8)
        natural = (8 * khalf + i).reshape(-1)                                          # column of (khalf, i) inside a natural k-step
        acc_order = ((i & 3) + 8 * (i >> 2) + 4 * khalf).reshape(-1)                   # ... inside a k-step made of accumulator registers
        out = []
        zero = torch.zeros(512, dtype=torch.float16, device=dev)

        def emit(w, r0, cols):                                                         # lo before hi; lane (khalf, row m): 8 halves
            for plane in ((w[1], w[0]) if pm == 2 else (w[0],)):
                out.append(plane[r0:r0 + 32][:, cols].reshape(32, 2, 8).permute(1, 0, 2).reshape(512))

        def pad():
            while len(out) % self.S:
                out.append(zero)

        for t in range(nc):                                                            # phase 1: pw row tiles over the natural k-steps
            for k in range(ks):
                emit(w1, 32 * t, 16 * k + natural)
            pad()
        for th in range(nh):                                                           # phase 2: per 32 hidden rows
            for k in range(ks):                                                        # ffn2.0 over x4 (k-step = (tile k / 2, half k % 2))
                emit(w2, 32 * th, 32 * (k // 2) + 16 * (k % 2) + acc_order)
            for s_ in range(2):                                                        # ffn2.2's two k-steps from this hidden tile
                for m in range(nm):
                    emit(w3, 32 * m, 32 * th + 16 * s_ + acc_order)
            pad()
        st = torch.cat(out).contiguous()
        assert st.numel() == total * 512, (st.numel() // 512, self.C, self.H, self.M2, pm)
        return st


def sk_tail_ok(tail: Optional[PackedTail], X: Planes, Y: Planes, cx: Optional["Ctx"] = None) -> bool:
    """Does sf_sk_tail run this block's back half?  fp16-activation arithmetic, x3 as fp16 ROWS, one product count for the three
    layers, a built shape, k-octet and / or fp32 outputs.  Any pixel count: the kernel guards every lane (the C ABI takes any N > 0,
    tests/test_gpu_chain_descriptors.py part B), so P % 4 is no condition here -- the engine's fp16 hand-over, which produces X, has
    its own (engine.hidden_f16_ok)."""
    cx = _cx(cx)
    if tail is None or not cx.sk_tail or cx.precision not in (PRECISION_F16X2, PRECISION_F16) or not (cx.hidden_f16 and cx.hidden_koct):
        return False
    if not (X.f16 and not X.koct and X.group == 0 and Y.group == 0 and X.rows == tail.C and Y.rows == tail.M2):
        return False
    if Y.f16 and not Y.koct:
        return False
    return tail.built(tail.products(cx))


@on_tensor_device
def sk_tail(tail: PackedTail, X: Planes, Y: Planes, gelu_out: bool = False, cx: Optional["Ctx"] = None) -> None:
    """Y = ffn2(gelu(x3 + pw(x3))) [gelu'ed with gelu_out] (update.py:35-36): X = x3 as fp16 rows; Y fp16 k-octet planes, or fp32 planes
    (+ their k-octet copy Y.shadow)."""
    cx = _cx(cx)
    assert sk_tail_ok(tail, X, Y, cx) and Y.n_img == X.n_img and Y.P == X.P
    pm = tail.products(cx)
    st = tail.stream(pm)
    A1, A2, A3 = tail.layers
    g = _lib.SfSkTail()
    g.X, g.strideX, g.ldx = X.ptr, X.img_stride, X.P
    g.wstream, g.wstream_bytes = st.data_ptr(), st.numel() * 2
    g.bias1, g.bias2, g.bias3 = _bias_ptr(A1), _bias_ptr(A2), _bias_ptr(A3)
    g.alpha1, g.alpha2, g.alpha3 = 1.0 / A1.split_scale, 1.0 / A2.split_scale, 1.0 / A3.split_scale
    g.N, g.batch, g.C, g.H, g.M2, g.pm, g.gelu_out = X.P, X.n_img, tail.C, tail.H, tail.M2, pm, int(bool(gelu_out))
    out_bytes = 2.0
    if Y.f16:
        g.Y16, g.strideY16, g.ldy16 = Y.ptr, Y.img_stride, Y.P
    else:
        g.Y, g.strideY, g.ldy = Y.ptr, Y.img_stride, Y.P
        out_bytes = 4.0
        if Y.shadow is not None and cx.shadows:
            sh = Y.shadow
            g.Y16, g.strideY16, g.ldy16 = sh.ptr, sh.img_stride, sh.P
            g.y16_partial = 1 if tail.M2 % 8 else 0
            out_bytes = 6.0
    n, P = X.n_img, X.P
    macs = tail.C * tail.C + tail.C * tail.H + tail.H * tail.M2
    name = "sk_tail" if not PROFILE_SHAPES else f"sk_tail C{tail.C} H{tail.H} M{tail.M2} b{n}"
    _launch(name, 2.0 * n * P * macs, n * P * (2.0 * tail.C + out_bytes * tail.M2) + 2.0 * macs * pm,
            lambda: _lib.check(_lib.load().sf_sk_tail(C.byref(g), _lib.stream()), "sf_sk_tail"), products=float(pm))
    if g.Y and not g.Y16:
        refresh_shadow(Y, cx)


class PackedTemporal(_PackedStream):
    """The four contractions of the temporal transformer block (update.py:459-484 -> timm Block: qkv, proj, fc1, fc2) as ONE weight
    stream for sf_temporal_block (csrc/temporal.hip): 1-KB MFMA fragments in consumption order (layout: include/streamflow_hip.h).
    The PackedLinear objects stay the source of truth (rounding, power-of-two scales, biases, `single` flags)."""

    def __init__(self, qkv: "PackedLinear", proj: "PackedLinear", fc1: "PackedLinear", fc2: "PackedLinear"):
        super().__init__()
        self.layers = (qkv, proj, fc1, fc2)
        self.C, self.H = qkv.K, fc1.M

    def built(self) -> bool:
        qkv, proj, fc1, fc2 = self.layers
        return (self.C == 128 and self.H == 256 and qkv.M == 384 and qkv.bias is None and (proj.M, proj.K) == (128, 128) and
                fc1.K == 128 and (fc2.M, fc2.K) == (128, 256) and not any(l.conv3x3 for l in self.layers))

    def products(self, cx: "Ctx") -> Optional[int]:
        return _shared_products(self.layers, cx)

    def prebuild(self, cx: "Ctx") -> None:
        pm = self.products(cx)
        if self.built() and pm is not None:
            self.stream(pm)

    def stream(self, pm: int) -> torch.Tensor:
        return self._cached(pm, lambda: self._pack(pm))

    def _pack(self, pm: int) -> torch.Tensor:
        qkv, proj, fc1, fc2 = (self._split(l, l.M, l.K) for l in self.layers)       # (hi, lo) of scale * W, [M, K] fp16
        dev = qkv[0].device
        kq = torch.arange(4, device=dev).view(4, 1)
        i = torch.arange(8, device=dev).view(1, 8)
        perm = torch.where(i < 4, 4 * kq + i, 16 + 4 * kq + i - 4).reshape(-1)             # input row of column (kq, i) of a k-step
        out = []

        def emit(w, m, s, permuted):
            for plane in ((w[1], w[0]) if pm == 2 else (w[0],)):                           # lo before hi
                blk = plane[16 * m:16 * m + 16, 32 * s:32 * s + 32]
                if permuted:
                    blk = blk[:, perm]
                out.append(blk.reshape(16, 4, 8).permute(1, 0, 2).reshape(512))           # lane (kq, row): 8 halves

        for m in range(16):                                                                # q and k rows
            for s in range(4):
                emit(qkv, m, s, False)
        for p_ in range(4):                                                                # v two tiles at a time, then proj's k-step
            for tile in (16 + 2 * p_, 16 + 2 * p_ + 1):
                for s in range(4):
                    emit(qkv, tile, s, False)
            for m in range(8):
                emit(proj, m, p_, True)
        for h in range(8):                                                                 # fc1 two tiles at a time, then fc2's k-step
            for tile in (2 * h, 2 * h + 1):
                for s in range(4):
                    emit(fc1, tile, s, True)
            for m in range(8):
                emit(fc2, m, h, True)
        st = torch.cat(out).contiguous()
        assert st.numel() == int(_lib.load().sf_temporal_block_frags(pm)) * 512
        return st


class PackedMask(_PackedStream):
    """mask.2 (update.py:758: Conv1x1 256 -> 576) as the weight stream of sf_mask_upsample (csrc/mask_upsample.hip): row tile 0 .. 35,
    k-step 0 .. 7, `lo` before `hi`."""

    def __init__(self, layer: "PackedLinear"):
        super().__init__()
        self.layer = layer

    def built(self) -> bool:
        return (self.layer.M, self.layer.K) == (576, 256) and not self.layer.conv3x3

    def products(self, cx: "Ctx") -> int:
        return 1 if (cx.precision == PRECISION_F16 or self.layer.single) else 2

    def prebuild(self, cx: "Ctx") -> None:
        if self.built():
            self.stream(self.products(cx))

    def stream(self, pm: int) -> torch.Tensor:
        return self._cached(pm, lambda: self._pack(pm))

    def _pack(self, pm: int) -> torch.Tensor:
        hi, lo = self._split(self.layer, 576, 256)
        planes = [lo, hi] if pm == 2 else [hi]
        f = torch.stack([w.view(36, 16, 8, 4, 8) for w in planes], dim=0)                   # [plane, tile, row, s, kq, i]
        st = f.permute(1, 3, 0, 4, 2, 5).reshape(-1).contiguous()                           # [tile][s][plane][(kq, row), i]
        assert st.numel() == int(_lib.load().sf_mask_upsample_frags(pm)) * 512
        return st


def mask_upsample_ok(pack: Optional[PackedMask], M256: Planes, cx: Optional["Ctx"] = None) -> bool:
    cx = _cx(cx)
    return (pack is not None and pack.built() and cx.precision in (PRECISION_F16X2, PRECISION_F16) and cx.shadows and
            M256.shadow is not None and M256.rows == 256 and M256.group == 0)


@on_tensor_device
def mask_upsample(pack: PackedMask, M256: Planes, flow: torch.Tensor, out: torch.Tensor, h: int, w: int,
                  cx: Optional["Ctx"] = None) -> None:
    """out [n, 2, 8h, 8w] = convex upsampling of flow [n, 2, h, w] with mask = 0.25 * mask.2(M256) (streamflow.py:82-93), the mask
    never written: M256 = relu(mask.0(net)) as planes with a k-octet copy (the operand)."""
    cx = _cx(cx)
    assert mask_upsample_ok(pack, M256, cx) and M256.P == h * w and flow.is_contiguous() and out.is_contiguous()
    sh, A = M256.shadow, pack.layer
    pm = pack.products(cx)
    st = pack.stream(pm)
    g = _lib.SfMaskUpsample()
    g.X16, g.strideX, g.ldx = sh.ptr, sh.img_stride, sh.P
    g.wstream, g.wstream_bytes = st.data_ptr(), st.numel() * 2
    g.bias = _bias_ptr(A)
    g.flow, g.out = flow.data_ptr(), out.data_ptr()
    g.n_img, g.h, g.w, g.K, g.M, g.pm = M256.n_img, h, w, 256, 576, pm
    g.alpha = 0.25 / A.split_scale
    n, P = M256.n_img, h * w
    _launch("mask_upsample", 2.0 * 576 * 256 * n * P, (2.0 * 256 + 4.0 * 2 + 4.0 * 128) * n * P,
            lambda: _lib.check(_lib.load().sf_mask_upsample(C.byref(g), _lib.stream()), "sf_mask_upsample"), products=float(pm))


def temporal_block_ok(pack: Optional[PackedTemporal], X: Planes, TT: int, cx: Optional["Ctx"] = None) -> bool:
    """Does sf_temporal_block run this block?  fp16-activation arithmetic with the k-octet copy of the tokens at hand, the built
    shape (C = 128, hidden 256, <= 3 tokens per pixel), one product count for all four layers."""
    cx = _cx(cx)
    if pack is None or cx.precision not in (PRECISION_F16X2, PRECISION_F16) or not (cx.shadows and cx.hidden_f16 and cx.hidden_koct):
        return False
    return (pack.built() and pack.products(cx) is not None and 1 <= TT <= 3 and X.shadow is not None and X.rows == 128 and
            X.group == 0 and X.n_img % TT == 0)


@on_tensor_device
def temporal_block(pack: PackedTemporal, X: Planes, Y: Planes, TT: int, ln1, ln2, eps: float = 1e-5, cx: Optional["Ctx"] = None) -> None:
    """Y = Block(X) over the TT tokens of every pixel (update.py:481-484): X fp32 planes with a k-octet copy (the operand), image =
    clip * TT + frame; Y fp32 planes (+ their k-octet copy Y.shadow).  ln1 / ln2 = (weight, bias) of the two LayerNorms."""
    cx = _cx(cx)
    assert temporal_block_ok(pack, X, TT, cx)
    sh = X.shadow
    assert sh.f16 and sh.koct and not Y.f16 and Y.rows == 128 and Y.n_img == X.n_img and Y.P == X.P and Y.group == 0
    pm = pack.products(cx)
    st = pack.stream(pm)
    qkv, proj, fc1, fc2 = pack.layers
    g = _lib.SfTemporalBlock()
    g.X16, g.strideX, g.ldx = sh.ptr, sh.img_stride, sh.P
    g.wstream, g.wstream_bytes = st.data_ptr(), st.numel() * 2
    g.ln1_w, g.ln1_b, g.ln2_w, g.ln2_b = ln1[0].data_ptr(), ln1[1].data_ptr(), ln2[0].data_ptr(), ln2[1].data_ptr()
    g.bias_proj, g.bias_fc1, g.bias_fc2 = _bias_ptr(proj), _bias_ptr(fc1), _bias_ptr(fc2)
    g.Y, g.strideY, g.ldy = Y.ptr, Y.img_stride, Y.P
    nbytes = 2.0 + 4.0
    if Y.shadow is not None and cx.shadows:
        g.Y16, g.strideY16, g.ldy16 = Y.shadow.ptr, Y.shadow.img_stride, Y.shadow.P
        nbytes += 2.0
    g.N, g.B, g.TT, g.C, g.H, g.pm = X.P, X.n_img // TT, TT, 128, 256, pm
    g.alpha_qkv, g.alpha_proj, g.alpha_fc1, g.alpha_fc2 = (1.0 / l.split_scale for l in pack.layers)
    g.ss_proj, g.ss_fc2, g.eps, g.scale = proj.split_scale, fc2.split_scale, eps, 128 ** -0.5
    n, P = X.n_img, X.P
    flops = 2.0 * n * P * (384 * 128 + 128 * 128 + 256 * 128 + 128 * 256) + 4.0 * n * P * TT * 128
    _launch("temporal_block", flops, nbytes * n * 128 * P,
            lambda: _lib.check(_lib.load().sf_temporal_block(C.byref(g), _lib.stream()), "sf_temporal_block"), products=float(pm))


# (K1, M2) of the shapes csrc/ffn_pair.hip is built for, by mode (0: an ffn2 pair, 1: an ffn1 pair)
PAIR_SHAPES = {1: {(128, 128), (256, 256), (324, 324), (384, 384)},
               0: {(128, 64), (256, 192), (256, 126), (324, 256), (384, 6), (256, 4), (128, 2)}}


def ffn_pair_ok(pair: Optional[PackedPair], X: Planes, mode: int, cx: Optional["Ctx"] = None) -> bool:
    """Does sf_ffn_pair run this FFN?  fp16-activation arithmetic with k-octet hand-over, a k-octet operand (the planes themselves
    or their copy; grouped '(B T) C -> B (T C)' views in groups of a multiple of 32 rows), one of the built shapes.  Any pixel count
    (sf_ffn_pair takes any N > 0: tests/test_gpu_chain_descriptors.py part B)."""
    cx = _cx(cx)
    if pair is None or cx.precision not in (PRECISION_F16X2, PRECISION_F16) or not (cx.shadows and cx.hidden_f16 and cx.hidden_koct):
        return False
    src = X if (X.f16 and X.koct) else X.shadow
    if src is None or (src.group and (src.group % 32 or pair.K1 % src.group)):
        return False
    pm = pair.products(cx)
    return (pair.K1, pair.M2) in PAIR_SHAPES[mode] and pm in ((1, 1), (2, 1), (2, 2))


@on_tensor_device
def ffn_pair(pair: PackedPair, X: Planes, Y: Planes, mode: int, dw_w: Optional[torch.Tensor] = None,
             dw_b: Optional[torch.Tensor] = None, gelu_out: bool = False, cx: Optional["Ctx"] = None) -> None:
    """mode 0: Y = ffn(X) [gelu'ed with gelu_out]: Y fp16 k-octet planes, or fp32 planes (+ their k-octet copy Y.shadow).
    mode 1: Y (fp16 ROWS) = gelu(x1 + dw_w * x1 + dw_b), x1 = gelu(X + ffn(X))  (update.py:31-32).  X: k-octet planes or planes
    with a k-octet copy."""
    cx = _cx(cx)
    assert ffn_pair_ok(pair, X, mode, cx)
    src = X if (X.f16 and X.koct) else X.shadow
    pm1, pm2 = pair.products(cx)
    st = pair.stream(pm1, pm2)
    g = _lib.SfFfnPair()
    g.X, g.strideX, g.ldx = src.ptr, src.img_stride, src.P
    g.x_group, g.x_group_stride = src.group, src.group_stride
    g.wstream, g.wstream_bytes = st.data_ptr(), st.numel() * 2
    A1, A2 = pair.first, pair.second
    g.bias1, g.bias2 = _bias_ptr(A1), _bias_ptr(A2)
    g.alpha1, g.alpha2 = 1.0 / A1.split_scale, 1.0 / A2.split_scale
    g.N, g.batch, g.K1, g.H, g.M2 = X.P, X.n_img, pair.K1, pair.H, pair.M2
    g.pm1, g.pm2, g.mode, g.gelu_out = pm1, pm2, int(mode), int(bool(gelu_out))
    assert Y.n_img == X.n_img and Y.P == X.P and Y.rows == pair.M2 and Y.group == 0
    out_bytes = 2.0
    if mode == 1:
        assert Y.f16 and not Y.koct and dw_w is not None and dw_b is not None
        g.dw_w, g.dw_b = dw_w.data_ptr(), dw_b.data_ptr()
        if not X.f16:                                 # fp32 planes with a k-octet copy: the residual stays the fp32 value
            assert X.group == src.group
            g.R32, g.strideR32, g.ldr32, g.r32_group_stride = X.ptr, X.img_stride, X.P, X.group_stride
        g.C16, g.strideC16, g.ldc16 = Y.ptr, Y.img_stride, Y.P
    elif Y.f16:
        assert Y.koct
        g.C16, g.strideC16, g.ldc16 = Y.ptr, Y.img_stride, Y.P
    else:
        g.C, g.strideC, g.ldc = Y.ptr, Y.img_stride, Y.P
        out_bytes = 4.0
        if Y.shadow is not None and cx.shadows:
            sh = Y.shadow
            g.C16, g.strideC16, g.ldc16 = sh.ptr, sh.img_stride, sh.P
            g.c16_partial = 1 if pair.M2 % 8 else 0
            out_bytes = 6.0
    n, P = X.n_img, X.P
    flops = 2.0 * n * P * (pair.K1 * pair.H + pair.H * pair.M2)
    mf = 2.0 * n * P * (pair.K1 * pair.H * pm1 + pair.H * pair.M2 * pm2)
    nbytes = n * P * (2.0 * pair.K1 * (2 if mode == 1 else 1) + out_bytes * pair.M2) + 2.0 * (pair.K1 * pair.H * pm1 + pair.H * pair.M2 * pm2)
    name = "ffn_pair" if not PROFILE_SHAPES else f"ffn_pair K{pair.K1} H{pair.H} M{pair.M2} b{n} m{mode}"
    _launch(name, flops, nbytes, lambda: _lib.check(_lib.load().sf_ffn_pair(C.byref(g), _lib.stream()), "sf_ffn_pair"),
            products=mf / flops)
    if g.C and not g.C16:
        refresh_shadow(Y, cx)


def new_shadow(X: Planes, device) -> Planes:
    """Allocate the k-octet copy of fp32 planes X (zeroed: rows past X.rows in the last octet must stay finite)."""
    assert not X.f16 and X.group == 0
    noct = (X.rows + 7) // 8
    base = torch.zeros(X.n_img * noct * X.P * 4, dtype=torch.float32, device=device)       # 8 halves = 4 floats
    return Planes(base, 0, noct * X.P * 8, X.n_img, X.rows, X.P, f16=True, koct=True)


@on_tensor_device
def pack_koct(X: Planes, Y: Planes) -> None:
    """fp32 planes -> their k-octet fp16 copy (sf_pack_koct)."""
    assert Y.f16 and Y.koct and not X.f16 and X.group == 0 and (X.rows, X.P, X.n_img) == (Y.rows, Y.P, Y.n_img)
    _launch("pack_koct", 0, 6.0 * X.n_img * X.rows * X.P,
            lambda: _lib.check(_lib.load().sf_pack_koct(X.ptr, X.img_stride, X.n_img, X.rows, X.P, Y.ptr, Y.img_stride,
                                                        _lib.stream()), "sf_pack_koct"))


def clock_probe(out: torch.Tensor, spin_us: int) -> None:
    """Enqueue sf_clock_probe on the CURRENT stream: out (int64[2], device) <- (shader cycles, 100 MHz ticks) over spin_us."""
    assert out.is_cuda and out.dtype == torch.int64 and out.numel() >= 2 and out.is_contiguous()
    _lib.check(_lib.load().sf_clock_probe(out.data_ptr(), int(spin_us), _lib.stream()), "sf_clock_probe")


def refresh_shadow(X: Planes, cx: Optional[Ctx] = None) -> None:
    """After a producer without a fused k-octet output wrote X: bring X.shadow up to date."""
    if X.shadow is not None and _cx(cx).shadows:
        pack_koct(replace(X, shadow=None), X.shadow)


def uses_dma_tile(M: int) -> bool:
    """Does sf_gemm run an M-row problem on the 128-row, DMA-fed tile (gemm_split.hip pick_tile)?  Of the tiled kernels only
    that one takes a k-octet fp16 B operand."""
    return (M + 127) // 128 * 128 * 4 <= M * 5


def takes_koct(M: int, K: int) -> bool:
    """Can sf_gemm read the B operand of an M x K layer as fp16 k-octet planes?  The activation-stationary kernel does for
    64 < K <= 640 at every M (gemm_bstat.hip), the tiled family on its 128-row tile."""
    return 64 < K <= 640 or uses_dma_tile(M)


def gemm(A: PackedLinear, X: Planes, Y: Planes, epilogue: int = EPI_NONE, R: Optional[Planes] = None,
         dw_w: Optional[torch.Tensor] = None, dw_b: Optional[torch.Tensor] = None, alpha: float = 1.0,
         hw: Optional[Sequence[int]] = None, algo: int = 0, cx: Optional[Ctx] = None) -> None:
    """Y[img] = epilogue(alpha * (W @ X[img] + bias)) for every image (batched over grid.z).
    algo: _lib.ALGO_AUTO / ALGO_TILED / ALGO_BSTAT (SfGemm.algo: force one kernel family; tests and A/B timing).
    cx: launch context (arithmetic mode, split-K scratch, hand-over switches); None = Ctx(ops.PRECISION)."""
    cx = _cx(cx)
    PRECISION, SHADOWS, SPLIT_WS = cx.precision, cx.shadows, cx.split_ws
    assert X.rows * (9 if A.conv3x3 else 1) == A.K, (X.rows, A.K)
    assert Y.rows == A.M and X.n_img == Y.n_img and X.P == Y.P, (Y.rows, A.M)
    if (X.shadow is not None and SHADOWS and PRECISION in (PRECISION_F16X2, PRECISION_F16) and not A.conv3x3 and
            takes_koct(A.M, A.K)):
        X = X.shadow                                  # the fp16 k-octet copy: both operands by LDS-DMA
    if DEBUG_RANGE and PRECISION != PRECISION_FP32:
        _check_range(X, f"sf_gemm M{A.M} K{A.K}")
    g = SfGemm()
    g.A, g.B, g.C = A.wt.data_ptr(), X.ptr, Y.ptr
    g.bias = None if A.bias is None else A.bias.data_ptr()
    g.M, g.N, g.K, g.batch = A.M, X.P, A.K, X.n_img
    g.lda, g.ldb, g.ldc = A.lda, X.P, Y.P
    g.strideA, g.strideB, g.strideC = 0, X.img_stride, Y.img_stride
    g.a_layout, g.b_layout = LAYOUT_K_MAJOR, LAYOUT_K_MAJOR
    g.a_padded = 1
    prec = PRECISION
    if A.single and prec == PRECISION_F16X2:
        prec = PRECISION_F16                          # per-layer single-product weights (same operand formats)
    if X.f16 or Y.f16:
        if prec not in (PRECISION_F16X2, PRECISION_F16):
            raise RuntimeError("fp16 activation planes are a hand-over format of the f16x2 / f16 modes only")
        if X.f16:
            g.b_layout = _lib.LAYOUT_F16_KOCT if X.koct else _lib.LAYOUT_F16_K_MAJOR
        if Y.f16:
            g.c_f16 = 2 if Y.koct else 1
    fused_shadow = False
    if (Y.shadow is not None and SHADOWS and not Y.f16 and prec in (PRECISION_F16X2, PRECISION_F16) and Y.P % 4 == 0
            and cx.shadow_fused):
        g.c_f16, g.C16, g.strideC16 = 3, Y.shadow.ptr, Y.shadow.img_stride       # fp32 planes + their k-octet copy
        fused_shadow = True
    if prec != PRECISION_FP32:
        g.a_layout = LAYOUT_SPLIT_F16
        g.A_hi, g.A_lo, g.lda_h, g.a_k_pad = A.hi.data_ptr(), A.lo.data_ptr(), A.lda_h, A.k_pad
        # the split image holds split_scale * W: C = alpha/s * (s W X + s b)
        alpha = alpha / A.split_scale
        g.bias = _bias_ptr(A)
    g.b_group, g.b_group_stride = X.group, X.group_stride
    if R is not None:
        assert R.rows == A.M and R.n_img == Y.n_img
        g.R, g.ldr, g.strideR = R.ptr, R.P, R.img_stride
        g.r_group, g.r_group_stride = R.group, R.group_stride
        if R.f16:                                     # the block input exists only as fp16 k-octets (correlation features)
            assert R.koct and R.group == 0
            g.r_f16 = 2
    if dw_w is not None:
        g.dw_w, g.dw_b = dw_w.data_ptr(), dw_b.data_ptr()
    if A.conv3x3:
        g.conv3x3, g.h, g.w = 1, int(hw[0]), int(hw[1])
    g.alpha, g.epilogue, g.precision, g.algo = float(alpha), int(epilogue), prec, int(algo)
    if SPLIT_WS is not None and prec != PRECISION_FP32:
        g.split_ws, g.split_ws_floats = SPLIT_WS.data_ptr(), SPLIT_WS.numel()
    name = "gemm" if not PROFILE_SHAPES else f"gemm M{g.M} K{g.K} b{g.batch} e{g.epilogue}"
    # algorithmic bytes: activations in (each input row once) + result out (+ residual in) per image, weights once
    nbytes = (g.batch * g.N * ((2.0 if X.f16 else 4.0) * X.rows + (2.0 if Y.f16 else 6.0 if fused_shadow else 4.0) * g.M +
                               ((2.0 if R.f16 else 4.0) * g.M if R is not None else 0.0)) + 4.0 * g.M * g.K)
    _launch(name, 2.0 * g.M * g.N * g.K * g.batch, nbytes,
            lambda: _lib.check(_lib.load().sf_gemm(C.byref(g), _lib.stream()), "sf_gemm"), products=_products(prec))
    if not fused_shadow:
        refresh_shadow(Y, cx)


def gemm_split_ws_floats(M: int, N: int, K: int, batch: int, cx: Optional[Ctx] = None) -> int:
    """floats of scratch with which sf_gemm would split K on its own for this shape (0: it would not); see Ctx.split_ws."""
    if _cx(cx).precision == PRECISION_FP32:
        return 0
    return int(_lib.load().sf_gemm_split_ws_floats(M, N, K, batch))


def gemm_raw(cx: Optional[Ctx] = None, **kw) -> None:
    """Fully explicit sf_gemm call (used for the attention logits and attn @ v contractions)."""
    PRECISION = _cx(cx).precision
    g = SfGemm()
    g.alpha = 1.0
    for k, v in kw.items():
        setattr(g, k, v)
    g.precision = PRECISION
    name = "gemm_attn" if g.a_layout == LAYOUT_K_MINOR else "gemm"
    eb = 2.0 if g.b_layout == LAYOUT_F16_K_MINOR else 4.0
    nbytes = g.batch * (4.0 * g.M * g.K + eb * g.K * g.N + 4.0 * g.M * g.N * (2 if g.R else 1) *
                        (g.k_splits if g.k_splits > 1 else 1))
    _launch(name, 2.0 * g.M * g.N * g.K * g.batch, nbytes,
            lambda: _lib.check(_lib.load().sf_gemm(C.byref(g), _lib.stream()), "sf_gemm"), products=_products(PRECISION))


@on_tensor_device
def splitk_combine(partial: torch.Tensor, split_stride: int, k_splits: int, part_img_stride: int, R: Planes,
                   gamma: torch.Tensor, out: Planes) -> None:
    assert R.rows == out.rows and R.n_img == out.n_img
    _launch("splitk_combine", 0, 4.0 * (k_splits + 2) * R.n_img * R.rows * R.P,
            lambda: _lib.check(_lib.load().sf_splitk_combine(
                partial.data_ptr(), split_stride, k_splits, part_img_stride, R.ptr, R.img_stride, gamma.data_ptr(),
                out.ptr, out.img_stride, R.n_img, R.rows * R.P, _lib.stream()), "sf_splitk_combine"))


@on_tensor_device
def dwconv_res_gelu(X: Planes, wgt: torch.Tensor, bias: torch.Tensor, Y: Planes, h: int, w: int, k: int,
                    single: bool = False, cx: Optional[Ctx] = None) -> None:
    """Y = gelu(X + dwconv_KxK(X) + bias).  Y may be fp16 row planes (Planes.f16, not koct): the hand-over to a GEMM.
    X may be fp16 row planes too (f16x2 / f16 arithmetic, fp16 Y): sf_dwconv_res_gelu_f16in.
    single (f16x2 mode only): the weights enter the products as ONE fp16 value (a single-product layer)."""
    PRECISION = _cx(cx).precision
    assert X.rows == Y.rows == wgt.shape[0] and X.P == h * w and not X.koct and not Y.koct
    if DEBUG_RANGE and PRECISION != PRECISION_FP32:
        _check_range(X, f"sf_dwconv_res_gelu C{X.rows} k{k}")
    prec = PRECISION_F16 if (single and PRECISION == PRECISION_F16X2) else PRECISION
    if X.f16:
        assert Y.f16, "fp16 input needs fp16 output"
        call = lambda: _lib.check(_lib.load().sf_dwconv_res_gelu_f16in(X.ptr, X.img_stride, wgt.data_ptr(), bias.data_ptr(),
                                                                       Y.ptr, Y.img_stride, X.n_img, X.rows, h, w, k, prec,
                                                                       _lib.stream()), "sf_dwconv_res_gelu_f16in")
    else:
        call = lambda: _lib.check(_lib.load().sf_dwconv_res_gelu(X.ptr, X.img_stride, wgt.data_ptr(), bias.data_ptr(),
                                                                 Y.ptr, Y.img_stride, int(Y.f16), X.n_img, X.rows, h, w, k,
                                                                 prec, _lib.stream()), "sf_dwconv_res_gelu")
    _launch("dwconv%d" % k, 2.0 * k * k * X.n_img * X.rows * h * w,
            ((2.0 if X.f16 else 4.0) + (2.0 if Y.f16 else 4.0)) * X.n_img * X.rows * h * w, call,
            # matrix-core work: banded Toeplitz GEMMs (32 / 15 of the algorithmic flops) for K = 15 in the split modes, 2 or 3
            # products; the fp32 and 7 x 7 stencils run on the VALU
            products=((32.0 / 15.0) * _products(prec)) if (k == 15 and PRECISION != PRECISION_FP32) else 0.0)


@on_tensor_device
def layernorm_cm(X: Planes, gamma: torch.Tensor, beta: torch.Tensor, Y: Planes, eps: float = 1e-5) -> None:
    """Y fp32 planes, or fp16 k-octet planes (Planes.koct: the hand-over to a GEMM on the DMA-fed tile)."""
    assert not X.f16 and (not Y.f16 or Y.koct)
    ko = Y.f16
    _launch("layernorm", 0, (6.0 if ko else 8.0) * X.n_img * X.rows * X.P,
            lambda: _lib.check(_lib.load().sf_layernorm_cm(X.ptr, X.img_stride, gamma.data_ptr(), beta.data_ptr(),
                                                           None if ko else Y.ptr, 0 if ko else Y.img_stride,
                                                           Y.ptr if ko else None, Y.img_stride if ko else 0,
                                                           X.n_img, X.rows, X.P, eps, _lib.stream()), "sf_layernorm_cm"))


@on_tensor_device
def temporal_attn(QKV: Planes, OUT: Planes, B: int, TT: int, C_: int) -> None:
    assert QKV.img_stride == 3 * C_ * QKV.P and OUT.img_stride == C_ * OUT.P and QKV.n_img == B * TT
    assert (not OUT.f16 or OUT.koct) and not QKV.koct
    ko = OUT.f16                                          # fp16 k-octet planes: the hand-over to the proj GEMM
    fn = _lib.load().sf_temporal_attn_f16in if QKV.f16 else _lib.load().sf_temporal_attn     # (fp16 rows: the qkv GEMM's c_f16 = 1)
    _launch("temporal_attn", 0, ((6.0 if QKV.f16 else 12.0) + (2.0 if ko else 4.0)) * QKV.n_img * C_ * QKV.P,
            lambda: _lib.check(fn(QKV.ptr, None if ko else OUT.ptr, OUT.ptr if ko else None,
                                  B, TT, C_, QKV.P, _lib.stream()), "sf_temporal_attn"))


@on_tensor_device
def softmax_rows(x: torch.Tensor, rows: int, cols: int, out16: Optional[torch.Tensor] = None) -> None:
    """In place, or (out16: fp16 [rows][cols]) written as half precision with x left as scratch."""
    assert out16 is None or (out16.dtype == torch.float16 and out16.numel() >= rows * cols)
    _launch("softmax_rows", 0, (8.0 if out16 is None else 6.0) * rows * cols,
            lambda: _lib.check(_lib.load().sf_softmax_rows(x.data_ptr(), rows, cols,
                                                           out16.data_ptr() if out16 is not None else None,
                                                           _lib.stream()), "sf_softmax_rows"))


@on_tensor_device
def window_attn(QKV: Planes, qkv_bias: torch.Tensor, OUT: Planes, heads: int, H: int, W: int, ws: int = 7,
                cx: Optional[Ctx] = None, exact: bool = False) -> None:
    """timm LocallyGroupedAttn core on token planes (encoder; see include/streamflow_hip.h).  PRECISION_FP32: the exact
    VALU kernel; every other class: the matrix-core kernel (3 products per contraction for F16X3, 1 for the fp16 classes)."""
    PRECISION = _cx(cx).precision
    C = OUT.rows
    assert QKV.rows == 3 * C and QKV.P == H * W == OUT.P and qkv_bias.numel() == 3 * C and (not OUT.f16 or OUT.koct)
    assert not QKV.f16 or (QKV.koct and PRECISION in (PRECISION_F16X2, PRECISION_F16))
    flops, nbytes = 4.0 * QKV.n_img * H * W * ws * ws * C, (2.0 if QKV.f16 else 4.0) * QKV.n_img * 3 * C * H * W + 4.0 * QKV.n_img * C * H * W
    if PRECISION == PRECISION_FP32 or exact:
        assert not OUT.f16 and not QKV.f16
        _launch("window_attn", flops, nbytes,
                lambda: _lib.check(_lib.load().sf_window_attn(QKV.ptr, QKV.img_stride, qkv_bias.data_ptr(), OUT.ptr, OUT.img_stride,
                                                              QKV.n_img, C, heads, H, W, ws, _lib.stream()), "sf_window_attn"))
        return
    prec = PRECISION
    ko = OUT.f16                                          # fp16 k-octet planes: the hand-over to the proj GEMM
    _launch("window_attn_mfma", flops, nbytes - (2.0 * QKV.n_img * C * H * W if ko else 0.0),
            lambda: _lib.check(_lib.load().sf_window_attn_mfma(QKV.ptr, QKV.img_stride, int(QKV.f16), qkv_bias.data_ptr(),
                                                               None if ko else OUT.ptr, 0 if ko else OUT.img_stride,
                                                               OUT.ptr if ko else None, OUT.img_stride if ko else 0,
                                                               QKV.n_img, C, heads, H, W, ws, prec, _lib.stream()),
                               "sf_window_attn_mfma"),
            products=3 if prec == PRECISION_F16X3 else 1)


@on_tensor_device
def subsample_attn(Q: Planes, KV: Planes, OUT: Planes, heads: int, ws: Optional[torch.Tensor] = None,
                   cx: Optional[Ctx] = None, exact: bool = False) -> None:
    """timm GlobalSubSampleAttn core: OUT = softmax(q k^T / sqrt(32)) v, keys/values = the M sub-sampled tokens.
    PRECISION_FP32: the exact VALU kernel; every other class: the matrix-core kernel (3 products per contraction for
    F16X3, 1 for the fp16 classes) over `ws` (uint8, >= subsample_attn_ws_bytes; allocated here when not given)."""
    PRECISION = _cx(cx).precision
    C = Q.rows
    assert KV.rows == 2 * C and OUT.rows == C and Q.P == OUT.P and Q.n_img == KV.n_img == OUT.n_img and (not OUT.f16 or OUT.koct)
    nbytes = 4.0 * Q.n_img * C * (2 * Q.P + 2 * KV.P)
    if PRECISION == PRECISION_FP32 or exact:
        assert not OUT.f16
        _launch("subsample_attn", 4.0 * Q.n_img * Q.P * KV.P * C, nbytes,
                lambda: _lib.check(_lib.load().sf_subsample_attn(Q.ptr, Q.img_stride, KV.ptr, KV.img_stride, OUT.ptr, OUT.img_stride,
                                                                 Q.n_img, C, heads, Q.P, KV.P, _lib.stream()), "sf_subsample_attn"))
        return
    need = subsample_attn_ws_bytes(Q.n_img, heads, KV.P)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=Q.base.device)
    assert ws.dtype == torch.uint8 and ws.numel() >= need and ws.device == Q.base.device
    prec = PRECISION
    ko = OUT.f16
    _launch("subsample_attn_mfma", 4.0 * Q.n_img * Q.P * KV.P * C, nbytes - (2.0 * Q.n_img * C * Q.P if ko else 0.0),
            lambda: _lib.check(_lib.load().sf_subsample_attn_mfma(Q.ptr, Q.img_stride, KV.ptr, KV.img_stride,
                                                                  None if ko else OUT.ptr, 0 if ko else OUT.img_stride,
                                                                  OUT.ptr if ko else None, OUT.img_stride if ko else 0,
                                                                  Q.n_img, C, heads, Q.P, KV.P, ws.data_ptr(), ws.numel(), prec,
                                                                  _lib.stream()), "sf_subsample_attn_mfma"),
            products=3 if prec == PRECISION_F16X3 else 1)


def subsample_attn_ws_bytes(n_img: int, heads: int, M: int) -> int:
    return int(_lib.load().sf_subsample_attn_ws_bytes(n_img, heads, M))


@on_tensor_device
def dwconv3x3_res(X: Planes, wgt: torch.Tensor, bias: torch.Tensor, Y: Planes, H: int, W: int) -> None:
    """timm PosConv: Y = X + depthwise3x3(X) + b on [n_img][C][H][W]."""
    assert X.rows == Y.rows == wgt.shape[0] and X.P == H * W
    _launch("dwconv3", 18.0 * X.n_img * X.rows * H * W, 8.0 * X.n_img * X.rows * H * W,
            lambda: _lib.check(_lib.load().sf_dwconv3x3_res(X.ptr, X.img_stride, wgt.data_ptr(), bias.data_ptr(), Y.ptr,
                                                            Y.img_stride, X.n_img, X.rows, H, W, _lib.stream()), "sf_dwconv3x3_res"))


def gma_flash_ws_bytes(n_img: int, P: int) -> int:
    return int(_lib.load().sf_gma_flash_ws_bytes(n_img, P))


def gma_flash_img_bytes(P: int) -> int:
    """Bytes of ONE image's section of the fused GMA workspace (the images lie back to back; the key-split partial buffers of a
    small launch follow the last image and are not part of it)."""
    big = 4096                                                        # (enough query tiles that no key split is planned)
    return (gma_flash_ws_bytes(big, P) - gma_flash_ws_bytes(big - 1, P))


def gma_no_key_split(n_img: int, P: int) -> bool:
    """The fused / stored GMA launch over n_img images runs WITHOUT its key-split form (whose partial buffers live behind the last
    image of the workspace): the condition for launching a sub-range of images out of a larger workspace."""
    return gma_flash_ws_bytes(n_img, P) == n_img * gma_flash_img_bytes(P)


@on_tensor_device
def gma_flash_pack_qk(QK: Planes, ws: torch.Tensor, scale: float, stats_qk_products: int = 0, cx: Optional[Ctx] = None) -> None:
    """QK [n_img][256][P] (to_qk output) -> packed fp16 operand images in ws (once per clip); stats_qk_products = 1 / 2 / 3
    also stores every query's softmax statistics for gma_flash_aggregate(..., use_stats=True) with the same product count."""
    assert QK.rows == 256 and ws.dtype == torch.uint8
    sq = int(stats_qk_products) if _cx(cx).flash_stats else 0
    _launch("flash_pack_qk", 2.0 * QK.n_img * QK.P * QK.P * 128 * (1 if sq else 0), 4.0 * QK.n_img * 256 * QK.P * 2,
            lambda: _lib.check(_lib.load().sf_gma_flash_pack_qk(QK.ptr, QK.img_stride, ws.data_ptr(), ws.numel(), QK.n_img,
                                                                QK.P, float(scale), sq, _lib.stream()), "sf_gma_flash_pack_qk"),
            products=(sq + 1) / 2.0 if sq else 1.0)


def gma_flash_project_ok(A: "PackedLinear", X: Planes, cx: Optional[Ctx] = None) -> bool:
    """Can to_v + the v pack run as ONE launch (sf_gma_flash_project_v)?  fp16-activation arithmetic, a 128 x 128 weight, and the
    k-octet copy of the motion features at hand."""
    cx = _cx(cx)
    return (cx.precision in (PRECISION_F16X2, PRECISION_F16) and cx.shadows and A.M == 128 and A.K == 128 and A.bias is None and
            X.shadow is not None and X.rows == 128)


@on_tensor_device
def gma_flash_project_v(ws: torch.Tensor, A: "PackedLinear", X: Planes, cx: Optional[Ctx] = None) -> None:
    """v = to_v(X) (gma.py:93) written straight into the packed v planes of the fused kernel's workspace; X.shadow (the k-octet
    fp16 copy) is the operand.  The following gma_flash_aggregate call passes V=None."""
    cx = _cx(cx)
    sh = X.shadow
    assert gma_flash_project_ok(A, X, cx) and sh.f16 and sh.koct
    products = 1 if (cx.precision == PRECISION_F16 or A.single) else 2
    n, P = X.n_img, X.P
    _launch("gma_project_v", 2.0 * 128 * 128 * n * P, 4.0 * n * 128 * P,
            lambda: _lib.check(_lib.load().sf_gma_flash_project_v(
                ws.data_ptr(), ws.numel(), sh.ptr, sh.img_stride, sh.P, A.hi.data_ptr(), A.lo.data_ptr(), A.lda_h,
                1.0 / A.split_scale, products, n, P, _lib.stream()), "sf_gma_flash_project_v"), products=float(products))


@on_tensor_device
def gma_flash_aggregate(ws: torch.Tensor, V: Optional[Planes], MF: Planes, gamma: torch.Tensor, OUT: Planes, qk_products: int = 3,
                        use_stats: bool = False, cx: Optional[Ctx] = None) -> None:
    """OUT = MF + gamma * softmax(scale q k^T) V, fused (no N x N tensor); q, k come packed in ws.  use_stats: the softmax
    statistics stored by gma_flash_pack_qk(..., stats_qk_products=qk_products) are used instead of an online softmax.
    V=None: the v planes of ws were written by gma_flash_project_v."""
    cx = _cx(cx)
    use_stats = bool(use_stats) and cx.flash_stats
    if V is None:
        V = Planes(MF.base, 0, 0, MF.n_img, 128, MF.P, f16=True)             # placeholder: pointer 0 is passed below
    assert V.rows == MF.rows == OUT.rows == 128 and V.n_img == MF.n_img == OUT.n_img and not V.koct
    n, P = V.n_img, V.P
    fn = _lib.load().sf_gma_flash_aggregate_f16v if V.f16 else _lib.load().sf_gma_flash_aggregate     # (v as fp16 rows)
    # algorithmic: the two contractions; bytes: v, mf in, out (q/k/v tiles are re-read from L2 by every query tile)
    sh = OUT.shadow if (OUT.shadow is not None and cx.shadows and cx.shadow_fused) else None
    _launch("gma_flash", 4.0 * n * P * P * 128,
            (2.0 if V.f16 else 4.0) * n * 128 * P + 4.0 * n * 128 * P * 2 + 2.0 * n * 128 * P * (2 if sh is None else 3),
            lambda: _lib.check(fn(
                ws.data_ptr(), ws.numel(), (V.ptr if V.img_stride else None), V.img_stride, MF.ptr, MF.img_stride, gamma.data_ptr(), OUT.ptr,
                OUT.img_stride, None if sh is None else sh.ptr, 0 if sh is None else sh.img_stride, n, P,
                int(qk_products), int(use_stats), _lib.stream()), "sf_gma_flash_aggregate"), products=(qk_products + 1) / 2.0)
    if sh is None:
        refresh_shadow(OUT, cx)


def gma_stored_p_bytes(n_img: int, P: int) -> int:
    return int(_lib.load().sf_gma_stored_p_bytes(n_img, P))


def gma_stored_image_ok(P: int) -> bool:
    """One image of P pixels is within what gma_flash_store_p / gma_stored_aggregate accept (under 4 GiB of stored weights)."""
    return bool(_lib.load().sf_gma_stored_image_ok(P))


@on_tensor_device
def gma_flash_store_p(ws: torch.Tensor, pbuf: torch.Tensor, n_img: int, P: int, qk_products: int, cx: Optional[Ctx] = None) -> None:
    """Once per clip, after gma_flash_pack_qk(stats_qk_products=qk_products): the softmax weights of every (query, key) as fp16 in
    the fragment order of the second contraction -> pbuf (gma.py:53-65: `attn`, kept for the refinement loop)."""
    assert ws.dtype == torch.uint8 and pbuf.dtype == torch.uint8
    _launch("gma_store_p", 2.0 * n_img * P * P * 128, 2.0 * n_img * P * P,
            lambda: _lib.check(_lib.load().sf_gma_flash_store_p(ws.data_ptr(), ws.numel(), pbuf.data_ptr(), pbuf.numel(), n_img, P,
                                                                int(qk_products), _lib.stream()), "sf_gma_flash_store_p"),
            products=(qk_products + 1) / 2.0)


@on_tensor_device
def gma_stored_aggregate(ws: torch.Tensor, pbuf: torch.Tensor, V: Optional[Planes], MF: Planes, gamma: torch.Tensor, OUT: Planes,
                         cx: Optional[Ctx] = None) -> None:
    """OUT = MF + gamma * attn V with the stored weights (gma.py:99-102), bit-identical to gma_flash_aggregate(use_stats=True) on the
    same workspace.  V=None: the v planes of ws were written by gma_flash_project_v."""
    cx = _cx(cx)
    if V is None:
        V = Planes(MF.base, 0, 0, MF.n_img, 128, MF.P, f16=True)             # placeholder: pointer 0 is passed below
    assert V.rows == MF.rows == OUT.rows == 128 and V.n_img == MF.n_img == OUT.n_img and not V.koct
    n, P = V.n_img, V.P
    sh = OUT.shadow if (OUT.shadow is not None and cx.shadows and cx.shadow_fused) else None
    # algorithmic: ONE contraction; bytes: the stored weights (once), v, mf in, out
    _launch("gma_stored", 2.0 * n * P * P * 128,
            2.0 * n * P * P + (2.0 if V.f16 else 4.0) * n * 128 * P + 4.0 * n * 128 * P * 2 + (2.0 * n * 128 * P if sh is not None else 0.0),
            lambda: _lib.check(_lib.load().sf_gma_stored_aggregate(
                ws.data_ptr(), ws.numel(), pbuf.data_ptr(), pbuf.numel(), (V.ptr if V.img_stride else None), int(V.f16), V.img_stride,
                MF.ptr, MF.img_stride, gamma.data_ptr(), OUT.ptr, OUT.img_stride, None if sh is None else sh.ptr,
                0 if sh is None else sh.img_stride, n, P, _lib.stream()), "sf_gma_stored_aggregate"), products=1.0)
    if sh is None:
        refresh_shadow(OUT, cx)


@on_tensor_device
def coords_grid(batch: int, ht: int, wd: int, device) -> torch.Tensor:
    out = torch.empty(batch, 2, ht, wd, dtype=torch.float32, device=device)
    _lib.ptr(out)
    _lib.check(_lib.load().sf_coords_grid(out.data_ptr(), batch, ht, wd, _lib.stream()), "sf_coords_grid")
    return out


@on_tensor_device
def context_split(cnets: torch.Tensor, nets: Planes, inps: Planes, hdim: int) -> None:
    """cnets [n_img, 2*hdim, P]-like contiguous tensor."""
    _dev_check(cnets)
    _lib.check(_lib.load().sf_context_split(cnets.data_ptr(), nets.ptr, nets.img_stride, inps.ptr, inps.img_stride,
                                            nets.n_img, hdim, nets.P, _lib.stream()), "sf_context_split")


@on_tensor_device
def flow_update(coords1: Planes, delta: Optional[Planes], flow_a: Optional[Planes], flow_b: Optional[Planes],
                n_img: int, h: int, w: int, koct: Optional[Planes] = None, koct_row: int = 0, cx: Optional[Ctx] = None) -> None:
    """koct / koct_row: k-octet planes (Planes.shadow of the tensor flow_b is a slice of) and the row the x component
    goes to: keeps that copy's flow rows current."""
    assert coords1.img_stride == 2 * h * w and (delta is None or delta.img_stride == 2 * h * w)
    if not _cx(cx).shadows:
        koct = None
    assert koct is None or (koct.f16 and koct.koct and koct_row + 2 <= (koct.rows + 7) // 8 * 8)
    _launch("flow_update", 0, 0, lambda: _lib.check(_lib.load().sf_flow_update(
        coords1.ptr, None if delta is None else delta.ptr,
        None if flow_a is None else flow_a.ptr, 0 if flow_a is None else flow_a.img_stride,
        None if flow_b is None else flow_b.ptr, 0 if flow_b is None else flow_b.img_stride,
        None if koct is None else koct.ptr, 0 if koct is None else koct.img_stride, int(koct_row),
        n_img, h, w, _lib.stream()), "sf_flow_update"))


@on_tensor_device
def upsample_flow(flow: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """flow [n,2,h,w], mask [n,576,h,w] -> [n,2,8h,8w] (reference streamflow.py:82-93)."""
    _dev_check(flow)
    _dev_check(mask)
    n, _, h, w = flow.shape
    out = torch.empty(n, 2, 8 * h, 8 * w, dtype=torch.float32, device=flow.device)
    _lib.check(_lib.load().sf_upsample_flow(flow.data_ptr(), mask.data_ptr(), out.data_ptr(), n, h, w, _lib.stream()),
               "sf_upsample_flow")
    return out


@on_tensor_device
def forward_interpolate(flow: torch.Tensor) -> torch.Tensor:
    """flow [n,2,h,w] -> [n,2,h,w] (reference utils.py:34-62, on the device)."""
    _dev_check(flow)
    n, _, h, w = flow.shape
    out = torch.empty_like(flow)
    _lib.check(_lib.load().sf_forward_interpolate(flow.data_ptr(), out.data_ptr(), n, h, w, _lib.stream()),
               "sf_forward_interpolate")
    return out


@on_tensor_device
def tile_blend(flows: torch.Tensor, weights: torch.Tensor, plan, n_clips: int = 1) -> torch.Tensor:
    """Gaussian-weighted blend of tiled inference (reference evaluate_mf.py:1021-1035): flows [n_clips * n_distinct, pairs, 2, th, tw]
    (the distinct crops of every clip, clip-major), weights [th, tw] (tiling.tile_weights), plan a tiling.TilePlan ->
    [n_clips, pairs, 2, h, w] over plan.crop, bitwise the reference's fp32 accumulation over plan.sequence."""
    _dev_check(flows)
    _dev_check(weights)
    th, tw = plan.tile_hw
    nd = plan.n_distinct
    if flows.dim() != 5 or flows.shape[0] != n_clips * nd or flows.shape[2:] != (2, th, tw):
        raise RuntimeError(f"tile_blend: flows {tuple(flows.shape)} do not match {n_clips} clip(s) x {nd} crop(s) of {th} x {tw}")
    if tuple(weights.shape) != (th, tw) or weights.device != flows.device:
        raise RuntimeError(f"tile_blend: weights {tuple(weights.shape)} on {weights.device} for crops of {th} x {tw} on {flows.device}")
    pairs = int(flows.shape[1])
    y0, x0, h, w = plan.crop
    desc = _lib.SfTilePlan(n_seq=len(plan.sequence), n_distinct=nd, tile_h=th, tile_w=tw, img_h=plan.image_hw[0],
                           img_w=plan.image_hw[1], out_y0=y0, out_x0=x0, out_h=h, out_w=w)
    if len(plan.sequence) > len(desc.tile_y):
        raise RuntimeError(f"tile_blend: {len(plan.sequence)} crops exceed the limit of {len(desc.tile_y)}")
    for k, ((ty, tx), d) in enumerate(zip(plan.sequence, plan.index)):
        desc.tile_y[k], desc.tile_x[k], desc.tile_id[k] = ty, tx, d
    out = torch.empty(n_clips, pairs, 2, h, w, dtype=torch.float32, device=flows.device)
    _lib.check(_lib.load().sf_tile_blend(flows.data_ptr(), weights.data_ptr(), out.data_ptr(), C.byref(desc), n_clips, pairs,
                                         _lib.stream()), "sf_tile_blend")
    return out


@on_tensor_device
def flow_to_image(flows: torch.Tensor, clip_flow: Optional[float] = None, rad_max: Optional[float] = None,
                  convert_to_bgr: bool = False, return_rad_max: bool = False):
    """Middlebury colour-wheel images of flow fields (reference core/utils/flow_viz.py: flow_to_image): flows [N, 2, H, W] ->
    uint8 [N, H, W, 3] on the same device, all N fields in one sf_flow_to_image call, each normalised by its OWN largest radius
    (or all by `rad_max` when given: one scale for a whole video, values above it are drawn at 0.75 brightness).  `clip_flow`
    clamps both components to [0, clip_flow] first, as the reference's np.clip does (a quirk: negative components become 0).
    A pixel with a non-finite component is black and does not enter the maximum.  return_rad_max: also the fp32 maxima [N]
    (None with a fixed `rad_max`)."""
    _dev_check(flows)
    if flows.dim() != 4 or flows.shape[1] != 2 or flows.numel() == 0:
        raise RuntimeError(f"flow_to_image: expected flows [N, 2, H, W], got {tuple(flows.shape)}")
    if (clip_flow is not None and not clip_flow >= 0) or (rad_max is not None and not rad_max >= 0):
        raise RuntimeError(f"flow_to_image: clip_flow / rad_max must be >= 0 (got {clip_flow}, {rad_max})")
    n, _, h, w = flows.shape
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=flows.device)
    ws = torch.empty(n, dtype=torch.float32, device=flows.device) if rad_max is None else None
    _lib.check(_lib.load().sf_flow_to_image(flows.data_ptr(), out.data_ptr(), None if ws is None else ws.data_ptr(), n, h, w,
                                            -1.0 if clip_flow is None else float(clip_flow),
                                            -1.0 if rad_max is None else float(rad_max), int(bool(convert_to_bgr)), _lib.stream()),
               "sf_flow_to_image")
    return (out, ws) if return_rad_max else out


@on_tensor_device
def flow_score(pred: torch.Tensor, gt: torch.Tensor, acc: torch.Tensor, step: int = 1) -> None:
    """Add the Spring scores of one field to `acc` (sf_flow_score; reference evaluate_mf.py:60-102): pred fp32 [2, h, w] on the GPU,
    any view whose rows are contiguous (padder.unpad(flow[0]) of the model's padded output needs no copy); gt fp32 [Hg, Wg, 2]
    contiguous (read_flo5's array), pixel (y, x) scored against gt[step * y, step * x]; acc float64 [scoring.LEN] contiguous on the
    same device.  Enqueued on the current stream, no synchronisation; streamflow_amd.scoring.report(acc) forms the dictionary."""
    from . import scoring
    if not (pred.is_cuda and gt.is_cuda and acc.is_cuda) or len({pred.device, gt.device, acc.device}) != 1:
        raise RuntimeError(f"flow_score: pred, gt and acc must be on one GPU (got {pred.device}, {gt.device}, {acc.device}); "
                           "host flows are scored by streamflow_amd.scoring.score_host")
    if pred.dtype != torch.float32 or pred.dim() != 3 or pred.shape[0] != 2 or pred.stride(2) != 1:
        raise RuntimeError(f"flow_score: pred must be fp32 [2, h, w] with contiguous rows (got {pred.dtype} {tuple(pred.shape)}, "
                           f"strides {pred.stride()})")
    if gt.dtype != torch.float32 or not gt.is_contiguous():
        raise RuntimeError(f"flow_score: gt must be contiguous fp32 [Hg, Wg, 2] (got {gt.dtype}, contiguous={gt.is_contiguous()})")
    if acc.dtype != torch.float64 or acc.numel() != scoring.LEN or not acc.is_contiguous():
        raise RuntimeError(f"flow_score: acc must be a contiguous float64 vector of {scoring.LEN} (got {acc.dtype} {tuple(acc.shape)})")
    h, w = int(pred.shape[1]), int(pred.shape[2])
    scoring.check_gt(tuple(gt.shape), h, w, int(step))
    ws = torch.empty(scoring.WS_BYTES, dtype=torch.uint8, device=pred.device)
    _lib.check(_lib.load().sf_flow_score(pred.data_ptr(), pred.stride(0), pred.stride(1), gt.data_ptr(), int(gt.shape[0]),
                                         int(gt.shape[1]), int(step), h, w, acc.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _lib.stream()), "sf_flow_score")


@on_tensor_device
def flow_score_batch(preds: Sequence[torch.Tensor], gts: Sequence[torch.Tensor], acc: torch.Tensor, kind: str = "flo",
                     masks: Optional[Sequence[torch.Tensor]] = None) -> None:
    """Add the Sintel / KITTI scores of field i to row i of `acc` (sf_flow_score_batch; reference evaluate_mf.py:106-142, :468-503,
    :549-592), up to 32 fields per call (two launches), longer sequences in several calls.  preds: fp32 [2, h, w] views on one GPU
    whose rows are contiguous and whose strides agree (padder.unpad(flow[k]) of the model's padded outputs, slices of
    predict_video's result: no copy); gts: per field, contiguous, as decoded -- kind "flo": fp32 [h, w, 2] (flow_io.read_flo), kind
    "kitti": the 16-bit samples [h, w, 3] of a flow_occ PNG (flow_io.read_png) as uint16 or, the same bits, int16; masks: None or
    per field contiguous uint8 [h, w], occluded where 255; acc: contiguous float64 [len(preds), scoring.EVAL_LEN].  Enqueued on
    the current stream, no synchronisation; scoring.sintel_from / kitti_from form the reports."""
    from . import scoring
    preds, gts = list(preds), list(gts)
    masks = None if masks is None else list(masks)
    n = len(preds)
    if kind not in scoring.GT_KINDS:
        raise ValueError(f"flow_score_batch: kind {kind!r} ('flo' or 'kitti')")
    if n == 0 or len(gts) != n or (masks is not None and len(masks) != n):
        raise ValueError(f"flow_score_batch: {n} predictions, {len(gts)} ground truths"
                         + ("" if masks is None else f", {len(masks)} masks") + " (equal and at least one)")
    if not isinstance(acc, torch.Tensor) or not acc.is_cuda:
        raise RuntimeError("flow_score_batch: acc must be on the GPU; host flows are scored by streamflow_amd.scoring.score_host_fields")
    dev, p0 = acc.device, preds[0]
    if acc.dtype != torch.float64 or tuple(acc.shape) != (n, scoring.EVAL_LEN) or not acc.is_contiguous():
        raise RuntimeError(f"flow_score_batch: acc must be contiguous float64 [{n}, {scoring.EVAL_LEN}] "
                           f"(got {acc.dtype} {tuple(acc.shape)})")
    h, w = (int(p0.shape[1]), int(p0.shape[2])) if p0.dim() == 3 else (0, 0)
    gt_shape = (h, w, 2) if kind == "flo" else (h, w, 3)
    gt_dtypes = (torch.float32,) if kind == "flo" else tuple(d for d in (getattr(torch, "uint16", None), torch.int16) if d is not None)
    for i, p in enumerate(preds):
        if not p.is_cuda or p.device != dev:
            raise RuntimeError(f"flow_score_batch: prediction {i} on {p.device}, acc on {dev}; there is no CPU fallback")
        if p.dtype != torch.float32 or p.dim() != 3 or p.shape[0] != 2 or p.numel() == 0 or p.stride(2) != 1:
            raise RuntimeError(f"flow_score_batch: prediction {i} must be fp32 [2, h, w] with contiguous rows (got {p.dtype} "
                               f"{tuple(p.shape)}, strides {p.stride()})")
        if p.shape != p0.shape or p.stride() != p0.stride():
            raise RuntimeError(f"flow_score_batch: prediction {i} is {tuple(p.shape)} with strides {p.stride()}, prediction 0 "
                               f"{tuple(p0.shape)} with {p0.stride()}")
        g = gts[i]
        if not g.is_cuda or g.device != dev:
            raise RuntimeError(f"flow_score_batch: ground truth {i} on {g.device}, acc on {dev}; there is no CPU fallback")
        if g.dtype not in gt_dtypes or tuple(g.shape) != gt_shape or not g.is_contiguous():
            raise RuntimeError(f"flow_score_batch: ground truth {i} of kind {kind!r} must be contiguous {gt_dtypes[0]} "
                               f"{list(gt_shape)} (got {g.dtype} {tuple(g.shape)}, contiguous={g.is_contiguous()})")
        if masks is not None:
            m = masks[i]
            if not m.is_cuda or m.device != dev:
                raise RuntimeError(f"flow_score_batch: mask {i} on {m.device}, acc on {dev}; there is no CPU fallback")
            if m.dtype != torch.uint8 or tuple(m.shape) != (h, w) or not m.is_contiguous():
                raise RuntimeError(f"flow_score_batch: mask {i} must be contiguous uint8 [{h}, {w}] (got {m.dtype} {tuple(m.shape)})")
    lib = _lib.load()
    step = scoring.SCORE_BATCH_MAX
    ws = torch.empty(int(lib.sf_flow_score_batch_ws_bytes(min(n, step), h, w)), dtype=torch.uint8, device=dev)
    for lo in range(0, n, step):
        k = min(step, n - lo)
        tab = _lib.SfScoreFields()
        for i in range(k):
            tab.pred[i], tab.gt[i] = preds[lo + i].data_ptr(), gts[lo + i].data_ptr()
            if masks is not None:
                tab.mask[i] = masks[lo + i].data_ptr()
        need = int(lib.sf_flow_score_batch_ws_bytes(k, h, w))
        if need > ws.numel():                                           # (a shorter last call may give each field more blocks)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _lib.check(lib.sf_flow_score_batch(C.byref(tab), k, p0.stride(0), p0.stride(1), scoring.GT_KINDS[kind], h, w,
                                           acc[lo:lo + k].data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream()),
                   "sf_flow_score_batch")


_NORM_LUT = {}            # device -> the normalisation table of frames_to_clips


def refuse_first_use_in_capture(what: str, build_before: str) -> None:
    """A device-side table cached on first use must not be built inside a graph capture: the cached tensor would belong to the graph's
    memory pool and hold nothing until a replay, yet every later eager call would read it (the rule of _PackedStream._cached)."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{what} requested for the first time inside a graph capture; build it before ({build_before})")


def norm_lut(device) -> torch.Tensor:
    """The 256 floats a byte value maps to, built once per device ON that device with the model's own expression
    (SKFlow_MF8.forward, reference streamflow.py:102: 2 * (x / 255.0) - 1.0): whatever the device's division by a scalar rounds to,
    the table holds exactly what the model computes from the same byte value.  The first use per device must come outside a graph
    capture (inside one it raises and caches nothing) and synchronises the stream that builds the table ONCE, so that the cached
    table is complete for every stream that reads it afterwards; later uses enqueue nothing and wait for nothing."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"norm_lut: the table is built on the GPU it is used on (got {device}); there is no CPU fallback")
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _NORM_LUT:
        refuse_first_use_in_capture("norm_lut: the normalisation table", "one eager ops.norm_lut(device) or frames_to_clips call")
        lut = (2 * (torch.arange(256, device=device).float() / 255.0) - 1.0).contiguous()
        torch.cuda.current_stream(device).synchronize()
        _NORM_LUT[key] = lut
    return _NORM_LUT[key]


@on_tensor_device
def frames_to_clips(frames: torch.Tensor, n: int, T: int, first_clip: int, n_clips: int, pad: Sequence[int] = (0, 0, 0, 0),
                    frame0: int = 0, channels_last: Optional[bool] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 frames -> the normalised, replicate-padded clip batch the encoders take (sf_frames_to_clips, one launch): frames uint8
    on the GPU, [n_buf, H, W, 3] or [n_buf, 3, H, W] (any strides; `channels_last` decides when both readings fit, default: HWC if
    the last dimension is 3), holding the frames frame0 .. frame0 + n_buf - 1 of a video of `n` frames; pad = [left, right, top,
    bottom] as InputPadder._pad.  Returns fp32 [n_clips, T, 3, Hp, Wp] for the clips first_clip .. first_clip + n_clips - 1 of the
    schedule in include/streamflow_hip.h (= video.clip_count / clip_start).  Enqueued on the current stream, no synchronisation --
    except on the FIRST use per device, which builds the normalisation table (norm_lut): that use synchronises the current stream
    once and raises inside a graph capture, so make one eager call (or ops.norm_lut(device)) before capturing."""
    if not frames.is_cuda:
        raise RuntimeError(f"frames_to_clips: frames must be on the GPU (got {frames.device}); there is no CPU fallback")
    if frames.dtype != torch.uint8 or frames.dim() != 4:
        raise RuntimeError(f"frames_to_clips: frames must be uint8 [n, H, W, 3] or [n, 3, H, W] (got {frames.dtype} {tuple(frames.shape)})")
    if channels_last is None:
        channels_last = frames.shape[3] == 3
    if frames.shape[3 if channels_last else 1] != 3:
        raise RuntimeError(f"frames_to_clips: no channel dimension of 3 in {tuple(frames.shape)} (channels_last={channels_last})")
    fs = frames.stride(0)
    if channels_last:
        (H, W), (rs, ps, cs) = frames.shape[1:3], frames.stride()[1:]
    else:
        (H, W), (cs, rs, ps) = frames.shape[2:], frames.stride()[1:]
    left, right, top, bottom = (int(p) for p in pad)
    Hp, Wp = int(H) + top + bottom, int(W) + left + right
    shape = (int(n_clips), int(T), 3, Hp, Wp)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=frames.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != frames.device or not out.is_contiguous():
        raise RuntimeError(f"frames_to_clips: out must be contiguous fp32 {shape} on {frames.device} "
                           f"(got {out.dtype} {tuple(out.shape)} on {out.device})")
    lut = norm_lut(frames.device)
    _lib.check(_lib.load().sf_frames_to_clips(frames.data_ptr(), fs, rs, ps, cs, int(frame0), int(frames.shape[0]), int(n), int(T),
                                              int(first_clip), int(n_clips), int(H), int(W), top, left, Hp, Wp, lut.data_ptr(),
                                              out.data_ptr(), _lib.stream()), "sf_frames_to_clips")
    return out


@on_tensor_device
def clips_to_flows(pairs: Sequence[torch.Tensor], n: int, T: int, first_clip: int, pair0: int, n_pairs: int, hw: Sequence[int],
                   pad: Sequence[int] = (0, 0, 0, 0), out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The model's T - 1 per-pair outputs of one clip batch -> flow fields in video order (sf_clips_to_flows, one launch): pairs[k]
    fp32 [n_clips, 2, Hp, Wp] on the GPU with contiguous rows (views of larger buffers are fine; all k share shape and strides), the
    batch starting at clip `first_clip` of a video of `n` frames.  Returns (or fills `out`, contiguous) fp32 [n_pairs, 2, H, W] =
    the pairs pair0 .. pair0 + n_pairs - 1, cropped by pad = [left, right, top, bottom]; the duplicates of the tail clip are dropped.
    Enqueued on the current stream, no synchronisation."""
    pairs = list(pairs)
    if len(pairs) != T - 1 or T < 2:
        raise RuntimeError(f"clips_to_flows: {len(pairs)} pair tensors for clips of T = {T}")
    if T - 1 > len(_lib.SfPairPtrs().p):
        raise RuntimeError(f"clips_to_flows: {T - 1} pairs per clip (at most {len(_lib.SfPairPtrs().p)})")
    p0 = pairs[0]
    for p in pairs:
        if not p.is_cuda or p.device != p0.device:
            raise RuntimeError(f"clips_to_flows: pair tensors must be on one GPU (got {p.device}); there is no CPU fallback")
        if p.dtype != torch.float32 or p.dim() != 4 or p.shape[1] != 2 or p.stride(3) != 1:
            raise RuntimeError(f"clips_to_flows: a pair tensor must be fp32 [n_clips, 2, Hp, Wp] with contiguous rows "
                               f"(got {p.dtype} {tuple(p.shape)}, strides {p.stride()})")
        if p.shape != p0.shape or p.stride() != p0.stride():
            raise RuntimeError("clips_to_flows: the pair tensors differ in shape or strides")
    H, W = int(hw[0]), int(hw[1])
    left, right, top, bottom = (int(p) for p in pad)
    if (H + top + bottom, W + left + right) != tuple(p0.shape[2:]):
        raise RuntimeError(f"clips_to_flows: {H} x {W} plus pad {list(pad)} is not the pair tensors' {tuple(p0.shape[2:])}")
    shape = (int(n_pairs), 2, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=p0.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != p0.device or not out.is_contiguous():
        raise RuntimeError(f"clips_to_flows: out must be contiguous fp32 {shape} on {p0.device} "
                           f"(got {out.dtype} {tuple(out.shape)} on {out.device})")
    ptrs = _lib.SfPairPtrs()
    for k, p in enumerate(pairs):
        ptrs.p[k] = p.data_ptr()
    _lib.check(_lib.load().sf_clips_to_flows(C.byref(ptrs), p0.stride(0), p0.stride(1), p0.stride(2), int(n), int(T), int(first_clip),
                                             int(p0.shape[0]), int(pair0), int(n_pairs), H, W, top, left, out.data_ptr(),
                                             _lib.stream()), "sf_clips_to_flows")
    return out


FBC_LEN, WARP_LEN = 7, 2     # SF_FBC_LEN, SF_WARP_LEN: doubles per stats row of flow_consistency / warp_frames
FBC_PIXELS, FBC_VISIBLE, FBC_OCCLUDED, FBC_OUTSIDE, FBC_SUM_FB, FBC_SUM_MAG, FBC_FINITE = range(7)
WARP_SUM_ABS, WARP_TERMS = range(2)


def _flow_fields(t, name: str, what: str):
    """Checks of a batch of flow fields fp32 [n, 2, h, w] with contiguous rows -> (n, h, w)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what}: {name} must be a tensor on the GPU (got {getattr(t, 'device', type(t).__name__)}); "
                           "there is no CPU fallback")
    if t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 2 or t.numel() == 0 or t.stride(3) != 1:
        raise RuntimeError(f"{what}: {name} must be fp32 [n, 2, h, w] with contiguous rows (got {t.dtype} {tuple(t.shape)}, "
                           f"strides {t.stride()})")
    if t.stride(2) < t.shape[3] or t.stride(0) < 0 or t.stride(1) == 0:
        raise RuntimeError(f"{what}: {name} has strides {t.stride()} (rows must not overlap)")
    return int(t.shape[0]), int(t.shape[2]), int(t.shape[3])


def _stats_rows(stats, n: int, length: int, dev, what: str) -> torch.Tensor:
    if stats is None:
        return torch.zeros(n, length, dtype=torch.float64, device=dev)
    if (not isinstance(stats, torch.Tensor) or stats.device != dev or stats.dtype != torch.float64 or tuple(stats.shape) != (n, length)
            or not stats.is_contiguous()):
        raise RuntimeError(f"{what}: stats must be contiguous float64 [{n}, {length}] on {dev} "
                           f"(got {getattr(stats, 'dtype', None)} {tuple(getattr(stats, 'shape', ()))})")
    return stats


def _frame_strides(t, name: str, channels_last, hw, n: int, dev, what: str):
    """Checks of a batch of uint8 frames [n, H, W, 3] / [n, 3, H, W] -> byte strides (frame, row, pixel, channel)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what}: {name} must be a tensor on the GPU (got {getattr(t, 'device', type(t).__name__)}); "
                           "there is no CPU fallback")
    if t.dtype != torch.uint8 or t.dim() != 4:
        raise RuntimeError(f"{what}: {name} must be uint8 [n, H, W, 3] or [n, 3, H, W] (got {t.dtype} {tuple(t.shape)})")
    if channels_last is None:
        channels_last = t.shape[3] == 3
    if t.shape[3 if channels_last else 1] != 3:
        raise RuntimeError(f"{what}: no channel dimension of 3 in {name} {tuple(t.shape)} (channels_last={channels_last})")
    fs = t.stride(0)
    if channels_last:
        shape, (rs, ps, cs) = tuple(t.shape[1:3]), t.stride()[1:]
    else:
        shape, (cs, rs, ps) = tuple(t.shape[2:]), t.stride()[1:]
    if int(t.shape[0]) != n or tuple(int(v) for v in shape) != tuple(hw) or t.device != dev:
        raise RuntimeError(f"{what}: {name} holds {int(t.shape[0])} frames of {tuple(shape)} on {t.device}, the flows are {n} fields of "
                           f"{tuple(hw)} on {dev}")
    if min(fs, rs, ps, cs) < 0:
        raise RuntimeError(f"{what}: {name} has a negative stride {t.stride()}")
    return fs, rs, ps, cs


@on_tensor_device
def flow_consistency(fwd: torch.Tensor, bwd: torch.Tensor, alpha: float = 0.01, beta: float = 0.5, codes: Sequence[int] = (0, 1, 2),
                     stats: Optional[torch.Tensor] = None):
    """Forward-backward consistency classes of n flow fields (sf_flow_consistency, two launches for the whole batch): fwd, bwd fp32
    [n, 2, h, w] on one GPU, any views with contiguous rows (slices of predict_video's outputs need no copy); bwd[i] is the flow
    that leads back from the frame fwd[i] leads to.  A pixel is visible when |fwd + bwd(x + fwd)|^2 <= alpha (|fwd|^2 + |bwd|^2) +
    beta (alpha, beta: the constants of Sundaram et al. 2010 / UnFlow), occluded when not, outside when x + fwd leaves the frame (NaN
    and infinite flows included).  codes = the bytes written for (visible, occluded, outside); (255, 0, 128) gives a mask image.
    Returns (cls uint8 [n, h, w], stats float64 [n, FBC_LEN]); a given `stats` is ADDED to (rows: FBC_PIXELS, FBC_VISIBLE,
    FBC_OCCLUDED, FBC_OUTSIDE, FBC_SUM_FB, FBC_SUM_MAG, FBC_FINITE; include/streamflow_hip.h).  Enqueued on the current stream,
    no synchronisation."""
    what = "flow_consistency"
    n, h, w = _flow_fields(fwd, "fwd", what)
    if _flow_fields(bwd, "bwd", what) != (n, h, w) or bwd.device != fwd.device:
        raise RuntimeError(f"{what}: fwd is {tuple(fwd.shape)} on {fwd.device}, bwd {tuple(bwd.shape)} on {bwd.device}")
    codes = tuple(int(c) for c in codes)
    if len(codes) != 3 or any(not 0 <= c <= 255 for c in codes):
        raise RuntimeError(f"{what}: codes must be three byte values (visible, occluded, outside), got {codes}")
    if alpha != alpha or beta != beta:
        raise RuntimeError(f"{what}: alpha / beta is NaN")
    dev = fwd.device
    stats = _stats_rows(stats, n, FBC_LEN, dev, what)
    lib = _lib.load()
    cls = torch.empty(n, h, w, dtype=torch.uint8, device=dev)
    ws = torch.empty(int(lib.sf_flow_consistency_ws_bytes(n, h, w)), dtype=torch.uint8, device=dev)
    _lib.check(lib.sf_flow_consistency(fwd.data_ptr(), fwd.stride(0), fwd.stride(1), fwd.stride(2), bwd.data_ptr(), bwd.stride(0),
                                       bwd.stride(1), bwd.stride(2), n, h, w, float(alpha), float(beta), codes[0], codes[1], codes[2],
                                       cls.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream()),
               "sf_flow_consistency")
    return cls, stats


@on_tensor_device
def warp_frames(src: torch.Tensor, flows: torch.Tensor, cls: Optional[torch.Tensor] = None, ref: Optional[torch.Tensor] = None,
                channels_last: Optional[bool] = None, stats: Optional[torch.Tensor] = None, visible: int = 0):
    """Frames warped back along flow fields (sf_warp_frames): src uint8 [n, H, W, 3] or [n, 3, H, W] on the GPU, any strides
    (`channels_last` decides when both readings fit, default: HWC if the last dimension is 3); flows fp32 [n, 2, H, W] with contiguous
    rows, flows[i] leading from the frame the result is aligned with to src[i] (in a video: src = frames 1 .. n, flows = the forward
    flows).  Returns (warped uint8 [n, H, W, 3]: bilinear taps rounded to nearest, 0 where the target leaves the frame; stats).
    With `cls` (flow_consistency's map for the same flows, uint8 [n, H, W] contiguous, `visible` = its byte for visible pixels) and
    `ref` (the frames the result is aligned with, laid out like src) the photometric error is ADDED into stats float64 [n, WARP_LEN]:
    WARP_SUM_ABS = sum of |warped value - ref byte| over visible pixels and channels, WARP_TERMS = the number of terms; without
    them stats is None.  Enqueued on the current stream, no synchronisation."""
    what = "warp_frames"
    n, h, w = _flow_fields(flows, "flows", what)
    dev = flows.device
    s = _frame_strides(src, "src", channels_last, (h, w), n, dev, what)
    if (cls is None) != (ref is None):
        raise RuntimeError(f"{what}: cls and ref come together (got cls={'given' if cls is not None else None}, "
                           f"ref={'given' if ref is not None else None})")
    if cls is None and stats is not None:
        raise RuntimeError(f"{what}: stats without cls and ref")
    lib = _lib.load()
    r, ws, cls_ptr, ref_ptr = (0, 0, 0, 0), None, None, None
    if cls is not None:
        if not cls.is_cuda or cls.device != dev or cls.dtype != torch.uint8 or tuple(cls.shape) != (n, h, w) or not cls.is_contiguous():
            raise RuntimeError(f"{what}: cls must be contiguous uint8 [{n}, {h}, {w}] on {dev} (got {cls.dtype} {tuple(cls.shape)} on "
                               f"{cls.device}); there is no CPU fallback")
        if not 0 <= int(visible) <= 255:
            raise RuntimeError(f"{what}: visible must be a byte value, got {visible}")
        r = _frame_strides(ref, "ref", channels_last, (h, w), n, dev, what)
        stats = _stats_rows(stats, n, WARP_LEN, dev, what)
        ws = torch.empty(int(lib.sf_warp_frames_ws_bytes(n, h, w)), dtype=torch.uint8, device=dev)
        cls_ptr, ref_ptr = cls.data_ptr(), ref.data_ptr()
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
    _lib.check(lib.sf_warp_frames(src.data_ptr(), s[0], s[1], s[2], s[3], flows.data_ptr(), flows.stride(0), flows.stride(1),
                                  flows.stride(2), n, h, w, out.data_ptr(), cls_ptr, int(visible), ref_ptr, r[0], r[1], r[2], r[3],
                                  None if stats is None else stats.data_ptr(), None if ws is None else ws.data_ptr(),
                                  0 if ws is None else ws.numel(), _lib.stream()), "sf_warp_frames")
    return out, stats


MOTION_KINDS = {"translation": 0, "similarity": 1, "affine": 2}      # SF_MOTION_*
BORDERS = {"constant": 0, "replicate": 1}                             # SF_BORDER_*
MOT_LEN, MOT_TRACE_LEN, MOT_MAX_ROUNDS = 14, 23, 16                   # SF_MOT_LEN, SF_MOT_TRACE_LEN, SF_MOT_MAX_ROUNDS
(MOT_S1, MOT_SX, MOT_SY, MOT_SXX, MOT_SXY, MOT_SYY, MOT_SU, MOT_SXU, MOT_SYU, MOT_SV, MOT_SXV, MOT_SYV, MOT_SQQ, MOT_N) = range(14)
MOT_TRACE_MOMENTS, MOT_TRACE_MODEL, MOT_TRACE_C, MOT_TRACE_INV_C2, MOT_TRACE_STATUS = 0, 14, 20, 21, 22
MOT_OK, MOT_DEGENERATE, MOT_EMPTY = range(3)


def motion_to_pixels(models: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """Normalised models float64 [..., 6] (include/streamflow_hip.h, "video stabilisation") -> [..., 2, 3] with p' = M [x, y, 1] in
    pixels: the point a pixel of the field's first frame moves to.  float64 throughout, on the models' device."""
    m = models.to(torch.float64)
    cx, cy, s = (w - 1) * 0.5, (h - 1) * 0.5, 2.0 / max(w - 1, h - 1, 1)
    a0, a1, a2, a3, a4, a5 = (m[..., k] for k in range(6))
    rows = [1.0 + a1 * s, a2 * s, a0 - (a1 * s) * cx - (a2 * s) * cy, a4 * s, 1.0 + a5 * s, a3 - (a4 * s) * cx - (a5 * s) * cy]
    return torch.stack(rows, dim=-1).reshape(*m.shape[:-1], 2, 3)


@on_tensor_device
def motion_fit(flows: torch.Tensor, cls: Optional[torch.Tensor] = None, kind: str = "similarity", rounds: int = 6, step: int = 1,
               kappa: float = 2.0, c_floor: float = 1.0, max_mag: Optional[float] = None, codes: Sequence[int] = (0, 1, 2),
               class_weights: Sequence[float] = (1.0, 0.0, 0.0)):
    """A global (camera) motion per flow field by iteratively reweighted least squares (sf_motion_fit: 2 * rounds launches for the
    whole batch, no host synchronisation).  flows fp32 [n, 2, h, w] on the GPU, any views with contiguous rows.  kind: "translation",
    "similarity" or "affine".  Round 0 is plain (class-weighted) least squares; every later round weighs a pixel by Tukey's biweight
    of its residual against the previous model, with the scale c = max(c_floor, kappa * RMS residual of that model) in pixels.
    cls (flow_consistency's class map for the same flows, uint8 [n, h, w] contiguous, `codes` its bytes for visible / occluded /
    outside) gives the classes `class_weights`; step > 1 uses every step-th pixel of every step-th row; flows beyond max_mag
    (default 4 * max(h, w)), NaN and Inf weigh nothing.
    Returns (models float64 [n, 2, 3] on the GPU: p' = M [x, y, 1] in pixels, the point a pixel moves to; info): info["status"]
    int32 [n] (MOT_OK, MOT_DEGENERATE: too few pixels for `kind`, a translation was fitted; MOT_EMPTY: no pixel, zero motion),
    info["c"] float64 [n] the last scale, info["inlier_share"] float64 [n] the last round's weight sum over round 0's,
    info["normalised"] float64 [n, 6] and info["trace"] float64 [n, rounds, MOT_TRACE_LEN], every round's moments, model and scale."""
    what = "motion_fit"
    if kind not in MOTION_KINDS:
        raise ValueError(f"{what}: kind {kind!r} (one of {', '.join(MOTION_KINDS)})")
    if not isinstance(rounds, int) or isinstance(rounds, bool) or not 1 <= rounds <= MOT_MAX_ROUNDS:
        raise ValueError(f"{what}: rounds must be an integer 1 .. {MOT_MAX_ROUNDS}, got {rounds!r}")
    if not isinstance(step, int) or isinstance(step, bool) or step < 1:
        raise ValueError(f"{what}: step must be an integer >= 1, got {step!r}")
    n, h, w = _flow_fields(flows, "flows", what)
    dev = flows.device
    if max_mag is None:
        max_mag = 4.0 * max(h, w)
    if not (kappa >= 0 and kappa < float("inf")) or not (c_floor > 0 and c_floor < float("inf")) or not max_mag >= 0:
        raise ValueError(f"{what}: kappa must be finite and >= 0, c_floor finite and > 0, max_mag >= 0 (got {kappa}, {c_floor}, {max_mag})")
    codes, cw = tuple(int(c) for c in codes), tuple(float(v) for v in class_weights)
    if len(codes) != 3 or any(not 0 <= c <= 255 for c in codes):
        raise ValueError(f"{what}: codes must be three byte values (visible, occluded, outside), got {codes}")
    if len(cw) != 3 or any(not (0 <= v < float("inf")) for v in cw):
        raise ValueError(f"{what}: class_weights must be three finite weights >= 0, got {cw}")
    if cls is not None and (not isinstance(cls, torch.Tensor) or cls.device != dev or cls.dtype != torch.uint8
                            or tuple(cls.shape) != (n, h, w) or not cls.is_contiguous()):
        raise RuntimeError(f"{what}: cls must be contiguous uint8 [{n}, {h}, {w}] on {dev} (got {getattr(cls, 'dtype', None)} "
                           f"{tuple(getattr(cls, 'shape', ()))} on {getattr(cls, 'device', None)}); there is no CPU fallback")
    lib = _lib.load()
    trace = torch.empty(n, rounds, MOT_TRACE_LEN, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.sf_motion_fit_ws_bytes(n, h, w, step)), dtype=torch.uint8, device=dev)
    _lib.check(lib.sf_motion_fit(flows.data_ptr(), flows.stride(0), flows.stride(1), flows.stride(2), n, h, w,
                                 None if cls is None else cls.data_ptr(), codes[0], codes[1], codes[2], cw[0], cw[1], cw[2], step,
                                 float(max_mag), MOTION_KINDS[kind], rounds, float(kappa), float(c_floor), trace.data_ptr(), ws.data_ptr(),
                                 ws.numel(), _lib.stream()), "sf_motion_fit")
    last = trace[:, -1]
    normalised = last[:, MOT_TRACE_MODEL:MOT_TRACE_MODEL + 6]
    total = trace[:, 0, MOT_S1]
    info = {"status": last[:, MOT_TRACE_STATUS].to(torch.int32), "c": last[:, MOT_TRACE_C],
            "inlier_share": torch.where(total > 0, last[:, MOT_S1] / total, torch.zeros_like(total)),
            "normalised": normalised, "trace": trace}
    return motion_to_pixels(normalised, h, w), info


@on_tensor_device
def warp_affine(frames: torch.Tensor, inv_maps: torch.Tensor, border: str = "replicate", fill: Sequence[int] = (0, 0, 0),
                out: Optional[torch.Tensor] = None, channels_last: Optional[bool] = None):
    """Frames rendered through affine maps (sf_warp_affine_u8): frames uint8 [n, H, W, 3] or [n, 3, H, W] on the GPU, any strides
    (`channels_last` as warp_frames); inv_maps [n, 2, 3] (or [n, 6]), any float type on any device: the source coordinate of output
    pixel (x, y) is inv_maps[i] @ [x, y, 1] (rounded to fp32 here).  Bilinear taps rounded to nearest.  border: "replicate" clamps
    the source coordinate to the frame, "constant" writes the three `fill` bytes outside (a NaN coordinate gets them in either mode).
    Returns (uint8 [n, H, W, 3] -- `out` when given: contiguous, on the frames' GPU --, outside uint32-valued int32 [n]: the pixels
    whose source lies outside the frame).  Enqueued on the current stream."""
    what = "warp_affine"
    if border not in BORDERS:
        raise ValueError(f"{what}: border {border!r} (one of {', '.join(BORDERS)})")
    fill = tuple(int(v) for v in fill)
    if len(fill) != 3 or any(not 0 <= v <= 255 for v in fill):
        raise ValueError(f"{what}: fill must be three byte values, got {fill}")
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
        raise RuntimeError(f"{what}: frames must be a uint8 tensor [n, H, W, 3] or [n, 3, H, W], got {type(frames).__name__} "
                           f"{tuple(getattr(frames, 'shape', ()))}")
    if channels_last is None:
        channels_last = frames.shape[3] == 3
    n = int(frames.shape[0])
    hw = tuple(int(v) for v in (frames.shape[1:3] if channels_last else frames.shape[2:]))
    dev = frames.device
    s = _frame_strides(frames, "frames", channels_last, hw, n, dev, what)
    if n < 1 or min(hw) < 1:
        raise RuntimeError(f"{what}: no frames or empty frames {tuple(frames.shape)}")
    maps = torch.as_tensor(inv_maps)
    if not maps.is_floating_point() or maps.numel() != 6 * n or tuple(maps.shape) not in ((n, 2, 3), (n, 6)):
        raise RuntimeError(f"{what}: inv_maps must be floating point [{n}, 2, 3] (got {maps.dtype} {tuple(maps.shape)})")
    maps = maps.to(device=dev, dtype=torch.float32).contiguous()
    h, w = hw
    if out is None:
        out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3)
          or not out.is_contiguous()):
        raise RuntimeError(f"{what}: out must be contiguous uint8 [{n}, {h}, {w}, 3] on {dev}")
    lib = _lib.load()
    outside = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.sf_warp_affine_ws_bytes(n, h, w)), dtype=torch.uint8, device=dev)
    _lib.check(lib.sf_warp_affine_u8(frames.data_ptr(), s[0], s[1], s[2], s[3], maps.data_ptr(), n, h, w, BORDERS[border], fill[0],
                                     fill[1], fill[2], out.data_ptr(), outside.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream()),
               "sf_warp_affine_u8")
    return out, outside


INTERP_LEN = 5               # SF_INTERP_LEN: doubles per stats row of frame_interp
INTERP_PIXELS, INTERP_BOTH, INTERP_A_ONLY, INTERP_B_ONLY, INTERP_HOLES = range(5)
INTERP_MAX_DEN = 64


@on_tensor_device
def frame_interp(a: torch.Tensor, b: torch.Tensor, fwd: torch.Tensor, bwd: torch.Tensor, num: int, den: int, cls=None,
                 importance: Sequence[int] = (16, 1, 16), cover: bool = False, stats: Optional[torch.Tensor] = None,
                 codes: Sequence[int] = (0, 1), channels_last: Optional[bool] = None, max_ws_bytes: int = 1 << 30):
    """The frames at time num / den (0 < num < den <= 64) between n frame pairs, by forward splatting with integer weights
    (sf_frame_interp; include/streamflow_hip.h has the arithmetic): a, b uint8 [n, H, W, 3] or [n, 3, H, W] on the GPU, any strides
    (as warp_frames; in a video a = frames[:-1], b = frames[1:]); fwd the flows a -> b, bwd the flows b -> a, fp32 [n, 2, H, W] with
    contiguous rows.  cls: None or (cls_f, cls_b), flow_consistency's maps of (fwd, bwd) and of (bwd, fwd), uint8 [n, H, W]
    contiguous, with codes = their bytes for (visible, occluded); importance = the integer weights 1 .. 16 of a (visible, occluded,
    other) source pixel, the first for every pixel without cls.  Returns (out uint8 [n, H, W, 3], cover uint8 [n, H, W] or None:
    0 both sides, 1 a only, 2 b only, 3 hole; stats float64 [n, INTERP_LEN], a given `stats` is ADDED to: INTERP_PIXELS and the
    pixels of each cover code).  The workspace (64 bytes per pixel and pair) is allocated per call; the pairs are split into chunks so
    that one call's workspace stays under `max_ws_bytes` (one pair at least).  The bytes do not depend on the chunking: all sums are
    integer.  Enqueued on the current stream, no synchronisation."""
    what = "frame_interp"
    n, h, w = _flow_fields(fwd, "fwd", what)
    dev = fwd.device
    if _flow_fields(bwd, "bwd", what) != (n, h, w) or bwd.device != dev:
        raise RuntimeError(f"{what}: fwd is {tuple(fwd.shape)} on {fwd.device}, bwd {tuple(bwd.shape)} on {bwd.device}")
    sa = _frame_strides(a, "a", channels_last, (h, w), n, dev, what)
    sb = _frame_strides(b, "b", channels_last, (h, w), n, dev, what)
    num, den = int(num), int(den)
    if not 0 < num < den <= INTERP_MAX_DEN:
        raise RuntimeError(f"{what}: t = {num} / {den} (0 < num < den <= {INTERP_MAX_DEN})")
    imp = tuple(int(v) for v in importance)
    if len(imp) != 3 or any(not 1 <= v <= 16 for v in imp):
        raise RuntimeError(f"{what}: importance must be three integers 1 .. 16 (visible, occluded, other), got {tuple(importance)}")
    codes = tuple(int(c) for c in codes)
    if len(codes) != 2 or any(not 0 <= c <= 255 for c in codes):
        raise RuntimeError(f"{what}: codes must be two byte values (visible, occluded), got {codes}")
    if cls is not None:
        if not isinstance(cls, (tuple, list)) or len(cls) != 2:
            raise RuntimeError(f"{what}: cls must be a pair (cls_f, cls_b) of class maps")
        for c in cls:
            if (not isinstance(c, torch.Tensor) or not c.is_cuda or c.device != dev or c.dtype != torch.uint8
                    or tuple(c.shape) != (n, h, w) or not c.is_contiguous()):
                raise RuntimeError(f"{what}: a class map must be contiguous uint8 [{n}, {h}, {w}] on {dev} (got "
                                   f"{getattr(c, 'dtype', None)} {tuple(getattr(c, 'shape', ()))} on {getattr(c, 'device', None)}); "
                                   "there is no CPU fallback")
    stats = _stats_rows(stats, n, INTERP_LEN, dev, what)
    lib = _lib.load()
    per = int(lib.sf_frame_interp_ws_bytes(1, h, w))
    if per < 0:
        _lib.check(per, "sf_frame_interp_ws_bytes")
    m = min(n, max(1, int(max_ws_bytes) // per))
    while m > 1 and int(lib.sf_frame_interp_ws_bytes(m, h, w)) > int(max_ws_bytes):
        m -= 1
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
    cov = torch.empty(n, h, w, dtype=torch.uint8, device=dev) if cover else None
    ws = torch.empty(int(lib.sf_frame_interp_ws_bytes(m, h, w)), dtype=torch.uint8, device=dev)
    for lo in range(0, n, m):
        k = min(m, n - lo)
        _lib.check(lib.sf_frame_interp(a.data_ptr() + lo * sa[0], sa[0], sa[1], sa[2], sa[3], b.data_ptr() + lo * sb[0], sb[0], sb[1],
                                       sb[2], sb[3], fwd[lo:].data_ptr(), fwd.stride(0), fwd.stride(1), fwd.stride(2),
                                       bwd[lo:].data_ptr(), bwd.stride(0), bwd.stride(1), bwd.stride(2), k, h, w, num, den,
                                       None if cls is None else cls[0][lo:].data_ptr(), None if cls is None else cls[1][lo:].data_ptr(),
                                       codes[0], codes[1], imp[0], imp[1], imp[2], out[lo:].data_ptr(),
                                       None if cov is None else cov[lo:].data_ptr(), stats[lo:].data_ptr(), ws.data_ptr(), ws.numel(),
                                       _lib.stream()), "sf_frame_interp")
    return out, cov, stats


def _resize_size(size, what: str):
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise RuntimeError(f"{what}: size must be (h, w), got {size!r}") from None
    if h < 1 or w < 1:
        raise RuntimeError(f"{what}: size must be positive, got {(h, w)}")
    return h, w


def _resize_tables(H: int, W: int, h: int, w: int, filter: str, dev, kind: str):
    """(bounds_x, kx, ksize_x, bounds_y, ky, ksize_y) as pointers / ints: None / 0 for an axis that has no pass.  The tensors stay
    alive in resize.device_table's cache."""
    from . import resize
    bx = kx = by = ky = None
    nx = ny = 0
    if w != W:
        tb, tk, nx = resize.device_table(W, w, filter, dev, kind)
        bx, kx = tb.data_ptr(), tk.data_ptr()
    if h != H:
        tb, tk, ny = resize.device_table(H, h, filter, dev, kind)
        by, ky = tb.data_ptr(), tk.data_ptr()
    return bx, kx, nx, by, ky, ny


@on_tensor_device
def resize_frames(frames: torch.Tensor, size: Sequence[int], filter: str = "bilinear", channels_last: Optional[bool] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 frames resampled to size = (h, w) (sf_resize_u8: Pillow's 8-bit resampler, byte for byte what PIL.Image.resize gives
    with the same filter): frames uint8 [n, H, W, 3] or [n, 3, H, W] on the GPU, any strides (`channels_last` decides when both
    readings fit, default: HWC if the last dimension is 3); filter: 'box', 'bilinear', 'bicubic' or 'lanczos'.  Returns (or fills
    `out`, contiguous) uint8 [n, h, w, 3].  The coefficient tables are built on the host once per (size pair, filter, device)
    (resize.device_table); the workspace is allocated per call.  Enqueued on the current stream, no synchronisation."""
    what = "resize_frames"
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise RuntimeError(f"{what}: frames must be a tensor on the GPU (got {getattr(frames, 'device', type(frames).__name__)}); "
                           "there is no CPU fallback")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.numel() == 0:
        raise RuntimeError(f"{what}: frames must be uint8 [n, H, W, 3] or [n, 3, H, W] (got {frames.dtype} {tuple(frames.shape)})")
    if channels_last is None:
        channels_last = frames.shape[3] == 3
    H, W = (int(v) for v in (frames.shape[1:3] if channels_last else frames.shape[2:]))
    n, dev = int(frames.shape[0]), frames.device
    fs, rs, ps, cs = _frame_strides(frames, "frames", channels_last, (H, W), n, dev, what)
    h, w = _resize_size(size, what)
    shape = (n, h, w, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous():
        raise RuntimeError(f"{what}: out must be contiguous uint8 {shape} on {dev} (got {out.dtype} {tuple(out.shape)} on {out.device})")
    lib = _lib.load()
    need = int(lib.sf_resize_u8_ws_bytes(n, H, W, h, w))
    if need < 0:
        _lib.check(need, "sf_resize_u8_ws_bytes")
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    bx, kx, nx, by, ky, ny = _resize_tables(H, W, h, w, filter, dev, "u8")
    _lib.check(lib.sf_resize_u8(frames.data_ptr(), fs, rs, ps, cs, n, H, W, h, w, bx, kx, nx, by, ky, ny, out.data_ptr(),
                                None if ws is None else ws.data_ptr(), need, _lib.stream()), "sf_resize_u8")
    return out


@on_tensor_device
def resize_flows(flows: torch.Tensor, size: Sequence[int], filter: str = "bilinear", rescale: bool = True,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Flow fields resampled to size = (h, w) (sf_resize_f32): flows fp32 [n, 2, H, W] on the GPU with contiguous rows (views are
    fine).  rescale=True: the values are brought to the new grid's pixels, u times w / W and v times h / H (one fp32 multiply on the
    final store); False: plain resampling of two planes.  Returns (or fills `out`, contiguous) fp32 [n, 2, h, w].  Enqueued on the
    current stream, no synchronisation."""
    what = "resize_flows"
    n, H, W = _flow_fields(flows, "flows", what)
    dev = flows.device
    h, w = _resize_size(size, what)
    shape = (n, 2, h, w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise RuntimeError(f"{what}: out must be contiguous fp32 {shape} on {dev} (got {out.dtype} {tuple(out.shape)} on {out.device})")
    lib = _lib.load()
    need = int(lib.sf_resize_f32_ws_bytes(n, H, W, h, w))
    if need < 0:
        _lib.check(need, "sf_resize_f32_ws_bytes")
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    bx, kx, nx, by, ky, ny = _resize_tables(H, W, h, w, filter, dev, "f32")
    sx, sy = (w / W, h / H) if rescale else (1.0, 1.0)
    _lib.check(lib.sf_resize_f32(flows.data_ptr(), flows.stride(0), flows.stride(1), flows.stride(2), n, H, W, h, w, bx, kx, nx, by, ky,
                                 ny, float(sx), float(sy), out.data_ptr(), None if ws is None else ws.data_ptr(), need, _lib.stream()),
               "sf_resize_f32")
    return out


PNG_BPP = (1, 2, 3, 4, 6, 8)         # PNG filter distances sf_png_unfilter is built for: 8 / 16-bit grey, grey + alpha, RGB, RGBA


@on_tensor_device
def png_unfilter(scan: torch.Tensor, h: int, w: int, bpp: int, out: Optional[torch.Tensor] = None, swap16: bool = False) -> torch.Tensor:
    """Undo the PNG row filters of a batch of inflated IDAT streams (sf_png_unfilter, one launch; the host side of it is
    flow_io.png_scanlines): scan uint8 [n, h * (1 + w * bpp)] on the GPU, rows contiguous (any row stride), image i's h scanlines
    with their filter-type bytes; bpp the filter distance (PNG_BPP).  Returns (or fills `out`: uint8 [n, h, w * bpp] on the same
    GPU with contiguous bytes in a row, any row / image strides) the reconstructed bytes; swap16 swaps the bytes of every 16-bit
    sample, so `.view(torch.uint16)` of a contiguous result holds the samples in host order.  Enqueued on the current stream, no
    synchronisation."""
    if not isinstance(scan, torch.Tensor) or not scan.is_cuda:
        raise RuntimeError(f"png_unfilter: scan must be on the GPU (got {getattr(scan, 'device', type(scan).__name__)}); "
                           "there is no CPU fallback -- flow_io.read_png is the host-side path")
    h, w, bpp = int(h), int(w), int(bpp)
    if bpp not in PNG_BPP or h < 1 or w < 1:
        raise RuntimeError(f"png_unfilter: h = {h}, w = {w}, bpp = {bpp} (bpp one of {PNG_BPP})")
    if scan.dtype != torch.uint8 or scan.dim() != 2 or scan.shape[0] < 1 or scan.shape[1] != h * (1 + w * bpp) or scan.stride(1) != 1:
        raise RuntimeError(f"png_unfilter: scan must be uint8 [n, {h * (1 + w * bpp)}] with contiguous rows (got {scan.dtype} "
                           f"{tuple(scan.shape)}, strides {scan.stride()})")
    if swap16 and bpp % 2:
        raise RuntimeError(f"png_unfilter: swap16 needs an even bpp (got {bpp})")
    n = int(scan.shape[0])
    shape = (n, h, w * bpp)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=scan.device)
    elif (tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != scan.device or out.stride(2) != 1
          or out.stride(1) < w * bpp or (n > 1 and out.stride(0) < (h - 1) * out.stride(1) + w * bpp)):
        raise RuntimeError(f"png_unfilter: out must be uint8 {shape} on {scan.device} with contiguous bytes in a row and "
                           f"non-overlapping rows and images (got {out.dtype} {tuple(out.shape)} on {out.device}, strides {out.stride()})")
    scan_stride = scan.stride(0) if n > 1 else h * (1 + w * bpp)
    out_stride = out.stride(0) if n > 1 else (h - 1) * out.stride(1) + w * bpp
    _lib.check(_lib.load().sf_png_unfilter(scan.data_ptr(), scan_stride, n, h, w, bpp, out.data_ptr(), out_stride, out.stride(1),
                                           1 if swap16 else 0, _lib.stream()), "sf_png_unfilter")
    return out


@on_tensor_device
def png_encode(images: torch.Tensor):
    """The zlib streams of a PNG's IDAT chunk for a batch of device images (sf_png_encode: adaptive row filter and Huffman-only
    deflate, csrc/png_encode.hip; the host half is flow_io.png_file): images [n, H, W, C] uint8 or torch.uint16 (host order; written
    big-endian) on the GPU, C = 1 .. 4, the samples of a row contiguous, any row and image strides.  Returns (streams uint8
    [n, sf_png_encode_bound], lengths int64 [n]) on the same GPU: stream i is streams[i, :lengths[i]], the bytes behind it are
    unspecified.  Enqueued on the current stream, no synchronisation."""
    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        raise RuntimeError(f"png_encode: images must be on the GPU (got {getattr(images, 'device', type(images).__name__)}); "
                           "there is no CPU fallback -- flow_io.write_png is the host-side path")
    if images.dtype not in (torch.uint8, torch.uint16) or images.dim() != 4 or images.numel() == 0 or images.shape[3] > 4:
        raise RuntimeError(f"png_encode: expected uint8 / uint16 [n, H, W, C <= 4], got {images.dtype} {tuple(images.shape)}")
    n, h, w, c = (int(v) for v in images.shape)
    size = images.element_size()
    if images.stride(3) != 1 or images.stride(2) != c or images.stride(1) < w * c or (n > 1 and images.stride(0) < (h - 1) * images.stride(1) + w * c):
        raise RuntimeError(f"png_encode: the samples of a row must be contiguous and rows / images must not overlap (strides {images.stride()})")
    lib = _lib.load()
    bound, ws_bytes = lib.sf_png_encode_bound(h, w, c * size), lib.sf_png_encode_ws_bytes(n, h, w, c * size)
    if bound < 0 or ws_bytes < 0:
        raise RuntimeError(f"png_encode: n = {n}, h = {h}, w = {w}, bpp = {c * size} is outside what sf_png_encode takes")
    streams = torch.empty(n, bound, dtype=torch.uint8, device=images.device)
    lengths = torch.empty(n, dtype=torch.int64, device=images.device)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=images.device)
    image_stride = images.stride(0) if n > 1 else (h - 1) * images.stride(1) + w * c
    _lib.check(lib.sf_png_encode(images.data_ptr(), image_stride * size, images.stride(1) * size, n, h, w, c * size, 1 if size == 2 else 0,
                                 streams.data_ptr(), bound, lengths.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream()), "sf_png_encode")
    return streams, lengths


@on_tensor_device
def jpeg_encode(images: torch.Tensor, qtables):
    """The entropy-coded segments of baseline JPEG files for a batch of device images (sf_jpeg_encode: JFIF YCbCr 4:4:4, integer DCT,
    the Annex K.3 Huffman tables, one restart interval per MCU row, csrc/jpeg_encode.hip; the host half is jpeg_gpu.jpeg_file):
    images uint8 [n, H, W, 3] (RGB) or [n, H, W] (grey) on the GPU, the samples of a row contiguous, any row and image strides;
    qtables: [2, 64] steps 1 .. 255 in natural order (jpeg_gpu.quant_tables).  Returns (segments uint8 [n, sf_jpeg_encode_bound],
    lengths int64 [n]) on the same GPU: segment i is segments[i, :lengths[i]], the bytes behind it are unspecified.  Enqueued on the
    current stream, no synchronisation."""
    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        raise RuntimeError(f"jpeg_encode: images must be on the GPU (got {getattr(images, 'device', type(images).__name__)}); "
                           "there is no CPU fallback")
    if images.dtype != torch.uint8 or images.dim() not in (3, 4) or images.numel() == 0 or (images.dim() == 4 and images.shape[3] != 3):
        raise RuntimeError(f"jpeg_encode: expected uint8 [n, H, W, 3] or [n, H, W], got {images.dtype} {tuple(images.shape)}")
    n, h, w = (int(v) for v in images.shape[:3])
    c = 3 if images.dim() == 4 else 1
    if (c == 3 and images.stride(3) != 1) or images.stride(2) != c or images.stride(1) < w * c or \
            (n > 1 and images.stride(0) < (h - 1) * images.stride(1) + w * c):
        raise RuntimeError(f"jpeg_encode: the samples of a row must be contiguous and rows / images must not overlap (strides {images.stride()})")
    q = np.ascontiguousarray(np.asarray(qtables)).reshape(-1)
    if q.size != 128 or q.min() < 1 or q.max() > 255:
        raise RuntimeError("jpeg_encode: qtables must be two tables of 64 steps in 1 .. 255")
    q = q.astype(np.uint16)
    lib = _lib.load()
    bound, ws_bytes = lib.sf_jpeg_encode_bound(h, w, c), lib.sf_jpeg_encode_ws_bytes(n, h, w, c)
    if bound < 0 or ws_bytes < 0:
        raise RuntimeError(f"jpeg_encode: n = {n}, h = {h}, w = {w} is outside what sf_jpeg_encode takes")
    segments = torch.empty(n, bound, dtype=torch.uint8, device=images.device)
    lengths = torch.empty(n, dtype=torch.int64, device=images.device)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=images.device)
    image_stride = images.stride(0) if n > 1 else (h - 1) * images.stride(1) + w * c
    _lib.check(lib.sf_jpeg_encode(images.data_ptr(), image_stride, images.stride(1), n, h, w, c, q.ctypes.data, segments.data_ptr(), bound,
                                  lengths.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream()), "sf_jpeg_encode")
    return segments, lengths


JPEG_DESC_WORDS, JPEG_TABLE_SET_BYTES = 6, 1824


@on_tensor_device
def jpeg_decode(data: torch.Tensor, desc: torch.Tensor, tables: torch.Tensor, n_images: int, h: int, w: int, components: int, hs: int,
                vs: int, out_channels: int = 3, segment_bytes: Optional[int] = None, split_min_bytes: Optional[int] = None):
    """Baseline JPEG files of one geometry -> pixels (sf_jpeg_decode, csrc/jpeg_decode.hip: Huffman decoding a wave per restart
    interval, libjpeg's integer inverse DCT, fancy chroma upsampling, YCbCr -> RGB; the host half is jpeg_gpu.parse / pack).  With
    segment_bytes and / or split_min_bytes it is sf_jpeg_decode_split: an interval of at least split_min_bytes (default 0: every one)
    is decoded a thread per segment of segment_bytes (default 128; a power of two in 8 .. 4096) unstuffed bytes -- what a file without
    restart markers needs; the pixels of an image whose status is 0 are the same either way.  data
    uint8 [B]: the entropy-coded bytes, still stuffed; desc int64 [n_intervals, 6] = (in_off, in_len, image, first_mcu, n_mcus,
    table_set) per restart interval; tables uint8 [n_sets, 1824]; all three on the same GPU.  components 1 or 3, hs x vs the luma
    sampling (1 x 1, 2 x 1, 2 x 2).  Returns (images uint8 [n_images, h, w, out_channels], status int32 [n_images]) on that GPU:
    status 0, or an index into jpeg_gpu.DECODE_STATUS (include/streamflow_hip.h SF_JPEG_*) for an image whose pixels are then
    unspecified.  Enqueued on the current stream, no synchronisation: reading the status is the caller's."""
    for name, t, dt in (("data", data, torch.uint8), ("desc", desc, torch.int64), ("tables", tables, torch.uint8)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"jpeg_decode: {name} must be on the GPU (got {getattr(t, 'device', type(t).__name__)}); "
                               "there is no CPU fallback")
        if t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"jpeg_decode: {name} must be a contiguous {dt} tensor, got {t.dtype} {tuple(t.shape)}")
    if data.dim() != 1 or desc.dim() != 2 or desc.shape[1] != JPEG_DESC_WORDS or desc.shape[0] < 1 or tables.dim() != 2 or \
            tables.shape[1] != JPEG_TABLE_SET_BYTES or tables.shape[0] < 1:
        raise RuntimeError(f"jpeg_decode: expected data [B], desc [n >= 1, {JPEG_DESC_WORDS}], tables [s >= 1, {JPEG_TABLE_SET_BYTES}]; "
                           f"got {tuple(data.shape)}, {tuple(desc.shape)}, {tuple(tables.shape)}")
    if data.device != desc.device or data.device != tables.device:
        raise RuntimeError(f"jpeg_decode: data, desc and tables must share a device ({data.device}, {desc.device}, {tables.device})")
    n, h, w, c, hs, vs, oc = (int(v) for v in (n_images, h, w, components, hs, vs, out_channels))
    lib = _lib.load()
    split = segment_bytes is not None or split_min_bytes is not None
    seg, smin = int(128 if segment_bytes is None else segment_bytes), int(0 if split_min_bytes is None else split_min_bytes)
    if split and (seg < 8 or seg > 4096 or seg & (seg - 1) or smin < 0):
        raise RuntimeError(f"jpeg_decode: segment_bytes = {seg} (a power of two in 8 .. 4096), split_min_bytes = {smin} (>= 0)")
    ws_bytes = lib.sf_jpeg_decode_split_ws_bytes(n, h, w, c, hs, vs, data.numel(), int(desc.shape[0]), seg) if split else \
        lib.sf_jpeg_decode_ws_bytes(n, h, w, c, hs, vs)
    if ws_bytes < 0 or oc not in (1, 3):
        raise RuntimeError(f"jpeg_decode: n = {n}, h = {h}, w = {w}, components = {c}, sampling {hs} x {vs}, out_channels = {oc} is "
                           "outside what sf_jpeg_decode takes")
    out = torch.empty(n, h, w, oc, dtype=torch.uint8, device=data.device)
    status = torch.empty(n, dtype=torch.int32, device=data.device)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=data.device)
    # an empty tensor has no storage to point at: any non-null, never dereferenced address stands for it
    if split:
        _lib.check(lib.sf_jpeg_decode_split(data.data_ptr() or status.data_ptr(), data.numel(), desc.data_ptr(), int(desc.shape[0]),
                                            tables.data_ptr(), int(tables.shape[0]), n, h, w, c, hs, vs, out.data_ptr(), h * w * oc, w * oc, oc,
                                            status.data_ptr(), seg, smin, ws.data_ptr(), ws_bytes, _lib.stream()), "sf_jpeg_decode_split")
        return out, status
    _lib.check(lib.sf_jpeg_decode(data.data_ptr() or status.data_ptr(), data.numel(), desc.data_ptr(), int(desc.shape[0]), tables.data_ptr(),
                                  int(tables.shape[0]), n, h, w, c, hs, vs, out.data_ptr(), h * w * oc, w * oc, oc, status.data_ptr(),
                                  ws.data_ptr(), ws_bytes, _lib.stream()), "sf_jpeg_decode")
    return out, status


@on_tensor_device
def flow_to_kitti16(flows: torch.Tensor) -> torch.Tensor:
    """KITTI flow codes of device flows (sf_flow_to_kitti16; flow_io.kitti_encode for float32): flows fp32 [N, 2, H, W] -> torch.uint16
    [N, H, W, 3] = (64 u + 2^15, 64 v + 2^15, 1), truncated; NaN and values below 0 give 0, values above 65535 give 65535."""
    _dev_check(flows)
    if flows.dim() != 4 or flows.shape[1] != 2 or flows.numel() == 0:
        raise RuntimeError(f"flow_to_kitti16: expected flows [N, 2, H, W], got {tuple(flows.shape)}")
    n, _, h, w = flows.shape
    out = torch.empty(n, h, w, 3, dtype=torch.uint16, device=flows.device)
    _lib.check(_lib.load().sf_flow_to_kitti16(flows.data_ptr(), out.data_ptr(), n, h, w, _lib.stream()), "sf_flow_to_kitti16")
    return out


@on_tensor_device
def flo5_encode(flows: torch.Tensor, rows_per_chunk: int = 0):
    """The compressed HDF5 chunks of Spring .flo5 files for a batch of device flows (sf_flo5_encode: byte shuffle and Huffman-only
    deflate, csrc/flo5_encode.hip; the host half is flo5.flo5_file with shuffle=True): flows fp32 [n, 2, H, W] on the GPU, the
    samples of a row contiguous, any row / channel / field strides that do not overlap (an unpadded view of the model's padded output
    goes in without a copy).  rows_per_chunk = 0: flo5.write_flo5's rule, ceil(H / 32).  Returns (streams uint8 [n, nchunks,
    sf_flo5_chunk_bound], lengths int64 [n, nchunks]) on the same GPU: chunk c of field i is streams[i, c, :lengths[i, c]], the bytes
    behind it are unspecified.  Enqueued on the current stream, no synchronisation."""
    if not isinstance(flows, torch.Tensor) or not flows.is_cuda:
        raise RuntimeError(f"flo5_encode: flows must be on the GPU (got {getattr(flows, 'device', type(flows).__name__)}); "
                           "there is no CPU fallback -- flo5.write_flo5 is the host-side path")
    if flows.dtype != torch.float32 or flows.dim() != 4 or flows.shape[1] != 2 or flows.numel() == 0:
        raise RuntimeError(f"flo5_encode: expected float32 [n, 2, H, W], got {flows.dtype} {tuple(flows.shape)}")
    n, _, h, w = (int(v) for v in flows.shape)
    rpc = int(rows_per_chunk)
    if rpc < 0:
        raise RuntimeError(f"flo5_encode: rows_per_chunk = {rows_per_chunk}")
    if rpc == 0:
        rpc = max(1, -(-h // 32))
    plane = (h - 1) * flows.stride(2) + w
    if flows.stride(3) != 1 or flows.stride(2) < w or flows.stride(1) < plane or (n > 1 and flows.stride(0) < flows.stride(1) + plane):
        raise RuntimeError(f"flo5_encode: the samples of a row must be contiguous and rows / channels / fields must not overlap "
                           f"(strides {flows.stride()})")
    lib = _lib.load()
    bound, ws_bytes = lib.sf_flo5_chunk_bound(rpc, w), lib.sf_flo5_encode_ws_bytes(n, h, w, rpc)
    if bound < 0 or ws_bytes < 0:
        raise RuntimeError(f"flo5_encode: n = {n}, h = {h}, w = {w}, rows_per_chunk = {rpc} is outside what sf_flo5_encode takes")
    nchunks = -(-h // rpc)
    streams = torch.empty(n, nchunks, bound, dtype=torch.uint8, device=flows.device)
    lengths = torch.empty(n, nchunks, dtype=torch.int64, device=flows.device)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=flows.device)
    field_stride = flows.stride(0) if n > 1 else flows.stride(1) + plane
    _lib.check(lib.sf_flo5_encode(flows.data_ptr(), field_stride, flows.stride(1), flows.stride(2), n, h, w, rpc, streams.data_ptr(), bound,
                                  lengths.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream()), "sf_flo5_encode")
    return streams, lengths


INFLATE_DESC_WORDS, INFLATE_STORED = 5, 1
INFLATE_STATUS = ("ok", "bad zlib header", "truncated input", "block type 3", "bad code-length set", "invalid symbol",
                  "distance before the start of the output", "output longer than expected", "output shorter than expected",
                  "Adler-32 mismatch", "stored block LEN / NLEN mismatch", "preset dictionary", "stream outside the buffers")


@on_tensor_device
def inflate(comp: torch.Tensor, desc: torch.Tensor, out: torch.Tensor):
    """A batch of zlib streams inflated on the GPU (sf_inflate, csrc/flo5_decode.hip: one wave per stream).  comp uint8 [B], the
    compressed bytes; desc int64 [n, 5] = (in_off, in_len, out_off, out_len, flags) per stream, flags & 1: the bytes are stored as
    they are and are copied; out uint8 [O], written inside the streams' slots only.  All three on the same GPU.  Returns status
    int32 [n] on that GPU: 0, or an index into INFLATE_STATUS (include/streamflow_hip.h SF_INFLATE_*).  Enqueued on the current
    stream, no synchronisation: reading the status is the caller's."""
    for name, t, dt in (("comp", comp, torch.uint8), ("desc", desc, torch.int64), ("out", out, torch.uint8)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"inflate: {name} must be on the GPU (got {getattr(t, 'device', type(t).__name__)}); "
                               "there is no CPU fallback -- zlib.decompress is the host-side path")
        if t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"inflate: {name} must be a contiguous {dt} tensor, got {t.dtype} {tuple(t.shape)}")
    if comp.dim() != 1 or out.dim() != 1 or desc.dim() != 2 or desc.shape[1] != INFLATE_DESC_WORDS or desc.shape[0] < 1:
        raise RuntimeError(f"inflate: expected comp [B], desc [n >= 1, {INFLATE_DESC_WORDS}], out [O]; got {tuple(comp.shape)}, "
                           f"{tuple(desc.shape)}, {tuple(out.shape)}")
    if comp.device != desc.device or comp.device != out.device:
        raise RuntimeError(f"inflate: comp, desc and out must share a device ({comp.device}, {desc.device}, {out.device})")
    n = int(desc.shape[0])
    status = torch.empty(n, dtype=torch.int32, device=comp.device)
    lib = _lib.load()
    # an empty tensor has no storage to point at: any non-null, never dereferenced address stands for it
    ptr = lambda t: t.data_ptr() or status.data_ptr()
    _lib.check(lib.sf_inflate(ptr(comp), comp.numel(), desc.data_ptr(), n, ptr(out), out.numel(), status.data_ptr(), _lib.stream()),
               "sf_inflate")
    return status


@on_tensor_device
def flo5_assemble(chunks: torch.Tensor, grid: torch.Tensor, h: int, w: int, chunk_shape, shuffle: bool) -> torch.Tensor:
    """Inflated .flo5 chunks -> the datasets (sf_flo5_assemble).  chunks uint8 [n_slots, chunk_stride] on the GPU, a slot's first
    4 ch cw cc bytes one inflated chunk of a float32 (h, w, 2) dataset in chunks of chunk_shape = (ch, cw, cc), cc 1 or 2,
    byte-shuffled when `shuffle`; grid int32 [n, ceil(h / ch), ceil(w / cw), 2 // cc]: the slot of every chunk of every file, -1
    for a chunk the file does not store (0.0).  Returns float32 [n, h, w, 2], file i bit for bit flo5.read_flo5's array."""
    for name, t, dt in (("chunks", chunks, torch.uint8), ("grid", grid, torch.int32)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"flo5_assemble: {name} must be on the GPU (got {getattr(t, 'device', type(t).__name__)}); "
                               "there is no CPU fallback -- flo5.read_flo5 is the host-side path")
        if t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"flo5_assemble: {name} must be a contiguous {dt} tensor, got {t.dtype} {tuple(t.shape)}")
    ch, cw, cc = (int(v) for v in chunk_shape)
    h, w = int(h), int(w)
    if h < 1 or w < 1 or ch < 1 or cw < 1 or cc not in (1, 2):
        raise RuntimeError(f"flo5_assemble: h = {h}, w = {w}, chunk_shape = {(ch, cw, cc)} (cc must be 1 or 2)")
    want = (-(-h // ch), -(-w // cw), 2 // cc)
    if grid.dim() != 4 or tuple(grid.shape[1:]) != want or grid.shape[0] < 1 or chunks.dim() != 2 or chunks.device != grid.device:
        raise RuntimeError(f"flo5_assemble: expected grid [n, {want[0]}, {want[1]}, {want[2]}] and chunks [n_slots, stride] on one "
                           f"device, got {tuple(grid.shape)} and {tuple(chunks.shape)}")
    n = int(grid.shape[0])
    out = torch.empty(n, h, w, 2, dtype=torch.float32, device=chunks.device)
    lib = _lib.load()
    _lib.check(lib.sf_flo5_assemble(chunks.data_ptr() or out.data_ptr(), int(chunks.shape[1]), int(chunks.shape[0]), grid.data_ptr(), n, h, w,
                                    ch, cw, cc, 1 if shuffle else 0, out.data_ptr(), _lib.stream()), "sf_flo5_assemble")
    return out


def pair_strides(arr: Optional[Sequence[int]]):
    if arr is None:
        return None
    return (C.c_int64 * 4)(*[int(a) for a in arr])


def corr_build_ws_bytes(B: int, pairs: int, D: int, h: int, w: int) -> int:
    return int(_lib.load().sf_corr_build_ws_bytes(B, pairs, D, h, w))


def corr_pitch(h: int, w: int) -> Optional[tuple]:
    """Row pitch (cells) of the fp32 volume maps of an h x w feature grid, or None where the reference's dense [N, h_l, w_l] layout
    already starts every level-0 row on a cache line (w % 32 == 0: Sintel 128, Spring 240 is NOT): every level's rows are rounded
    up to 32 cells = 128 bytes (sf_corr_build_pyramid_pitched; DESIGN.md section 12.7: KITTI's 156-cell rows)."""
    if w % 32 == 0:
        return None
    return tuple(((w >> l) + 31) // 32 * 32 for l in range(4))


def _pitch_arg(pitch):
    return None if pitch is None else (C.c_int32 * 4)(*[int(p) for p in pitch])


@on_tensor_device
def corr_build(f1_ptr: int, f2_ptr: int, clip_stride: int, pair_stride: int, lvls: Sequence[torch.Tensor],
               lvl_pair_stride: Optional[Sequence[int]], B: int, pairs: int, D: int, h: int, w: int,
               ws: Optional[torch.Tensor] = None, cx: Optional[Ctx] = None, pitch: Optional[Sequence[int]] = None) -> None:
    """ws: scratch of corr_build_ws_bytes() bytes for the split-precision / fp16 builds (allocated here when omitted).
    The dtype of `lvls` selects the volume format: float32 (arithmetic = the package precision, fp32 or f16x3) or
    float16 (SF_PRECISION_F16: single f16 products, fp16 cells).  pitch: row pitch of the maps in cells per level (corr_pitch),
    None = dense."""
    N = h * w
    vol16 = lvls[0].dtype == torch.float16
    assert all(t.dtype == lvls[0].dtype for t in lvls) and lvls[0].dtype in (torch.float16, torch.float32)
    prec = PRECISION_F16 if vol16 else min(_cx(cx).precision, PRECISION_F16X3)
    need = corr_build_ws_bytes(B, pairs, D, h, w) if prec != PRECISION_FP32 else 0
    if need and (ws is None or ws.numel() * ws.element_size() < need):
        ws = torch.empty(need, dtype=torch.uint8, device=lvls[0].device)
    cells = sum((h >> l) * (w >> l) for l in range(4))
    # algorithmic bytes per (clip, pair): both feature maps read once + every pyramid cell written once
    nbytes = B * pairs * (2.0 * N * D * 4 + (2.0 if vol16 else 4.0) * N * cells)
    _launch("corr_build", 2.0 * N * N * D * B * pairs, nbytes, lambda: _lib.check(
        _lib.load().sf_corr_build_pyramid_pitched(
            f1_ptr, f2_ptr, clip_stride, pair_stride, lvls[0].data_ptr(), lvls[1].data_ptr(), lvls[2].data_ptr(),
            lvls[3].data_ptr(), pair_strides(lvl_pair_stride), _pitch_arg(pitch), B, pairs, D, h, w, 4, prec,
            ws.data_ptr() if need else None, need, _lib.stream()),
        "sf_corr_build_pyramid"), products=_products(prec))


@on_tensor_device
def corr_lookup(lvls: Sequence[torch.Tensor], lvl_pair_stride: Optional[Sequence[int]], coords: Planes,
                out: Planes, B: int, pairs: int, h: int, w: int, cx: Optional[Ctx] = None,
                pitch: Optional[Sequence[int]] = None) -> None:
    assert out.rows == 324 and out.n_img == B * pairs and coords.img_stride == 2 * h * w
    N = h * w
    vol16 = lvls[0].dtype == torch.float16
    # algorithmic bytes per image: 10x10 footprint x 4 levels read + coords + 324 output channels
    # the k-octet copy of the output (Planes.shadow) comes out of the same kernel when the volumes are fp16
    cx = _cx(cx)
    sh = out.shadow if (out.shadow is not None and cx.shadows and vol16 and cx.shadow_fused) else None
    # (footprints + coords + the 324 fp32 output channels; the k-octet copy is extra traffic)
    nbytes = B * pairs * (N * 4 * 100 * (2.0 if vol16 else 4.0) + N * 2 * 4.0 + N * 324 * 4.0)
    _launch("corr_lookup", 0, nbytes, lambda: _lib.check(_lib.load().sf_corr_lookup_pitched(
        lvls[0].data_ptr(), lvls[1].data_ptr(), lvls[2].data_ptr(), lvls[3].data_ptr(),
        pair_strides(lvl_pair_stride), _pitch_arg(pitch), coords.ptr, out.ptr, out.img_stride,
        None if sh is None else sh.ptr, 0 if sh is None else sh.img_stride, B, pairs, h, w, 4, 4,
        PRECISION_F16 if vol16 else PRECISION_FP32, _lib.stream()), "sf_corr_lookup"))
    if sh is None:
        refresh_shadow(out, cx)


@dataclass(frozen=True)
class BlockedVolume:
    """Correlation pyramids of `n_img` images in the blocked layout (one buffer): fp16 cells in 8 x 8-cell blocks
    (csrc/corr_blocked.hip) or, `f32`, fp32 cells in 4-row x 8-column blocks (csrc/corr_blocked32.hip)."""
    buf: torch.Tensor          # uint8
    img_stride: int            # bytes
    n_img: int
    h: int
    w: int
    rec: int                   # bytes per source pixel
    off: tuple                 # byte offset of each level inside a record
    nby: tuple
    nbx: tuple
    src_rows: int              # records per image (h*w rounded up to 128)
    f32: bool = False          # fp32 cells, blocks of 4 rows x 8 columns

    def levels(self):
        """The four levels as [n_img, h*w, hl, wl] tensors of the cell type (copies; tests and API parity only)."""
        N = self.h * self.w
        bh = 4 if self.f32 else 8                                         # block rows (8 columns either way)
        out = []
        for l in range(4):
            hl, wl, nby, nbx = self.h >> l, self.w >> l, self.nby[l], self.nbx[l]
            blk = torch.as_strided(self.buf[self.off[l]:], (self.n_img, N, nby * nbx * 128), (self.img_stride, self.rec, 1))
            blk = blk.contiguous().view(torch.float32 if self.f32 else torch.float16)
            blk = blk.view(self.n_img, N, nby, nbx, 8, bh)                # [by][bx][tx % 8][ty % bh]
            out.append(blk.permute(0, 1, 2, 5, 3, 4).reshape(self.n_img, N, nby * bh, nbx * 8)[:, :, :hl, :wl].contiguous())
        return out


def blocked_geometry(h: int, w: int, f32: bool = False):
    rec, src = C.c_int64(), C.c_int64()
    off, nby, nbx = (C.c_int64 * 4)(), (C.c_int32 * 4)(), (C.c_int32 * 4)()
    name = "sf_corr_blocked32_geometry" if f32 else "sf_corr_blocked_geometry"
    _lib.check(getattr(_lib.load(), name)(h, w, C.byref(rec), off, nby, nbx, C.byref(src)), name)
    return int(rec.value), tuple(int(v) for v in off), tuple(int(v) for v in nby), tuple(int(v) for v in nbx), int(src.value)


def new_blocked_volume(n_img: int, h: int, w: int, device, f32: bool = False) -> BlockedVolume:
    rec, off, nby, nbx, src = blocked_geometry(h, w, f32)
    stride = src * rec                                      # a multiple of 128 (rec is)
    buf = torch.empty(n_img * stride + 128, dtype=torch.uint8, device=device)
    pad = (-buf.data_ptr()) % 128
    return BlockedVolume(buf[pad: pad + n_img * stride], stride, n_img, h, w, rec, off, nby, nbx, src, f32)


def corr_build_blocked_ws_bytes(n_img: int, D: int, h: int, w: int, f32: bool = False) -> int:
    if f32:
        return int(_lib.load().sf_corr_build_blocked32_ws_bytes(n_img, D, h, w))
    return int(_lib.load().sf_corr_build_blocked_ws_bytes(n_img, D, h, w))


@on_tensor_device
def corr_build_blocked(f1_ptr: int, f2_ptr: int, clip_stride: int, pair_stride: int, vol: BlockedVolume, B: int,
                       pairs: int, D: int, ws: Optional[torch.Tensor] = None) -> None:
    """a1 + a2 into a BlockedVolume: fp16 cells (single f16 MFMA products, fp32 accumulation) or, for an f32 volume, fp32
    cells (split fp16 operands, three products, fp32 accumulation)."""
    h, w = vol.h, vol.w
    N = h * w
    assert vol.n_img == B * pairs
    need = corr_build_blocked_ws_bytes(B * pairs, D, h, w, vol.f32)
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=vol.buf.device)
    cells = sum((h >> l) * (w >> l) for l in range(4))
    e = 4.0 if vol.f32 else 2.0
    nbytes = B * pairs * (2.0 * N * D * 4 + e * N * cells)
    name = "sf_corr_build_blocked32" if vol.f32 else "sf_corr_build_blocked"
    _launch("corr_build", 2.0 * N * N * D * B * pairs, nbytes, lambda: _lib.check(
        getattr(_lib.load(), name)(f1_ptr, f2_ptr, clip_stride, pair_stride, vol.buf.data_ptr(), vol.img_stride,
                                   B, pairs, D, h, w, ws.data_ptr(), need, _lib.stream()), name))


@on_tensor_device
def corr_lookup_blocked(vol: BlockedVolume, coords: Planes, out: Optional[Planes], out_koct: Optional[Planes], B: int,
                        pairs: int) -> None:
    """a3 from a BlockedVolume: `out_koct` (fp16 k-octet planes of the 324 features) and / or `out` (fp32 planes)."""
    h, w = vol.h, vol.w
    N = h * w
    assert coords.img_stride == 2 * N and vol.n_img == B * pairs
    assert out is None or (out.rows == 324 and out.n_img == B * pairs and not out.f16)
    assert out_koct is None or (out_koct.rows == 324 and out_koct.n_img == B * pairs and out_koct.koct)
    if vol.f32:                                           # fp32 cells: fp32 planes out (the fp32-class operand format)
        assert out is not None and out_koct is None
        nbytes = B * pairs * (N * 4 * 100 * 4.0 + N * 2 * 4.0 + N * 324 * 4.0)  # SURVEY.md section 8d, e = 4
        _launch("corr_lookup", 0, nbytes, lambda: _lib.check(_lib.load().sf_corr_lookup_blocked32(
            vol.buf.data_ptr(), vol.img_stride, coords.ptr, out.ptr, out.img_stride, B, pairs, h, w, _lib.stream()),
            "sf_corr_lookup_blocked32"))
        return
    nbytes = B * pairs * (N * 4 * 100 * 2.0 + N * 2 * 4.0 + N * 324 * 4.0)      # SURVEY.md section 8d, e = 2
    _launch("corr_lookup", 0, nbytes, lambda: _lib.check(_lib.load().sf_corr_lookup_blocked(
        vol.buf.data_ptr(), vol.img_stride, coords.ptr, None if out is None else out.ptr,
        0 if out is None else out.img_stride, None if out_koct is None else out_koct.ptr,
        0 if out_koct is None else out_koct.img_stride, B, pairs, h, w, _lib.stream()), "sf_corr_lookup_blocked"))


def corr_direct_ws_bytes(B: int, pairs: int, D: int, h: int, w: int, precision: int = PRECISION_F16) -> int:
    """Bytes of the packed features of the volume-free route (csrc/corr_direct.hip): f1 and the four-level pyramid of f2."""
    return int(_lib.load().sf_corr_direct_ws_bytes(B, pairs, D, h, w, precision))


@on_tensor_device
def corr_direct_pack(f1_ptr: int, f2_ptr: int, clip_stride: int, pair_stride: int, ws: torch.Tensor, B: int, pairs: int,
                     D: int, h: int, w: int, precision: int = PRECISION_F16) -> None:
    """Once per clip: f1 and the pooled pyramid of f2 into `ws` (uint8, corr_direct_ws_bytes() bytes, 16-byte aligned)."""
    N = h * w
    need = corr_direct_ws_bytes(B, pairs, D, h, w, precision)
    assert ws.dtype == torch.uint8 and ws.numel() >= need
    nbytes = B * pairs * (2.0 * N * D * 4 + need / (B * pairs))       # both feature maps read once + the workspace written once
    _launch("corr_direct_pack", 0, nbytes, lambda: _lib.check(_lib.load().sf_corr_direct_pack(
        f1_ptr, f2_ptr, clip_stride, pair_stride, ws.data_ptr(), need, B, pairs, D, h, w, precision, _lib.stream()),
        "sf_corr_direct_pack"))


@on_tensor_device
def corr_direct_lookup(ws: torch.Tensor, coords: Planes, out: Optional[Planes], out_koct: Optional[Planes], B: int, pairs: int,
                       D: int, h: int, w: int, precision: int = PRECISION_F16) -> None:
    """a3 from the packed features: `out_koct` (fp16 k-octet planes of the 324 features) and / or `out` (fp32 planes)."""
    N = h * w
    assert coords.img_stride == 2 * N
    assert out is None or (out.rows == 324 and out.n_img == B * pairs and not out.f16)
    assert out_koct is None or (out_koct.rows == 324 and out_koct.n_img == B * pairs and out_koct.koct)
    parts = 2 if precision == PRECISION_F16X3 else 1
    cells = sum((h >> l) * (w >> l) for l in range(4))
    # algorithmic bytes per image: the packed features read once + coords + the outputs written
    nbytes = B * pairs * ((N + cells) * D * 2.0 * parts + N * 2 * 4.0 + N * 324 * 4.0 * (out is not None)
                          + N * 328 * 2.0 * (out_koct is not None))
    _launch("corr_lookup", 2.0 * 400 * D * N * B * pairs, nbytes, lambda: _lib.check(_lib.load().sf_corr_direct_lookup(
        ws.data_ptr(), coords.ptr, None if out is None else out.ptr, 0 if out is None else out.img_stride,
        None if out_koct is None else out_koct.ptr, 0 if out_koct is None else out_koct.img_stride, B, pairs, D, h, w,
        precision, _lib.stream()), "sf_corr_direct_lookup"), products=_products(precision))


@on_tensor_device
def bilinear_sampler(img: torch.Tensor, coords: torch.Tensor, want_mask: bool = False):
    _dev_check(img)
    _dev_check(coords)
    M, Cc, Hi, Wi = img.shape
    _, Ho, Wo, _ = coords.shape
    out = torch.empty(M, Cc, Ho, Wo, dtype=torch.float32, device=img.device)
    mask = torch.empty(M, Ho, Wo, 1, dtype=torch.float32, device=img.device) if want_mask else None
    _lib.check(_lib.load().sf_bilinear_sampler(img.data_ptr(), coords.data_ptr(), out.data_ptr(),
                                               None if mask is None else mask.data_ptr(), M, Cc, Hi, Wi, Ho, Wo,
                                               _lib.stream()), "sf_bilinear_sampler")
    return (out, mask) if want_mask else out


# ---- point tracking (libstreamflow_track, include/streamflow_track.h) ------------------------------------------------------------
TRACK_VISIBLE, TRACK_OCCLUDED, TRACK_LOST, TRACK_PENDING = range(4)      # SFT_VISIBLE ... SFT_PENDING
TRACK_ALPHA, TRACK_BETA = 0.01, 0.5                                      # consistency.ALPHA, consistency.BETA


@on_tensor_device
def track_advance(fwd: torch.Tensor, bwd: Optional[torch.Tensor] = None, state=None, start: Optional[torch.Tensor] = None,
                  frame0: int = 0, alpha: float = TRACK_ALPHA, beta: float = TRACK_BETA, sticky: bool = False, counts: bool = False):
    """P points through K flow fields in one launch (sft_track_advance): p <- p + bilinear(fwd_k, p) per step, with a visibility
    decision from bwd when it is given.  fwd, bwd fp32 [K, 2, h, w] on one GPU, any views with contiguous rows (slices of
    predict_video's outputs need no copy); field k is the pair (frame0 + k, frame0 + k + 1).  state = (xy fp32 [2, P] contiguous,
    status uint8 [P]) as a previous call returned it, or as track.TrackSink builds it (queries, all TRACK_PENDING); None: dense mode,
    a point per pixel of the grid, all started.  start int32 [P]: the frame at which each point becomes active (None: at once).
    Returns (xy fp32 [K, 2, P], status uint8 [K, P], new_state): row k describes frame frame0 + k + 1; new_state is the last row
    (views, no copy).  counts=True: a fourth result, int32 [K, 4], the points of each status per row.  Enqueued on the current
    stream, no synchronisation."""
    from . import _track_lib
    what = "track_advance"
    K, h, w = _flow_fields(fwd, "fwd", what)
    dev = fwd.device
    if bwd is not None and (_flow_fields(bwd, "bwd", what) != (K, h, w) or bwd.device != dev):
        raise RuntimeError(f"{what}: fwd is {tuple(fwd.shape)} on {dev}, bwd {tuple(bwd.shape)} on {bwd.device}")
    if min(fwd.stride(0), fwd.stride(1)) < 1 or (bwd is not None and min(bwd.stride(0), bwd.stride(1)) < 1):
        raise RuntimeError(f"{what}: field and channel strides must be positive (fwd {fwd.stride()}, bwd {None if bwd is None else bwd.stride()})")
    if alpha != alpha or beta != beta:
        raise RuntimeError(f"{what}: alpha / beta is NaN")
    sxy = sst = None
    if state is None:
        P = h * w
        if start is not None:
            raise RuntimeError(f"{what}: dense mode (state=None) starts every point at once; `start` needs a state")
    else:
        sxy, sst = state
        for t, name, dt in ((sxy, "state xy", torch.float32), (sst, "state status", torch.uint8)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev or t.dtype != dt or not t.is_contiguous():
                raise RuntimeError(f"{what}: {name} must be a contiguous {dt} tensor on {dev} (got {getattr(t, 'dtype', type(t).__name__)} on "
                                   f"{getattr(t, 'device', None)}); there is no CPU fallback")
        if sxy.dim() != 2 or sxy.shape[0] != 2 or sxy.shape[1] < 1 or tuple(sst.shape) != (sxy.shape[1],):
            raise RuntimeError(f"{what}: state must be (xy [2, P], status [P]), got {tuple(sxy.shape)} and {tuple(sst.shape)}")
        P = int(sxy.shape[1])
        if start is not None and (not isinstance(start, torch.Tensor) or start.device != dev or start.dtype != torch.int32
                                  or tuple(start.shape) != (P,) or not start.is_contiguous()):
            raise RuntimeError(f"{what}: start must be contiguous int32 [{P}] on {dev} (got {getattr(start, 'dtype', None)} "
                               f"{tuple(getattr(start, 'shape', ()))})")
    lib = _track_lib.load()
    xy = torch.empty(K, 2, P, dtype=torch.float32, device=dev)
    status = torch.empty(K, P, dtype=torch.uint8, device=dev)
    cnt = torch.empty(K, 4, dtype=torch.int32, device=dev) if counts else None
    b = bwd if bwd is not None else fwd
    _track_lib.check(lib.sft_track_advance(fwd.data_ptr(), fwd.stride(0), fwd.stride(1), fwd.stride(2),
                                           None if bwd is None else bwd.data_ptr(), b.stride(0), b.stride(1), b.stride(2), K, h, w,
                                           int(frame0), None if sxy is None else sxy.data_ptr(), None if sst is None else sst.data_ptr(),
                                           None if start is None else start.data_ptr(), P, float(alpha), float(beta), int(bool(sticky)),
                                           xy.data_ptr(), status.data_ptr(), None, None, None if cnt is None else cnt.data_ptr(), None, 0,
                                           _track_lib.stream()), "sft_track_advance")
    new_state = (xy[K - 1], status[K - 1])
    return (xy, status, new_state, cnt) if counts else (xy, status, new_state)


@on_tensor_device
def draw_tracks(frames: torch.Tensor, xy: torch.Tensor, status: torch.Tensor, first_frame: int, trail: int = 16, radius: int = 3,
                trail_radius: int = 1, palette: Optional[torch.Tensor] = None, draw_occluded: bool = False, first_row: int = 0,
                alpha_table: Optional[torch.Tensor] = None, channels_last: Optional[bool] = None) -> torch.Tensor:
    """Tracks drawn on frames (sft_draw_tracks: a key image per frame, atomic maxima, then a blend; bitwise reproducible).  frames
    uint8 [n, H, W, 3] or [n, 3, H, W] on the GPU, any strides; frames[j] is frame first_frame + j of the video.  xy fp32 [N, 2, P],
    status uint8 [N, P] contiguous: row r describes frame first_row + r (track_advance's rows, stacked).  Every frame shows each
    point's last `trail` samples: a disc of `radius` at the newest, discs of `trail_radius` joined by lines behind it.  palette uint8
    [L, 3] (default: track.default_palette), alpha_table uint8 [trail] (default: track.alpha_fade).  Returns uint8 [n, H, W, 3].
    Enqueued on the current stream, no synchronisation."""
    from . import _track_lib, track
    what = "draw_tracks"
    for t, name, dt in ((xy, "xy", torch.float32), (status, "status", torch.uint8)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} must be a contiguous {dt} tensor on the GPU (got {getattr(t, 'dtype', type(t).__name__)} on "
                               f"{getattr(t, 'device', None)}); there is no CPU fallback")
    if xy.dim() != 3 or xy.shape[1] != 2 or xy.numel() == 0 or tuple(status.shape) != (xy.shape[0], xy.shape[2]) or status.device != xy.device:
        raise RuntimeError(f"{what}: xy must be [N, 2, P] and status [N, P] on one GPU, got {tuple(xy.shape)} and {tuple(status.shape)}")
    dev = xy.device
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.shape[0] < 1:
        raise RuntimeError(f"{what}: frames must be uint8 [n, H, W, 3] or [n, 3, H, W] on the GPU")
    if channels_last is None:
        channels_last = frames.shape[3] == 3
    n = int(frames.shape[0])
    h, w = (int(v) for v in (frames.shape[1:3] if channels_last else frames.shape[2:]))
    s = _frame_strides(frames, "frames", channels_last, (h, w), n, dev, what)
    N, P = int(xy.shape[0]), int(xy.shape[2])
    trail, radius, trail_radius = int(trail), int(radius), int(trail_radius)
    if not 1 <= trail <= _track_lib.DRAW_MAX_TRAIL or not 0 <= radius <= _track_lib.DRAW_MAX_RADIUS or not 0 <= trail_radius <= _track_lib.DRAW_MAX_RADIUS:
        raise RuntimeError(f"{what}: trail {trail} (1 .. {_track_lib.DRAW_MAX_TRAIL}), radius {radius} / trail_radius {trail_radius} "
                           f"(0 .. {_track_lib.DRAW_MAX_RADIUS})")
    if P > _track_lib.DRAW_MAX_POINTS:
        raise RuntimeError(f"{what}: {P} points (at most {_track_lib.DRAW_MAX_POINTS} can be drawn)")
    if palette is None:
        palette = torch.from_numpy(track.default_palette()).to(dev)
    if alpha_table is None:
        alpha_table = torch.from_numpy(track.alpha_fade(trail)).to(dev)
    for t, name, shape in ((palette, "palette", (-1, 3)), (alpha_table, "alpha_table", (trail,))):
        ok = isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.uint8 and t.is_contiguous() and t.numel() > 0
        if not ok or (name == "palette" and (t.dim() != 2 or t.shape[1] != 3)) or (name == "alpha_table" and tuple(t.shape) != shape):
            raise RuntimeError(f"{what}: {name} must be contiguous uint8 {'[L, 3]' if name == 'palette' else [trail]} on {dev}")
    lib = _track_lib.load()
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
    ws = torch.empty(int(lib.sft_draw_tracks_ws_bytes(n, h, w)), dtype=torch.uint8, device=dev)
    _track_lib.check(lib.sft_draw_tracks(frames.data_ptr(), s[0], s[1], s[2], s[3], n, h, w, int(first_frame), xy.data_ptr(), status.data_ptr(),
                                         N, P, int(first_row), trail, radius, trail_radius, int(bool(draw_occluded)), palette.data_ptr(),
                                         int(palette.shape[0]), alpha_table.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _track_lib.stream()), "sft_draw_tracks")
    return out
