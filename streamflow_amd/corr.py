"""A correlation store in one of the four storage forms (CorrPlan, CorrStore) and CorrBlock with the reference's interface
(core/corr.py:6-54) on top of it, backed by the HIP kernels."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import torch

from . import ops
from .ops import Planes

FORMS = ("direct", "blocked16", "blocked32", "rows")


@dataclass(frozen=True)
class CorrPlan:
    """How the correlation features of a set of frame pairs are stored and handed over.
    form: 'direct' = no volume, the packed features of every pair and the cells computed at every lookup (csrc/corr_direct.hip);
    'blocked16' = fp16 cells in 8 x 8-cell blocks (csrc/corr_blocked.hip); 'blocked32' = fp32 cells in blocks of 4 rows x 8 columns
    (csrc/corr_blocked32.hip); 'rows' = row-major maps per level, fp32 rows pitched to cache lines (csrc/corr.hip)."""
    form: str
    f16: bool          # fp16 cells; under 'direct' the one-product class (fp32: the three-product class)
    koct_out: bool     # the lookup hands the 324 features over as fp16 k-octet planes ONLY (no fp32 planes exist)
    prec = property(lambda self: ops.PRECISION_F16 if self.f16 else ops.PRECISION_F16X3)


class CorrStore:
    """The correlation buffers of `B` clips x `pairs` pairs of h x w feature maps (image = clip * pairs + pair) in the form of `plan`,
    their build and their lookup -- what CorrBlock runs on; HotPathEngine still issues the same calls itself (_Plan, _setup, _iteration).  vol: the BlockedVolume of the blocked forms;
    lvls / pair_stride / pitch: the four row-major maps of 'rows', their per-pair strides and row pitch in cells (ops.corr_pitch, fp32
    maps only); ws: the build's scratch or, under 'direct', the packed features themselves.  What a form does not have is None."""

    def __init__(self, plan: CorrPlan, B: int, pairs: int, D: int, h: int, w: int, device):
        if plan.form not in FORMS:
            raise RuntimeError(f"CorrStore: form must be one of {FORMS}, got {plan.form!r}")
        self.plan, self.B, self.pairs, self.D, self.h, self.w = plan, B, pairs, D, h, w
        n, N = B * pairs, h * w
        self.vol = self.lvls = self.pair_stride = self.pitch = None
        if plan.form == "direct":
            self.ws = torch.empty(ops.corr_direct_ws_bytes(B, pairs, D, h, w, plan.prec), dtype=torch.uint8, device=device)
        elif plan.form != "rows":
            # one buffer, blocks = cache lines
            f32 = plan.form == "blocked32"
            self.vol = ops.new_blocked_volume(n, h, w, device, f32=f32)
            self.ws = torch.empty(max(ops.corr_build_blocked_ws_bytes(n, D, h, w, f32), 16), dtype=torch.uint8, device=device)
        else:
            # fp32 maps: rows padded to whole cache lines where the dense layout would straddle them (ops.corr_pitch: KITTI's 156-cell
            # rows); fp16 cells (half the bytes of the HBM-bound build and lookups; BASELINE.json configs 2 and 5) stay dense
            self.pitch = None if plan.f16 else ops.corr_pitch(h, w)
            self.pair_stride = [B * N * (h >> l) * (self.pitch[l] if self.pitch else w >> l) for l in range(4)]
            self.lvls = [torch.empty(pairs * s, dtype=torch.float16 if plan.f16 else torch.float32, device=device)
                         for s in self.pair_stride]
            # scratch of the split-precision volume build: (hi, lo) fp16 planes of every f1 / f2 image
            self.ws = torch.empty(max(ops.corr_build_ws_bytes(B, pairs, D, h, w), 16), dtype=torch.uint8, device=device)

    def build(self, f1_ptr: int, f2_ptr: int, clip_stride: int, pair_stride: int, cx=None) -> None:
        """Once per clip, all pairs in one launch: the volumes (reference corr.py:13-21) or, under 'direct', f1 and the pooled pyramid
        of f2 in the operand format.  Strides of the features in floats."""
        B, pairs, D, h, w = self.B, self.pairs, self.D, self.h, self.w
        if self.plan.form == "direct":
            ops.corr_direct_pack(f1_ptr, f2_ptr, clip_stride, pair_stride, self.ws, B, pairs, D, h, w, self.plan.prec)
        elif self.plan.form != "rows":
            ops.corr_build_blocked(f1_ptr, f2_ptr, clip_stride, pair_stride, self.vol, B, pairs, D, ws=self.ws)
        else:
            ops.corr_build(f1_ptr, f2_ptr, clip_stride, pair_stride, self.lvls, self.pair_stride, B, pairs, D, h, w, ws=self.ws,
                           cx=cx, pitch=self.pitch)

    def lookup(self, coords: Planes, out: Planes, cx=None) -> None:
        """The 324 windowed features of every image at `coords` (corr.py:23-44) into `out`: the k-octet buffer itself under
        plan.koct_out, else fp32 planes, whose k-octet copy (out.shadow, if any) is current afterwards."""
        form, koct_out = self.plan.form, self.plan.koct_out
        if form == "rows":                         # (writes the copy itself where it can, refreshes it where it cannot)
            ops.corr_lookup(self.lvls, self.pair_stride, coords, out, self.B, self.pairs, self.h, self.w, cx=cx, pitch=self.pitch)
            return
        planes, koct = (None, out) if koct_out else (replace(out, shadow=None), None)
        if form == "direct":
            ops.corr_direct_lookup(self.ws, coords, planes, koct, self.B, self.pairs, self.D, self.h, self.w, self.plan.prec)
        else:
            ops.corr_lookup_blocked(self.vol, coords, planes, koct, self.B, self.pairs)
        if not koct_out:
            ops.refresh_shadow(out, cx)

    def pyramid(self) -> list:
        """The four levels as [pairs, B * N, h_l, w_l] -- per pair the reference's corr_pyramid[l] (corr.py:13-21) without its singleton
        dimension: strided VIEWS of the (possibly row-pitched) storage of 'rows', row-major COPIES of blocked volumes (tests and API
        parity only)."""
        B, pairs, h, w = self.B, self.pairs, self.h, self.w
        if self.plan.form == "direct":
            raise RuntimeError("this plan keeps no correlation volume (corr_direct): there is no 'volume' to tap")
        if self.plan.form != "rows":               # (image = clip * pairs + pair)
            return [t.view(B, pairs, h * w, h >> l, w >> l).permute(1, 0, 2, 3, 4).reshape(pairs, B * h * w, h >> l, w >> l)
                    for l, t in enumerate(self.vol.levels())]
        return [t.view(pairs, B * h * w, h >> l, self.pitch[l] if self.pitch else w >> l)[..., : w >> l]
                for l, t in enumerate(self.lvls)]

    def level_maps(self, l: int) -> torch.Tensor:
        """pyramid()[l]: free for 'rows' (views); blocked volumes unpack all four levels whichever is asked for (BlockedVolume.levels)."""
        return self.pyramid()[l]


class CorrBlock:
    """All-pairs correlation pyramid + windowed lookup for ONE frame pair.

    ``CorrBlock(fmap1, fmap2, num_levels=4, radius=4)`` builds ``corr_pyramid`` (list of
    ``[B*h*w, 1, h>>l, w>>l]`` tensors, reference corr.py:13-21) in a single fused kernel;
    ``blk(coords)`` returns ``[B, 4*81, h, w]`` float32 contiguous (corr.py:23-44).
    ``dtype=torch.float16`` (an extension; the reference always keeps fp32 volumes) stores the pyramid as fp16
    cells built with single f16 MFMA products -- the bf16/fp16 volume configurations of BASELINE.json.
    ``layout="rows"`` keeps row-major maps, fp32 rows with a pitch of a multiple of 32 cells where they would straddle cache lines;
    ``corr_pyramid`` is then the strided [..., :w_l] view of them: the reference's shape and values, no copy.
    ``layout="blocked"`` keeps them in cache-line blocks -- 8 x 8 fp16 cells (csrc/corr_blocked.hip) or 4 rows x 8 columns of
    fp32 cells (csrc/corr_blocked32.hip) -- what the fused engine uses; ``corr_pyramid`` is then a row-major COPY made on first access.
    ``layout="direct"`` keeps NO volume: the features are packed once (csrc/corr_direct.hip) and every call computes the cells its
    windows touch; ``dtype`` selects the class (float16: one fp16 product, float32: three split products).  ``corr_pyramid`` is then
    computed on first access by ``CorrBlock.corr`` and pooling (reference shapes, a copy).
    The buffers, the build and the lookup are a CorrStore's (``store``); its build scratch is allocated with it and kept.
    """

    @ops.on_tensor_device
    def __init__(self, fmap1: torch.Tensor, fmap2: torch.Tensor, num_levels: int = 4, radius: int = 4,
                 dtype: torch.dtype = torch.float32, layout: str = "rows"):
        if num_levels != 4 or radius != 4:
            raise RuntimeError("CorrBlock: the HIP path is built for num_levels=4, radius=4 "
                               "(the only values the StreamFlow model uses, streamflow.py:38-39)")
        f1 = fmap1.contiguous().float()
        f2 = fmap2.contiguous().float()
        ops._dev_check(f1)
        ops._dev_check(f2)
        B, D, h, w = f1.shape
        self.num_levels, self.radius = num_levels, radius
        self.shape = (B, h, w)
        if dtype not in (torch.float32, torch.float16):
            raise RuntimeError(f"CorrBlock: volume dtype must be float32 or float16, got {dtype}")
        if layout not in ("rows", "blocked", "direct"):
            raise RuntimeError("CorrBlock: layout must be 'rows', 'blocked' or 'direct'")
        f16 = dtype == torch.float16
        form = {"rows": "rows", "blocked": "blocked16" if f16 else "blocked32", "direct": "direct"}[layout]
        self._keep = (f1, f2)
        self._pyr = None
        self.store = CorrStore(CorrPlan(form, f16, koct_out=False), B, 1, D, h, w, f1.device)     # (fp32 planes out: the reference's)
        self.store.build(f1.data_ptr(), f2.data_ptr(), D * h * w, 0)

    vol = property(lambda self: self.store.vol)
    direct_ws = property(lambda self: self.store.ws if self.store.plan.form == "direct" else None)

    @property
    def corr_pyramid(self):
        if self._pyr is None and self.store.plan.form == "direct":   # no volume is kept: the reference's own construction, on first access
            B, h, w = self.shape
            c = CorrBlock.corr(*self._keep).reshape(B * h * w, 1, h, w)
            self._pyr = [c]
            for _ in range(3):
                self._pyr.append(torch.nn.functional.avg_pool2d(self._pyr[-1], 2, stride=2))
        if self._pyr is None:                                        # reference shapes: the store's one pair in the singleton dimension
            self._pyr = [t.transpose(0, 1) for t in self.store.pyramid()]
        return self._pyr

    @ops.on_tensor_device
    def __call__(self, coords: torch.Tensor) -> torch.Tensor:
        B, h, w = self.shape
        c = coords.contiguous().float()
        ops._dev_check(c)
        assert tuple(c.shape) == (B, 2, h, w), (c.shape, self.shape)
        out = torch.empty(B, 4 * 81, h, w, dtype=torch.float32, device=c.device)
        self.store.lookup(Planes.of(c), Planes.of(out))
        return out

    @staticmethod
    @ops.on_tensor_device
    def corr(fmap1: torch.Tensor, fmap2: torch.Tensor) -> torch.Tensor:
        """[B,h,w,1,h,w] = f1^T f2 / sqrt(D) (corr.py:46-54)."""
        f1 = fmap1.contiguous().float()
        f2 = fmap2.contiguous().float()
        ops._dev_check(f1)
        ops._dev_check(f2)
        B, D, h, w = f1.shape
        N = h * w
        out = torch.empty(B, N, N, dtype=torch.float32, device=f1.device)
        ops.gemm_raw(A=f1.data_ptr(), B=f2.data_ptr(), C=out.data_ptr(), M=N, N=N, K=D, batch=B, lda=N, ldb=N, ldc=N,
                     strideA=D * N, strideB=D * N, strideC=N * N, a_layout=ops.LAYOUT_K_MAJOR,
                     b_layout=ops.LAYOUT_K_MAJOR, alpha=1.0 / math.sqrt(D), epilogue=ops.EPI_NONE)
        return out.view(B, h, w, 1, h, w)
