"""Encoders: the reference's ``Twins_CSC`` on the HIP kernels, plus two stand-ins for plumbing and tests.

``Twins_CSC`` (reference core/encoders/twins_csc.py:14-85) = the first two stages of timm's
``twins_svt_large`` run over the T frames of a clip concatenated along the height.  timm is not in the image and is
unpinned upstream, so its published arithmetic (``timm/models/twins.py``: LocallyGroupedAttn, GlobalSubSampleAttn,
Block, PosConv) is restated -- that boundary is "parity unpinned", exactly like the temporal block; what IS pinned is
the reference's own PatchEmbed / stage loop (golden vectors from the reference's ``Twins_CSC.forward``) and the
checkpoint key names / shapes (``svt.patch_embeds.*``, ``svt.blocks.*``, ``svt.pos_block.*``, ``svt.norm.*``: strict load).
Every Linear and strided conv runs through ``sf_gemm``, LayerNorms through ``sf_layernorm_cm``, the attention cores and the
positional conv through the kernels of ``csrc/encoder.hip``; torch is used for memory reordering (im2col) only.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F


class InjectEncoder(nn.Module):
    """Returns the tensor stored in `.features` ([B,T,256,h,w]), sliced to the number of frames it is called
    with.  Used by parity tests to feed identical features to the reference and to this build."""

    def __init__(self, args=None, norm_fn=None):
        super().__init__()
        self.features = None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.features is None:
            raise RuntimeError("InjectEncoder.features is not set")
        return self.features[:, : x.shape[1]]


class PatchEncoder(nn.Module):
    """Deterministic 8x8 patch embedding (+ a temporal mix) in plain PyTorch -- NOT Twins_CSC, plumbing only."""

    def __init__(self, args=None, norm_fn=None, out_dim: int = 256):
        super().__init__()
        g = torch.Generator().manual_seed(1234)
        self.register_buffer("proj", torch.randn(out_dim, 3, 8, 8, generator=g) / (3 * 64) ** 0.5, persistent=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, T, C, H, W = x.shape
        f = F.conv2d(x.reshape(B * T, C, H, W).float(), self.proj, stride=8)
        return f.view(B, T, -1, H // 8, W // 8)


# ---- Twins_CSC ---------------------------------------------------------------------------------------------------------------
class _PatchEmbed(nn.Module):
    """reference twins_csc.py:14-34 (parameter holder; the forward below uses the kernels)."""

    def __init__(self, patch_size: int, in_chans: int, embed_dim: int):
        super().__init__()
        self.patch_size = patch_size
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.norm = nn.LayerNorm(embed_dim)


class _Mlp(nn.Module):
    def __init__(self, dim: int, hidden: int):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class _LocalAttn(nn.Module):          # timm LocallyGroupedAttn: qkv, proj
    def __init__(self, dim: int):
        super().__init__()
        self.qkv = nn.Linear(dim, dim * 3, bias=True)
        self.proj = nn.Linear(dim, dim)


class _GlobalAttn(nn.Module):         # timm GlobalSubSampleAttn: q, kv, proj, sr, norm
    def __init__(self, dim: int, sr: int):
        super().__init__()
        self.q = nn.Linear(dim, dim, bias=True)
        self.kv = nn.Linear(dim, dim * 2, bias=True)
        self.proj = nn.Linear(dim, dim)
        self.sr = nn.Conv2d(dim, dim, kernel_size=sr, stride=sr)
        self.norm = nn.LayerNorm(dim)


class _Block(nn.Module):
    def __init__(self, dim: int, sr: int, local: bool):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _LocalAttn(dim) if local else _GlobalAttn(dim, sr)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, 4 * dim)


class _PosConv(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.proj = nn.Sequential(nn.Conv2d(dim, dim, 3, 1, 1, bias=True, groups=dim))


class _Svt(nn.Module):
    """What is left of timm's twins_svt_large after twins_csc.py:42-57: two stages + the (unused) final norm."""

    def __init__(self):
        super().__init__()
        dims, srs, patch = (128, 256), (8, 4), (4, 2)
        self.patch_embeds = nn.ModuleList([_PatchEmbed(patch[0], 3, dims[0]), _PatchEmbed(patch[1], dims[0], dims[1])])
        self.blocks = nn.ModuleList([nn.ModuleList([_Block(d, sr, local=(j == 0)) for j in range(2)]) for d, sr in zip(dims, srs)])
        self.pos_block = nn.ModuleList([_PosConv(d) for d in dims])
        self.norm = nn.LayerNorm(1024, eps=1e-6)              # kept by the reference (never applied): checkpoint key


def _im2col(grid: torch.Tensor, k: int) -> torch.Tensor:
    """[B,C,GH,GW] -> [B, C*k*k, (GH//k)*(GW//k)]: the columns of a k x k / stride k conv (rows ordered c, ky, kx like the
    flattened conv weight; a remainder of the grid is dropped like F.conv2d drops it).  Memory reordering only."""
    B, C, GH, GW = grid.shape
    oh, ow = GH // k, GW // k
    g = grid[:, :, : oh * k, : ow * k].reshape(B, C, oh, k, ow, k).permute(0, 1, 3, 5, 2, 4)
    return g.reshape(B, C * k * k, oh * ow).contiguous()


class Twins_CSC(nn.Module):
    """``Twins_CSC(args, norm_fn=...)(x [B,T,3,H,W] in [-1,1]) -> [B,T,256,H/8,W/8]`` (reference twins_csc.py:37-85).
    The reference passes `args` in the `pretrained` slot (streamflow.py:45 vs twins_csc.py:38) and would try to load
    ./pretrained/twins_svt_large-90f6aaa9.pth; weights here come from the StreamFlow checkpoint (`fnet.svt.*`)."""

    DIMS, HEADS, SRS, PATCH, WS = (128, 256), (4, 8), (8, 4), (4, 2), 7

    def __init__(self, pretrained=False, args=None, **kwargs):
        super().__init__()
        self.svt = _Svt()
        self._pack = None
        self._pack_key = None
        self.koct_handover = True        # fp16 k-octet hand-over between the kernels in the two-product / fp16 classes
        self.exact_attention = False     # the exact-fp32 VALU attention cores in every class (tests)

    def _packed(self, device):
        from . import ops
        key = (str(device),) + tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._pack_key != key:
            f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()
            pk = {}
            for n, m in self.svt.named_modules():
                if isinstance(m, nn.Linear) or (isinstance(m, nn.Conv2d) and m.groups == 1):
                    pk[n] = ops.PackedLinear(m.weight, m.bias, device)
                elif isinstance(m, nn.Conv2d):               # depthwise 3x3
                    pk[n] = (f32(m.weight.reshape(m.weight.shape[0], 9)), f32(m.bias))
                elif isinstance(m, nn.LayerNorm):
                    pk[n] = (f32(m.weight), f32(m.bias), float(m.eps))
            pk["qkv_bias"] = [f32(self.svt.blocks[i][0].attn.qkv.bias) for i in range(2)]
            self._pack, self._pack_key = pk, key
        return self._pack

    @torch.no_grad()
    def forward(self, x: torch.Tensor, precision=None, taps=None) -> torch.Tensor:
        """precision: 'fp32' | 'f16x3' | 'f16x2' | 'f16' (or the integer constant): the arithmetic class of this call; None = the
        package default (ops.PRECISION).  Passed explicitly to every launch: the module keeps no launch state.
        taps: a dict that receives clones of the fp32 token planes, each [B, E_i, gh_i, gw_i], at four points of stage i:
        'embed{i}' (after the patch-embed LayerNorm), 'block{i}.0', 'peg{i}', 'block{i}.1' (tests; nothing else is launched differently)."""
        from . import ops
        from .ops import EPI_GELU, EPI_NONE, EPI_RES, Planes
        prec = ops.PRECISION if precision is None else (ops._PRECISION_NAMES[precision] if isinstance(precision, str) else int(precision))
        cx0 = ops.Ctx(prec)
        x = x.float().contiguous()
        ops._dev_check(x)
        B, T, C, H, W = x.shape
        if H % 8 or W % 8:
            raise RuntimeError("Twins_CSC: H and W must be multiples of 8")
        dev = x.device
        with torch.cuda.device(dev):
            pk = self._packed(dev)
            new = lambda rows, n: Planes.of(torch.empty(B, rows, n, dtype=torch.float32, device=dev))
            # fp16 k-octet planes [rows/8][n][8] (ops.Planes.koct): in the two-product / fp16 classes every tensor that only
            # feeds a GEMM (LayerNorm outputs, attention outputs, the MLP hidden) is handed over as the consumer's operand
            # image, exactly as in the refinement loop; the fp32-class modes keep fp32 planes throughout
            handover = prec in (ops.PRECISION_F16X2, ops.PRECISION_F16) and (T * H * W) % 256 == 0 and self.koct_handover

            # the exact VALU attention cores read and write fp32 planes only: their qkv input and output are never k-octets
            attn_koct = not self.exact_attention

            def tap(name, X):
                if taps is not None:
                    taps[name] = X.tensor().view(B, X.rows, gh, gw).clone()

            def newk(rows, n, koct=True):
                if not (handover and koct):
                    return new(rows, n)
                assert rows % 8 == 0
                return Planes(torch.empty(B * rows * n // 2, dtype=torch.float32, device=dev), 0, rows * n, B, rows, n,
                              f16=True, koct=True)

            def ln(X, name, koct=False):
                w, b, eps = pk[name]
                Y = newk(X.rows, X.P) if koct else new(X.rows, X.P)
                ops.layernorm_cm(X, w, b, Y, eps)
                return Y

            def lin(name, X, epi=EPI_NONE, R=None, koct=False):
                A = pk[name]
                Y = newk(A.M, X.P) if koct else new(A.M, X.P)
                need = ops.gemm_split_ws_floats(A.M, X.P, A.K, B, cx=cx0)   # skinny outputs over a deep K (the sr convs): split-K
                ws = torch.empty(need, dtype=torch.float32, device=dev) if need else None
                ops.gemm(A, X, Y, epi, R=R, cx=ops.Ctx(prec, split_ws=ws))
                return Y

            grid = x.permute(0, 2, 1, 3, 4).reshape(B, C, T * H, W)     # frames stacked along the height (twins_csc.py:30-32)
            gh, gw = T * H, W
            for i in range(2):
                E, heads, sr, k = self.DIMS[i], self.HEADS[i], self.SRS[i], self.PATCH[i]
                gh, gw = gh // k, gw // k
                N = gh * gw
                tok = ln(lin(f"patch_embeds.{i}.proj", Planes.of(_im2col(grid, k))), f"patch_embeds.{i}.norm")
                tap(f"embed{i}", tok)
                # block 0: locally grouped (7x7 window) attention + MLP, both residual
                b0 = f"blocks.{i}.0"
                qkv = lin(b0 + ".attn.qkv", ln(tok, b0 + ".norm1", koct=True), koct=attn_koct)
                att = newk(E, N, attn_koct)
                ops.window_attn(qkv, pk["qkv_bias"][i], att, heads, gh, gw, self.WS, cx=cx0, exact=self.exact_attention)
                tok = lin(b0 + ".attn.proj", att, EPI_RES, R=tok)
                tok = lin(b0 + ".mlp.fc2", lin(b0 + ".mlp.fc1", ln(tok, b0 + ".norm2", koct=True), EPI_GELU, koct=True), EPI_RES, R=tok)
                tap(f"block{i}.0", tok)
                # positional conv after the first block (twins_csc.py:73-74)
                pw, pb = pk[f"pos_block.{i}.proj.0"]
                peg = new(E, N)
                ops.dwconv3x3_res(tok, pw, pb, peg, gh, gw)
                tok = peg
                tap(f"peg{i}", tok)
                # block 1: global sub-sampled attention + MLP
                b1 = f"blocks.{i}.1"
                y = ln(tok, b1 + ".norm1")
                q = lin(b1 + ".attn.q", y)
                s = lin(b1 + ".attn.sr", Planes.of(_im2col(y.tensor().view(B, E, gh, gw), sr)))
                kv = lin(b1 + ".attn.kv", ln(s, b1 + ".attn.norm"))
                att = newk(E, N, attn_koct)
                ops.subsample_attn(q, kv, att, heads, cx=cx0, exact=self.exact_attention)
                tok = lin(b1 + ".attn.proj", att, EPI_RES, R=tok)
                tok = lin(b1 + ".mlp.fc2", lin(b1 + ".mlp.fc1", ln(tok, b1 + ".norm2", koct=True), EPI_GELU, koct=True), EPI_RES, R=tok)
                tap(f"block{i}.1", tok)
                grid = tok.tensor().view(B, E, gh, gw)
            h, w = H // 8, W // 8
            return grid.view(B, self.DIMS[1], T, h, w).permute(0, 2, 1, 3, 4).contiguous()


ENCODERS = {"InjectEncoder": InjectEncoder, "PatchEncoder": PatchEncoder, "Twins_CSC": Twins_CSC}
