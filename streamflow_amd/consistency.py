"""Forward-backward consistency of the flows of a video: occlusion masks, frames warped back, and a report for footage without
ground truth.

The check is the one of Sundaram et al. 2010 with the constants of UnFlow (Meister et al. 2018): a pixel is visible when the
backward flow, sampled where the forward flow points, leads back to within  |f + b|^2 <= alpha (|f|^2 + |b|^2) + beta;  the constants
are theirs (0.01, 0.5), not tuned here.  Everything per pixel is the two kernels of csrc/flow_consistency.hip
(ops.flow_consistency, ops.warp_frames), a whole batch of pairs per call; the backward flows come from
video.predict_video(..., bidirectional=True); streamflow_amd.interpolate splats frames in between along the same flows.  Out of
scope: scoring the masks against ground-truth occlusion maps.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import torch

ALPHA, BETA = 0.01, 0.5
MASK_CODES = (255, 0, 128)          # visible, occluded, outside: the class map as an 8-bit grey image
DIRECTIONS = ("forward", "backward")


def check_pairs(fwd: torch.Tensor, bwd: torch.Tensor, alpha: float = ALPHA, beta: float = BETA, codes: Sequence[int] = (0, 1, 2),
                stats: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """Both directions of the check for k pairs: fwd, bwd fp32 [k, 2, H, W] on the GPU (bwd[j]: frame j + 1 -> frame j).  The kernel
    runs twice with the arguments swapped.  Returns ((cls_f, stats_f), (cls_b, stats_b)): cls_f classifies the pixels of frame j
    (occluded = not seen in frame j + 1), cls_b those of frame j + 1; stats = a pair of float64 [k, ops.FBC_LEN] to ADD to."""
    from . import ops
    sf, sb = (None, None) if stats is None else stats
    return (ops.flow_consistency(fwd, bwd, alpha, beta, codes, stats=sf), ops.flow_consistency(bwd, fwd, alpha, beta, codes, stats=sb))


def warp_back(frames: torch.Tensor, fwd: torch.Tensor, cls: Optional[torch.Tensor] = None, visible: int = 0, reverse: bool = False,
              stats: Optional[torch.Tensor] = None):
    """frames uint8 [k + 1, H, W, 3] (or [k + 1, 3, H, W]) on the GPU, fwd [k, 2, H, W]: frame j + 1 warped onto frame j, uint8
    [k, H, W, 3].  With `cls` (check_pairs' map of the same flows, `visible` its byte for visible pixels) also the photometric error
    against frame j over visible pixels: returns (warped, stats float64 [k, ops.WARP_LEN]), stats None without cls.
    reverse=True: `fwd` holds the backward flows and frame j is warped onto frame j + 1."""
    from . import ops
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.shape[0] != fwd.shape[0] + 1:
        raise RuntimeError(f"warp_back: {tuple(fwd.shape)} flows need one frame more, got frames {tuple(getattr(frames, 'shape', ()))}")
    src, ref = (frames[:-1], frames[1:]) if reverse else (frames[1:], frames[:-1])
    return ops.warp_frames(src, fwd, cls=cls, ref=None if cls is None else ref, stats=stats, visible=visible)


def report_from(fbc: torch.Tensor, warp: torch.Tensor, pairs: int) -> dict:
    """One direction's entries from the summed stats rows (host or device tensors of ops.FBC_LEN and ops.WARP_LEN doubles)."""
    from . import ops
    f, w = [float(v) for v in fbc.reshape(-1).cpu()], [float(v) for v in warp.reshape(-1).cpu()]
    px = f[ops.FBC_PIXELS]
    share = lambda v: v / px if px else float("nan")
    mean = lambda s, c: s / c if c else float("nan")
    return {"pairs": int(pairs), "pixels": int(px),
            "visible": share(f[ops.FBC_VISIBLE]), "occluded": share(f[ops.FBC_OCCLUDED]), "outside": share(f[ops.FBC_OUTSIDE]),
            "fb_error": mean(f[ops.FBC_SUM_FB], f[ops.FBC_VISIBLE]),
            "mean_flow": mean(f[ops.FBC_SUM_MAG], f[ops.FBC_FINITE]),
            "photo_error": mean(w[ops.WARP_SUM_ABS], w[ops.WARP_TERMS])}


def report_line(name: str, r: dict) -> str:
    return ("Consistency (%s) pairs: %d, visible: %f, occluded: %f, outside: %f, fb error: %f, flow: %f, photo error: %f"
            % (name, r["pairs"], r["visible"], r["occluded"], r["outside"], r["fb_error"], r["mean_flow"], r["photo_error"]))


class ReportSink:
    """A predict_video(bidirectional=True) sink that keeps nothing but two summed stats rows per direction (on the device, no host
    synchronisation); `then(first_pair, fwd, bwd, frames, (cls_f, cls_b), (warped_f, warped_b))`, when given, sees every batch
    with its class maps (codes = MASK_CODES) and warped frames.  report() copies the sums to the host: the one synchronisation."""

    def __init__(self, alpha: float = ALPHA, beta: float = BETA, then: Optional[Callable] = None):
        self.alpha, self.beta, self.then = alpha, beta, then
        self.pairs, self.fbc, self.warp = 0, None, None

    def __call__(self, first_pair: int, fwd: torch.Tensor, bwd: torch.Tensor, frames: torch.Tensor) -> None:
        from . import ops
        if self.fbc is None:
            self.fbc = torch.zeros(2, ops.FBC_LEN, dtype=torch.float64, device=fwd.device)
            self.warp = torch.zeros(2, ops.WARP_LEN, dtype=torch.float64, device=fwd.device)
        (cls_f, st_f), (cls_b, st_b) = check_pairs(fwd, bwd, self.alpha, self.beta, MASK_CODES)
        warped_f, ph_f = warp_back(frames, fwd, cls_f, visible=MASK_CODES[0])
        warped_b, ph_b = warp_back(frames, bwd, cls_b, visible=MASK_CODES[0], reverse=True)
        self.fbc += torch.stack([st_f.sum(0), st_b.sum(0)])
        self.warp += torch.stack([ph_f.sum(0), ph_b.sum(0)])
        self.pairs += int(fwd.shape[0])
        if self.then is not None:
            self.then(first_pair, fwd, bwd, frames, (cls_f, cls_b), (warped_f, warped_b))

    def report(self) -> dict:
        if self.fbc is None:
            raise RuntimeError("consistency.ReportSink: no batch has been seen")
        fbc, warp = self.fbc.cpu(), self.warp.cpu()
        return {name: report_from(fbc[i], warp[i], self.pairs) for i, name in enumerate(DIRECTIONS)}


def video_report(model: Callable, frames, T: int = 4, iters: Optional[int] = None, clips_per_step: int = 8, mode: str = "sintel",
                 alpha: float = ALPHA, beta: float = BETA, device=None, verbose: bool = True) -> dict:
    """How consistent the model's flows are on a video without ground truth: predict_video(..., bidirectional=True) through a sink
    that checks every batch in both directions, warps the neighbouring frame back and keeps only the stats rows; one synchronisation
    with the host at the end.  Returns {"forward": {...}, "backward": {...}}, each with pairs, pixels, the visible / occluded /
    outside shares, `fb_error` (mean |f + b| over visible pixels, in pixels), `mean_flow` (mean flow magnitude) and `photo_error`
    (mean absolute difference between frame and warped neighbour over visible pixels and channels, in 0 .. 255 units); prints one
    line per direction."""
    from . import video
    sink = ReportSink(alpha, beta)
    video.predict_video(model, frames, T=T, iters=iters, clips_per_step=clips_per_step, mode=mode, device=device, sink=sink,
                        bidirectional=True)
    rep = sink.report()
    if verbose:
        for name in DIRECTIONS:
            print(report_line(name, rep[name]))
    return rep
