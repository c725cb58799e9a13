"""Frame interpolation of a video from its bidirectional flows: slow motion and frame-rate conversion on the GPU.

The frame at time t between frames j and j + 1 is made by forward splatting (ops.frame_interp, csrc/frame_interp.hip): the pixels
of frame j are pushed along t * (forward flow), those of frame j + 1 along (1 - t) * (backward flow), and what lands on a target
pixel is averaged with integer bilinear weights; the two sides are cross-faded by t.  With `masks` the forward-backward consistency
classes (consistency.check_pairs) choose the importance of a source pixel: occluded pixels, which have no counterpart in the other
frame and whose flow is a guess, weigh 1 where visible ones weigh 16, so they fill a target only where nothing better lands.

Limits: there is no refinement network behind the splat, and targets that nothing reaches (holes) are filled by cross-fading the two
frames in place.  All sums are integer, so the frames are bitwise reproducible and do not depend on the batching.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import torch

IMPORTANCE = (16, 1, 16)            # visible, occluded, outside (a pixel that leaves frame j + 1 may still be inside at time t)
COVER_NAMES = ("both", "a_only", "b_only", "holes")


def _check_factor(factor, what: str) -> int:
    from . import ops
    if not isinstance(factor, int) or isinstance(factor, bool) or not 2 <= factor <= ops.INTERP_MAX_DEN:
        raise ValueError(f"{what}: factor must be an integer 2 .. {ops.INTERP_MAX_DEN}, got {factor!r}")
    return factor


def between(frames: torch.Tensor, fwd: torch.Tensor, bwd: torch.Tensor, factor: int, masks: bool = True,
            importance: Sequence[int] = IMPORTANCE):
    """The factor - 1 frames between every two frames: frames uint8 [k + 1, H, W, 3] (or [k + 1, 3, H, W]) on the GPU, fwd, bwd fp32
    [k, 2, H, W] (bwd[j]: frame j + 1 -> frame j, as predict_video(bidirectional=True) returns them).  Returns (uint8
    [k, factor - 1, H, W, 3]: entry [j, i - 1] is the frame at time i / factor between frames j and j + 1; stats float64
    [k, factor - 1, ops.INTERP_LEN]).  masks=True: consistency.check_pairs runs first and both class maps go to the splat."""
    from . import consistency, ops
    factor = _check_factor(factor, "between")
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.shape[0] != fwd.shape[0] + 1:
        raise RuntimeError(f"between: {tuple(fwd.shape)} flows need one frame more, got frames {tuple(getattr(frames, 'shape', ()))}")
    cls = None
    if masks:
        (cls_f, _), (cls_b, _) = consistency.check_pairs(fwd, bwd)
        cls = (cls_f, cls_b)
    outs, rows = [], []
    for i in range(1, factor):
        out, _, st = ops.frame_interp(frames[:-1], frames[1:], fwd, bwd, i, factor, cls=cls, importance=importance)
        outs.append(out)
        rows.append(st)
    return torch.stack(outs, dim=1), torch.stack(rows, dim=1)


def _hwc(frames: torch.Tensor) -> torch.Tensor:
    return frames if frames.shape[3] == 3 else frames.permute(0, 2, 3, 1)


class InterpSink:
    """A predict_video(bidirectional=True) sink: for every batch `emit(first_output_index, frames uint8 [m, H, W, 3])` in video
    order -- frame j, then its factor - 1 intermediates, and so on; finish() emits the very last frame of the video once.  The
    summed stats stay on the device; report() copies them to the host (the one synchronisation) and returns the shares of the four
    cover codes over all interpolated pixels."""

    def __init__(self, factor: int, emit: Callable, masks: bool = True, importance: Sequence[int] = IMPORTANCE):
        self.factor, self.emit, self.masks, self.importance = _check_factor(factor, "InterpSink"), emit, masks, importance
        self.stats, self.last, self.next = None, None, 0

    def __call__(self, first_pair: int, fwd: torch.Tensor, bwd: torch.Tensor, frames: torch.Tensor) -> None:
        mid, st = between(frames, fwd, bwd, self.factor, self.masks, self.importance)
        k = int(fwd.shape[0])
        seq = torch.cat([_hwc(frames)[:-1].unsqueeze(1), mid], dim=1).reshape(k * self.factor, *mid.shape[2:])
        self.stats = st.sum((0, 1)) if self.stats is None else self.stats + st.sum((0, 1))
        self.last = _hwc(frames)[-1:].clone()                             # (the batch's frame buffer may be reused)
        self.next = (first_pair + k) * self.factor
        self.emit(first_pair * self.factor, seq)

    def finish(self) -> None:
        if self.last is None:
            raise RuntimeError("interpolate.InterpSink: no batch has been seen")
        self.emit(self.next, self.last)
        self.last = None

    def report(self) -> dict:
        from . import ops
        if self.stats is None:
            raise RuntimeError("interpolate.InterpSink: no batch has been seen")
        s = [float(v) for v in self.stats.cpu()]
        px = s[ops.INTERP_PIXELS]
        rep = {"pixels": int(px)}
        for name, k in zip(COVER_NAMES, (ops.INTERP_BOTH, ops.INTERP_A_ONLY, ops.INTERP_B_ONLY, ops.INTERP_HOLES)):
            rep[name] = s[k] / px if px else float("nan")
        return rep


def report_line(r: dict) -> str:
    return ("Interpolation cover, pixels: %d, both: %f, first only: %f, second only: %f, holes: %f"
            % (r["pixels"], r["both"], r["a_only"], r["b_only"], r["holes"]))


def interpolate_video(model: Callable, frames, factor: int = 2, T: int = 4, iters: Optional[int] = None, clips_per_step: int = 8,
                      mode: str = "sintel", masks: bool = True, device=None, emit: Optional[Callable] = None):
    """`factor` times as many frames: video.predict_video(..., bidirectional=True) through an InterpSink.  frames as predict_video
    takes them (N of them).  Returns a uint8 device tensor [(N - 1) * factor + 1, H, W, 3] whose frames at multiples of `factor` are
    the input frames bit for bit; with `emit` the frames go to `emit(first_output_index, frames[m, H, W, 3])` batch by batch in order,
    nothing is kept and the result is None."""
    from . import video
    if factor == 1 or not isinstance(factor, int) or isinstance(factor, bool):
        raise ValueError(f"interpolate_video: factor must be an integer 2 .. 64, got {factor!r} (1 would return the video itself)")
    _check_factor(factor, "interpolate_video")
    n = len(frames)
    held = []

    def keep(first: int, batch: torch.Tensor) -> None:
        if not held:
            held.append(torch.empty((n - 1) * factor + 1, *batch.shape[1:], dtype=torch.uint8, device=batch.device))
        held[0][first:first + batch.shape[0]] = batch

    sink = InterpSink(factor, keep if emit is None else emit, masks)
    video.predict_video(model, frames, T=T, iters=iters, clips_per_step=clips_per_step, mode=mode, device=device, sink=sink,
                        bidirectional=True)
    sink.finish()
    return held[0] if emit is None else None
