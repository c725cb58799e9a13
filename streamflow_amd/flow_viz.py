"""Flow colour-wheel images with the reference's names (core/utils/flow_viz.py): ``make_colorwheel`` and ``flow_to_image``.

The colouring runs on the GPU (ops.flow_to_image, the sf_flow_to_image kernel of csrc/flow_viz.hip); this module is the
host-facing wrapper that takes what callers have -- a device tensor ``[2, H, W]`` or ``[N, 2, H, W]``, or the reference's
``[H, W, 2]`` numpy array / CPU tensor -- and returns a numpy uint8 image, so that ``Image.fromarray(flow_to_image(x))`` and
``flow_io.write_png(path, flow_to_image(x))`` work as with the reference.  There is no CPU colouring path: without a GPU the
call raises, like every other op of this package.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops

# (steps, channel that moves, rising?) of the six wheel segments R -> Y -> G -> C -> B -> M -> R (Baker et al., "A Database and
# Evaluation Methodology for Optical Flow", ICCV 2007; Scharstein's / Sun's 55-entry wheel)
_SEGMENTS = ((15, 1, True), (6, 0, False), (4, 2, True), (11, 1, False), (13, 0, True), (6, 2, False))


def make_colorwheel() -> np.ndarray:
    """[55, 3] float64 wheel (RGB, 0..255).  Along a segment one channel runs floor(255 i / steps) up from 0 or down from 255
    while the two others rest at the pure hue the segment starts from.  The kernel's table (csrc/flow_viz.hip: kWheel) holds
    these values; tests/test_flow_viz_cpu.py checks one against the other and both against the reference's wheel."""
    wheel = np.zeros((sum(s for s, _, _ in _SEGMENTS), 3), np.float64)
    hue = np.array([255.0, 0.0, 0.0])                                       # red
    row = 0
    for steps, ch, rising in _SEGMENTS:
        ramp = np.floor(255 * np.arange(steps) / steps)
        wheel[row:row + steps] = hue
        wheel[row:row + steps, ch] = ramp if rising else 255 - ramp
        hue[ch] = 255.0 if rising else 0.0
        row += steps
    return wheel


def _as_fields(flow) -> tuple:
    """-> (device tensor [N, 2, H, W] float32 contiguous, had a batch dimension?).  A 3-d device tensor is [2, H, W] (what the
    model returns); a 3-d numpy array or CPU tensor is the reference's [H, W, 2] unless only its first dimension is 2."""
    if isinstance(flow, np.ndarray):
        flow = torch.from_numpy(np.ascontiguousarray(flow))
    if not isinstance(flow, torch.Tensor):
        raise TypeError(f"flow_to_image: expected a tensor or a numpy array, got {type(flow).__name__}")
    batched = flow.dim() == 4
    if flow.dim() == 3:
        channel_first = flow.shape[0] == 2 and (flow.is_cuda or flow.shape[2] != 2)
        if not channel_first and flow.shape[2] == 2:
            flow = flow.permute(2, 0, 1)
        flow = flow[None]
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise ValueError(f"flow_to_image: expected [2, H, W], [N, 2, H, W] or [H, W, 2], got {tuple(flow.shape)}")
    if not flow.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("flow_to_image colours on the GPU (sf_flow_to_image) and no GPU is available; "
                               "there is no CPU fallback")
        flow = flow.to(torch.device("cuda", torch.cuda.current_device()))
    return flow.detach().float().contiguous(), batched


def flow_to_image(flow, clip_flow: Optional[float] = None, convert_to_bgr: bool = False, rad_max: Optional[float] = None
                  ) -> np.ndarray:
    """The reference's ``flow_to_image(flow_uv, clip_flow=None, convert_to_bgr=False)``: numpy uint8 [H, W, 3] (or [N, H, W, 3] for
    a batch [N, 2, H, W], every field on its own scale).  `clip_flow` is the reference's np.clip(flow, 0, clip_flow) -- negative
    components become 0.  `rad_max` (an extension) fixes the normalisation instead of each field's largest radius, so that the
    frames of a video share one scale; radii above it are drawn at 0.75 brightness.  Non-finite pixels are black."""
    fields, batched = _as_fields(flow)
    img = ops.flow_to_image(fields, clip_flow=clip_flow, rad_max=rad_max, convert_to_bgr=convert_to_bgr).cpu().numpy()
    return img if batched else img[0]
