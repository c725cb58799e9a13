"""Host-side plan of tiled inference (the reference's KITTI tile protocol, evaluate_mf.py:858-1053).

A padded frame is cut into overlapping crops of the training size; the model runs on every crop and the crops' flows are
blended with one Gaussian weight patch per crop: ``out = sum_k f_k * w / sum_k w`` over the crops k that cover a pixel, in the
order of the reference's crop sequence.

* ``tile_grid`` -- the reference's crop origins, duplicates and order included (at every KITTI shape each crop appears twice:
  ``range(0, 432, 412)`` is ``[0, 412]`` and the last entry is then set back to 0).
* ``tile_weights`` -- the weight patch, bitwise the reference's (torch fp32 CPU arithmetic in the reference's operation order; its
  corners are fp32 subnormals, ~3e-43 at sigma = 0.05), uploaded once per (tile, sigma, device).
* ``TilePlan`` -- the distinct crops (each runs through the model once), the map from the reference's sequence to them (the blend
  still adds every entry, duplicates included, in the reference's order: fp32 addition does not associate) and the output crop.
* ``FixedHeightPadder`` -- the 'kitti432' / 'kitti376' modes of the reference's ``InputPadder2``: all padding at the bottom, up to
  a fixed height; the width is left alone.

The blend itself is one HIP kernel (csrc/tile_blend.hip, ``ops.tile_blend``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import torch
import torch.nn.functional as F

KITTI_MF_TILE = (432, 960)      # validate_kitti_mf_tile: crops of the training size, frames replicate-padded to 432 rows
KITTI_TILE = (376, 720)         # validate_kitti_tile: zero-padded to 376 rows
TILE_SIGMA = 0.05
MAX_TILES = 64                  # SF_TILE_MAX of include/streamflow_hip.h


def tile_grid(image_hw: Sequence[int], tile_hw: Sequence[int], min_overlap: int = 20) -> List[Tuple[int, int]]:
    """Crop origins (y, x), row-major, exactly as the reference lists them: starts every ``tile - min_overlap`` pixels below the
    image size, the last one in each direction moved flush with the image's far edge (which can repeat an earlier start)."""
    H, W = int(image_hw[0]), int(image_hw[1])
    th, tw = int(tile_hw[0]), int(tile_hw[1])
    if min_overlap >= th or min_overlap >= tw:
        raise ValueError(f"min_overlap {min_overlap} must be smaller than the tile {th} x {tw}")
    if H < th or W < tw:
        raise ValueError(f"image {H} x {W} is smaller than the tile {th} x {tw}")
    ys = list(range(0, H, th - min_overlap))
    xs = list(range(0, W, tw - min_overlap))
    ys[-1] = H - th
    xs[-1] = W - tw
    return [(y, x) for y in ys for x in xs]


def _weights_cpu(th: int, tw: int, sigma: float) -> torch.Tensor:
    # the reference's expression, operation by operation and on tensors of the same shapes (torch's CPU exp takes a vector or a
    # scalar path depending on the position inside the tensor, so the shapes matter for the last bit)
    gy, gx = torch.meshgrid(torch.arange(th), torch.arange(tw), indexing="ij")
    gy, gx = gy / float(th), gx / float(tw)
    gy, gx = gy - 0.5, gx - 0.5
    r = (gy ** 2 + gx ** 2) ** 0.5 / sigma
    norm = 1 / (sigma * math.sqrt(2 * math.pi))
    return (norm * torch.exp(-0.5 * r ** 2)).contiguous()


_WEIGHTS: Dict[tuple, torch.Tensor] = {}


def tile_weights(tile_hw: Sequence[int], sigma: float = TILE_SIGMA, device=None) -> torch.Tensor:
    """[th, tw] fp32 Gaussian weight patch of one crop (bitwise one ``patch_weights[i]`` of the reference's compute_weight),
    computed on the host and cached per (tile, sigma, device).  The first use on a GPU uploads from the host, which blocks: inside a
    graph capture it raises (and caches nothing for that device), so call once eagerly before capturing."""
    th, tw = int(tile_hw[0]), int(tile_hw[1])
    dev = torch.device("cpu") if device is None else torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (th, tw, float(sigma), str(dev))
    w = _WEIGHTS.get(key)
    if w is None:
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():    # the upload blocks the host: not recordable
            raise RuntimeError(f"tile_weights: the {th} x {tw} patch requested for the first time inside a graph capture; build it "
                               "before (one eager tile_weights call for that device)")
        cpu_key = (th, tw, float(sigma), "cpu")
        if cpu_key not in _WEIGHTS:
            _WEIGHTS[cpu_key] = _weights_cpu(th, tw, float(sigma))
        w = _WEIGHTS[key] = _WEIGHTS[cpu_key].to(dev)
    return w


@dataclass(frozen=True)
class TilePlan:
    """Everything the blend needs about one padded frame size.

    ``sequence``: the reference's crop origins (duplicates included); ``distinct``: the distinct origins in order of first
    appearance (the crops the model runs on); ``index[k]``: the distinct crop of ``sequence[k]``; ``crop``: (y0, x0, h, w) of the
    output inside the padded canvas (how the padding is removed)."""
    image_hw: Tuple[int, int]
    tile_hw: Tuple[int, int]
    sequence: Tuple[Tuple[int, int], ...]
    distinct: Tuple[Tuple[int, int], ...]
    index: Tuple[int, ...]
    crop: Tuple[int, int, int, int]

    @property
    def n_distinct(self) -> int:
        return len(self.distinct)

    def crops(self, x: torch.Tensor) -> List[torch.Tensor]:
        """The distinct crops of x [..., H, W] (views, no arithmetic)."""
        th, tw = self.tile_hw
        return [x[..., y:y + th, x0:x0 + tw] for (y, x0) in self.distinct]


def make_plan(image_hw: Sequence[int], tile_hw: Sequence[int], min_overlap: int = 20, pad: Sequence[int] = (0, 0, 0, 0)
              ) -> TilePlan:
    """Plan of a padded canvas image_hw; `pad` = [left, right, top, bottom] as an InputPadder's ``_pad`` (removed from the output)."""
    H, W = int(image_hw[0]), int(image_hw[1])
    seq = tile_grid((H, W), tile_hw, min_overlap)
    distinct: List[Tuple[int, int]] = []
    index = []
    for o in seq:
        if o not in distinct:
            distinct.append(o)
        index.append(distinct.index(o))
    th, tw = int(tile_hw[0]), int(tile_hw[1])
    if any(y + th > H or x + tw > W for (y, x) in seq):
        # (the reference's grid does this when a start before the last one already overshoots: 64 x 96 with 48 x 64 crops
        # starts rows at 0, 28, 16 -- it would then run the model on a truncated crop)
        raise ValueError(f"the crop grid of {H} x {W} with {th} x {tw} crops and min_overlap {min_overlap} leaves the image: {seq}")
    if len(seq) > MAX_TILES:
        raise ValueError(f"{len(seq)} crops exceed the blend's limit of {MAX_TILES}")
    left, right, top, bottom = (int(p) for p in pad)
    if min(left, right, top, bottom) < 0 or left + right >= W or top + bottom >= H:
        raise ValueError(f"padding {list(pad)} does not fit the canvas {H} x {W}")
    return TilePlan((H, W), (th, tw), tuple(seq), tuple(distinct), tuple(index),
                    (top, left, H - top - bottom, W - left - right))


class FixedHeightPadder:
    """The fixed-height modes of the reference's InputPadder2 ('kitti432', 'kitti376'): all padding below the frame, up to
    `height` rows; the width is left as it is.  ``pad`` fills with zeros, ``pad_list`` replicates the last row (as the
    reference's methods of those names do); ``_pad`` = [left, right, top, bottom]."""

    def __init__(self, dims, height: int, mode: str = "replicate"):
        self.ht, self.wd = int(dims[-2]), int(dims[-1])
        if self.ht > height:
            raise ValueError(f"frame of {self.ht} rows is taller than the padded height {height}")
        if mode not in ("replicate", "zeros"):
            raise ValueError(f"mode must be 'replicate' or 'zeros', got {mode!r}")
        self.height, self.mode = int(height), mode
        self._pad = [0, 0, 0, self.height - self.ht]

    def pad(self, *inputs):
        return [F.pad(x, self._pad, mode="constant", value=0.0) for x in inputs]

    def pad_list(self, inputs):
        return [F.pad(x, self._pad, mode="replicate") for x in inputs]

    def apply(self, inputs):
        """pad_list or pad, whichever `mode` names."""
        return self.pad_list(inputs) if self.mode == "replicate" else self.pad(*inputs)

    def unpad(self, x):
        left, right, top, bottom = self._pad
        rows, cols = x.shape[-2:]
        return x[..., top:rows - bottom, left:cols - right]
