"""Coefficient tables and working sizes for running inference at a chosen resolution (csrc/resize.hip; include/streamflow_hip.h,
"resize").

`coeff_table` is Pillow's `precompute_coeffs` (Resample.c) in numpy float64, `quantise` its conversion to the 8-bit resampler's
fixed point.  The tables are built on the host -- a few hundred doubles per axis, the filters' sin / polynomial in float64 -- and
cached on the device per (in, out, filter, device); the kernels do the per-pixel arithmetic only (ops.resize_frames,
ops.resize_flows).  `scaled_size` chooses the working size.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

PRECISION_BITS = 22          # Pillow's 32 - 8 - 2: the 8-bit resampler's coefficients are scaled by 2^22
MAX_KSIZE = 97               # SF_RESIZE_MAX_KSIZE


def _box(x: np.ndarray) -> np.ndarray:
    return np.where((x > -0.5) & (x <= 0.5), 1.0, 0.0)


def _bilinear(x: np.ndarray) -> np.ndarray:
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _bicubic(x: np.ndarray) -> np.ndarray:
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def _sinc(x: np.ndarray) -> np.ndarray:
    px = x * math.pi
    sin = np.array([math.sin(v) for v in px.ravel()], np.float64).reshape(px.shape)     # libm's sin, as the C code calls it
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(x == 0.0, 1.0, sin / px)


def _lanczos(x: np.ndarray) -> np.ndarray:
    return np.where((-3.0 <= x) & (x < 3.0), _sinc(x) * _sinc(x / 3), 0.0)


FILTERS = {"box": (_box, 0.5), "bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}


def coeff_table(in_size: int, out_size: int, filter: str = "bilinear") -> Tuple[np.ndarray, np.ndarray]:
    """(bounds int32 [out, 2] = (first tap, tap count), k float64 [out, ksize]) of one axis: output position xx takes the input
    positions bounds[xx, 0] .. + bounds[xx, 1] - 1 with the weights k[xx, :count]; the entries past the count are zero."""
    if filter not in FILTERS:
        raise ValueError(f"coeff_table: filter {filter!r} (one of {', '.join(FILTERS)})")
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"coeff_table: sizes must be positive, got {in_size} -> {out_size}")
    f, fsupport = FILTERS[filter]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)                    # (int): truncation
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    count = xmax - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = f((x + xmin[:, None] - center[:, None] + 0.5) * (1.0 / filterscale))
    w = np.where(np.arange(ksize)[None, :] < count[:, None], w, 0.0)
    ww = np.zeros(out_size, np.float64)
    for i in range(ksize):                                                             # the sum in tap order
        ww = ww + w[:, i]
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(ww[:, None] != 0.0, w / ww[:, None], w)
    k = np.where(np.arange(ksize)[None, :] < count[:, None], k, 0.0)
    return np.stack([xmin, count], 1).astype(np.int32), k


def quantise(k: np.ndarray) -> np.ndarray:
    """Pillow's fixed point of the 8-bit resampler: (int)(k * 2^22 +- 0.5), rounded away from zero -> int32."""
    v = np.asarray(k, np.float64) * float(1 << PRECISION_BITS)
    return np.where(v < 0, -0.5 + v, 0.5 + v).astype(np.int64).astype(np.int32)        # astype truncates towards zero, as (int)


def scaled_size(hw: Sequence[int], scale: Optional[float] = None, max_side: Optional[int] = None, multiple: int = 8) -> Tuple[int, int]:
    """The working size (h, w) for frames of hw = (H, W): the factor is `scale`, or min(1, max_side / max(H, W)) (max_side never
    enlarges); each side is max(multiple, multiple * round(side * factor / multiple)) (Python's round: halves go to the even
    neighbour, 188 -> 192 and 180 -> 176 at multiple 8), so the padder has nothing to add.  A pure
    function.  Exactly one of scale / max_side must be given (ValueError otherwise, and for values that are not positive)."""
    if (scale is None) == (max_side is None):
        raise ValueError("scaled_size: give exactly one of scale and max_side")
    H, W = int(hw[0]), int(hw[1])
    multiple = int(multiple)
    if H < 1 or W < 1 or multiple < 1:
        raise ValueError(f"scaled_size: bad size {(H, W)} or multiple {multiple}")
    if scale is not None:
        factor = float(scale)
        if not (factor > 0 and math.isfinite(factor)):
            raise ValueError(f"scaled_size: scale must be a positive number, got {scale}")
    else:
        if not max_side > 0:
            raise ValueError(f"scaled_size: max_side must be positive, got {max_side}")
        factor = min(1.0, float(max_side) / max(H, W))
    return tuple(max(multiple, multiple * int(round(side * factor / multiple))) for side in (H, W))


_TABLES: Dict[tuple, tuple] = {}


def device_table(in_size: int, out_size: int, filter: str, device, kind: str):
    """(bounds int32 [out, 2], k [out, ksize], ksize) on `device`, cached per (in, out, filter, device, kind); kind 'u8': k int32,
    quantised; 'f32': k fp32, the float64 table rounded once.  The first use of a key uploads from the host, which blocks: inside a
    graph capture it raises (and caches nothing), so call once eagerly before capturing."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"resize: the tables are used on the GPU (got {device}); there is no CPU fallback")
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (int(in_size), int(out_size), filter, index, kind)
    hit = _TABLES.get(key)
    if hit is None:
        if torch.cuda.is_current_stream_capturing():           # the upload below blocks the host, which a capture cannot record
            raise RuntimeError(f"resize: the {in_size} -> {out_size} {filter} table requested for the first time inside a graph "
                               "capture; build it before (one eager call at the same sizes)")
        bounds, k = coeff_table(in_size, out_size, filter)
        if k.shape[1] > MAX_KSIZE:
            raise ValueError(f"resize: {in_size} -> {out_size} with the {filter} filter needs {k.shape[1]} taps (at most {MAX_KSIZE})")
        kk = quantise(k) if kind == "u8" else k.astype(np.float32)
        dev = torch.device("cuda", index)
        hit = (torch.from_numpy(np.ascontiguousarray(bounds)).to(dev), torch.from_numpy(np.ascontiguousarray(kk)).to(dev), int(k.shape[1]))
        _TABLES[key] = hit
    return hit
