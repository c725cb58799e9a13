"""ctypes binding of libstreamflow_track.so (the C ABI declared in include/streamflow_track.h): point tracking and track drawing.

A library of its own next to libstreamflow_hip.so (_lib.py), with the same rule: there is NO fallback.  If the shared library is
missing or fails to load, the call raises; nothing routes through PyTorch ops or the host.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch  # noqa: F401  (imported first so the process-wide HIP runtime is torch's libamdhip64)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libstreamflow_track.so")

VERSION = 1                                                              # SFT_VERSION
VISIBLE, OCCLUDED, LOST, PENDING = range(4)                              # SFT_VISIBLE ...
MAX_STEPS, DRAW_MAX_SEG, DRAW_MAX_TRAIL, DRAW_MAX_RADIUS, DRAW_MAX_POINTS = 4096, 64, 255, 16, (1 << 20) - 1

_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float

SIGNATURES = {
    "sft_version": (_i, []),
    "sft_last_error": (C.c_char_p, []),
    "sft_track_advance_ws_bytes": (_i64, [_i, _i64]),
    "sft_track_advance": (_i, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _i, _i, _i, _i, _vp, _vp, _vp, _i64, _f, _f, _i, _vp, _vp, _vp,
                               _vp, _vp, _vp, _i64, _vp]),
    "sft_draw_tracks_ws_bytes": (_i64, [_i, _i, _i]),
    "sft_draw_tracks": (_i, [_vp, _i64, _i64, _i64, _i64, _i, _i, _i, _i, _vp, _vp, _i, _i64, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp,
                             _i64, _vp]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the shared library (once).  Raises RuntimeError if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. "
            "Run `python -m streamflow_amd.build` (needs hipcc); there is no CPU/PyTorch fallback.")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise RuntimeError(f"failed to load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.sft_version() < VERSION:
        raise RuntimeError("libstreamflow_track.so is too old; rebuild")
    _lib = lib
    return lib


def check(status: int, what: str = "") -> None:
    if status != 0:
        msg = load().sft_last_error().decode(errors="replace")
        raise RuntimeError(f"libstreamflow_track {what} failed ({status}): {msg}")


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream
