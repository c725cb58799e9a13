"""Streaming, batched video inference: uint8 frames in, flow fields out, `clips_per_step` clips per model call.

The counterpart of the reference's `read_video_and_group_predict` (demo.py:502-534) for frames that arrive as bytes -- from a decoder,
from PNG files (`FrameDir`), or already on the GPU.  Per batch of clips: the uint8 frames the batch needs are uploaded (nothing when
they are device-resident), ONE sf_frames_to_clips launch normalises, replicate-pads and groups them into [n_clips, T, 3, Hp, Wp], the
model runs once, ONE sf_clips_to_flows launch crops the kept flow fields into video order.  The host never holds a frame in fp32.

`clip_count`, `clip_start` and `pair_clip` are the one host-side definition of the clip schedule (include/streamflow_hip.h, "video
clips": the kernels compute the same closed form); `demo.group_clips` and `datasets.sintel_clip_schedule` are views of it with the
reference's keep flags and frame ids.  `demo.predict_frames` stays the one-clip-per-call host path.
"""
from __future__ import annotations

import glob
import os
import struct
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .datasets import batched_call, model_device, read_frame
from .utils import InputPadder

MAX_PAIRS = 8               # SF_VIDEO_MAX_PAIRS: pair pointers one sf_clips_to_flows call takes


def clip_count(n: int, T: int) -> int:
    """Clips of T frames that cover a video of n frames: ceil((n - 1) / (T - 1))."""
    if T < 2 or n < T:
        raise ValueError(f"need at least T={T} >= 2 frames, got {n}")
    return -(-(n - 1) // (T - 1))


def clip_start(c: int, n: int, T: int) -> int:
    """First frame of clip c: clips advance by T - 1 frames, the last one is aligned to the end of the video."""
    if not 0 <= c < clip_count(n, T):
        raise ValueError(f"clip {c} of a video with {clip_count(n, T)}")
    return min(c * (T - 1), n - T)


def pair_clip(j: int, n: int, T: int) -> Tuple[int, int]:
    """(clip, slot inside it) that produces pair j (frames j -> j + 1): the earliest clip that contains the pair."""
    if not 0 <= j < n - 1:
        raise ValueError(f"pair {j} of a video with {n - 1}")
    c = min(j // (T - 1), clip_count(n, T) - 1)
    return c, j - clip_start(c, n, T)


def plan_batches(n: int, T: int, clips_per_step: int) -> List[Tuple[int, int, int, int, int, int]]:
    """[(first_clip, n_clips, frame_lo, frame_hi, pair_lo, pair_hi)] per model call: the clips first_clip .. first_clip + n_clips - 1
    read the frames [frame_lo, frame_hi) and produce the pairs [pair_lo, pair_hi) of the video (half-open ranges); the pair ranges
    of consecutive batches tile 0 .. n - 2 in order.  The last batch may hold fewer clips."""
    if clips_per_step < 1:
        raise ValueError(f"clips_per_step must be at least 1, got {clips_per_step}")
    nc = clip_count(n, T)
    out = []
    for first in range(0, nc, clips_per_step):
        k = min(clips_per_step, nc - first)
        last = first + k - 1
        out.append((first, k, clip_start(first, n, T), clip_start(last, n, T) + T, first * (T - 1), min((last + 1) * (T - 1), n - 1)))
    return out


def _png_size(path: str) -> Tuple[int, int]:
    with open(path, "rb") as f:
        head = f.read(24)
    if len(head) < 24 or head[:8] != b"\x89PNG\r\n\x1a\n" or head[12:16] != b"IHDR":
        raise IOError(f"{path}: not a PNG file")
    w, h = struct.unpack(">II", head[16:24])
    return h, w


class FrameDir:
    """The PNG frames of a directory, sorted by name, as a lazy sequence of uint8 [H, W, 3] arrays: a frame is decoded
    (datasets.read_frame: grey replicated to three channels, alpha dropped) when it is indexed and not kept.  All frames must have
    one size: the headers are compared when the object is made, the decoded arrays again when they are read.

    decode="gpu": predict_video takes a batch's frames through `device_batch` -- inflated on the host, unfiltered on the device
    (png_gpu.decode_frames), the same bytes -- instead of indexing them one by one; indexing a single frame still decodes on the
    host.  The default "host" is the path above alone."""

    def __init__(self, path: str, pattern: str = "*.png", decode: str = "host"):
        if decode not in ("host", "gpu"):
            raise ValueError(f"FrameDir: decode {decode!r} ('host' or 'gpu')")
        if decode == "gpu":
            self.device_batch = self._device_batch                       # (_Source looks for the attribute)
        self.paths = sorted(glob.glob(os.path.join(path, pattern)))
        if not self.paths:
            raise FileNotFoundError(f"no frames matching {pattern!r} in {path}")
        self.hw = _png_size(self.paths[0])
        for p in self.paths[1:]:
            if _png_size(p) != self.hw:
                raise ValueError(f"{p}: frame size {_png_size(p)} differs from {self.hw} of {self.paths[0]}")

    def __len__(self) -> int:
        return len(self.paths)

    def __getitem__(self, i: int) -> np.ndarray:
        if isinstance(i, slice):
            raise TypeError("FrameDir is indexed by frame number")
        img = read_frame(self.paths[i])
        if img.shape[:2] != self.hw:
            raise ValueError(f"{self.paths[i]}: frame size {img.shape[:2]} differs from {self.hw}")
        return img

    def _device_batch(self, lo: int, hi: int, dev: torch.device) -> torch.Tensor:
        """The frames lo .. hi - 1 as uint8 [hi - lo, H, W, 3] on `dev`; raises without a GPU (no fallback to the host decoder)."""
        from . import png_gpu
        out = png_gpu.decode_frames(self.paths[lo:hi], dev)
        if tuple(out.shape[1:3]) != self.hw:
            raise ValueError(f"{self.paths[lo]}: frame size {tuple(out.shape[1:3])} differs from {self.hw}")
        return out


def _jpeg_size(path: str) -> Tuple[int, int]:
    from .avi import jpeg_size
    with open(path, "rb") as f:
        head = f.read(65536)
        try:
            w, h = jpeg_size(head)
        except ValueError:
            try:
                w, h = jpeg_size(head + f.read())                        # a long APPn segment (a thumbnail, a profile) before the frame header
            except ValueError as e:
                raise IOError(f"{path}: {e}") from None
    return h, w


JPEG_PATTERNS = ("*.jpg", "*.jpeg", "*.JPG", "*.JPEG")


class JpegDir:
    """The baseline JPEG frames of a directory (`pattern`, default *.jpg and *.jpeg), sorted by name, as a lazy sequence.  They are
    decoded on the GPU only (jpeg_gpu.decode_batch: one sf_jpeg_decode call per batch): predict_video takes a batch's frames through
    `device_batch`, and frames[i] decodes one frame on the current GPU and returns the host array uint8 [H, W, 3] (grey replicated
    to three channels).  All frames must have one size: the frame headers are compared when the object is made.  `split` is
    jpeg_gpu.decode_batch's: how files without restart markers are decoded in parallel."""

    def __init__(self, path: str, pattern: Optional[str] = None, split: str = "auto"):
        from .jpeg_gpu import SPLIT_MODES
        if split not in SPLIT_MODES:
            raise ValueError(f"JpegDir: split = {split!r} (one of {', '.join(SPLIT_MODES)})")
        self.split = split
        patterns = JPEG_PATTERNS if pattern is None else (pattern,)
        self.paths = sorted({p for pat in patterns for p in glob.glob(os.path.join(path, pat))})
        if not self.paths:
            raise FileNotFoundError(f"no frames matching {' / '.join(patterns)} in {path}")
        self.hw = _jpeg_size(self.paths[0])
        for p in self.paths[1:]:
            if _jpeg_size(p) != self.hw:
                raise ValueError(f"{p}: frame size {_jpeg_size(p)} differs from {self.hw} of {self.paths[0]}")

    def __len__(self) -> int:
        return len(self.paths)

    def device_batch(self, lo: int, hi: int, dev: torch.device) -> torch.Tensor:
        """The frames lo .. hi - 1 as uint8 [hi - lo, H, W, 3] on `dev`; raises without a GPU (there is no host decoder)."""
        from . import jpeg_gpu
        out = jpeg_gpu.decode_batch(self.paths[lo:hi], dev, split=self.split)
        if tuple(out.shape[1:3]) != self.hw:
            raise ValueError(f"{self.paths[lo]}: frame size {tuple(out.shape[1:3])} differs from {self.hw}")
        return out

    def __getitem__(self, i: int) -> np.ndarray:
        if isinstance(i, slice):
            raise TypeError("JpegDir is indexed by frame number")
        i = range(len(self.paths))[i]
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        return self.device_batch(i, i + 1, dev)[0].cpu().numpy()


def open_frames(path: str, png_decode: str = "host", jpeg_split: str = "auto"):
    """The frame source behind a path: a FrameDir for a directory of .png files (png_decode: its `decode`), a JpegDir for a directory
    of .jpg / .jpeg files, an avi.MjpegReader for a file (jpeg_split: their `split`).  A directory that holds both kinds is a ValueError, one that holds neither
    and a path that does not exist a FileNotFoundError."""
    if os.path.isdir(path):
        png = glob.glob(os.path.join(path, "*.png"))
        jpg = [p for pat in JPEG_PATTERNS for p in glob.glob(os.path.join(path, pat))]
        if png and jpg:
            raise ValueError(f"{path} holds {len(png)} .png and {len(jpg)} .jpg / .jpeg frames: one kind per directory")
        if jpg:
            return JpegDir(path, split=jpeg_split)
        return FrameDir(path, decode=png_decode)                         # raises FileNotFoundError for a directory without frames
    if os.path.isfile(path):
        from .avi import MjpegReader
        return MjpegReader(path, split=jpeg_split)
    raise FileNotFoundError(f"{path}: neither a directory of frames nor a video file")


class _Source:
    """The frames argument of predict_video behind one face: n, (H, W), and `device_frames(lo, hi, dev)` -> (uint8 device tensor,
    channels_last, number of its first frame).  Everything is checked that can be without touching the GPU or decoding a frame."""

    def __init__(self, frames):
        self.stack = None                                                # a whole-video tensor / array
        self.seq = None                                                  # a sequence of [H, W, 3] frames
        if isinstance(frames, np.ndarray):
            if frames.dtype != np.uint8:
                raise TypeError(f"predict_video: frames must be uint8, got {frames.dtype}")
            frames = torch.from_numpy(frames)
        if isinstance(frames, torch.Tensor):
            if frames.dtype != torch.uint8:
                raise TypeError(f"predict_video: frames must be uint8, got {frames.dtype} (normalised fp32 frames: demo.predict_frames)")
            if frames.dim() != 4 or 3 not in (frames.shape[3], frames.shape[1]):
                raise ValueError(f"predict_video: expected frames [N, H, W, 3] or [N, 3, H, W], got {tuple(frames.shape)}")
            self.stack = frames
            self.channels_last = frames.shape[3] == 3
            self.n = int(frames.shape[0])
            self.hw = tuple(int(s) for s in (frames.shape[1:3] if self.channels_last else frames.shape[2:]))
            return
        if not hasattr(frames, "__len__") or not hasattr(frames, "__getitem__"):
            raise TypeError(f"predict_video: frames must be a uint8 tensor / array or a sequence of frames, got {type(frames).__name__}")
        self.seq, self.n, self.channels_last = frames, len(frames), True
        if isinstance(frames, (list, tuple)):                            # frames already in memory: look at all of them now
            for i, f in enumerate(frames):
                self._check(f, i)
                if tuple(f.shape[:2]) != tuple(frames[0].shape[:2]):
                    raise ValueError(f"predict_video: frame {i} is {tuple(f.shape[:2])}, frame 0 is {tuple(frames[0].shape[:2])}")
            self.hw = tuple(int(s) for s in frames[0].shape[:2]) if frames else None
        else:                                                            # lazy: a `hw` attribute (FrameDir) or the first frame
            hw = getattr(frames, "hw", None)
            if hw is None and self.n:
                first = frames[0]
                self._check(first, 0)
                hw = first.shape[:2]
            self.hw = None if hw is None else (int(hw[0]), int(hw[1]))

    @staticmethod
    def _check(f, i: int) -> None:
        dt = getattr(f, "dtype", None)
        if dt not in (np.uint8, torch.uint8):
            raise TypeError(f"predict_video: frame {i} must be uint8, got {dt}")
        if len(f.shape) != 3 or f.shape[2] != 3:
            raise ValueError(f"predict_video: frame {i} must be [H, W, 3], got {tuple(f.shape)}")

    def device_frames(self, lo: int, hi: int, dev: torch.device):
        if self.stack is not None:
            if self.stack.is_cuda:
                if self.stack.device != dev:
                    raise RuntimeError(f"predict_video: frames on {self.stack.device}, model on {dev}")
                return self.stack, self.channels_last, 0
            return self.stack[lo:hi].to(dev), self.channels_last, lo
        if hasattr(self.seq, "device_batch"):                            # FrameDir(decode="gpu"): decoded where they are used
            return self.seq.device_batch(lo, hi, dev), True, lo
        batch = []
        for i in range(lo, hi):
            f = self.seq[i]
            self._check(f, i)
            if tuple(f.shape[:2]) != self.hw:
                raise ValueError(f"predict_video: frame {i} is {tuple(f.shape[:2])}, frame 0 is {self.hw}")
            batch.append(f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f)))
        if all(f.is_cuda for f in batch):
            return torch.stack(batch), True, lo
        return torch.stack([f.cpu() for f in batch]).to(dev), True, lo


@torch.no_grad()
def predict_video(model: Callable, frames, T: int = 4, iters: Optional[int] = None, clips_per_step: int = 8, mode: str = "sintel",
                  device=None, sink: Optional[Callable[..., None]] = None, bidirectional: bool = False,
                  size: Optional[Sequence[int]] = None, frame_filter: str = "bilinear", flow_filter: str = "bilinear"):
    """Flow fields of every consecutive frame pair of a video, `clips_per_step` clips per model call.

    frames: a uint8 tensor / array [N, H, W, 3] or [N, 3, H, W] (HWC when both readings fit) on the host or the GPU, or a sequence
    of uint8 [H, W, 3] frames (`FrameDir`, a list), read batch by batch.  model: `model.forward_normalised(imgs, iters)` when it has
    one (SKFlow_MF8, StreamFlowT4; `iters=None` = the class's default), else `model(imgs)` as demo.predict_frames calls it; imgs is
    fp32 [n_clips, T, 3, Hp, Wp] in [-1, 1], the result T - 1 flows [n_clips, 2, Hp, Wp].  mode: InputPadder's.  device: default the
    frames' GPU, else the model's, else the current one.

    Returns a device tensor [N - 1, 2, H, W]; with `sink`, calls `sink(first_pair, flows[k, 2, H, W])` per batch in video order,
    keeps nothing and returns None (long videos, writing to disk).  Nothing here synchronises with the host.

    bidirectional=True: every batch's clip tensor is also run time-reversed (`imgs.flip(1)`, a second model call of the same batch
    size: an engine's plan and graph are reused, `clips_per_step` keeps its memory meaning) and the result is `(fwd, bwd)`, both
    [N - 1, 2, H, W].  bwd[j] is the flow from frame j + 1 to frame j, computed from the REVERSED clip that holds pair j in the
    forward schedule (slot T - 2 - k of the reversed clip for slot k of the forward one).  It is not predict_video on the reversed
    video, whose clip boundaries differ when (N - 1) % (T - 1) != 0.  With `sink` the call is `sink(first_pair, fwd, bwd, frames)`:
    frames is the uint8 device tensor [k + 1, H, W, 3] of the frames first_pair .. first_pair + k (a view of the batch's frame
    buffer).  streamflow_amd.consistency turns the two fields into occlusion masks, warped frames and a report.

    size=(h, w): the model runs at that resolution (resize.scaled_size chooses one from a factor or a longest side).  Each batch's
    frame buffer is resampled once with ops.resize_frames (`frame_filter`; once for both directions), the clips, the padder and the
    model see (h, w), and the gathered flows are brought back to (H, W) with ops.resize_flows (`flow_filter`, values scaled by W / w
    and H / h) before they are returned or handed to `sink`, which still receives the ORIGINAL frames.  None (the default): the
    frames go through at their own size, the code above alone."""
    from . import ops
    src = _Source(frames)
    if T < 2 or T - 1 > MAX_PAIRS:
        raise ValueError(f"predict_video: T = {T} (2 .. {MAX_PAIRS + 1}: at most {MAX_PAIRS} pairs per clip)")
    if src.n < T:
        raise ValueError(f"predict_video: need at least T={T} frames, got {src.n}")
    batches = plan_batches(src.n, T, int(clips_per_step))
    if device is None:
        device = src.stack.device if src.stack is not None and src.stack.is_cuda else model_device(model)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"predict_video runs on the GPU (device {dev}, GPU available: {torch.cuda.is_available()}); there is no CPU "
                           "fallback -- demo.predict_frames is the host-side path")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    H, W = src.hw
    if size is not None:
        return _predict_video_resized(call=batched_call(model, iters), src=src, T=T, batches=batches, dev=dev, mode=mode, sink=sink,
                                      bidirectional=bidirectional, size=size, frame_filter=frame_filter, flow_filter=flow_filter)
    pad = InputPadder((H, W), mode=mode)._pad
    call = batched_call(model, iters)
    out = None if sink is not None else torch.empty(src.n - 1, 2, H, W, dtype=torch.float32, device=dev)
    out_b = torch.empty_like(out) if bidirectional and out is not None else None
    with torch.cuda.device(dev):
        for first, k, f_lo, f_hi, p_lo, p_hi in batches:
            buf, channels_last, frame0 = src.device_frames(f_lo, f_hi, dev)
            imgs = ops.frames_to_clips(buf, src.n, T, first, k, pad, frame0=frame0, channels_last=channels_last)
            flows = list(call(imgs))
            if len(flows) != T - 1:
                raise RuntimeError(f"predict_video: the model returned {len(flows)} flows for clips of T = {T}")
            got = ops.clips_to_flows(flows, src.n, T, first, p_lo, p_hi - p_lo, (H, W), pad,
                                     out=None if out is None else out[p_lo:p_hi])
            if not bidirectional:
                if sink is not None:
                    sink(p_lo, got)
                continue
            back = list(call(imgs.flip(1)))
            if len(back) != T - 1:
                raise RuntimeError(f"predict_video: the model returned {len(back)} flows for reversed clips of T = {T}")
            got_b = ops.clips_to_flows(back[::-1], src.n, T, first, p_lo, p_hi - p_lo, (H, W), pad,
                                       out=None if out_b is None else out_b[p_lo:p_hi])
            if sink is not None:
                held = buf[p_lo - frame0:p_hi + 1 - frame0]
                sink(p_lo, got, got_b, held if channels_last else held.permute(0, 2, 3, 1))
    return (out, out_b) if bidirectional and sink is None else out


def _predict_video_resized(call, src, T, batches, dev, mode, sink, bidirectional, size, frame_filter, flow_filter):
    """predict_video's loop with the model at size = (h, w): frames down (or up) once per batch, flows back to the frames' grid."""
    from . import ops, resize
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"predict_video: size must be (h, w), got {size!r}") from None
    if h < 1 or w < 1:
        raise ValueError(f"predict_video: size must be positive, got {(h, w)}")
    for f in (frame_filter, flow_filter):
        if f not in resize.FILTERS:
            raise ValueError(f"predict_video: filter {f!r} (one of {', '.join(resize.FILTERS)})")
    H, W = src.hw
    pad = InputPadder((h, w), mode=mode)._pad
    out = None if sink is not None else torch.empty(src.n - 1, 2, H, W, dtype=torch.float32, device=dev)
    out_b = torch.empty_like(out) if bidirectional and out is not None else None
    with torch.cuda.device(dev):
        for first, k, f_lo, f_hi, p_lo, p_hi in batches:
            buf, channels_last, frame0 = src.device_frames(f_lo, f_hi, dev)
            if src.stack is not None and src.stack.is_cuda:             # the whole video is resident: only this batch's frames
                buf, frame0 = buf[f_lo:f_hi], f_lo
            small = ops.resize_frames(buf, (h, w), frame_filter, channels_last=channels_last)
            imgs = ops.frames_to_clips(small, src.n, T, first, k, pad, frame0=frame0, channels_last=True)
            passes = [(False, out)] + ([(True, out_b)] if bidirectional else [])
            got = []
            for reverse, dst in passes:
                flows = list(call(imgs.flip(1) if reverse else imgs))
                if len(flows) != T - 1:
                    raise RuntimeError(f"predict_video: the model returned {len(flows)} flows for {'reversed ' if reverse else ''}clips "
                                       f"of T = {T}")
                low = ops.clips_to_flows(flows[::-1] if reverse else flows, src.n, T, first, p_lo, p_hi - p_lo, (h, w), pad)
                got.append(ops.resize_flows(low, (H, W), flow_filter, out=None if dst is None else dst[p_lo:p_hi]))
            if sink is None:
                continue
            if not bidirectional:
                sink(p_lo, got[0])
            else:
                held = buf[p_lo - frame0:p_hi + 1 - frame0]
                sink(p_lo, got[0], got[1], held if channels_last else held.permute(0, 2, 3, 1))
    return (out, out_b) if bidirectional and sink is None else out
