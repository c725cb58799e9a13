"""PNG files <-> frames on the GPU.  Decoding: the inflate on the host (zlib, in a thread pool: it releases the GIL), the row unfilter
as one sf_png_unfilter launch for the whole batch (csrc/png_unfilter.hip).  flow_io.read_png's Average / Paeth branches walk a row
byte by byte in Python, and libpng-written files (Sintel, KITTI, exported videos) are mostly Paeth rows; here that arithmetic runs
where the decoded bytes are wanted anyway (sf_frames_to_clips, sf_flow_score_batch).

Encoding (`encode_batch`): the adaptive row filter and a Huffman-only deflate as one sf_png_encode call for the whole batch
(csrc/png_encode.hip); only the compressed streams cross to the host, where the chunk framing, the CRC-32 and the file writes run in
the same thread pool.

There is no fallback: without a GPU `decode_batch` and `encode_batch` raise; flow_io.read_png / write_png stay the host-side codec.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import flow_io


def pool_threads(threads: Optional[int] = None) -> int:
    """Threads of the inflate pool: `threads`, else min(8, the cores this process may use: bench.usable_cores, the affinity mask
    where the benchmark module is not on the path) -- never the machine's core count."""
    if threads is not None:
        if int(threads) < 1:
            raise ValueError(f"threads must be at least 1, got {threads}")
        return int(threads)
    try:
        from bench import usable_cores
        cores = usable_cores()
    except ImportError:
        cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1
    return max(1, min(8, cores))


def inflate(paths: Sequence[str], threads: Optional[int] = None) -> List[tuple]:
    """flow_io.png_scanlines of every file, in a thread pool (zlib releases the GIL)."""
    paths = list(paths)
    if not paths:
        raise ValueError("png_gpu: no files")
    k = min(pool_threads(threads), len(paths))
    if k == 1:
        return [flow_io.png_scanlines(p) for p in paths]
    with ThreadPoolExecutor(max_workers=k) as ex:
        return list(ex.map(flow_io.png_scanlines, paths))


def _need_gpu(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"png_gpu decodes on the GPU (device {dev}, GPU available: {torch.cuda.is_available()}); there is "
                           "no CPU fallback -- flow_io.read_png is the host-side path")
    return dev


def _unfilter(got: Sequence[tuple], dev: torch.device) -> torch.Tensor:
    """Scanline blocks of one format -> [n, H, W, C] on `dev`: one host array, one upload, one launch."""
    from . import ops
    _, h, w, depth, c = got[0]
    host = np.empty((len(got), got[0][0].size), np.uint8)
    for i, g in enumerate(got):
        host[i] = g[0]
    scan = torch.from_numpy(host).to(dev, non_blocking=True)
    out = ops.png_unfilter(scan, h, w, c * depth // 8, swap16=depth == 16)
    if depth == 16:
        return out.view(torch.uint16).view(len(got), h, w, c)
    return out.view(len(got), h, w, c)


def decode_batch(paths: Sequence[str], device, threads: Optional[int] = None) -> torch.Tensor:
    """The PNG files `paths` -> one device tensor [n, H, W, C], uint8 or (16-bit files) torch.uint16, C as in the files (1, 2, 3
    or 4: no squeeze), bitwise what np.stack([flow_io.read_png(p)]) holds.  All files must share (h, w, depth, channels):
    ValueError naming the first file that differs (raised before the GPU is looked at).  One host array, one upload, one sf_png_unfilter launch; enqueued on the current
    stream of `device`, no synchronisation with the host."""
    paths = list(paths)
    got = inflate(paths, threads)
    for p, g in zip(paths, got):
        if g[1:] != got[0][1:]:
            raise ValueError(f"{p}: (h, w, depth, channels) = {g[1:]} differs from {got[0][1:]} of {paths[0]}")
    dev = _need_gpu(device)
    with torch.cuda.device(dev):
        return _unfilter(got, dev)


def to_rgb8(frames: torch.Tensor) -> torch.Tensor:
    """decode_batch's [n, H, W, C] -> uint8 [n, H, W, 3] as datasets.read_frame makes it on the host: grey (with or without alpha)
    replicated to three channels, alpha dropped, 16-bit samples reduced to their low byte (numpy's astype(uint8))."""
    n, h, w, c = frames.shape
    if frames.dtype != torch.uint8:                                      # host-order 16-bit samples: the low byte comes first
        frames = frames.contiguous().view(torch.uint8).view(n, h, w, c, 2)[..., 0]
    if c <= 2:
        return frames[..., :1].expand(n, h, w, 3).contiguous()
    return frames[..., :3].contiguous()


def decode_frames(paths: Sequence[str], device, threads: Optional[int] = None) -> torch.Tensor:
    """Frame files -> uint8 [n, H, W, 3] on the GPU, frame i what datasets.read_frame(paths[i]) returns.  The files must share
    (h, w) (ValueError naming the file) but not the format: a directory may mix grey and colour frames; each format present is one
    upload and one launch."""
    paths = list(paths)
    got = inflate(paths, threads)
    groups = {}
    for i, (p, g) in enumerate(zip(paths, got)):
        if g[1:3] != got[0][1:3]:
            raise ValueError(f"{p}: frame size {g[1:3]} differs from {got[0][1:3]} of {paths[0]}")
        groups.setdefault(g[3:], []).append(i)
    dev = _need_gpu(device)
    with torch.cuda.device(dev):
        if len(groups) == 1:
            return to_rgb8(_unfilter(got, dev))
        out = torch.empty(len(paths), got[0][1], got[0][2], 3, dtype=torch.uint8, device=dev)
        for idx in groups.values():
            out[torch.tensor(idx, device=dev)] = to_rgb8(_unfilter([got[i] for i in idx], dev))
        return out


def encode_batch(images: torch.Tensor, paths: Sequence[str], threads: Optional[int] = None) -> List[int]:
    """Device images [n, H, W, C] uint8 or torch.uint16 (C = 1 .. 4) -> the PNG files `paths`, image i decoding to images[i] exactly
    (flow_io.read_png, any PNG reader).  One ops.png_encode call on the current stream; the n stream lengths are copied first, then
    only the used bytes of every slot (pinned memory); flow_io.png_file and the file writes run in the thread pool.  Returns the
    files' sizes in bytes."""
    from . import ops
    paths = list(paths)
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or len(paths) != images.shape[0] or not paths:
        raise ValueError(f"png_gpu.encode_batch: images [n, H, W, C] and n paths (got {getattr(images, 'shape', type(images).__name__)}, "
                         f"{len(paths)} paths)")
    _need_gpu(images.device)
    n, h, w, c = (int(v) for v in images.shape)
    depth = 8 * images.element_size()
    streams, lengths = ops.png_encode(images)
    used = [int(v) for v in lengths.cpu()]
    start = [sum(used[:i]) for i in range(n)]
    host = torch.empty(sum(used), dtype=torch.uint8, pin_memory=True)
    for i in range(n):
        host[start[i]:start[i] + used[i]].copy_(streams[i, :used[i]], non_blocking=True)
    torch.cuda.current_stream(images.device).synchronize()
    data = host.numpy()

    def write(i: int) -> int:
        blob = flow_io.png_file(data[start[i]:start[i] + used[i]].tobytes(), h, w, depth, c)
        with open(paths[i], "wb") as f:
            f.write(blob)
        return len(blob)

    k = min(pool_threads(threads), n)
    if k == 1:
        return [write(i) for i in range(n)]
    with ThreadPoolExecutor(max_workers=k) as ex:
        return list(ex.map(write, range(n)))
