"""Baseline JPEG files from device images.  The colour conversion, the DCT, the quantisation and the Huffman coding of a whole batch
are one sf_jpeg_encode call (csrc/jpeg_encode.hip); only the entropy-coded segments cross to the host, where `jpeg_file` puts the
marker segments around them: SOI, APP0 (JFIF 1.01), DQT, SOF0 (4:4:4), the four typical Huffman tables of T.81 Annex K.3 as DHT, DRI
(one restart interval per MCU row), SOS, the segment, EOI.  The files are what avi.MjpegWriter takes as frames.

There is no fallback: without a GPU `encode_batch` raises.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

from .png_gpu import pool_threads

# T.81 Annex K.1: the luminance and chrominance quantisation tables, natural (row-major) order
K1_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
           100, 103, 99)
K1_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) \
    + (99,) * 32

# scan position k -> natural index
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)

# T.81 Annex K.3: (table class << 4 | destination, BITS, HUFFVAL) in the order the DHT segments are written
_AC_LUMA = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546474849"
    "4a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
    "c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFFMAN_TABLES = ((0x00, bytes((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)), bytes(range(12))),
                  (0x10, bytes((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125)), _AC_LUMA),
                  (0x01, bytes((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)), bytes(range(12))),
                  (0x11, bytes((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119)), _AC_CHROMA))


def quant_tables(quality: int) -> np.ndarray:
    """uint16 [2, 64], natural order: the Annex K.1 tables scaled as the IJG library scales them (jpeg_quality_scaling):
    s = 5000 // quality below 50, else 200 - 2 quality; (t s + 50) // 100 clamped to 1 .. 255.  quality: 1 .. 100."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"jpeg quality must be in 1 .. 100, got {quality}")
    s = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([K1_LUMA, K1_CHROMA], np.int64)
    return np.clip((base * s + 50) // 100, 1, 255).astype(np.uint16)


def _check_tables(qtables) -> np.ndarray:
    q = np.ascontiguousarray(np.asarray(qtables)).reshape(-1)
    if q.size != 128 or q.min() < 1 or q.max() > 255:
        raise ValueError("qtables: two tables of 64 steps in 1 .. 255 (natural order)")
    return q.astype(np.uint16).reshape(2, 64)


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes((0xFF, marker)) + (len(payload) + 2).to_bytes(2, "big") + payload


def dht_segments(channels: int = 3) -> List[bytes]:
    """The DHT marker segments of a file: DC and AC luma, and for colour DC and AC chroma; one table per segment."""
    return [_segment(0xC4, bytes((tc,)) + bits + vals) for tc, bits, vals in HUFFMAN_TABLES[:4 if channels == 3 else 2]]


def jpeg_file(segment: bytes, h: int, w: int, channels: int, qtables) -> bytes:
    """The JFIF file around one entropy-coded segment of sf_jpeg_encode (h x w, channels 1 or 3, the qtables it was made with)."""
    if channels not in (1, 3) or not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"jpeg_file: h = {h}, w = {w}, channels = {channels}")
    q = _check_tables(qtables)
    nt = 2 if channels == 3 else 1
    parts = [b"\xff\xd8", _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    parts += [_segment(0xDB, bytes((t,)) + bytes(int(q[t, z]) for z in ZIGZAG)) for t in range(nt)]
    comps = b"".join(bytes((c + 1, 0x11, 1 if c else 0)) for c in range(channels))
    parts.append(_segment(0xC0, b"\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes((channels,)) + comps))
    parts += dht_segments(channels)
    parts.append(_segment(0xDD, ((w + 7) // 8).to_bytes(2, "big")))
    scan = b"".join(bytes((c + 1, 0x11 if c else 0x00)) for c in range(channels))
    parts.append(_segment(0xDA, bytes((channels,)) + scan + b"\x00\x3f\x00"))
    parts += [bytes(segment), b"\xff\xd9"]
    return b"".join(parts)


def encode_batch(images: torch.Tensor, paths: Optional[Sequence[str]] = None, quality: int = 90,
                 threads: Optional[int] = None) -> List[bytes]:
    """Device images uint8 [n, H, W, 3] or [n, H, W] -> n JPEG files as bytes (written to `paths` where given), at the IJG quality
    `quality`.  One ops.jpeg_encode call on the current stream; the n segment lengths are copied first, then only the used bytes of
    every slot (pinned memory); the framing and the file writes run in the thread pool."""
    from . import ops
    if not isinstance(images, torch.Tensor) or images.dim() not in (3, 4) or images.shape[0] == 0:
        raise ValueError(f"jpeg_gpu.encode_batch: images [n, H, W, 3] or [n, H, W] (got {getattr(images, 'shape', type(images).__name__)})")
    if paths is not None:
        paths = list(paths)
        if len(paths) != images.shape[0]:
            raise ValueError(f"jpeg_gpu.encode_batch: {images.shape[0]} images, {len(paths)} paths")
    if not images.is_cuda or not torch.cuda.is_available():
        raise RuntimeError(f"jpeg_gpu encodes on the GPU (device {images.device}, GPU available: {torch.cuda.is_available()}); "
                           "there is no CPU fallback")
    n, h, w = (int(v) for v in images.shape[:3])
    channels = 3 if images.dim() == 4 else 1
    q = quant_tables(quality)
    segments, lengths = ops.jpeg_encode(images, q)
    used = [int(v) for v in lengths.cpu()]
    start = [sum(used[:i]) for i in range(n)]
    host = torch.empty(sum(used), dtype=torch.uint8, pin_memory=True)
    for i in range(n):
        host[start[i]:start[i] + used[i]].copy_(segments[i, :used[i]], non_blocking=True)
    torch.cuda.current_stream(images.device).synchronize()
    data = host.numpy()

    def frame(i: int) -> bytes:
        blob = jpeg_file(data[start[i]:start[i] + used[i]].tobytes(), h, w, channels, q)
        if paths is not None:
            with open(paths[i], "wb") as f:
                f.write(blob)
        return blob

    k = min(pool_threads(threads), n)
    if k == 1:
        return [frame(i) for i in range(n)]
    with ThreadPoolExecutor(max_workers=k) as ex:
        return list(ex.map(frame, range(n)))
