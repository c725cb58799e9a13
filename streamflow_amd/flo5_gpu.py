"""Spring .flo5 files from flows on the GPU.  `write_batch`: the HDF5 filters shuffle -> deflate of every chunk of every field as one
sf_flo5_encode call for the whole batch (csrc/flo5_encode.hip: byte shuffle, Huffman-only deflate); only the compressed chunk
streams cross to the host, where the container framing (flo5.flo5_file) and the file writes run in png_gpu's thread pool.

The files hold the same float32 [H, W, 2] dataset 'flow' as flo5.write_flo5's, bit for bit, with another filter pipeline (shuffle,
then deflate with client value 1: the streams start `78 01`); h5py undoes both filters on reading.  There is no fallback: without a
GPU `write_batch` raises; flo5.write_flo5 stays the host-side writer.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import torch

from . import flo5
from .png_gpu import pool_threads

DEFLATE_LEVEL = 1          # deflate's client value in the files: what `78 01` says (h5py reports it as compression_opts)


def write_batch(flows: torch.Tensor, paths: Sequence[str], threads: Optional[int] = None, rows_per_chunk: int = 0) -> List[int]:
    """Device flows fp32 [n, 2, H, W] (unit x stride; any other strides, as ops.flo5_encode takes them) -> the .flo5 files `paths`,
    file i reading back (flo5.read_flo5, h5py) as flows[i].permute(1, 2, 0) bit for bit.  One ops.flo5_encode call on the current
    stream; the chunk lengths are copied first, then only the used bytes of every slot (pinned memory); flo5.flo5_file and the file
    writes run in the thread pool.  Returns the files' sizes in bytes."""
    from . import ops
    paths = list(paths)
    if not isinstance(flows, torch.Tensor) or flows.dim() != 4 or len(paths) != flows.shape[0] or not paths:
        raise ValueError(f"flo5_gpu.write_batch: flows [n, 2, H, W] and n paths (got {getattr(flows, 'shape', type(flows).__name__)}, "
                         f"{len(paths)} paths)")
    n, _, h, w = (int(v) for v in flows.shape)
    rpc = int(rows_per_chunk) if rows_per_chunk else max(1, -(-h // 32))            # flo5.write_flo5's rule
    streams, lengths = ops.flo5_encode(flows, rpc)
    nchunks = int(lengths.shape[1])
    used = [int(v) for v in lengths.cpu().reshape(-1)]
    start = [0] * (len(used) + 1)
    for k, u in enumerate(used):
        start[k + 1] = start[k] + u
    host = torch.empty(start[-1], dtype=torch.uint8, pin_memory=True)
    flat = streams.view(n * nchunks, -1)
    for k, u in enumerate(used):
        host[start[k]:start[k] + u].copy_(flat[k, :u], non_blocking=True)
    torch.cuda.current_stream(flows.device).synchronize()
    data = host.numpy()

    def write(i: int) -> int:
        chunks = [data[start[k]:start[k + 1]].tobytes() for k in range(i * nchunks, (i + 1) * nchunks)]
        blob = flo5.flo5_file(chunks, h, w, rpc, shuffle=True, level=DEFLATE_LEVEL)
        with open(paths[i], "wb") as f:
            f.write(blob)
        return len(blob)

    k = min(pool_threads(threads), n)
    if k == 1:
        return [write(i) for i in range(n)]
    with ThreadPoolExecutor(max_workers=k) as ex:
        return list(ex.map(write, range(n)))
