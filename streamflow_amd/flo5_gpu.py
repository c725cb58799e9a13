"""Spring .flo5 files to and from the GPU.

`read_batch`: the chunks of a batch of files inflated by one sf_inflate call (a wave per zlib stream) and put together by one
sf_flo5_assemble call per geometry (csrc/flo5_decode.hip); the host only walks the HDF5 index (flo5.chunk_table) and uploads the
compressed bytes.  What the device path does not take goes through flo5.read_flo5, with the same values.

`write_batch`: the HDF5 filters shuffle -> deflate of every chunk of every field as one
sf_flo5_encode call for the whole batch (csrc/flo5_encode.hip: byte shuffle, Huffman-only deflate); only the compressed chunk
streams cross to the host, where the container framing (flo5.flo5_file) and the file writes run in png_gpu's thread pool.

The files hold the same float32 [H, W, 2] dataset 'flow' as flo5.write_flo5's, bit for bit, with another filter pipeline (shuffle,
then deflate with client value 1: the streams start `78 01`); h5py undoes both filters on reading.  There is no fallback: without a
GPU `write_batch` raises; flo5.write_flo5 stays the host-side writer.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
import zlib
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import flo5
from .png_gpu import pool_threads

# read_batch inflates a file on the host when one of its chunks is larger than this many bytes (raw).  One wave decodes one chunk, so
# a file of few large chunks (flo5.write_flo5 and write_batch make at most 64, of up to 2 MB) keeps few waves busy for long while the
# host pool inflates it at zlib's speed; a file h5py wrote is a thousand chunks of 65 280 bytes.  Measured (MI355X, pool of 8 threads,
# one synthetic 2160 x 3840 field in row chunks, read_batch end to end, device inflate / host inflate, profiles/flo5_decode_bench.jsonl):
# 61 440 B 50 / 192 ms, 122 880 B 73 / 197 ms, 245 760 B 109 / 193 ms, 522 240 B 210 / 193 ms, 1 044 480 B 400 / 195 ms, 2 088 960 B
# 784 / 193 ms.  The device time grows with the chunk, the host time does not; they cross near 480 000 B.
HOST_INFLATE_CHUNK_BYTES = 448 * 1024
# the faster of the two on h5py-layout files in the same run: 94 ms (85 - 106) against 263 ms (247 - 265) for three fields
DEFAULT_INFLATE = "gpu"

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


# ---- reading ------------------------------------------------------------------------------------------------------------------------
def _device_plan(table: dict):
    """What the device path needs of a chunk_table, or None for a file it does not take (-> flo5.read_flo5): the geometry
    (H, W, ch, cw, cc, shuffle) and per stored chunk (grid cell, address, nbytes, stored as is)."""
    shape, cs, filters = table["shape"], table["chunk_shape"], list(table["filters"])
    if not table["chunked"] or table["dtype"] != np.dtype("<f4") or len(shape) != 3 or shape[2] != 2:
        return None
    if filters not in ([], [1], [2], [2, 1]) or min(shape) < 1 or shape[0] > 65535 or min(cs) < 1 or cs[2] not in (1, 2):
        return None
    if 4 * cs[0] * cs[1] * cs[2] >= 1 << 31:
        return None
    shuffle = 2 in filters
    deflate_bit = 1 << filters.index(1) if 1 in filters else 0
    gy, gx, gc = -(-shape[0] // cs[0]), -(-shape[1] // cs[1]), 2 // cs[2]
    entries, seen = [], set()
    for offs, addr, nbytes, mask in table["chunks"]:
        if mask & ~deflate_bit:                                                # a skipped shuffle stage: the host reader's case
            return None
        cell = tuple(o // c for o, c in zip(offs, cs))
        if any(o % c for o, c in zip(offs, cs)) or cell[0] >= gy or cell[1] >= gx or cell[2] >= gc or cell in seen:
            return None
        seen.add(cell)
        entries.append(((cell[0] * gx + cell[1]) * gc + cell[2], offs, addr, nbytes, not deflate_bit or bool(mask & deflate_bit)))
    return (shape[0], shape[1], cs[0], cs[1], cs[2], shuffle), entries


def read_batch(paths: Sequence[str], device, threads: Optional[int] = None, inflate: Optional[str] = None) -> List[torch.Tensor]:
    """The .flo5 files `paths` -> one tensor per file on `device`, tensor i bit for bit torch.from_numpy(flo5.read_flo5(paths[i]))
    (NaN payloads included), for every file read_flo5 reads.

    The files are read and indexed (flo5.chunk_table) in png_gpu's thread pool.  inflate="gpu": the compressed chunks of the whole
    batch go into one pinned buffer and one upload, ONE ops.inflate call decodes them (a wave per chunk), ops.flo5_assemble runs once
    per geometry present (shape, chunk shape, shuffle), and one small copy brings the status words back -- that copy synchronises
    with the host, and it is what lets a corrupt file raise: any non-zero status is an IOError naming the file, the chunk's offsets
    and the status.  inflate="host": the pool inflates with zlib, the raw chunks are uploaded and only the assemble kernel runs (the
    split of png_gpu.decode_batch).  inflate=None: DEFAULT_INFLATE.  Whatever `inflate` says, a file with a chunk of more than
    HOST_INFLATE_CHUNK_BYTES raw bytes is inflated on the host (this project's own writers make such files: at most 64 chunks, little
    for a wave per chunk to share out).

    The device path takes little-endian float32 datasets of shape (H, W, 2), chunked with a chunk shape (ch, cw, 1 or 2), filters
    deflate and / or shuffle.  Everything else read_flo5 reads (other types, contiguous or compact layouts, other ranks, a chunk whose
    filter mask skips the shuffle) goes through flo5.read_flo5 and one upload, with its values and dtype.  The device path is STRICT
    where the host reader is lax: a chunk must inflate to exactly the chunk's size (read_flo5 ignores extra bytes); libhdf5 never
    writes such a chunk.  There is no CPU fallback: `device` must be a GPU."""
    from . import ops
    from .png_gpu import _need_gpu
    mode = DEFAULT_INFLATE if inflate is None else inflate
    if mode not in ("gpu", "host"):
        raise ValueError(f"flo5_gpu.read_batch: inflate must be 'gpu' or 'host' (got {inflate!r})")
    paths = [str(p) for p in paths]
    if not paths:
        return []
    dev = _need_gpu(device)

    def load(path: str):
        table = flo5.chunk_table(path)
        plan = _device_plan(table)
        if plan is None:
            a = flo5.read_flo5(path)
            return None, np.ascontiguousarray(a.astype(a.dtype.newbyteorder("="), copy=False)), None
        geom, entries = plan
        size = 4 * geom[2] * geom[3] * geom[4]
        raw = None
        if mode == "host" or size > HOST_INFLATE_CHUNK_BYTES:
            raw = []
            for _, offs, addr, nbytes, stored in entries:
                blob = table["data"][addr:addr + nbytes]
                try:
                    blob = blob if stored else zlib.decompress(blob)
                except zlib.error as e:
                    raise IOError(f"{path}: chunk at offsets {offs} does not inflate: {e}") from None
                if len(blob) != size:
                    raise IOError(f"{path}: chunk at offsets {offs} holds {len(blob)} bytes, not the chunk's {size}")
                raw.append(blob)
        return plan, table["data"], raw

    k = min(pool_threads(threads), len(paths))
    if k == 1:
        loaded = [load(p) for p in paths]
    else:
        with ThreadPoolExecutor(max_workers=k) as ex:
            loaded = list(ex.map(load, paths))

    result: List[Optional[torch.Tensor]] = [None] * len(paths)
    geoms = {}                                                                  # geometry -> [file index]
    for i, (plan, data, _) in enumerate(loaded):
        if plan is None:
            result[i] = torch.from_numpy(data).to(dev)
        else:
            geoms.setdefault(plan[0], []).append(i)
    with torch.cuda.device(dev):
        # slots of the device-inflated geometries share one buffer (one sf_inflate call); each region starts at a multiple of 16
        comp_bytes = out_bytes = 0
        desc, who, regions = [], [], {}
        for geom, files in geoms.items():
            size = 4 * geom[2] * geom[3] * geom[4]
            if loaded[files[0]][2] is not None:
                continue
            regions[geom] = out_bytes
            slot = 0
            for i in files:
                for _, offs, addr, nbytes, stored in loaded[i][0][1]:
                    desc.append((comp_bytes, nbytes, out_bytes + slot * size, size, ops.INFLATE_STORED if stored else 0))
                    who.append((i, offs))
                    comp_bytes += nbytes
                    slot += 1
            out_bytes = (out_bytes + slot * size + 15) // 16 * 16
        status = None
        inflated = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
        if desc:
            host = torch.empty(comp_bytes, dtype=torch.uint8, pin_memory=True)
            hv = host.numpy()
            at = 0
            for geom in regions:
                for i in geoms[geom]:
                    data = loaded[i][1]
                    for _, _, addr, nbytes, _ in loaded[i][0][1]:
                        hv[at:at + nbytes] = np.frombuffer(data, np.uint8, nbytes, addr)
                        at += nbytes
            comp = host.to(dev, non_blocking=True)
            status = ops.inflate(comp, torch.tensor(desc, dtype=torch.int64).to(dev), inflated)
        outs = {}
        for geom, files in geoms.items():
            H, W, ch, cw, cc, shuffle = geom
            size = 4 * ch * cw * cc
            cells = -(-H // ch) * -(-W // cw) * (2 // cc)
            grid = np.full((len(files), cells), -1, np.int32)
            slot = 0
            for j, i in enumerate(files):
                for cell, *_ in loaded[i][0][1]:
                    grid[j, cell] = slot
                    slot += 1
            if geom in regions:
                chunks = inflated[regions[geom]:regions[geom] + slot * size].view(slot, size)
            else:
                raw = torch.empty(slot * size, dtype=torch.uint8, pin_memory=True)
                rv, at = raw.numpy(), 0
                for i in files:
                    for blob in loaded[i][2]:
                        rv[at:at + size] = np.frombuffer(blob, np.uint8)
                        at += size
                chunks = raw.to(dev, non_blocking=True).view(slot, size)
            g = torch.from_numpy(grid.reshape(len(files), -(-H // ch), -(-W // cw), 2 // cc)).to(dev)
            outs[geom] = ops.flo5_assemble(chunks, g, H, W, (ch, cw, cc), shuffle)
        if status is not None:
            st = status.cpu()                                                   # the one synchronisation: a corrupt chunk raises here
            bad = torch.nonzero(st).reshape(-1)
            if bad.numel():
                b = int(bad[0])
                code = int(st[b])
                name = ops.INFLATE_STATUS[code] if 0 <= code < len(ops.INFLATE_STATUS) else "?"
                raise IOError(f"{paths[who[b][0]]}: chunk at offsets {who[b][1]} does not inflate on the GPU: status {code} ({name})"
                              + (f"; {int(bad.numel()) - 1} more chunks failed" if bad.numel() > 1 else ""))
        else:
            torch.cuda.current_stream(dev).synchronize()                        # the pinned buffers are free to go
    for geom, files in geoms.items():
        for j, i in enumerate(files):
            result[i] = outs[geom][j]
    return result
