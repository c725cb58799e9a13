#!/usr/bin/env python3
"""Spring .flo5 output, the host writer against the GPU encoder, at Spring's frame size.

    python tools/flo5_encode_bench.py [--launches 20] [--windows 5] [--runs 3] [--out profiles/flo5_encode_bench.jsonl]
    python tools/flo5_encode_bench.py --block-sizes          # CPU only: stream sizes at 16 / 64 / 256 KiB blocks

Three fields of 1080 x 1920 (one Spring clip of T = 4).  The data is SYNTHETIC (tests/flo5_encode_cases.bench_field: a seeded
bilinear upsampling of coarse Gaussian noise plus 0.01 px of noise); no Spring frame or model output is involved, and real flow
compresses differently.  In one run on one box, everything starting from the flows on the device:
  host_loop_ms       the path before the GPU encoder, as create_spring_submission_mf(flo5_encode="host") runs it: per field
                     .permute(1, 2, 0).float().cpu().numpy() and flo5.write_flo5 (gzip level 5, one thread), the files written; the
                     median of --runs
  kernel_ms          sf_flo5_encode alone for the batch (its memset and four launches; output and workspace allocated once): device
                     events around --launches calls after a warm-up, the median of --windows windows
  write_batch_ms     flo5_gpu.write_batch end to end (allocation, the call, lengths and used bytes to the host, framing and file
                     writes in the thread pool), the median of --runs
  host_bytes / gpu_bytes   the sizes of the files of both paths, and of the raw float32 data
The files of the GPU path are read back (flo5.read_flo5) and compared bit for bit with the device flows before anything is timed.
One JSON line; a GPU is required (no fallback) except for --block-sizes."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tests import flo5_encode_cases as fc

N_FIELDS, H, W = 3, 1080, 1920


def fields():
    return np.stack([fc.bench_field(H, W, 200 + i) for i in range(N_FIELDS)])


def block_sizes() -> dict:
    """Total stream bytes of the bench fields' chunks under the Python restatement, per block size."""
    rpc = fc.default_rows_per_chunk(H)
    sizes = {bb: 0 for bb in (16384, 65536, 262144)}
    for f in fields():
        for c in range(-(-H // rpc)):
            data = fc.shuffled(f, c, rpc)
            for bb in sizes:
                sizes[bb] += 2 + -(-fc.stream_bits(data, bb) // 8) + 4
    raw = N_FIELDS * H * W * 8
    return {"data": "synthetic", "fields": N_FIELDS, "shape": [H, W], "rows_per_chunk": rpc, "raw_bytes": raw,
            "stream_bytes": {str(bb): v for bb, v in sizes.items()},
            "over_raw": {str(bb): round(v / raw, 4) for bb, v in sizes.items()},
            "over_64k": {str(bb): round(v / sizes[65536], 4) for bb, v in sizes.items()}}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--block-sizes", action="store_true", help="CPU only: the stream sizes at 16 / 64 / 256 KiB blocks")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args(argv)
    if a.block_sizes:
        print(json.dumps(block_sizes()), flush=True)
        return 0
    if not torch.cuda.is_available():
        raise RuntimeError("flo5_encode_bench needs the GPU; there is no CPU fallback")
    if a.launches < 10 or a.windows < 1 or a.runs < 1:
        raise ValueError("--launches at least 10, --windows and --runs at least 1")
    from bench import usable_cores
    from streamflow_amd import _lib, flo5, flo5_gpu, png_gpu
    torch.set_num_threads(min(usable_cores(), 64))
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    host_fields = fields()
    flows = torch.from_numpy(host_fields).to(dev)
    torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as tmp:
        host_paths = [os.path.join(tmp, f"host_{i}.flo5") for i in range(N_FIELDS)]
        gpu_paths = [os.path.join(tmp, f"gpu_{i}.flo5") for i in range(N_FIELDS)]

        def host_loop():
            for i, p in enumerate(host_paths):
                flo5.write_flo5(p, flows[i].permute(1, 2, 0).float().cpu().numpy(), compression_level=5)

        flo5_gpu.write_batch(flows, gpu_paths)                              # warm-up, and the check of what is timed
        for i in (0, N_FIELDS - 1):
            got = flo5.read_flo5(gpu_paths[i])
            assert np.array_equal(got.view(np.uint32), host_fields[i].transpose(1, 2, 0).view(np.uint32)), i
        host_ms, e2e_ms = [], []
        for _ in range(a.runs):                                             # the two paths in turn
            t0 = time.perf_counter()
            host_loop()
            host_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            flo5_gpu.write_batch(flows, gpu_paths)
            e2e_ms.append((time.perf_counter() - t0) * 1e3)
        rpc = fc.default_rows_per_chunk(H)
        nchunks = -(-H // rpc)
        bound, ws_bytes = lib.sf_flo5_chunk_bound(rpc, W), lib.sf_flo5_encode_ws_bytes(N_FIELDS, H, W, rpc)
        out = torch.empty(N_FIELDS * nchunks, bound, dtype=torch.uint8, device=dev)
        lengths = torch.empty(N_FIELDS * nchunks, dtype=torch.int64, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

        def call():
            _lib.check(lib.sf_flo5_encode(flows.data_ptr(), 2 * H * W, H * W, W, N_FIELDS, H, W, rpc, out.data_ptr(), bound,
                                          lengths.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream()), "sf_flo5_encode")

        for _ in range(3):
            call()
        torch.cuda.synchronize()
        windows = []
        for _ in range(a.windows):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.launches):
                call()
            e.record()
            e.synchronize()
            windows.append(s.elapsed_time(e) / a.launches)
        kernel_ms = float(np.median(windows))
        host_bytes, gpu_bytes = sum(map(os.path.getsize, host_paths)), sum(map(os.path.getsize, gpu_paths))
    raw = N_FIELDS * H * W * 8
    rec = {"bench": "flo5_encode", "data": "synthetic (bilinear upsampling of coarse Gaussian noise + 0.01 px noise)",
           "fields": N_FIELDS, "shape": [H, W], "rows_per_chunk": rpc, "pool_threads": png_gpu.pool_threads(),
           "host_loop_ms": round(float(np.median(host_ms)), 1), "host_loop_ms_runs": [round(x, 1) for x in host_ms],
           "kernel_ms": round(kernel_ms, 4), "kernel_ms_windows": [round(x, 4) for x in windows],
           "kernel_GBps_read": round(raw / kernel_ms / 1e6, 2),
           "write_batch_ms": round(float(np.median(e2e_ms)), 2), "write_batch_ms_runs": [round(x, 2) for x in e2e_ms],
           "raw_bytes": raw, "host_bytes": host_bytes, "gpu_bytes": gpu_bytes, "gpu_over_host_bytes": round(gpu_bytes / host_bytes, 3),
           "host_over_raw": round(host_bytes / raw, 3), "gpu_over_raw": round(gpu_bytes / raw, 3),
           "host_loop_over_write_batch": round(float(np.median(host_ms)) / float(np.median(e2e_ms)), 1)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
