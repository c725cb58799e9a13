#!/usr/bin/env python3
"""PNG decode, host against GPU, on files with adaptive row filters (what libpng writes; flow_io.write_png writes type 0 only).

    python tools/png_decode_bench.py [--host-frames 2] [--launches 50] [--windows 5] [--runs 5] [--out FILE]

17 frames of 436 x 1024 x 3 (the frames of 8 clips at T = 3) of uniform random bytes, written by the test encoder
(tests/png_cases.py) with every row Paeth, every row Average, and the type drawn per row; then 8 KITTI-shape files, 16-bit RGB
375 x 1242, types drawn per row.  Per set, in one run on one box:
  host_read_png_ms_per_frame   flow_io.read_png, the mean over --host-frames files (the Paeth / Average branches are Python loops)
  inflate_ms_per_frame         flow_io.png_scanlines (file read, CRC, zlib) one file after the other, and through png_gpu's thread pool
  upload_ms                    the batch's scanline blocks, host -> device, ending in a synchronise
  kernel_ms                    sf_png_unfilter alone for the whole batch: device events around --launches launches after a warm-up,
                               the median of --windows windows
  decode_batch_ms              png_gpu.decode_batch end to end (inflate pool, one upload, one launch) ending in a synchronise, the
                               median of --runs
One JSON line per set; the last line states the condition the kernel is held to: for the all-Paeth frames its time for the batch
is below the single-threaded inflate time of the same files.  Needs no dataset; a GPU is required (no fallback)."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from streamflow_amd import flow_io, ops, png_gpu
from tests import png_cases as pc

SETS = [("sintel_paeth", 17, 436, 1024, 3, 8, 4), ("sintel_average", 17, 436, 1024, 3, 8, 3), ("sintel_mixed", 17, 436, 1024, 3, 8, "mixed"),
        ("kitti_16bit_mixed", 8, 375, 1242, 3, 16, "mixed")]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--host-frames", type=int, default=2, help="files timed through flow_io.read_png per set (about a second each)")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("png_decode_bench needs the GPU; there is no CPU fallback")
    if a.launches < 50 or a.windows < 1:
        raise ValueError("--launches at least 50, --windows at least 1")
    from bench import usable_cores
    torch.set_num_threads(min(usable_cores(), 64))
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    paeth = None
    with tempfile.TemporaryDirectory() as tmp:
        for name, n, h, w, c, depth, how in SETS:
            paths = []
            for i in range(n):
                paths.append(os.path.join(tmp, f"{name}_{i:02d}.png"))
                pc.encode(pc.image(h, w, c, depth, 1000 + i), pc.filter_types(how, h, i), paths[-1], depth)
            t0 = time.perf_counter()
            host = [flow_io.read_png(p) for p in paths[:a.host_frames]]
            read_ms = (time.perf_counter() - t0) * 1e3 / max(1, len(host))
            for p in paths:                                             # page cache warm for both inflate timings
                flow_io.png_scanlines(p)
            t0 = time.perf_counter()
            got = [flow_io.png_scanlines(p) for p in paths]
            inflate_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            png_gpu.inflate(paths)
            pooled_ms = (time.perf_counter() - t0) * 1e3
            bpp = c * depth // 8
            block = np.stack([g[0] for g in got])
            torch.from_numpy(block).to(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scan = torch.from_numpy(block).to(dev)
            torch.cuda.synchronize()
            upload_ms = (time.perf_counter() - t0) * 1e3
            out = torch.empty(n, h, w * bpp, dtype=torch.uint8, device=dev)
            for _ in range(5):
                ops.png_unfilter(scan, h, w, bpp, out=out, swap16=depth == 16)
            torch.cuda.synchronize()
            windows = []
            for _ in range(a.windows):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.launches):
                    ops.png_unfilter(scan, h, w, bpp, out=out, swap16=depth == 16)
                e.record()
                e.synchronize()
                windows.append(s.elapsed_time(e) / a.launches)
            kernel_ms = float(np.median(windows))
            res = png_gpu.decode_batch(paths, dev)
            torch.cuda.synchronize()
            for i, img in enumerate(host):                              # the timed path decodes what the host decodes
                want = torch.from_numpy(img.view(np.int16) if depth == 16 else img)
                assert torch.equal((res[i].view(torch.int16) if depth == 16 else res[i]).cpu(), want), (name, i)
            e2e = []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                png_gpu.decode_batch(paths, dev)
                torch.cuda.synchronize()
                e2e.append((time.perf_counter() - t0) * 1e3)
            rec = {"set": name, "files": n, "shape": [h, w, c], "depth": depth, "filters": how if how == "mixed" else int(how),
                   "host_read_png_ms_per_frame": round(read_ms, 2), "inflate_ms_per_frame": round(inflate_ms / n, 3),
                   "inflate_pooled_ms_per_frame": round(pooled_ms / n, 3), "pool_threads": png_gpu.pool_threads(),
                   "inflate_ms_batch": round(inflate_ms, 2), "upload_ms": round(upload_ms, 3), "kernel_ms": round(kernel_ms, 4),
                   "kernel_ms_windows": [round(x, 4) for x in windows], "kernel_GBps_written": round(n * h * w * bpp / kernel_ms / 1e6, 2),
                   "decode_batch_ms": round(float(np.median(e2e)), 2),
                   "read_png_loop_over_decode_batch": round(read_ms * n / float(np.median(e2e)), 1)}
            emit(rec)
            if name == "sintel_paeth":
                paeth = rec
    ok = paeth["kernel_ms"] < paeth["inflate_ms_batch"]
    emit({"condition": "kernel_ms < single-threaded inflate of the same 17 all-Paeth files", "kernel_ms": paeth["kernel_ms"],
          "inflate_ms_batch": paeth["inflate_ms_batch"], "holds": bool(ok)})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
