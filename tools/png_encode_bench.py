#!/usr/bin/env python3
"""PNG output, the host writer against the GPU encoder, on the images the demo and the submission writers produce.

    python tools/png_encode_bench.py [--launches 20] [--windows 5] [--runs 5] [--out FILE]

24 colour-wheel images of 436 x 1024 x 3 (the fields of one model step at 8 clips of T = 4, DESIGN.md 9.5: ops.flow_to_image of
smooth synthetic fields, tests/png_encode_cases.smooth_field) and 8 KITTI code images of 375 x 1242 (ops.flow_to_kitti16).  Per
set, in one run on one box, everything starting from the images on the device:
  host_loop_ms       the path before the GPU encoder: one .cpu() copy of the batch, then flow_io.write_png per image (filter 0,
                     zlib level 6, one thread), the files written; the median of --runs
  kernel_ms          sf_png_encode alone for the whole batch (its memset and four launches; output and workspace allocated once):
                     device events around --launches calls after a warm-up, the median of --windows windows
  encode_batch_ms    png_gpu.encode_batch end to end (allocation, the call, lengths and used bytes to the host, framing, CRC and
                     file writes in the thread pool), the median of --runs
  host_bytes / gpu_bytes   the sizes of the files of both paths
The files of the GPU path are read back (flow_io.read_png) and compared with the device images before anything is timed.  One JSON
line per set; the last line is the ratio of the two end-to-end times.  Needs no dataset; a GPU is required (no fallback)."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from streamflow_amd import _lib, flow_io, ops, png_gpu
from tests import png_encode_cases as ec

SETS = [("colour_wheel_rgb8", 24, 436, 1024), ("kitti_codes_rgb16", 8, 375, 1242)]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("png_encode_bench needs the GPU; there is no CPU fallback")
    if a.launches < 10 or a.windows < 1 or a.runs < 1:
        raise ValueError("--launches at least 10, --windows and --runs at least 1")
    from bench import usable_cores
    torch.set_num_threads(min(usable_cores(), 64))
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    ratios = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, n, h, w in SETS:
            flows = torch.from_numpy(np.stack([ec.smooth_field(h, w, 100 + i) for i in range(n)])).to(dev)
            images = ops.flow_to_kitti16(flows) if "kitti" in name else ops.flow_to_image(flows)
            torch.cuda.synchronize()
            host_paths = [os.path.join(tmp, f"{name}_host_{i:02d}.png") for i in range(n)]
            gpu_paths = [os.path.join(tmp, f"{name}_gpu_{i:02d}.png") for i in range(n)]

            def host_loop():
                arr = images.cpu().numpy()
                for i, p in enumerate(host_paths):
                    flow_io.write_png(p, arr[i])

            png_gpu.encode_batch(images, gpu_paths)                         # warm-up, and the check of what is timed
            want = images.cpu().numpy()
            for i in (0, n - 1):
                assert np.array_equal(flow_io.read_png(gpu_paths[i]), want[i]), (name, i)
            host_ms, e2e_ms = [], []
            for _ in range(a.runs):                                         # the two paths in turn
                t0 = time.perf_counter()
                host_loop()
                host_ms.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                png_gpu.encode_batch(images, gpu_paths)
                e2e_ms.append((time.perf_counter() - t0) * 1e3)
            bpp = 3 * images.element_size()
            bound, ws_bytes = lib.sf_png_encode_bound(h, w, bpp), lib.sf_png_encode_ws_bytes(n, h, w, bpp)
            out = torch.empty(n, bound, dtype=torch.uint8, device=dev)
            lengths = torch.empty(n, dtype=torch.int64, device=dev)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

            def call():
                _lib.check(lib.sf_png_encode(images.data_ptr(), h * w * bpp, w * bpp, n, h, w, bpp, 1 if bpp == 6 else 0, out.data_ptr(),
                                             bound, lengths.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream()), "sf_png_encode")

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
            rec = {"set": name, "images": n, "shape": [h, w, 3], "depth": 8 * images.element_size(), "pool_threads": png_gpu.pool_threads(),
                   "host_loop_ms": round(float(np.median(host_ms)), 1), "host_loop_ms_runs": [round(x, 1) for x in host_ms],
                   "kernel_ms": round(kernel_ms, 4), "kernel_ms_windows": [round(x, 4) for x in windows],
                   "kernel_GBps_read": round(n * h * w * bpp / kernel_ms / 1e6, 2),
                   "encode_batch_ms": round(float(np.median(e2e_ms)), 2), "encode_batch_ms_runs": [round(x, 2) for x in e2e_ms],
                   "host_bytes": host_bytes, "gpu_bytes": gpu_bytes, "gpu_over_host_bytes": round(gpu_bytes / host_bytes, 3),
                   "host_loop_over_encode_batch": round(float(np.median(host_ms)) / float(np.median(e2e_ms)), 1)}
            emit(rec)
            ratios[name] = rec["host_loop_over_encode_batch"]
    faster = all(r > 1 for r in ratios.values())
    emit({"condition": "encode_batch end to end is faster than the .cpu() + write_png loop on both sets", "ratios": ratios,
          "holds": bool(faster)})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
