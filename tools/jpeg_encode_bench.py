#!/usr/bin/env python3
"""JPEG / Motion-JPEG output on the GPU against a PIL (libjpeg) loop on the host, on the images the demo produces.

    python tools/jpeg_encode_bench.py [--launches 20] [--windows 5] [--runs 5] [--quality 90] [--out profiles/jpeg_encode_bench.jsonl]

24 colour-wheel images of 436 x 1024 x 3 (the fields of one model step at 8 clips of T = 4: ops.flow_to_image of smooth synthetic
fields, tests/png_encode_cases.smooth_field) and three of 1088 x 1920 x 3.  Per set, in one run on one box, everything starting from
the flows / images on the device:
  kernel_ms            sf_jpeg_encode alone for the whole batch (its five launches; output and workspace allocated once): device
                       events around --launches calls after a warm-up, the median of --windows windows
  encode_batch_ms      jpeg_gpu.encode_batch end to end (allocation, the call, lengths and used bytes to the host, framing and file
                       writes in the thread pool), the median of --runs
  vis_flow_video_ms    demo.vis_flow_video end to end from the flow fields (colouring, encode_batch, the AVI file), the median of --runs
  pil_loop_ms          one .cpu() copy of the batch, then PIL's save per image with the same tables (qtables=, subsampling=0,
                       optimize=False, one thread), the files written; the median of --runs; "skipped" where PIL is absent
  png_encode_batch_ms  png_gpu.encode_batch of the same images (the lossless path), the median of --runs
  gpu_bytes / pil_bytes / png_bytes / avi_bytes   the sizes of the files
The first GPU file of a set is compared byte for byte with tests/jpeg_cases.encode_ref, and with PIL every file is decoded and
its PSNR against the source reported next to PIL's own, before anything is timed.  The numbers are reported, not gated.  One JSON
line per set, written to --out.  Needs no dataset; a GPU is required (no fallback)."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from streamflow_amd import _lib, demo, jpeg_gpu, ops, png_gpu
from tests import jpeg_cases as jc
from tests import png_encode_cases as ec
from tests.avi_walk import walk

SETS = [("colour_wheel_436x1024", 24, 436, 1024), ("colour_wheel_1088x1920", 3, 1088, 1920)]


def median_ms(fn, runs):
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times)), 2), [round(x, 2) for x in times]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "jpeg_encode_bench.jsonl"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("jpeg_encode_bench needs the GPU; there is no CPU fallback")
    if a.launches < 10 or a.windows < 1 or a.runs < 1:
        raise ValueError("--launches at least 10, --windows and --runs at least 1")
    from bench import usable_cores
    torch.set_num_threads(min(usable_cores(), 64))
    try:
        from PIL import Image
    except ImportError:
        Image = None
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    q = jpeg_gpu.quant_tables(a.quality)
    pil_q = [[int(v) for v in t] for t in q]
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, n, h, w in SETS:
            flows = torch.from_numpy(np.stack([ec.smooth_field(h, w, 100 + i) for i in range(n)])).to(dev)
            images = ops.flow_to_image(flows)
            torch.cuda.synchronize()
            gpu_paths = [os.path.join(tmp, f"{name}_gpu_{i:02d}.jpg") for i in range(n)]
            pil_paths = [os.path.join(tmp, f"{name}_pil_{i:02d}.jpg") for i in range(n)]
            png_paths = [os.path.join(tmp, f"{name}_{i:02d}.png") for i in range(n)]
            avi_path = os.path.join(tmp, f"{name}.avi")
            fields = list(flows)

            def pil_loop():
                arr = images.cpu().numpy()
                for i, p in enumerate(pil_paths):
                    Image.fromarray(arr[i]).save(p, "JPEG", qtables=pil_q, subsampling=0, optimize=False)

            blobs = jpeg_gpu.encode_batch(images, gpu_paths, quality=a.quality)        # warm-up, and the check of what is timed
            want = images.cpu().numpy()
            assert blobs[0] == jpeg_gpu.jpeg_file(jc.encode_ref(want[0], q), h, w, 3, q), name
            demo.vis_flow_video(fields, avi_path, fps=8, quality=a.quality)
            assert walk(open(avi_path, "rb").read())["frames"] == blobs, name
            png_gpu.encode_batch(images, png_paths)
            rec = {"set": name, "images": n, "shape": [h, w, 3], "quality": a.quality, "pool_threads": png_gpu.pool_threads()}
            if Image is not None:
                pil_loop()
                ours = [jc.psnr(want[i], np.asarray(jc.pil_decode(blobs[i]))) for i in range(n)]
                theirs = [jc.psnr(want[i], np.asarray(Image.open(pil_paths[i]))) for i in range(n)]
                rec["psnr_db_gpu_min_mean"] = [round(min(ours), 3), round(float(np.mean(ours)), 3)]
                rec["psnr_db_pil_min_mean"] = [round(min(theirs), 3), round(float(np.mean(theirs)), 3)]
            rec["encode_batch_ms"], rec["encode_batch_ms_runs"] = median_ms(lambda: jpeg_gpu.encode_batch(images, gpu_paths, quality=a.quality), a.runs)
            rec["vis_flow_video_ms"], rec["vis_flow_video_ms_runs"] = median_ms(
                lambda: demo.vis_flow_video(fields, avi_path, fps=8, quality=a.quality), a.runs)
            if Image is not None:
                rec["pil_loop_ms"], rec["pil_loop_ms_runs"] = median_ms(pil_loop, a.runs)
            else:
                rec["pil_loop_ms"] = "skipped"
            rec["png_encode_batch_ms"], rec["png_encode_batch_ms_runs"] = median_ms(lambda: png_gpu.encode_batch(images, png_paths), a.runs)
            bound, ws_bytes = lib.sf_jpeg_encode_bound(h, w, 3), lib.sf_jpeg_encode_ws_bytes(n, h, w, 3)
            out = torch.empty(n, bound, dtype=torch.uint8, device=dev)
            lengths = torch.empty(n, dtype=torch.int64, device=dev)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            qh = np.ascontiguousarray(q, np.uint16)

            def call():
                _lib.check(lib.sf_jpeg_encode(images.data_ptr(), h * w * 3, w * 3, n, h, w, 3, qh.ctypes.data, out.data_ptr(), bound,
                                              lengths.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream()), "sf_jpeg_encode")

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
            rec.update({"kernel_ms": round(kernel_ms, 4), "kernel_ms_windows": [round(x, 4) for x in windows],
                        "kernel_GBps_read": round(n * h * w * 3 / kernel_ms / 1e6, 2), "slot_bytes": bound, "workspace_bytes": ws_bytes,
                        "gpu_bytes": sum(map(os.path.getsize, gpu_paths)), "png_bytes": sum(map(os.path.getsize, png_paths)),
                        "avi_bytes": os.path.getsize(avi_path), "raw_bytes": n * h * w * 3})
            if Image is not None:
                rec["pil_bytes"] = sum(map(os.path.getsize, pil_paths))
                rec["gpu_over_pil_bytes"] = round(rec["gpu_bytes"] / rec["pil_bytes"], 4)
                rec["pil_loop_over_encode_batch"] = round(rec["pil_loop_ms"] / rec["encode_batch_ms"], 1)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
