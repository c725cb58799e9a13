#!/usr/bin/env python3
"""sf_flow_to_image (csrc/flow_viz.hip) at the shapes users colour: 436 x 1024 x 3 (a Sintel clip) and 1088 x 1920 x 3 (a Spring
clip), HIP events around batches of calls, the median over the batches.

    python tools/flow_viz_bench.py [--batches 30] [--calls 10] [--no-host]

Per shape: the whole call (memset + maximum + colour pass), the colour pass alone (a call with fixed_rad_max: the same kernel,
the maximum read from an argument) and their difference = memset + maximum; achieved bytes/s on 11 h w n bytes (colour pass:
8 in, 3 out) and 8 h w n (maximum), and the colour pass as a fraction of the 8 TB/s HBM roof.  The inputs rotate through enough
buffers to exceed the 256 MB last-level cache, so the reads come from HBM.  What it replaces, timed here too: the device-to-host
copy of the flows plus the numpy colouring (tests/viz_cases.py: flow_to_image_np) of every field on this box's CPU.
One JSON line per shape."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from streamflow_amd import _lib
from tests import viz_cases as vc

HBM_ROOF = 8.0e12
SHAPES = ((3, 436, 1024), (3, 1088, 1920))


def median_us(fn, batches, calls):
    for _ in range(3 * calls):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(batches):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) * 1e3 / calls)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the host (numpy + copy) comparison")
    a = ap.parse_args()
    assert a.batches >= 20, "the median needs at least 20 batches"
    assert torch.cuda.is_available(), "flow_viz_bench.py needs an MI355X"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    for n, h, w in SHAPES:
        nbuf = max(2, int(np.ceil(320e6 / (8 * n * h * w))))
        host = vc.gaussian_fields(n, h, w, [6.0, 25.0, 1.5][:n], seed=h)
        bufs = [torch.from_numpy(host).to(dev) * (1.0 + 0.01 * k) for k in range(nbuf)]
        out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
        ws = torch.empty(n, device=dev)
        turn = [0]

        def call(fixed):
            t = bufs[turn[0] % nbuf]
            turn[0] += 1
            _lib.check(lib.sf_flow_to_image(t.data_ptr(), out.data_ptr(), ws.data_ptr(), n, h, w, -1.0, fixed, 0, _lib.stream()),
                       "sf_flow_to_image")

        full = median_us(lambda: call(-1.0), a.batches, a.calls)
        colour = median_us(lambda: call(30.0), a.batches, a.calls)
        px = n * h * w
        res = {"shape": [n, h, w], "input_buffers": nbuf, "batches": a.batches, "calls_per_batch": a.calls,
               "full_call_us": {"median": full[0], "min": full[1], "max": full[2]},
               "colour_pass_us": {"median": colour[0], "min": colour[1], "max": colour[2]},
               "memset_plus_maximum_us_by_difference": full[0] - colour[0],
               "colour_pass_bytes_per_s": 11 * px / (colour[0] * 1e-6),
               "colour_pass_fraction_of_hbm_roof": 11 * px / (colour[0] * 1e-6) / HBM_ROOF,
               "maximum_bytes_per_s": 8 * px / max(full[0] - colour[0], 1e-3) / 1e-6}
        if not a.no_host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            flows = bufs[0].cpu()
            t1 = time.perf_counter()
            imgs = [vc.flow_to_image_np(flows[i].numpy().transpose(1, 2, 0)) for i in range(n)]
            t2 = time.perf_counter()
            call(-1.0)
            torch.cuda.synchronize()
            worst = [vc.image_mismatch(out[i].cpu().numpy(), vc.flow_to_image_np((bufs[(turn[0] - 1) % nbuf][i]).cpu().numpy().transpose(1, 2, 0)))
                     for i in range(n)]
            res.update({"host_copy_ms": (t1 - t0) * 1e3, "host_numpy_colouring_ms": (t2 - t1) * 1e3,
                        "host_total_over_device_call": (t2 - t0) * 1e6 / full[0],
                        "mismatch_vs_numpy_(levels,pixels,allowed)": worst, "host_images": len(imgs)})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
