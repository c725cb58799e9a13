#!/usr/bin/env python3
"""Video inference end to end: video.predict_video against demo.predict_frames on the same box in the same run, and the two kernels
of csrc/video_io.hip alone.

    python tools/video_bench.py [--frames 98] [--runs 3] [--batches 30] [--calls 10] [--preset config2_mixed]

A 436 x 1024 video of 98 uint8 frames (33 clips of T = 4, the last one a tail clip), StreamFlowT4 on seeded random weights (Twins_CSC
encoders, 15 iterations, graphs on):
(a) demo.predict_frames: every frame normalised to fp32 and padded on the host beforehand (not timed), one clip per model call, one
    blocking copy to the host per flow field (timed: it is part of the function);
(b) video.predict_video at clips_per_step 1 and 8, the uint8 frames on the host (the upload of every batch is timed) and on the
    device; the result stays on the device, the run ends in a synchronise.
    Wall clock per whole video after one untimed run per configuration (graph capture, engine plans); the median of --runs.
(c) sf_frames_to_clips for one batch of 8 clips and sf_clips_to_flows for its 24 pairs, the entry points called directly: HIP events
    around batches of --calls calls, the median over --batches batches; inputs and outputs rotate through more than 256 MB so that
    nothing is served from a cache.  Bytes moved per call: 3 B read + 12 B written per pixel of a padded frame copy; 4 B read + 4 B
    written per flow value.  The share of the 8 TB/s HBM roof follows from them.
One JSON line per measurement, then one with the ratios."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from streamflow_amd import _lib, ops, presets, synthetic as syn, video
from streamflow_amd.demo import predict_frames
from streamflow_amd.model import StreamFlowT4
from streamflow_amd.utils import InputPadder

HBM_ROOF = 8.0e12
H, W, T = 436, 1024, 4


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


def wall_ms(fn, runs):
    fn()                                                                # graph capture, engine plans, code objects
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def kernels_alone(dev, n, a):
    lib = _lib.load()
    pad = InputPadder((H, W))._pad
    Hp, Wp = H + pad[2] + pad[3], W + pad[0] + pad[1]
    first, k, f_lo, f_hi, p_lo, p_hi = video.plan_batches(n, T, 8)[0]
    lut = ops.norm_lut(dev)
    in_bytes, out_bytes = (f_hi - f_lo) * H * W * 3, k * T * 3 * Hp * Wp * 4
    nbuf = max(2, int(np.ceil(320e6 / (in_bytes + out_bytes))))
    g = torch.Generator().manual_seed(0)
    frames = [torch.randint(0, 256, (f_hi - f_lo, H, W, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(nbuf)]
    clips = [torch.empty(k, T, 3, Hp, Wp, device=dev) for _ in range(nbuf)]
    turn = [0]

    def to_clips():
        i = turn[0] % nbuf
        turn[0] += 1
        f = frames[i]
        _lib.check(lib.sf_frames_to_clips(f.data_ptr(), f.stride(0), f.stride(1), f.stride(2), f.stride(3), f_lo, f.shape[0], n, T, first,
                                          k, H, W, pad[2], pad[0], Hp, Wp, lut.data_ptr(), clips[i].data_ptr(), _lib.stream()),
                   "sf_frames_to_clips")

    def to_clips_wrapper():
        i = turn[0] % nbuf
        turn[0] += 1
        ops.frames_to_clips(frames[i], n, T, first, k, pad, frame0=f_lo, out=clips[i])

    moved = k * T * Hp * Wp * (3 + 12)
    t, tw = median_us(to_clips, a.batches, a.calls), median_us(to_clips_wrapper, a.batches, a.calls)
    res = {"kernel": "sf_frames_to_clips", "clips": k, "T": T, "frame": [H, W], "padded": [Hp, Wp], "buffer_sets": nbuf,
           "rotating_bytes": nbuf * (in_bytes + out_bytes), "batches": a.batches, "calls_per_batch": a.calls,
           "us": {"median": t[0], "min": t[1], "max": t[2]}, "ops_wrapper_us": {"median": tw[0], "min": tw[1], "max": tw[2]},
           "bytes_moved": moved, "bytes_per_s": moved / (t[0] * 1e-6), "fraction_of_hbm_roof": moved / (t[0] * 1e-6) / HBM_ROOF}
    print(json.dumps(res), flush=True)
    del frames, clips
    torch.cuda.empty_cache()

    npairs = p_hi - p_lo
    pair_bytes, flow_bytes = (T - 1) * k * 2 * Hp * Wp * 4, npairs * 2 * H * W * 4
    nbuf = max(2, int(np.ceil(320e6 / (pair_bytes + flow_bytes))))
    outs = [[torch.randn(k, 2, Hp, Wp, device=dev) for _ in range(T - 1)] for _ in range(nbuf)]
    flows = [torch.empty(npairs, 2, H, W, device=dev) for _ in range(nbuf)]
    ptrs = []
    for o in outs:
        p = _lib.SfPairPtrs()
        for j, t_ in enumerate(o):
            p.p[j] = t_.data_ptr()
        ptrs.append(p)

    def to_flows():
        i = turn[0] % nbuf
        turn[0] += 1
        o = outs[i][0]
        _lib.check(lib.sf_clips_to_flows(ctypes.byref(ptrs[i]), o.stride(0), o.stride(1), o.stride(2), n, T, first, k, p_lo, npairs, H, W,
                                         pad[2], pad[0], flows[i].data_ptr(), _lib.stream()), "sf_clips_to_flows")

    def to_flows_wrapper():
        i = turn[0] % nbuf
        turn[0] += 1
        ops.clips_to_flows(outs[i], n, T, first, p_lo, npairs, (H, W), pad, out=flows[i])

    moved = 2 * flow_bytes
    t, tw = median_us(to_flows, a.batches, a.calls), median_us(to_flows_wrapper, a.batches, a.calls)
    res2 = {"kernel": "sf_clips_to_flows", "pairs": npairs, "field": [H, W], "buffer_sets": nbuf,
            "rotating_bytes": nbuf * (pair_bytes + flow_bytes), "batches": a.batches, "calls_per_batch": a.calls,
            "us": {"median": t[0], "min": t[1], "max": t[2]}, "ops_wrapper_us": {"median": tw[0], "min": tw[1], "max": tw[2]},
            "bytes_moved": moved, "bytes_per_s": moved / (t[0] * 1e-6), "fraction_of_hbm_roof": moved / (t[0] * 1e-6) / HBM_ROOF}
    print(json.dumps(res2), flush=True)
    return res, res2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=98)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--preset", default=presets.BENCH_PRESET, choices=list(presets.PRESETS))
    a = ap.parse_args()
    assert a.batches >= 20, "the median needs at least 20 batches"
    assert torch.cuda.is_available(), "video_bench.py needs an MI355X"
    dev = torch.device("cuda:0")
    from bench import usable_cores
    torch.set_num_threads(min(usable_cores(), 64))                      # the cores this process may use, as tests/conftest.py does
    n = a.frames
    kernels_alone(dev, n, a)
    sd = dict(syn.make_params(0, T))
    sd.update({"fnet." + k: v for k, v in syn.make_twins_params(1).items()})
    sd.update({"cnet." + k: v for k, v in syn.make_twins_params(2).items()})
    model = StreamFlowT4({"model": sd}, preset=a.preset).to(dev).eval()
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    frames_dev = frames.to(dev)
    normalised = [2 * (f.permute(2, 0, 1).float() / 255.0) - 1.0 for f in frames]          # what predict_frames takes (host, fp32)
    pairs = n - 1
    out = {}

    def record(name, t, **kw):
        res = {"path": name, "frames": n, "pairs": pairs, "shape": [H, W], "T": T, "iters": a.iters, "preset": a.preset, "runs": a.runs,
               "ms_per_video": {"median": t[0], "min": t[1], "max": t[2]}, "flow_fields_per_s": pairs / (t[0] * 1e-3), **kw}
        out[name] = res
        print(json.dumps(res), flush=True)

    record("predict_frames (host fp32 frames, 1 clip per call, flows to the host)",
           wall_ms(lambda: predict_frames(lambda imgs: model(imgs, iters=a.iters), normalised, T=T, device=dev), a.runs), clips_per_step=1)
    for cps in (1, 8):
        for where, src in (("host", frames), ("device", frames_dev)):
            record(f"predict_video (uint8 frames on the {where}, {cps} clip(s) per call)",
                   wall_ms(lambda: video.predict_video(model, src, T=T, iters=a.iters, clips_per_step=cps), a.runs), clips_per_step=cps)
    base = out["predict_frames (host fp32 frames, 1 clip per call, flows to the host)"]["flow_fields_per_s"]
    print(json.dumps({"speedup_over_predict_frames": {k: v["flow_fields_per_s"] / base for k, v in out.items() if k.startswith("predict_video")},
                      "host_fp32_bytes_predict_frames_holds": 2 * n * 3 * 440 * 1024 * 4,
                      "host_bytes_predict_video_holds": n * H * W * 3}), flush=True)


if __name__ == "__main__":
    main()
