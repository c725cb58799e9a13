#!/usr/bin/env python3
"""Frame interpolation by forward splatting: sf_frame_interp (csrc/frame_interp.hip) and its three parts against what a user would
write today, on the same GPU in the same run, and the cost of interpolate_video over predict_video(bidirectional=True).

    python tools/frame_interp_bench.py [--batches 30] [--calls 10] [--frames 50] [--runs 3] [--no-video]

At 24 pairs of 436 x 1024 (one model call of 8 clips at T = 4) and 3 pairs of 1088 x 1920 (one Spring clip), seeded smooth flows (a
translation plus a low-frequency wave plus low-amplitude noise, the backward flow its negative plus noise) and noise frames, t = 1/2,
no class maps:
(a) sf_frame_interp called directly, and sf_frame_interp_phases restricted to the clear (a memset of the accumulators), the splat
    and the resolve with its stats finish (on the accumulators of one clear and one splat, as in a full call): HIP events around
    batches of --calls calls after warming every shape up, the median over --batches batches; operands and outputs rotate through more than 256 MB.  The splat's added bytes are counted exactly (every
    tap with a non-zero weight inside the frame adds 4 x 8 bytes; at most 128 bytes per source pixel and side) and set against the
    1.3 TB/s that fp32 atomic adds of the same shape reach on this chip; 64-bit integer adds had not been measured before.
(b) the same result as torch expressions: index_add_ into float32 accumulators with unquantised bilinear weights (a tap that does
    not count adds zero to its own source pixel, so no address collects the masked taps), normalise, blend, fill holes; timed the
    same way.  Its sums depend on the order of arrival, its bytes are within 1 of the kernel's almost everywhere
    (the share that is not is reported).
(c) interpolate.interpolate_video with factor 2 and 4 against video.predict_video(bidirectional=True) alone on the synthetic
    436 x 1024 video tools/video_bench.py uses (StreamFlowT4 on seeded random weights, 15 iterations, 8 clips per call), wall clock
    per video, the median of --runs.
One JSON line per measurement, appended to profiles/frame_interp_bench.jsonl."""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from streamflow_amd import _lib, ops

ATOMIC_RATE = 1.3e12                # added bytes per second of fp32 atomic adds, 256 contiguous bytes per wave-instruction
OUT = os.path.join(REPO, "profiles", "frame_interp_bench.jsonl")
NUM, DEN = 1, 2
CLEAR, SPLAT, RESOLVE = 1, 2, 4


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


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
    return {"median": float(np.median(times)), "min": float(np.min(times)), "max": float(np.max(times))}


def make_fields(n, h, w, dev, seed):
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    tx, ty = 0.02 * w + 0.37, -0.015 * h - 0.21
    u = tx + 1.5 * torch.sin(2 * math.pi * xs / w + 0.3) * torch.cos(2 * math.pi * ys / h)
    v = ty + 1.0 * torch.cos(2 * math.pi * xs / w) * torch.sin(2 * math.pi * ys / h + 0.7)
    fwd = torch.stack([u + 0.05 * torch.randn(n, h, w, generator=g), v + 0.05 * torch.randn(n, h, w, generator=g)], 1)
    bwd = torch.stack([-u + 0.05 * torch.randn(n, h, w, generator=g), -v + 0.05 * torch.randn(n, h, w, generator=g)], 1)
    a = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)
    b = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)
    return [t.contiguous().to(dev) for t in (a, b, fwd, bwd)]


def _taps(flow, ts):
    """Per source pixel: (inside, x0, y0, fx, fy) as the kernel computes them, float32 on the device."""
    n, _, h, w = flow.shape
    px = torch.arange(w, device=flow.device, dtype=torch.float32) + ts * flow[:, 0]
    py = torch.arange(h, device=flow.device, dtype=torch.float32)[:, None] + ts * flow[:, 1]
    ok = (px > -1) & (px < w) & (py > -1) & (py < h)
    px, py = torch.where(ok, px, 0), torch.where(ok, py, 0)
    x0, y0 = torch.floor(px), torch.floor(py)
    return ok, x0.long(), y0.long(), px - x0, py - y0


def torch_side(img, flow, ts):
    """One side as torch expressions: float32 accumulators, unquantised weights, index_add_ (order-dependent sums)."""
    n, _, h, w = flow.shape
    ok, x0, y0, fx, fy = _taps(flow, ts)
    W = torch.zeros(n * h * w, dtype=torch.float32, device=flow.device)
    C = torch.zeros(n * h * w, 3, dtype=torch.float32, device=flow.device)
    pair = torch.arange(n, device=flow.device)[:, None, None]
    own = torch.arange(n * h * w, device=flow.device).view(n, h, w)      # a tap that does not count adds 0 to its own source pixel:
    col = img.float()                                                    # no single address collects them
    for ty, wy in ((0, 1 - fy), (1, fy)):
        for tx, wx in ((0, 1 - fx), (1, fx)):
            xi, yi, wt = x0 + tx, y0 + ty, wx * wy
            m = ok & (wt > 0) & (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            wt = torch.where(m, wt, 0).reshape(-1)
            idx = torch.where(m, (pair * h + yi) * w + xi, own).reshape(-1)
            W.index_add_(0, idx, wt)
            C.index_add_(0, idx, wt[:, None] * col.reshape(-1, 3))
    return W.view(n, h, w), C.view(n, h, w, 3)


def torch_interp(a, b, fwd, bwd, t):
    WA, CA = torch_side(a, fwd, t)
    WB, CB = torch_side(b, bwd, 1 - t)
    ha, hb = (WA > 0)[..., None], (WB > 0)[..., None]
    ca = torch.where(ha, CA / WA.clamp_min(1e-20)[..., None], a.float())
    cb = torch.where(hb, CB / WB.clamp_min(1e-20)[..., None], b.float())
    both = (1 - t) * ca + t * cb
    val = torch.where(ha & ~hb, ca, torch.where(hb & ~ha, cb, both))
    return torch.floor(val + 0.5).clamp(0, 255).to(torch.uint8)


def added_bytes(flow, ts):
    """Bytes the splat of one side adds: 4 accumulators x 8 bytes per tap with a non-zero 1/64 weight inside the frame."""
    n, _, h, w = flow.shape
    ok, x0, y0, fx, fy = _taps(flow, ts)
    wx1, wy1 = torch.floor(fx * 64 + 0.5).long(), torch.floor(fy * 64 + 0.5).long()
    taps = 0
    for ty, wy in ((0, 64 - wy1), (1, wy1)):
        for tx, wx in ((0, 64 - wx1), (1, wx1)):
            xi, yi = x0 + tx, y0 + ty
            taps += int((ok & (wx * wy > 0) & (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)).sum())
    return 32 * taps


def kernels(dev, n, h, w, a):
    lib = _lib.load()
    px = n * h * w
    per_set = px * (3 + 3 + 8 + 8 + 3)
    nbuf = max(2, int(np.ceil(320e6 / per_set)))
    sets = [make_fields(n, h, w, dev, 10 + i) for i in range(nbuf)]
    out = [torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
    stats = torch.zeros(n, ops.INTERP_LEN, dtype=torch.float64, device=dev)
    ws_bytes = int(lib.sf_frame_interp_ws_bytes(n, h, w))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    turn = [0]

    def nxt():
        i = turn[0] % nbuf
        turn[0] += 1
        return i

    def call(phases):
        def run():
            i = nxt()
            fa, fb, f, b = sets[i]
            st = (3 * h * w, 3 * w, 3, 1)
            _lib.check(lib.sf_frame_interp_phases(fa.data_ptr(), *st, fb.data_ptr(), *st, f.data_ptr(), 2 * h * w, h * w, w, b.data_ptr(),
                                                  2 * h * w, h * w, w, n, h, w, NUM, DEN, None, None, 0, 1, 16, 1, 16, out[i].data_ptr(),
                                                  None, stats.data_ptr(), ws.data_ptr(), ws.numel(), phases, _lib.stream()),
                       "sf_frame_interp_phases")
        return run

    def t_form():
        i = nxt()
        return torch_interp(*sets[i], NUM / DEN)

    # agreement of the two forms on the first set, and the kernel's own result through the plain entry point
    got, cover, st0 = ops.frame_interp(*sets[0], NUM, DEN, cover=True)
    tt = torch_interp(*sets[0], NUM / DEN)
    diff = (tt.int() - got.int()).abs()
    again = ops.frame_interp(*sets[0], NUM, DEN)[0]
    agree = {"bytes": int(diff.numel()), "bytes_differing": int((diff > 0).sum()), "bytes_differing_by_more_than_1": int((diff > 1).sum()),
             "largest_difference": int(diff.max()), "kernel_repeat_is_bitwise_equal": bool(torch.equal(got, again)),
             "cover_shares": [float(v) / px for v in st0.sum(0)[1:].cpu()]}
    added = added_bytes(sets[0][2], NUM / DEN) + added_bytes(sets[0][3], 1 - NUM / DEN)
    shape = {"pairs": n, "field": [h, w], "t": [NUM, DEN], "buffer_sets": nbuf, "rotating_bytes": nbuf * per_set,
             "workspace_bytes": ws_bytes, "batches": a.batches, "calls_per_batch": a.calls}
    res = {}
    for name, phases in (("sf_frame_interp", CLEAR | SPLAT | RESOLVE), ("clear (memset of the accumulators)", CLEAR), ("splat", SPLAT),
                         ("resolve + stats finish", RESOLVE)):
        if phases == RESOLVE:
            # the splat timing above added hundreds of splats into the accumulators: restore the sums of ONE splat, which is what
            # the resolve of a full call reads (and which keeps it on the paths a full call takes)
            call(CLEAR | SPLAT)()
        t = median_us(call(phases), a.batches, a.calls)
        res[name] = t["median"]
        rec = {"kernel": name, **shape, "us": t}
        if phases == SPLAT:
            rate = added / (t["median"] * 1e-6)
            rec.update({"added_bytes": added, "added_bytes_per_source_pixel_and_side": added / (2 * px), "added_bytes_per_s": rate,
                        "fraction_of_fp32_atomic_rate": rate / ATOMIC_RATE})
        if phases == CLEAR:
            rec.update({"bytes_cleared": 64 * px, "bytes_per_s": 64 * px / (t["median"] * 1e-6)})
        if phases == RESOLVE:
            rec.update({"bytes_needed": 68 * px, "bytes_per_s": 68 * px / (t["median"] * 1e-6)})
        emit(rec)
    t = median_us(t_form, a.batches, max(1, a.calls // 5))
    emit({"path": "torch expressions: index_add_ into float32 accumulators, normalise, blend, fill holes", **shape, "us": t})
    emit({"ratio": f"{n} pairs of {h} x {w}", "agreement_with_torch_form": agree, "torch_over_kernel": t["median"] / res["sf_frame_interp"],
          "kernel_beats_torch_form": bool(res["sf_frame_interp"] < t["median"]),
          "share_of_call": {k: res[k] / res["sf_frame_interp"] for k in res if k != "sf_frame_interp"}})
    del sets, out
    torch.cuda.empty_cache()


def wall_ms(fn, runs):
    fn()                                                                # graph capture, engine plans, code objects
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median": float(np.median(times)), "min": float(np.min(times)), "max": float(np.max(times))}


def video_cost(dev, a):
    from streamflow_amd import interpolate, presets, synthetic as syn, video
    from streamflow_amd.model import StreamFlowT4
    H, W, T, n = 436, 1024, 4, a.frames
    sd = dict(syn.make_params(0, T))
    sd.update({"fnet." + k: v for k, v in syn.make_twins_params(1).items()})
    sd.update({"cnet." + k: v for k, v in syn.make_twins_params(2).items()})
    model = StreamFlowT4({"model": sd}, preset=presets.BENCH_PRESET).to(dev).eval()
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(dev)
    two = wall_ms(lambda: video.predict_video(model, frames, T=T, iters=a.iters, clips_per_step=8, bidirectional=True), a.runs)
    rec = {"path": "interpolate_video on device frames, 8 clips per call", "frames": n, "shape": [H, W], "T": T, "iters": a.iters,
           "preset": presets.BENCH_PRESET, "runs": a.runs, "bidirectional_ms_per_video": two}
    for factor in (2, 4):
        t = wall_ms(lambda: interpolate.interpolate_video(model, frames, factor=factor, T=T, iters=a.iters, clips_per_step=8), a.runs)
        rec["factor_%d_ms_per_video" % factor] = t
        rec["factor_%d_over_bidirectional" % factor] = t["median"] / two["median"]
        rec["factor_%d_frames_out" % factor] = (n - 1) * factor + 1
    emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--no-video", action="store_true")
    a = ap.parse_args()
    assert a.batches >= 20, "the median needs at least 20 batches"
    assert torch.cuda.is_available(), "frame_interp_bench.py needs an MI355X"
    dev = torch.device("cuda:0")
    kernels(dev, 24, 436, 1024, a)
    kernels(dev, 3, 1088, 1920, a)
    if not a.no_video:
        video_cost(dev, a)


if __name__ == "__main__":
    main()
