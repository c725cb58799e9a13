#!/usr/bin/env python3
"""Forward-backward consistency and backward warping: sf_flow_consistency and sf_warp_frames (csrc/flow_consistency.hip) against
what a user would write today, on the same GPU in the same run, and the cost of predict_video(bidirectional=True).

    python tools/flow_consistency_bench.py [--batches 30] [--calls 10] [--frames 50] [--runs 3] [--no-video]

At 24 pairs of 436 x 1024 (one model call of 8 clips at T = 4) and 3 pairs of 1088 x 1920 (one Spring clip), synthetic smooth flows
(a translation plus low-amplitude noise, a contradicting band: all three classes occur) and noise frames:
(a) the two entry points called directly: HIP events around batches of --calls calls after warming every shape up, the median over
    --batches batches; operands and outputs rotate through more than 256 MB so that nothing is served from a cache;
(b) the same results as torch expressions: F.grid_sample(align_corners=True) on the backward field / the float frame plus
    elementwise operations and masked sums (classes, counts and sums; warped bytes and the photometric sum), timed the same way;
(c) the same results in numpy after a copy to the host (tests/consistency_cases.py's float32 restatement), wall clock, one run.
Bytes a call must move, from the shapes alone: consistency 8 B (forward flow) + 8 B (backward field, every element once) + 1 B
(class) = 17 B per pixel; warp with statistics 8 B (flow) + 3 B (source, once) + 3 B (reference) + 1 B (class) + 3 B (out) = 18 B
per pixel, 14 B without.  "fraction_of_hbm_roof" is those bytes over the kernel time over the 8 TB/s roof the README uses.
(d) video.predict_video with and without bidirectional=True on the synthetic 436 x 1024 video tools/video_bench.py uses
    (StreamFlowT4 on seeded random weights, 15 iterations, 8 clips per call), wall clock per video, the median of --runs.
One JSON line per measurement, appended to profiles/flow_consistency_bench.jsonl."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
import torch.nn.functional as F

from streamflow_amd import _lib, consistency, ops

HBM_ROOF = 8.0e12
ALPHA, BETA = consistency.ALPHA, consistency.BETA
OUT = os.path.join(REPO, "profiles", "flow_consistency_bench.jsonl")


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
    tx, ty = 0.02 * w, -0.015 * h
    fwd = torch.stack([tx + 0.2 * torch.randn(n, h, w, generator=g), ty + 0.2 * torch.randn(n, h, w, generator=g)], 1)
    bwd = torch.stack([-tx + 0.1 * torch.randn(n, h, w, generator=g), -ty + 0.1 * torch.randn(n, h, w, generator=g)], 1)
    bwd[:, :, h // 3:h // 2] += 5.0
    src = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)
    ref = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)
    return [t.contiguous().to(dev) for t in (fwd, bwd, src, ref)]


def torch_consistency(fwd, bwd):
    n, _, h, w = fwd.shape
    xs = torch.arange(w, device=fwd.device, dtype=torch.float32) + fwd[:, 0]
    ys = torch.arange(h, device=fwd.device, dtype=torch.float32)[:, None] + fwd[:, 1]
    inside = (xs >= 0) & (xs <= w - 1) & (ys >= 0) & (ys <= h - 1)
    grid = torch.stack([2 * xs / (w - 1) - 1, 2 * ys / (h - 1) - 1], -1)
    samp = F.grid_sample(bwd, grid, mode="bilinear", padding_mode="border", align_corners=True)
    d = fwd + samp
    lhs = (d * d).sum(1)
    m2 = (fwd * fwd).sum(1)
    rhs = ALPHA * (m2 + (samp * samp).sum(1)) + BETA
    vis = inside & (lhs <= rhs)
    cls = torch.where(vis, 0, torch.where(inside, 1, 2)).to(torch.uint8)
    mag = m2.sqrt()
    fin = torch.isfinite(mag)
    stats = torch.stack([torch.full((n,), float(h * w), dtype=torch.float64, device=fwd.device), vis.sum((1, 2)).double(),
                         (inside & ~vis).sum((1, 2)).double(), (~inside).sum((1, 2)).double(),
                         (lhs.sqrt().double() * vis).sum((1, 2)), torch.where(fin, mag, 0).double().sum((1, 2)), fin.sum((1, 2)).double()], 1)
    return cls, stats, grid, inside


def torch_warp(src, fwd, cls, ref):
    n, _, h, w = fwd.shape
    xs = torch.arange(w, device=fwd.device, dtype=torch.float32) + fwd[:, 0]
    ys = torch.arange(h, device=fwd.device, dtype=torch.float32)[:, None] + fwd[:, 1]
    inside = (xs >= 0) & (xs <= w - 1) & (ys >= 0) & (ys <= h - 1)
    grid = torch.stack([2 * xs / (w - 1) - 1, 2 * ys / (h - 1) - 1], -1)
    val = F.grid_sample(src.permute(0, 3, 1, 2).float(), grid, mode="bilinear", padding_mode="border", align_corners=True)
    out = torch.where(inside[:, None], torch.floor(val + 0.5), 0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    take = (inside & (cls == 0))[:, None]
    err = ((val - ref.permute(0, 3, 1, 2).float()).abs().double() * take).sum((1, 2, 3))
    return out, torch.stack([err, 3 * take.sum((1, 2, 3)).double()], 1)


def kernels(dev, n, h, w, a):
    lib = _lib.load()
    px = n * h * w
    per_set = px * (8 + 8 + 3 + 3 + 1 + 3)
    nbuf = max(2, int(np.ceil(320e6 / per_set)))
    sets = [make_fields(n, h, w, dev, 10 + i) for i in range(nbuf)]
    cls = [torch.empty(n, h, w, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
    out = [torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
    stats, wstats = torch.zeros(n, ops.FBC_LEN, dtype=torch.float64, device=dev), torch.zeros(n, ops.WARP_LEN, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.sf_flow_consistency_ws_bytes(n, h, w)), dtype=torch.uint8, device=dev)
    wws = torch.empty(int(lib.sf_warp_frames_ws_bytes(n, h, w)), dtype=torch.uint8, device=dev)
    turn = [0]

    def nxt():
        i = turn[0] % nbuf
        turn[0] += 1
        return i

    def fbc():
        i = nxt()
        f, b = sets[i][0], sets[i][1]
        _lib.check(lib.sf_flow_consistency(f.data_ptr(), f.stride(0), f.stride(1), f.stride(2), b.data_ptr(), b.stride(0), b.stride(1),
                                           b.stride(2), n, h, w, ALPHA, BETA, 0, 1, 2, cls[i].data_ptr(), stats.data_ptr(), ws.data_ptr(),
                                           ws.numel(), _lib.stream()), "sf_flow_consistency")

    def warp(with_stats):
        def run():
            i = nxt()
            f, s, r = sets[i][0], sets[i][2], sets[i][3]
            st = (3 * h * w, 3 * w, 3, 1)
            _lib.check(lib.sf_warp_frames(s.data_ptr(), *st, f.data_ptr(), f.stride(0), f.stride(1), f.stride(2), n, h, w, out[i].data_ptr(),
                                          cls[i].data_ptr() if with_stats else None, 0, r.data_ptr() if with_stats else None, *st,
                                          wstats.data_ptr() if with_stats else None, wws.data_ptr() if with_stats else None,
                                          wws.numel() if with_stats else 0, _lib.stream()), "sf_warp_frames")
        return run

    def t_fbc():
        i = nxt()
        return torch_consistency(sets[i][0], sets[i][1])

    def t_warp():
        i = nxt()
        return torch_warp(sets[i][2], sets[i][0], cls[i], sets[i][3])

    for i in range(nbuf):                                               # every class map filled before the warps read them
        turn[0] = i
        fbc()
    # the torch forms give the same classes but for pixels on the threshold, and bytes within one
    tc, ts, _, _ = torch_consistency(sets[0][0], sets[0][1])
    tw, _ = torch_warp(sets[0][2], sets[0][0], cls[0], sets[0][3])
    turn[0] = 0
    warp(True)()
    torch.cuda.synchronize()
    agree = {"class_bytes_differing": int((tc != cls[0]).sum()), "warped_bytes_differing_by_more_than_1": int(((tw.int() - out[0].int()).abs() > 1).sum()),
             "pixels": px}
    shape = {"pairs": n, "field": [h, w], "buffer_sets": nbuf, "rotating_bytes": nbuf * per_set, "batches": a.batches,
             "calls_per_batch": a.calls}
    res = {}
    for name, fn, nbytes in (("sf_flow_consistency", fbc, 17 * px), ("sf_warp_frames (with class map and reference frames)", warp(True), 18 * px),
                             ("sf_warp_frames (bytes only)", warp(False), 14 * px)):
        t = median_us(fn, a.batches, a.calls)
        res[name] = t["median"]
        emit({"kernel": name, **shape, "us": t, "bytes_needed": nbytes, "bytes_needed_per_pixel": nbytes // px,
              "bytes_per_s": nbytes / (t["median"] * 1e-6), "fraction_of_hbm_roof": nbytes / (t["median"] * 1e-6) / HBM_ROOF})
    tt = {"torch expressions: consistency (grid_sample + elementwise + masked sums)": median_us(t_fbc, a.batches, max(1, a.calls // 5)),
          "torch expressions: warp with photometric sum (grid_sample + elementwise)": median_us(t_warp, a.batches, max(1, a.calls // 5))}
    for name, t in tt.items():
        emit({"path": name, **shape, "us": t})
    # numpy after a copy to the host: the float32 restatement of the tests, wall clock, one run
    from tests import consistency_cases as cc
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f_h, b_h = sets[0][0].cpu().numpy(), sets[0][1].cpu().numpy()
    c_h, _, _, _ = cc.restate32(f_h, b_h)
    t1 = time.perf_counter()
    s_h, r_h = sets[0][2].cpu().numpy(), sets[0][3].cpu().numpy()
    cc.warp32(s_h, f_h, c_h, r_h)
    t2 = time.perf_counter()
    emit({"path": "numpy on the host after .cpu() (float32 restatement)", **shape, "consistency_ms": (t1 - t0) * 1e3, "warp_ms": (t2 - t1) * 1e3,
          "class_bytes_differing_from_kernel": int((torch.from_numpy(c_h).to(dev) != cls[0]).sum())})
    names = list(tt)
    emit({"ratio": f"{n} pairs of {h} x {w}", "agreement_with_torch_form": agree,
          "torch_over_kernel_consistency": tt[names[0]]["median"] / res["sf_flow_consistency"],
          "torch_over_kernel_warp": tt[names[1]]["median"] / res["sf_warp_frames (with class map and reference frames)"],
          "numpy_over_kernel_consistency": (t1 - t0) * 1e6 / res["sf_flow_consistency"],
          "numpy_over_kernel_warp": (t2 - t1) * 1e6 / res["sf_warp_frames (with class map and reference frames)"]})
    del sets, cls, out
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
    from streamflow_amd import presets, synthetic as syn, video
    from streamflow_amd.model import StreamFlowT4
    H, W, T, n = 436, 1024, 4, a.frames
    sd = dict(syn.make_params(0, T))
    sd.update({"fnet." + k: v for k, v in syn.make_twins_params(1).items()})
    sd.update({"cnet." + k: v for k, v in syn.make_twins_params(2).items()})
    model = StreamFlowT4({"model": sd}, preset=presets.BENCH_PRESET).to(dev).eval()
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(dev)
    one = wall_ms(lambda: video.predict_video(model, frames, T=T, iters=a.iters, clips_per_step=8), a.runs)
    two = wall_ms(lambda: video.predict_video(model, frames, T=T, iters=a.iters, clips_per_step=8, bidirectional=True), a.runs)
    rep = wall_ms(lambda: consistency.video_report(model, frames, T=T, iters=a.iters, clips_per_step=8, verbose=False), a.runs)
    emit({"path": "predict_video on device frames, 8 clips per call", "frames": n, "shape": [H, W], "T": T, "iters": a.iters,
          "preset": presets.BENCH_PRESET, "runs": a.runs, "ms_per_video": one, "bidirectional_ms_per_video": two,
          "video_report_ms_per_video": rep, "bidirectional_over_forward": two["median"] / one["median"],
          "video_report_over_bidirectional": rep["median"] / two["median"]})


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
    assert torch.cuda.is_available(), "flow_consistency_bench.py needs an MI355X"
    dev = torch.device("cuda:0")
    kernels(dev, 24, 436, 1024, a)
    kernels(dev, 3, 1088, 1920, a)
    if not a.no_video:
        video_cost(dev, a)


if __name__ == "__main__":
    main()
