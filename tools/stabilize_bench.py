#!/usr/bin/env python3
"""Video stabilisation: sf_motion_moments, sf_motion_fit and sf_warp_affine_u8 (csrc/stabilize.hip) against the bytes they must
move and against what a user would write in torch today, on the same GPU in the same run; and stabilize_video against predict_video.

    python tools/stabilize_bench.py [--batches 30] [--calls 10] [--frames 50] [--runs 3] [--no-video] [--out FILE]

At 24 fields of 436 x 1024 (one model call of 8 clips at T = 4) and 3 of 1088 x 1920 (one Spring clip), synthetic fields (an affine
camera plus noise, a quarter of the frame moving on its own) and noise frames:
(a) the entry points called directly: HIP events around batches of --calls calls after warming every shape up, the median over
    --batches batches; operands and outputs rotate through more than 256 MB so that nothing is served from a cache;
(b) the same results as torch expressions: the weights and the thirteen weighted sums in float64 (a plain pass and a pass with a
    model, and the chain of six rounds with torch.linalg.solve between them); F.affine_grid + F.grid_sample(align_corners=True) with
    the conversions from and to uint8 HWC frames; timed the same way.
Bytes a call must move, from the shapes alone: a moments pass 8 B per pixel (the flow, once; 9 B with a class map), the fit
rounds x that; the warp 3 B (source, once) + 3 B (out) = 6 B per pixel.  "fraction_of_hbm_roof" is those bytes over the kernel time
over the 8 TB/s roof the README uses.
(c) stabilize.stabilize_video and video.predict_video around a stand-in model that costs nothing (it returns views of the clip
    tensor), on a synthetic 436 x 1024 video: wall clock per video, the median of --runs.  The difference is what the fit, the second
    read of the frames and the rendering cost; with a real model both grow by the model's time.
One JSON line per measurement, appended to profiles/stabilize_bench.jsonl (or --out)."""
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

from streamflow_amd import _lib, ops

HBM_ROOF = 8.0e12
OUT = [os.path.join(REPO, "profiles", "stabilize_bench.jsonl")]
ROUNDS, KAPPA, C_FLOOR = 6, 2.0, 1.0


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT[0], "a") as f:
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


def make_set(n, h, w, dev, seed):
    """(flows fp32 [n, 2, h, w], frames uint8 [n, h, w, 3], inverse maps fp32 [n, 6])."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.arange(w, dtype=torch.float32) - (w - 1) / 2) / w
    y = ((torch.arange(h, dtype=torch.float32) - (h - 1) / 2) / w)[:, None]
    flows = torch.empty(n, 2, h, w)
    for i in range(n):
        p = torch.randn(6, generator=g) * torch.tensor([4.0, 8.0, 8.0, 4.0, 8.0, 8.0])
        flows[i, 0] = p[0] + p[1] * x + p[2] * y
        flows[i, 1] = p[3] + p[4] * x + p[5] * y
    flows += 0.3 * torch.randn(n, 2, h, w, generator=g)
    flows[:, 0, h // 4:3 * h // 4, w // 4:3 * w // 4] += 9.0
    flows[:, 1, h // 4:3 * h // 4, w // 4:3 * w // 4] -= 6.0
    frames = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)
    th = 0.02 * torch.randn(n, generator=g)
    maps = torch.stack([torch.cos(th), -torch.sin(th), 6 * torch.randn(n, generator=g), torch.sin(th), torch.cos(th),
                        6 * torch.randn(n, generator=g)], 1)
    return [t.contiguous().to(dev) for t in (flows, frames, maps)]


class TorchFit:
    """The weighted sums and the chain as torch expressions on the GPU (float32 weights, float64 sums, affine model)."""

    def __init__(self, h, w, dev):
        s = 2.0 / max(w - 1, h - 1, 1)
        self.X = ((torch.arange(w, device=dev, dtype=torch.float32) - (w - 1) * 0.5) * s)[None, None, :]
        self.Y = ((torch.arange(h, device=dev, dtype=torch.float32) - (h - 1) * 0.5) * s)[None, :, None]
        self.max_mag = 4.0 * max(h, w)

    def moments(self, flows, model=None, inv_c2=None):
        u, v = flows[:, 0], flows[:, 1]
        wt = ((u.abs() <= self.max_mag) & (v.abs() <= self.max_mag)).float()
        if model is not None:
            m = model[:, :, None, None]
            ru = u - (m[:, 0] + (m[:, 1] * self.X + m[:, 2] * self.Y))
            rv = v - (m[:, 3] + (m[:, 4] * self.X + m[:, 5] * self.Y))
            t = (ru * ru + rv * rv) * inv_c2[:, None, None]
            wt = wt * torch.where(t < 1, (1 - t) * (1 - t), torch.zeros_like(t))
        W, X, Y, U, V = wt.double(), self.X.double(), self.Y.double(), u.double(), v.double()
        WX, WY = W * X, W * Y
        terms = (W, WX, WY, WX * X, WX * Y, WY * Y, W * U, WX * U, WY * U, W * V, WX * V, WY * V, W * (U * U + V * V), (wt > 0).double())
        return torch.stack([t.sum((1, 2)) for t in terms], 1)

    def solve(self, mom):
        M = torch.stack([mom[:, [0, 1, 2]], mom[:, [1, 3, 4]], mom[:, [2, 4, 5]]], 1)
        b = torch.stack([mom[:, [6, 7, 8]], mom[:, [9, 10, 11]]], 2)
        p = torch.linalg.solve(M, b)                                     # [n, 3, 2]
        rss = (mom[:, 12] - 2 * (p * b).sum((1, 2)) + (p * (M @ p)).sum((1, 2))).clamp_min(0) / mom[:, 0]
        c = (KAPPA * rss.sqrt()).clamp_min(C_FLOOR)
        return p.transpose(1, 2).reshape(-1, 6), (1 / (c * c)).float()

    def fit(self, flows):
        model, inv_c2 = None, None
        for _ in range(ROUNDS):
            model64, inv_c2 = self.solve(self.moments(flows, model, inv_c2))
            model = model64.float()
        return model64


def torch_warp(frames, theta, h, w):
    grid = F.affine_grid(theta, (frames.shape[0], 3, h, w), align_corners=True)
    val = F.grid_sample(frames.permute(0, 3, 1, 2).float(), grid, mode="bilinear", padding_mode="border", align_corners=True)
    return torch.floor(val + 0.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def theta_of(maps, h, w):
    """Pixel maps [n, 6] -> affine_grid's theta [n, 2, 3] (normalised coordinates, align_corners=True)."""
    n = maps.shape[0]
    B = torch.zeros(n, 3, 3, dtype=torch.float64, device=maps.device)
    B[:, :2] = maps.view(n, 2, 3).double()
    B[:, 2, 2] = 1
    to_px = torch.tensor([[(w - 1) / 2, 0, (w - 1) / 2], [0, (h - 1) / 2, (h - 1) / 2], [0, 0, 1]], dtype=torch.float64, device=maps.device)
    return (torch.linalg.inv(to_px) @ B @ to_px)[:, :2].float()


def kernels(dev, n, h, w, a):
    lib = _lib.load()
    px = n * h * w
    per_set = px * (8 + 3 + 3)
    nbuf = max(2, int(np.ceil(320e6 / per_set)))
    sets = [make_set(n, h, w, dev, 10 + i) for i in range(nbuf)]
    out = [torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
    mom = torch.empty(n, ops.MOT_LEN, dtype=torch.float64, device=dev)
    trace = torch.empty(n, ROUNDS, ops.MOT_TRACE_LEN, dtype=torch.float64, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.sf_motion_fit_ws_bytes(n, h, w, 1)), dtype=torch.uint8, device=dev)
    wws = torch.empty(int(lib.sf_warp_affine_ws_bytes(n, h, w)), dtype=torch.uint8, device=dev)
    max_mag = 4.0 * max(h, w)
    tf = TorchFit(h, w, dev)
    # a model to weigh against: the first set's fit, the same one for the kernel and the torch form
    ref_models, ref_info = ops.motion_fit(sets[0][0], kind="affine", rounds=ROUNDS)
    model32 = ref_info["normalised"].float().contiguous()
    inv_c2 = ref_info["trace"][:, -1, ops.MOT_TRACE_INV_C2].float().contiguous()
    thetas = [theta_of(s[2], h, w) for s in sets]
    turn = [0]

    def nxt():
        i = turn[0] % nbuf
        turn[0] += 1
        return i

    def moments(robust):
        def run():
            f = sets[nxt()][0]
            _lib.check(lib.sf_motion_moments(f.data_ptr(), f.stride(0), f.stride(1), f.stride(2), n, h, w, None, 0, 1, 2, 1.0, 0.0, 0.0, 1,
                                             max_mag, model32.data_ptr() if robust else None, inv_c2.data_ptr() if robust else None,
                                             mom.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream()), "sf_motion_moments")
        return run

    def fit():
        f = sets[nxt()][0]
        _lib.check(lib.sf_motion_fit(f.data_ptr(), f.stride(0), f.stride(1), f.stride(2), n, h, w, None, 0, 1, 2, 1.0, 0.0, 0.0, 1, max_mag,
                                     ops.MOTION_KINDS["affine"], ROUNDS, KAPPA, C_FLOOR, trace.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _lib.stream()), "sf_motion_fit")

    def warp():
        i = nxt()
        s, m = sets[i][1], sets[i][2]
        _lib.check(lib.sf_warp_affine_u8(s.data_ptr(), 3 * h * w, 3 * w, 3, 1, m.data_ptr(), n, h, w, ops.BORDERS["replicate"], 0, 0, 0,
                                         out[i].data_ptr(), counts.data_ptr(), wws.data_ptr(), wws.numel(), _lib.stream()),
                   "sf_warp_affine_u8")

    def t_moments(robust):
        return lambda: tf.moments(sets[nxt()][0], model32 if robust else None, inv_c2 if robust else None)

    def t_fit():
        return tf.fit(sets[nxt()][0])

    def t_warp():
        i = nxt()
        return torch_warp(sets[i][1], thetas[i], h, w)

    # agreement of the two forms on the first set
    turn[0] = 0
    moments(True)()
    turn[0] = 0
    warp()
    turn[0] = 0
    fit()
    torch.cuda.synchronize()
    tm = tf.moments(sets[0][0], model32, inv_c2)
    agree = {"moments_max_relative_difference": float(((tm - mom).abs() / tm.abs().clamp_min(1e-30)).max()),
             "fit_max_model_difference": float((tf.fit(sets[0][0]) - trace[:, -1, ops.MOT_TRACE_MODEL:ops.MOT_TRACE_MODEL + 6]).abs().max()),
             "warped_bytes_differing_by_more_than_1": int(((torch_warp(sets[0][1], thetas[0], h, w).int() - out[0].int()).abs() > 1).sum()),
             "pixels": px}
    shape = {"fields": n, "field": [h, w], "buffer_sets": nbuf, "rotating_bytes": nbuf * per_set, "batches": a.batches,
             "calls_per_batch": a.calls}
    res = {}
    for name, fn, nbytes in (("sf_motion_moments (plain pass)", moments(False), 8 * px), ("sf_motion_moments (pass with a model)", moments(True), 8 * px),
                             (f"sf_motion_fit ({ROUNDS} rounds, affine)", fit, ROUNDS * 8 * px), ("sf_warp_affine_u8 (replicate)", warp, 6 * px)):
        t = median_us(fn, a.batches, a.calls)
        res[name] = t["median"]
        emit({"kernel": name, **shape, "us": t, "bytes_needed": nbytes, "bytes_needed_per_pixel": nbytes // px,
              "bytes_per_s": nbytes / (t["median"] * 1e-6), "fraction_of_hbm_roof": nbytes / (t["median"] * 1e-6) / HBM_ROOF})
    few = max(1, a.calls // 5)
    tt = {"torch expressions: weighted sums, plain pass": median_us(t_moments(False), a.batches, few),
          "torch expressions: weighted sums, pass with a model": median_us(t_moments(True), a.batches, few),
          f"torch expressions: chain of {ROUNDS} rounds with torch.linalg.solve": median_us(t_fit, a.batches, 1),
          "torch expressions: affine_grid + grid_sample + conversions": median_us(t_warp, a.batches, few)}
    for name, t in tt.items():
        emit({"path": name, **shape, "us": t})
    kn, tn = list(res), list(tt)
    emit({"ratio": f"{n} fields of {h} x {w}", "agreement_with_torch_form": agree,
          **{"torch_over_kernel: " + k: tt[t_]["median"] / res[k] for k, t_ in zip(kn, tn)}})
    del sets, out
    torch.cuda.empty_cache()


def wall_ms(fn, runs):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median": float(np.median(times)), "min": float(np.min(times)), "max": float(np.max(times))}


def free_model(imgs):
    """A stand-in that costs nothing: pair k = views of the clip tensor's first two colour planes (values in [-1, 1])."""
    return [imgs[:, k, :2] for k in range(imgs.shape[1] - 1)]


def video_cost(dev, a):
    from streamflow_amd import stabilize, video
    H, W, T, n = 436, 1024, 4, a.frames
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(dev)
    sunk = lambda *args: None
    one = wall_ms(lambda: video.predict_video(free_model, frames, T=T, clips_per_step=8, sink=sunk), a.runs)
    stab = wall_ms(lambda: stabilize.stabilize_video(free_model, frames, sunk, kind="similarity", sigma=15.0, zoom="auto", T=T,
                                                     clips_per_step=8), a.runs)
    occ = wall_ms(lambda: stabilize.stabilize_video(free_model, frames, sunk, kind="similarity", sigma=15.0, zoom="auto", T=T,
                                                    clips_per_step=8, occlusion=True), a.runs)
    emit({"path": "stabilize_video around a stand-in model that costs nothing, device frames, 8 clips per call", "frames": n,
          "shape": [H, W], "T": T, "runs": a.runs, "predict_video_ms_per_video": one, "stabilize_video_ms_per_video": stab,
          "stabilize_video_with_occlusion_ms_per_video": occ, "added_ms_per_frame": (stab["median"] - one["median"]) / n,
          "added_with_occlusion_ms_per_frame": (occ["median"] - one["median"]) / n})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-video", action="store_true")
    ap.add_argument("--out", default=None, help="the JSON-lines file to append to (default: profiles/stabilize_bench.jsonl)")
    a = ap.parse_args()
    if a.out:
        OUT[0] = a.out
    assert a.batches >= 20, "the median needs at least 20 batches"
    assert torch.cuda.is_available(), "stabilize_bench.py needs an MI355X"
    dev = torch.device("cuda:0")
    kernels(dev, 24, 436, 1024, a)
    kernels(dev, 3, 1088, 1920, a)
    if not a.no_video:
        video_cost(dev, a)


if __name__ == "__main__":
    main()
