#!/usr/bin/env python3
"""Point tracking: sft_track_advance and sft_draw_tracks (csrc/track.hip) against the bytes they must move and against what a user
would write in torch today, on the same GPU in the same run; and track_points against predict_video alone.

    python tools/track_bench.py [--batches 20] [--calls 5] [--frames 50] [--runs 3] [--no-video] [--out FILE]

Measurements, not gates.  Synthetic smooth fields of a few pixels (bwd = the negated forward field plus noise), so neighbouring points
share taps as they do on footage.
(a) sft_track_advance, dense mode, 24 fields of 436 x 1024 (one model call of 8 clips at T = 4) and 3 of 1088 x 1920 (one Spring
    clip), with and without bwd: HIP events around batches of --calls calls after warming every shape up, the median over --batches
    batches; operands and outputs rotate through more than 256 MB so that nothing is served from a cache.  Bytes a call must move per
    point and step, from the shapes alone: 8 B of fwd, 8 B of bwd when given, 9 B written (two floats and a status byte);
    "fraction_of_hbm_roof" is those bytes over the time over the 8 TB/s roof the README uses.
(b) the same K steps in three forms: one launch; K calls with n_steps = 1 and the state carried; the torch form (a chain of
    F.grid_sample(align_corners=True) on the field with the positions normalised, the inside test and the forward-backward test as
    elementwise ops), timed the same way.
(c) sparse: 1024 points over 24 steps.
(d) sft_draw_tracks at 1024 points, trail 16, on 24 frames of 436 x 1024: the whole call, and the call with no drawable sample (the
    clear, an empty stamp pass and the resolve); the difference is what stamping costs.
(e) track.track_points and video.predict_video(bidirectional=True) around a stand-in model that costs nothing (it returns views
    of the clip tensor), on a synthetic 436 x 1024 video: wall clock per video, the median of --runs.  With a real model both grow by
    the model's time.
One JSON line per measurement, appended to profiles/track_bench.jsonl (or --out)."""
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

from streamflow_amd import _track_lib, ops, track

HBM_ROOF = 8.0e12
OUT = [os.path.join(REPO, "profiles", "track_bench.jsonl")]
ALPHA, BETA = 0.01, 0.5


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


def smooth_fields(n, h, w, dev, seed, amp=3.0):
    """(fwd, bwd) fp32 [n, 2, h, w]: low-pass noise of about `amp` pixels; bwd = -fwd + a little noise."""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(n, 2, max(2, h // 32), max(2, w // 32), generator=g)
    fwd = (F.interpolate(low, size=(h, w), mode="bicubic", align_corners=True) * amp).contiguous()
    bwd = (-fwd + 0.05 * torch.randn(n, 2, h, w, generator=g)).contiguous()
    return fwd.to(dev), bwd.to(dev)


class Rotation:
    """`count` operand sets used round robin."""

    def __init__(self, make, count):
        self.sets, self.i = [make(k) for k in range(count)], 0

    def next(self):
        self.i = (self.i + 1) % len(self.sets)
        return self.sets[self.i]


def raw_advance(lib, fwd, bwd, state, xy, st, K, frame0=0, first=0):
    """sft_track_advance on fields first .. first + K - 1, rows into xy / st [K..]; state (sxy, sst) or None: dense."""
    h, w = fwd.shape[-2:]
    P = xy.shape[-1]
    f = fwd[first:first + K]
    b = None if bwd is None else bwd[first:first + K]
    rc = lib.sft_track_advance(f.data_ptr(), f.stride(0), f.stride(1), f.stride(2), None if b is None else b.data_ptr(), f.stride(0), f.stride(1),
                               f.stride(2), K, h, w, frame0, None if state is None else state[0].data_ptr(),
                               None if state is None else state[1].data_ptr(), None, P, ALPHA, BETA, 0, xy[first:].data_ptr(),
                               st[first:].data_ptr(), None, None, None, None, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.sft_last_error()


def torch_chain(fwd, bwd, grid):
    """The K steps as torch ops: positions [2, P] carried, rows stacked.  Samples with grid_sample(align_corners=True, bilinear),
    which clamps nothing: the inside test is made before, and lost points are held."""
    K, _, h, w = fwd.shape
    p = grid.clone()
    lost = torch.zeros(p.shape[1], dtype=torch.bool, device=p.device)
    occ = torch.zeros_like(lost)
    scale = torch.tensor([2.0 / max(w - 1, 1), 2.0 / max(h - 1, 1)], device=p.device)[:, None]
    rows, stat = [], []

    def take(field, pos):
        g = (pos * scale - 1.0).t()[None, None]                          # [1, 1, P, 2]
        return F.grid_sample(field[None], g, mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0]   # [2, P]

    for k in range(K):
        f = take(fwd[k], p)
        q = p + f
        ok = (q[0] >= 0) & (q[0] <= w - 1) & (q[1] >= 0) & (q[1] <= h - 1) & ~lost
        lost = ~ok
        p = torch.where(ok[None], q, p)
        if bwd is not None:
            b = take(bwd[k], p)
            d = f + b
            occ = ~((d * d).sum(0) <= ALPHA * ((f * f).sum(0) + (b * b).sum(0)) + BETA)
        rows.append(p)
        stat.append(torch.where(lost, 2, occ.to(torch.uint8)).to(torch.uint8))
    return torch.stack(rows), torch.stack(stat)


def bench_advance(lib, dev, n, h, w, a):
    P = h * w
    per_set = n * P * (8 + 8 + 9)
    count = max(2, int(np.ceil(300e6 / per_set)) + 1)

    def make(k):
        fwd, bwd = smooth_fields(n, h, w, dev, 10 + k)
        return fwd, bwd, torch.empty(n, 2, P, dtype=torch.float32, device=dev), torch.empty(n, P, dtype=torch.uint8, device=dev)

    rot = Rotation(make, count)
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=dev), torch.arange(w, dtype=torch.float32, device=dev), indexing="ij")
    grid = torch.stack([gx.reshape(-1), gy.reshape(-1)]).contiguous()
    grid_state = (grid, torch.zeros(P, dtype=torch.uint8, device=dev))
    for with_bwd in (True, False):
        need = n * P * (8 + (8 if with_bwd else 0) + 9)

        def one_launch():
            fwd, bwd, xy, st = rot.next()
            raw_advance(lib, fwd, bwd if with_bwd else None, None, xy, st, n)

        def k_calls():
            fwd, bwd, xy, st = rot.next()
            state = grid_state
            for k in range(n):
                raw_advance(lib, fwd, bwd if with_bwd else None, state, xy, st, 1, frame0=k, first=k)
                state = (xy[k], st[k])

        def torch_form():
            fwd, bwd, _, _ = rot.next()
            torch_chain(fwd, bwd if with_bwd else None, grid)

        # the three forms give the same rows (the torch form up to rounding: its sampling order differs)
        fwd, bwd, xy, st = rot.sets[0]
        raw_advance(lib, fwd, bwd if with_bwd else None, None, xy, st, n)
        one = (xy.clone(), st.clone())
        state = grid_state
        for k in range(n):
            raw_advance(lib, fwd, bwd if with_bwd else None, state, xy, st, 1, frame0=k, first=k)
            state = (xy[k], st[k])
        same = bool(torch.equal(one[0], xy) and torch.equal(one[1], st))
        txy, tst = torch_chain(fwd, bwd if with_bwd else None, grid)
        agree = float((tst == one[1]).float().mean())
        both = (tst == one[1]).all(0)
        dev_px = float((txy - one[0])[:, :, both].abs().max()) if bool(both.any()) else None
        shared = {"fields": n, "h": h, "w": w, "points": P, "bwd": with_bwd, "operand_sets": count}
        t = median_us(one_launch, a.batches, a.calls)
        emit({"bench": "track_advance_dense", "form": "one_launch", **shared, "us": t, "bytes_needed": need,
              "bytes_per_point_step": need / (n * P), "fraction_of_hbm_roof": need / (t["median"] * 1e-6) / HBM_ROOF,
              "k_calls_bitwise_equal": same})
        t1 = median_us(k_calls, a.batches, max(1, a.calls // 2))
        emit({"bench": "track_advance_dense", "form": "k_calls_of_one_step", **shared, "us": t1, "ratio_to_one_launch": t1["median"] / t["median"]})
        t2 = median_us(torch_form, max(3, a.batches // 4), 1)
        emit({"bench": "track_advance_dense", "form": "torch_grid_sample_chain", **shared, "us": t2, "ratio_to_one_launch": t2["median"] / t["median"],
              "status_agreement_with_kernel": agree, "max_abs_position_difference_px_where_status_agrees": dev_px})


def bench_sparse(lib, dev, a, n=24, h=436, w=1024, P=1024):
    fwd, bwd = smooth_fields(n, h, w, dev, 77)
    q = torch.from_numpy(track.grid_queries((h, w), 1)[:: (h * w) // P][:P].copy()).to(dev)
    state = (q[:, 1:].t().contiguous(), torch.full((P,), 3, dtype=torch.uint8, device=dev))
    xy, st = torch.empty(n, 2, P, dtype=torch.float32, device=dev), torch.empty(n, P, dtype=torch.uint8, device=dev)
    for with_bwd in (True, False):
        t = median_us(lambda: raw_advance(lib, fwd, bwd if with_bwd else None, state, xy, st, n), a.batches, 4 * a.calls)
        emit({"bench": "track_advance_sparse", "fields": n, "h": h, "w": w, "points": P, "bwd": with_bwd, "us": t,
              "note": "24 dependent gathers per point on 16 waves: a latency chain, not a bandwidth figure"})


def bench_draw(lib, dev, a, n=24, h=436, w=1024, P=1024, trail=16):
    fwd, _ = smooth_fields(n + trail, h, w, dev, 78)
    q = torch.from_numpy(track.grid_queries((h, w), 1)[:: (h * w) // P][:P].copy()).to(dev)
    state = (q[:, 1:].t().contiguous(), torch.full((P,), 3, dtype=torch.uint8, device=dev))
    xy, st, _ = ops.track_advance(fwd, None, state=state)
    frames = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev)
    pal, fade = torch.from_numpy(track.default_palette()).to(dev), torch.from_numpy(track.alpha_fade(trail)).to(dev)
    out = torch.empty_like(frames)
    ws = torch.empty(int(lib.sft_draw_tracks_ws_bytes(n, h, w)), dtype=torch.uint8, device=dev)
    lost = torch.full_like(st, 2)

    def call(status):
        rc = lib.sft_draw_tracks(frames.data_ptr(), h * w * 3, w * 3, 3, 1, n, h, w, trail, xy.data_ptr(), status.data_ptr(), int(xy.shape[0]), P, 1,
                                 trail, 3, 1, 0, pal.data_ptr(), int(pal.shape[0]), fade.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.sft_last_error()

    whole = median_us(lambda: call(st), a.batches, a.calls)
    empty = median_us(lambda: call(lost), a.batches, a.calls)
    need = n * h * w * (3 + 3 + 4 + 4)                                   # source, out, key image written and read
    emit({"bench": "draw_tracks", "frames": n, "h": h, "w": w, "points": P, "trail": trail, "us_whole_call": whole,
          "us_clear_empty_stamp_resolve": empty, "us_stamp_by_difference": whole["median"] - empty["median"], "bytes_needed": need,
          "fraction_of_hbm_roof_whole_call": need / (whole["median"] * 1e-6) / HBM_ROOF,
          "drawable_share": float((st[1:] == 0).float().mean())})


def free_model(imgs):
    return [imgs[:, k, :2] for k in range(imgs.shape[1] - 1)]


def bench_video(dev, a, h=436, w=1024):
    from streamflow_amd import video
    g = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (a.frames, h, w, 3), dtype=torch.uint8, generator=g)
    q = track.grid_queries((h, w), 16)

    def wall(fn):
        times = []
        for _ in range(a.runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return float(np.median(times[1:]))

    base = wall(lambda: video.predict_video(free_model, frames, T=4, clips_per_step=8, bidirectional=True, sink=lambda *x: None))
    tr = wall(lambda: track.track_points(free_model, frames, q, T=4, clips_per_step=8))
    emit({"bench": "track_points_video", "frames": a.frames, "h": h, "w": w, "points": int(len(q)), "model": "stand-in that costs nothing",
          "s_predict_video_bidirectional": base, "s_track_points": tr, "s_added": tr - base})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-video", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        OUT[0] = a.out
    if not torch.cuda.is_available():
        raise SystemExit("track_bench measures on the GPU; there is nothing to measure without one")
    dev = torch.device("cuda:0")
    lib = _track_lib.load()
    emit({"bench": "track_bench", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "batches": a.batches, "calls": a.calls})
    bench_advance(lib, dev, 24, 436, 1024, a)
    bench_advance(lib, dev, 3, 1088, 1920, a)
    bench_sparse(lib, dev, a)
    bench_draw(lib, dev, a)
    if not a.no_video:
        bench_video(dev, a)


if __name__ == "__main__":
    main()
