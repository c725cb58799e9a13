#!/usr/bin/env python3
"""The volume-free correlation route (csrc/corr_direct.hip, EngineOptions.corr_direct) against the all-pairs volume, on the same GPU
in the same run.

    python tools/corr_direct_bench.py [--steps 7] [--calls 5] [--batches 9] [--presets config2_mixed,fp32_class] [--shapes sintel8,...]

Per preset (config2_mixed: fp16 volume / one fp16 product; fp32_class: fp32 volume / three split products) and shape -- Sintel 8
clips, KITTI T = 2 8 clips, Spring 1 and 8 clips, 1440 x 2560 one clip, 2160 x 3840 one clip (4 iterations) -- and per route:
(a) the step: HotPathEngine.forward on seeded synthetic features (graph replay), HIP events around each step after two warm-up steps,
    the median of --steps; torch.cuda.max_memory_allocated over engine construction and the steps, minus what was allocated before
    (the features included in neither).  A route whose plan cannot be allocated is reported as such.
(b) the correlation kernels alone, on the plan's own buffers and the coordinates the last step left (a smooth flow):
    sf_corr_direct_pack and sf_corr_direct_lookup against the blocked build and lookup; HIP events around batches of --calls calls,
    the median of --batches.  For the direct lookup: achieved FLOP/s on its 2 * 400 * D useful FLOPs per pixel, and the ratio of
    products computed (16 x 16 per chunk of box cells that is not skipped) to products needed (400 per pixel), counted on the host
    from the same coordinates by the kernel's rule over 64 sampled tiles per image.
(c) the direct lookup with adversarial coordinates (uniformly random over [-8, w + 8) x [-8, h + 8): every tile's box is the whole
    level), up to Spring's grid; beyond it the figure would take minutes and is left out.
One JSON line per measurement, appended to profiles/corr_direct_bench.jsonl."""
import argparse
import json
import os
import sys
from dataclasses import replace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from streamflow_amd import ops, presets, synthetic as syn
from streamflow_amd.engine import EngineOptions, HotPathEngine

OUT = os.path.join(REPO, "profiles", "corr_direct_bench.jsonl")
D = 256
SHAPES = {  # name: (H, W, T, clips, iters)
    "sintel8": (440, 1024, 4, 8, 15), "kitti8": (376, 1248, 2, 8, 15), "spring1": (1088, 1920, 4, 1, 15),
    "spring8": (1088, 1920, 4, 8, 15), "1440p1": (1440, 2560, 4, 1, 15), "2160p1": (2160, 3840, 4, 1, 4)}
ADVERSARIAL_MAX_PX = 40000


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def median_us(fn, batches, calls):
    for _ in range(calls):
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


def products_ratio(xy, h, w, tiles=64, seed=0):
    """Products computed / products needed by the lookup's rule (csrc/corr_direct.hip): per tile of 16 consecutive pixels and level
    the bounding box of the clipped windows in chunks of 16 cells, a chunk counted when any pixel's window holds one of its cells.
    xy [n][2][N] on the host; `tiles` sampled tiles per image."""
    n, _, N = xy.shape
    rng = np.random.default_rng(seed)
    computed = needed = 0
    for img in range(n):
        for t in rng.choice((N + 15) // 16, size=min(tiles, (N + 15) // 16), replace=False):
            p = np.arange(16 * t, min(16 * t + 16, N))
            needed += 400 * len(p)
            for l in range(4):
                hl, wl = h >> l, w >> l
                c = xy[img][:, p].astype(np.float32) * np.float32(2.0 ** -l)
                c = np.where((c > -1e6) & (c < 1e6), c, -1e6)
                x0, y0 = np.floor(c[0]).astype(np.int64) - 4, np.floor(c[1]).astype(np.int64) - 4
                lx, hx, ly, hy = np.maximum(x0, 0), np.minimum(x0 + 9, wl - 1), np.maximum(y0, 0), np.minimum(y0 + 9, hl - 1)
                ok = (lx <= hx) & (ly <= hy)
                if not ok.any():
                    continue
                bx0, bx1, by0, by1 = lx[ok].min(), hx[ok].max(), ly[ok].min(), hy[ok].max()
                bw = bx1 - bx0 + 1
                hit = np.zeros((by1 - by0 + 1) * bw, bool)
                for i in np.nonzero(ok)[0]:
                    box = np.zeros((by1 - by0 + 1, bw), bool)
                    box[ly[i] - by0: hy[i] - by0 + 1, lx[i] - bx0: hx[i] - bx0 + 1] = True
                    hit |= box.reshape(-1)
                hit = np.pad(hit, (0, -len(hit) % 16)).reshape(-1, 16).any(1)
                computed += 256 * int(hit.sum())
    return computed / max(1, needed)


def kernels_alone(eng, pl, fmaps, a, rec):
    Bc, Pn, h, w, P = pl.Bc, pl.Pn, pl.h, pl.w, pl.P
    T = Pn + 1
    f1, f2 = fmaps.data_ptr(), fmaps.data_ptr() + 4 * D * P
    if pl.corr_direct:
        koct = pl.corr_blocked
        out = None if koct else replace(pl.corr, shadow=None)
        look = lambda c=pl.coords1: ops.corr_direct_lookup(pl.corr_ws, c, out, pl.corr if koct else None, Bc, Pn, D, h, w, pl.corr_prec)
        rec["pack_us"] = median_us(lambda: ops.corr_direct_pack(f1, f2, T * D * P, D * P, pl.corr_ws, Bc, Pn, D, h, w, pl.corr_prec),
                                   a.batches, a.calls)
        rec["lookup_us"] = median_us(look, a.batches, a.calls)
        flops = 2.0 * 400 * D * P * pl.n
        rec["lookup_useful_tflops"] = flops / rec["lookup_us"]["median"] * 1e-6
        xy = pl.coords1.tensor().view(pl.n, 2, P).cpu().numpy()
        rec["products_computed_over_needed"] = products_ratio(xy, h, w)
        if P <= ADVERSARIAL_MAX_PX:
            g = torch.Generator().manual_seed(5)
            adv = torch.stack([torch.rand(pl.n, P, generator=g) * (w + 16) - 8, torch.rand(pl.n, P, generator=g) * (h + 16) - 8], 1)
            adv = ops.Planes.of(adv.contiguous().to(fmaps.device))
            rec["adversarial_lookup_us"] = median_us(lambda: look(adv), 3, 1)
            rec["adversarial_products_computed_over_needed"] = products_ratio(adv.tensor().view(pl.n, 2, P).cpu().numpy(), h, w, tiles=8)
    else:
        assert pl.vol is not None, "the bench presets keep blocked volumes"
        build = lambda: ops.corr_build_blocked(f1, f2, T * D * P, D * P, pl.vol, Bc, Pn, D, ws=pl.corr_ws)
        if pl.corr_blocked:
            look = lambda: ops.corr_lookup_blocked(pl.vol, pl.coords1, None, pl.corr, Bc, Pn)
        else:
            out = replace(pl.corr, shadow=None)
            look = lambda: ops.corr_lookup_blocked(pl.vol, pl.coords1, out, None, Bc, Pn)
        rec["build_us"] = median_us(build, a.batches, a.calls)
        rec["lookup_us"] = median_us(look, a.batches, a.calls)


def one(dev, preset, shape, route, a):
    H, W, T, clips, iters = SHAPES[shape]
    h, w = H // 8, W // 8
    rec = {"preset": preset, "shape": shape, "frame": [H, W], "grid": [h, w], "pixels": h * w, "T": T, "clips": clips, "iters": iters,
           "route": route, "steps": a.steps}
    fmaps, cnets = syn.make_features(7, clips, T, h, w)
    fmaps, cnets = fmaps.to(dev), cnets.to(dev)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    eng = None
    try:
        eng = HotPathEngine(syn.make_params(0, T), device=dev, T=T, use_graph=True, options=EngineOptions(corr_direct=route == "direct"),
                            **presets.engine_kwargs(preset))
        for _ in range(2):
            eng.forward(fmaps, cnets, iters=iters)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.steps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            eng.forward(fmaps, cnets, iters=iters)
            e.record()
            e.synchronize()
            times.append(s.elapsed_time(e))
        rec["step_ms"] = {"median": float(np.median(times)), "min": float(np.min(times)), "max": float(np.max(times))}
        rec["peak_memory_gb"] = (torch.cuda.max_memory_allocated() - before) / 1e9
        pl, = eng._plans.values()
        assert pl.corr_direct == (route == "direct")
        rec["correlation_buffer_gb"] = (pl.corr_ws.numel() + (0 if pl.vol is None else pl.vol.buf.numel())) / 1e9
        kernels_alone(eng, pl, fmaps, a, rec)
    except torch.cuda.OutOfMemoryError as err:
        rec["cannot_allocate"] = str(err).splitlines()[0][:200]
    emit(rec)
    del eng, fmaps, cnets
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--presets", default="config2_mixed,fp32_class")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "corr_direct_bench.py needs an MI355X"
    dev = torch.device("cuda:0")
    for preset in a.presets.split(","):
        for shape in a.shapes.split(","):
            for route in ("volume", "direct"):
                one(dev, preset, shape, route, a)


if __name__ == "__main__":
    main()
