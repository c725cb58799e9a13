#!/usr/bin/env python3
"""Sintel / KITTI scoring: sf_flow_score_batch (csrc/flow_score_batch.hip, ops.flow_score_batch) against the ways the validators
scored before it, on the same box in the same run, on seeded random data.

    python tools/eval_score_bench.py [--batches 30] [--calls 5] [--host-reps 20] [--skip-report]

(a) sf_flow_score_batch, the entry point called directly with a prebuilt pointer table (the ops.flow_score_batch wrapper, whose
    Python checks cost host time, is timed too): 24 fields of 436 x 1024 (one model call of 8 clips at T = 4) against .flo ground
    truth with and without occlusion masks, and 8 KITTI fields of 375 x 1242 against 16-bit samples (4-byte loads: w is even, no
    multiple of four) and the same with the samples 2 bytes off (element loads).  Predictions are padder.unpad windows of the
    model's padded output.  HIP events around batches of calls, the median over the batches; the inputs rotate through more than
    256 MB of buffers so that the reads come from HBM.  Bytes are those the kernel must read (8 B/px prediction, 8 or 6 B/px
    ground truth, 1 B/px mask); the fraction of the 8 TB/s HBM roof follows from them.
(b) the same 24 Sintel fields as 24 ops.flow_score calls (48 launches; the Spring kernel, which knows no mask), and the host
    scoring of sintel_report / _kitti_scores for the same fields: flows copied to the host, torch expressions, list appends, one
    concatenate -- wall clock, median of the reps.
(c) evaluate.sintel_report over a small synthetic tree (one pass, one scene of 17 frames of 436 x 1024, SKFlow_MF8 on seeded
    weights) at clips_per_step 1 and 8: wall clock, split into PNG decode (flow_io.read_png), model calls (synchronised) and the
    rest (ground-truth reads, uploads, scoring).  The tree's PNGs are written by flow_io.write_png (filter type 0), which the
    pure-Python decoder reads far faster than the adaptive filters of the real dataset's files.
One JSON line."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from streamflow_amd import _lib, evaluate, flow_io, ops, scoring
from streamflow_amd.utils import InputPadder

HBM_ROOF = 8.0e12


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


def make_set(rng, dev, n, h, w, kind, mode, gt_offset=0):
    """One set of n fields on the device: (windows of the padded output, ground truths, masks, the padded output)."""
    padder = InputPadder((1, 3, h, w), mode=mode)
    left, right, top, bottom = padder._pad
    out = torch.from_numpy(rng.standard_normal((n, 2, h + top + bottom, w + left + right), dtype=np.float32) * 3).to(dev)
    preds = [out[i, :, top:top + h, left:left + w] for i in range(n)]
    if kind == "flo":
        gts = list(torch.from_numpy(rng.standard_normal((n, h, w, 2), dtype=np.float32) * 5).to(dev))
    else:
        smp = rng.integers(0, 65536, size=(n, h * w * 3 + gt_offset), dtype=np.uint16)
        smp[:, gt_offset + 2::3] %= 2                                    # valid samples: 0 or 1
        flat = torch.from_numpy(smp.view(np.int16)).to(dev)
        gts = [flat[i, gt_offset:].view(h, w, 3) for i in range(n)]
    masks = list(torch.from_numpy(np.where(rng.random((n, h, w)) < 0.3, 255, 0).astype(np.uint8)).to(dev))
    return preds, gts, masks, out


def bench_batch(rng, dev, a, n, h, w, kind, mode, with_mask, gt_offset=0):
    lib = _lib.load()
    px_bytes = 8 + (8 if kind == "flo" else 6) + (1 if with_mask else 0)
    call_bytes = n * h * w * px_bytes
    nsets = max(2, int(np.ceil(320e6 / call_bytes)))
    sets = [make_set(rng, dev, n, h, w, kind, mode, gt_offset) for _ in range(nsets)]
    tabs = []
    for preds, gts, masks, _ in sets:
        t = _lib.SfScoreFields()
        for i in range(n):
            t.pred[i], t.gt[i] = preds[i].data_ptr(), gts[i].data_ptr()
            if with_mask:
                t.mask[i] = masks[i].data_ptr()
        tabs.append(t)
    acc = torch.zeros(n, scoring.EVAL_LEN, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.sf_flow_score_batch_ws_bytes(n, h, w)), dtype=torch.uint8, device=dev)
    p0 = sets[0][0][0]
    turn = [0]

    def raw():
        k = turn[0] % nsets
        turn[0] += 1
        _lib.check(lib.sf_flow_score_batch(ctypes.byref(tabs[k]), n, p0.stride(0), p0.stride(1), scoring.GT_KINDS[kind], h, w,
                                           acc.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream()), "sf_flow_score_batch")

    def wrapped():
        k = turn[0] % nsets
        turn[0] += 1
        preds, gts, masks, _ = sets[k]
        ops.flow_score_batch(preds, gts, acc, kind, masks if with_mask else None)

    t = median_us(raw, a.batches, a.calls)
    tw = median_us(wrapped, a.batches, a.calls)
    res = {"fields": n, "shape": [h, w], "kind": kind, "masks": with_mask, "gt_byte_offset": 2 * gt_offset, "input_sets": nsets,
           "batches": a.batches, "calls_per_batch": a.calls, "flow_score_batch_us": t, "ops_flow_score_batch_us_(python_wrapper)": tw,
           "bytes_per_call": call_bytes, "bytes_per_s": call_bytes / (t["median"] * 1e-6),
           "fraction_of_hbm_roof": call_bytes / (t["median"] * 1e-6) / HBM_ROOF}
    return res, sets


def sintel_host_scoring(outs, padder, gts_np):
    """sintel_report's scoring of a batch of pairs: flows to the host, torch expressions, list appends, one concatenate."""
    epe_list = []
    for f, g in zip(outs, gts_np):
        flow = padder.unpad(f).float().cpu()
        gt = torch.from_numpy(g).permute(2, 0, 1).float()
        epe_list.append(torch.sum((flow - gt) ** 2, dim=0).sqrt().view(-1).numpy())
    return flow_io.sintel_metrics(np.concatenate(epe_list))


def kitti_host_scoring(outs, padder, png_np):
    def pairs():
        for f, p in zip(outs, png_np):
            flow, valid = flow_io.kitti_decode(p)
            yield padder.unpad(f).float().cpu(), torch.from_numpy(flow).permute(2, 0, 1).float(), torch.from_numpy(valid)
    return evaluate._kitti_scores(pairs())


def wall_ms(fn, reps):
    times = []
    for r in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= 2:
            times.append((time.perf_counter() - t0) * 1e3)
    return {"median": float(np.median(times)), "min": float(np.min(times)), "max": float(np.max(times))}


def report_timing(dev, clips_per_step, root, model, T, iters):
    """Wall clock of one sintel_report call, split by wrapping the PNG decoder and the model with timers."""
    spent = {"png_decode": 0.0, "model": 0.0}
    read_png = flow_io.read_png

    def timed_read(path):
        t0 = time.perf_counter()
        try:
            return read_png(path)
        finally:
            spent["png_decode"] += time.perf_counter() - t0

    class Timed:
        def parameters(self):
            return model.parameters()

        def _run(self, fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            spent["model"] += time.perf_counter() - t0
            return out

        def __call__(self, images, **kw):
            return self._run(lambda: model(images, **kw))

        def forward_normalised(self, imgs, it=None):
            return self._run(lambda: model.forward_normalised(imgs, it))

    flow_io.read_png = timed_read
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = evaluate.sintel_report(Timed(), iters=iters, root=root, nframes=T, dstypes=("clean",), device=dev,
                                     clips_per_step=clips_per_step)["clean"]
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    finally:
        flow_io.read_png = read_png
    return {"clips_per_step": clips_per_step, "pairs": rep["pairs"], "epe": rep["epe"], "total_s": total,
            "png_decode_s": spent["png_decode"], "model_s": spent["model"], "rest_s": total - spent["png_decode"] - spent["model"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=20)
    ap.add_argument("--skip-report", action="store_true")
    a = ap.parse_args()
    assert a.batches >= 20 and a.host_reps >= 20, "the medians need at least 20 repetitions"
    assert torch.cuda.is_available(), "eval_score_bench.py needs an MI355X"
    dev = torch.device("cuda:0")
    from bench import usable_cores
    torch.set_num_threads(min(usable_cores(), 64))                      # the cores this process may use, as tests/conftest.py does
    rng = np.random.default_rng(0)
    out = {"gpu": torch.cuda.get_device_name(0), "torch_threads": torch.get_num_threads()}
    # (a)
    H, W, N = 436, 1024, 24
    out["sintel_masks"], sets = bench_batch(rng, dev, a, N, H, W, "flo", "sintel", True)
    del sets
    out["sintel"], sets = bench_batch(rng, dev, a, N, H, W, "flo", "sintel", False)
    # (b) the same 24 fields, one ops.flow_score call each (the sets rotate as above)
    acc1 = torch.zeros(scoring.LEN, dtype=torch.float64, device=dev)
    ws1 = torch.empty(scoring.WS_BYTES, dtype=torch.uint8, device=dev)
    lib = _lib.load()
    turn = [0]

    def per_field_wrapped():
        preds, gts, _, _ = sets[turn[0] % len(sets)]
        turn[0] += 1
        for p, g in zip(preds, gts):
            ops.flow_score(p, g, acc1, 1)

    def per_field_raw():
        preds, gts, _, _ = sets[turn[0] % len(sets)]
        turn[0] += 1
        for p, g in zip(preds, gts):
            _lib.check(lib.sf_flow_score(p.data_ptr(), p.stride(0), p.stride(1), g.data_ptr(), H, W, 1, H, W, acc1.data_ptr(),
                                         ws1.data_ptr(), ws1.numel(), _lib.stream()), "sf_flow_score")

    out["24_ops_flow_score_calls_us"] = median_us(per_field_wrapped, a.batches, a.calls)
    out["24_sf_flow_score_calls_us_(entry_point)"] = median_us(per_field_raw, a.batches, a.calls)
    out["gate_batch_no_slower_than_24_calls"] = bool(out["sintel"]["ops_flow_score_batch_us_(python_wrapper)"]["median"]
                                                     <= out["24_ops_flow_score_calls_us"]["median"]
                                                     and out["sintel"]["flow_score_batch_us"]["median"]
                                                     <= out["24_sf_flow_score_calls_us_(entry_point)"]["median"])
    padder = InputPadder((1, 3, H, W))
    preds, gts, _, padded = sets[0]
    gts_np = [g.cpu().numpy() for g in gts]
    out["sintel_host_scoring_24_pairs_ms"] = wall_ms(lambda: sintel_host_scoring(padded, padder, gts_np), a.host_reps)
    out["sintel_host_over_batch_kernel"] = out["sintel_host_scoring_24_pairs_ms"]["median"] * 1e3 / out["sintel"]["flow_score_batch_us"]["median"]
    del sets, preds, gts, padded
    # KITTI
    Hk, Wk, Nk = 375, 1242, 8
    out["kitti_unaligned"], sets = bench_batch(rng, dev, a, Nk, Hk, Wk, "kitti", "kitti", False, gt_offset=1)
    del sets
    out["kitti"], sets = bench_batch(rng, dev, a, Nk, Hk, Wk, "kitti", "kitti", False)
    kp = InputPadder((1, 3, Hk, Wk), mode="kitti")
    preds, gts, _, padded = sets[0]
    png_np = [g.cpu().numpy().view(np.uint16) for g in gts]
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        out["kitti_host_scoring_8_pairs_ms"] = wall_ms(lambda: kitti_host_scoring(padded, kp, png_np), a.host_reps)
    out["kitti_host_over_batch_kernel"] = out["kitti_host_scoring_8_pairs_ms"]["median"] * 1e3 / out["kitti"]["flow_score_batch_us"]["median"]
    del sets, preds, gts, padded
    # (c)
    if not a.skip_report:
        from streamflow_amd import synthetic as syn
        from streamflow_amd.model import SKFlow_MF8, default_args
        T, iters, n = 4, 6, 17
        sd = dict(syn.make_params(31, T))
        sd.update({"fnet." + k: v for k, v in syn.make_twins_params(32).items()})
        sd.update({"cnet." + k: v for k, v in syn.make_twins_params(33).items()})
        model = SKFlow_MF8(default_args(T=T, mixed_precision=True)).to(dev).eval()
        model.load_state_dict(sd, strict=True)
        with tempfile.TemporaryDirectory() as root:
            os.makedirs(os.path.join(root, "training", "clean", "scene"))
            os.makedirs(os.path.join(root, "training", "flow", "scene"))
            for i in range(n):
                flow_io.write_png(os.path.join(root, "training", "clean", "scene", f"frame_{i + 1:04d}.png"),
                                  rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8))
                if i:
                    flow_io.write_flo(os.path.join(root, "training", "flow", "scene", f"frame_{i:04d}.flo"),
                                      rng.standard_normal((H, W, 2), dtype=np.float32) * 3)
            with contextlib.redirect_stdout(io.StringIO()):
                for cps in (1, 8):
                    report_timing(dev, cps, root, model, T, iters)                 # warm-up: engines, workspaces
                out["sintel_report"] = [report_timing(dev, cps, root, model, T, iters) for cps in (1, 8)]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
