#!/usr/bin/env python3
"""Spring scoring of one 1080 x 1920 pair: sf_flow_score (csrc/flow_score.hip, ops.flow_score) against the reference's host-side
scoring of the same pair on the same box (evaluate_mf.py:63-79 with SpringEval's flow[::2, ::2], mf_datasets.py:189-190).

    python tools/spring_score_bench.py [--batches 30] [--calls 10] [--host-reps 20]

(a) sf_flow_score per pair at ground-truth steps 1 and 2, the entry point called directly (the ops.flow_score wrapper, whose
    Python checks and workspace allocation cost host time, is timed too); the prediction is padder.unpad(flow[0]) of the model's
    [1, 2, 1080, 1920] output, the ground truth on the device at 1080 x 1920 or 2160 x 3840; HIP events around batches of calls,
    the median over the batches;
    the inputs rotate through more than 256 MB of buffers so that the reads come from HBM.  Bytes per pair are the cache lines the
    kernel touches: the prediction (8 B/px) and the ground-truth rows it reads (8 B/px at step 1; every even row in full at step 2,
    16 B/px); the fraction of the 8 TB/s HBM roof follows from them.
(b) the reference's way for the same pair: subsample the decoded ground truth, torch.from_numpy(...).permute(2, 0, 1).float(), the
    valid / bucket masks, padder.unpad(flow[0]).cpu(), the EPE and the four list appends -- wall clock per pair, median of the reps.
    Also the host-to-device copy of the decoded ground truth that spring_report's device path makes per pair.
One JSON line per step, then one with the ratio."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from streamflow_amd import _lib, ops, scoring
from streamflow_amd.utils import InputPadder
from tests import score_cases as sc

HBM_ROOF = 8.0e12
H, W = 1080, 1920


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


def reference_scoring(flow_padded, padder, gt_decoded, lists):
    """evaluate_mf.py:63-79 for one pair (SpringEval's subsampling and tensor conversion included)."""
    flows_gt = [torch.from_numpy(gt_decoded[::2, ::2]).permute(2, 0, 1).float()]
    valid = [~torch.isnan(torch.sum(flows_gt[i], dim=0)) for i in range(len(flows_gt))]
    valid_10 = [valid[i] & (torch.sum(flows_gt[i] ** 2, dim=0).sqrt() < 10) for i in range(len(flows_gt))]
    valid_10_40 = [valid[i] & (torch.sum(flows_gt[i] ** 2, dim=0).sqrt() >= 10) & (torch.sum(flows_gt[i] ** 2, dim=0).sqrt() < 40)
                   for i in range(len(flows_gt))]
    valid_40 = [valid[i] & (torch.sum(flows_gt[i] ** 2, dim=0).sqrt() >= 40) for i in range(len(flows_gt))]
    flows = [padder.unpad(flow[0]).cpu() for flow in [flow_padded]]
    epe_list, epe_list_10, epe_list_10_40, epe_list_40 = lists
    for i in range(len(flows)):
        epe = torch.sum((flows[i] - flows_gt[i]) ** 2, dim=0).sqrt()
        epe_list.append(epe.view(-1).numpy())
        epe_list_10.append(epe.view(-1)[valid_10[i].view(-1)].numpy())
        epe_list_10_40.append(epe.view(-1)[valid_10_40[i].view(-1)].numpy())
        epe_list_40.append(epe.view(-1)[valid_40[i].view(-1)].numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=20)
    a = ap.parse_args()
    assert a.batches >= 20, "the median needs at least 20 batches"
    assert torch.cuda.is_available(), "spring_score_bench.py needs an MI355X"
    dev = torch.device("cuda:0")
    from bench import usable_cores
    torch.set_num_threads(min(usable_cores(), 64))                      # the cores this process may use, as tests/conftest.py does
    rng = np.random.default_rng(0)
    padder = InputPadder((1, 3, H, W))
    gt2 = sc.random_gt(rng, H, W, 2, 0.05)                              # decoded 2160 x 3840 ground truth
    g = sc.subsample(gt2, 2, H, W)
    pred_np = (np.nan_to_num(g) + rng.normal(0, 2.0, size=(2, H, W))).astype(np.float32)
    Hp, Wp = H + padder._pad[2] + padder._pad[3], W + padder._pad[0] + padder._pad[1]
    flow_padded = torch.zeros(1, 2, Hp, Wp)                             # the model's padded output (1080 is a multiple of 8)
    flow_padded[0, :, padder._pad[2]:padder._pad[2] + H, padder._pad[0]:padder._pad[0] + W] = torch.from_numpy(pred_np)
    acc = torch.zeros(scoring.LEN, dtype=torch.float64, device=dev)
    out = {}
    for step in (1, 2):
        gt = gt2 if step == 2 else np.ascontiguousarray(g.transpose(1, 2, 0))
        pair_bytes = 8 * H * W + (8 if step == 1 else 16) * H * W
        nbuf = max(2, int(np.ceil(320e6 / pair_bytes)))
        preds = [(flow_padded * (1.0 + 0.01 * k)).to(dev) for k in range(nbuf)]
        gts = [torch.from_numpy(gt).to(dev) for _ in range(nbuf)]
        views = [padder.unpad(p[0]) for p in preds]
        ws = torch.empty(scoring.WS_BYTES, dtype=torch.uint8, device=dev)
        lib = _lib.load()
        turn = [0]

        def call():                                                     # the wrapper: checks, workspace, launch
            k = turn[0] % nbuf
            turn[0] += 1
            ops.flow_score(padder.unpad(preds[k][0]), gts[k], acc, step)

        def raw():                                                      # the entry point alone (the kernels' time)
            k = turn[0] % nbuf
            turn[0] += 1
            v = views[k]
            _lib.check(lib.sf_flow_score(v.data_ptr(), v.stride(0), v.stride(1), gts[k].data_ptr(), gts[k].shape[0], gts[k].shape[1],
                                         step, H, W, acc.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream()), "sf_flow_score")

        t = median_us(raw, a.batches, a.calls)
        tw = median_us(call, a.batches, a.calls)
        res = {"step": step, "shape": [H, W], "gt_shape": list(gt.shape), "input_buffers": nbuf, "batches": a.batches,
               "calls_per_batch": a.calls, "flow_score_us": {"median": t[0], "min": t[1], "max": t[2]},
               "ops_flow_score_us_(python_wrapper)": {"median": tw[0], "min": tw[1], "max": tw[2]},
               "bytes_per_pair": pair_bytes, "bytes_per_s": pair_bytes / (t[0] * 1e-6),
               "fraction_of_hbm_roof": pair_bytes / (t[0] * 1e-6) / HBM_ROOF}
        out[step] = res
        print(json.dumps(res), flush=True)
        del preds, gts, views
    # (b) the reference's host-side scoring of one pair (the flow starts on the device, as the model leaves it)
    fp_dev = flow_padded.to(dev)
    times, uploads = [], []
    for r in range(a.host_reps + 2):
        lists = ([], [], [], [])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reference_scoring(fp_dev, padder, gt2, lists)
        t1 = time.perf_counter()
        torch.from_numpy(gt2).to(dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if r >= 2:
            times.append((t1 - t0) * 1e3)
            uploads.append((t2 - t1) * 1e3)
    host_ms = float(np.median(times))
    res = {"reference_host_scoring_ms": {"median": host_ms, "min": float(np.min(times)), "max": float(np.max(times))},
           "host_reps": a.host_reps, "torch_threads": torch.get_num_threads(),
           "gt_upload_ms_(device_path,_step_2)": float(np.median(uploads)),
           "ratio_host_over_kernel_step2": host_ms * 1e3 / out[2]["flow_score_us"]["median"],
           "ratio_host_over_kernel_step1": host_ms * 1e3 / out[1]["flow_score_us"]["median"]}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
