"""Dataset scoring loops with the reference's signatures and result dictionaries.

* ``validate_sintel_mf(model, iters, root, nframes)`` -- reference evaluate_mf.py:468-503 over a Sintel-layout tree
  ``root/training/{clean,final}/<scene>/frame_XXXX.png`` + ``root/training/flow/<scene>/frame_XXXX.flo``: every scene is cut
  into clips of ``nframes`` frames that overlap by one frame; the tail of a scene is covered by ONE clip aligned to the scene's
  end whose already-scored pairs carry frame id -1 and are skipped (core/mf_datasets.py:1125-1149); pad -> model -> unpad;
  per-pixel EPE over all scored pairs; returns ``{'clean': epe, 'final': epe}`` (the 1 / 3 / 5 px rates are printed like the
  reference prints them and returned by ``sintel_report``).
* ``validate_kitti_mf(model, iters, multi_root, nframes)`` -- evaluate_mf.py:106-142 over the multi-frame KITTI-2015 layout
  ``multi_root/training/image_2/000NNN_FF.png`` + ``flow_occ/000NNN_10.png``: the clip is frames 12 - nframes .. 11, only the
  LAST pair (frames 10 -> 11) has ground truth (core/mf_datasets.py:946-952); 'kitti' padding; EPE and the F1-all outlier rate
  (epe > 3 px and epe / |gt| > 5 %) over pixels with valid >= 0.5; returns ``{'kitti_epe': .., 'kitti_f1': ..}``.
* ``validate_kitti_mf_tile(model, iters, multi_root, nframes)`` / ``validate_kitti_tile(model, iters, root)`` -- the tiled KITTI
  protocols (evaluate_mf.py:985-1053 / :919-982): fixed-height bottom padding, overlapping crops of the training size, crops
  blended with a Gaussian weight each (streamflow_amd.tiling, the sf_tile_blend kernel); same scoring.
* ``validate_spring_mf(model, iters, root, tqdm_miniters, nframes, split)`` / ``spring_report`` -- evaluate_mf.py:50-102 over the
  Spring layout ``root/train/<scene>/frame_{left,right}/*.png`` + ``flow_{FW,BW}_<cam>/*.flo5`` (forward and backward clips, the
  ground truth subsampled [::2, ::2]); device flows are scored where they are by the sf_flow_score kernel (ops.flow_score),
  host flows by streamflow_amd.scoring.score_host with the same arithmetic.

* ``validate_sintel_occ_mf(model, iters, root, tqdm_miniters, nframes)`` -- evaluate_mf.py:549-592: the passes albedo, clean and
  final with the EPE also taken over occluded and non-occluded pixels apart (``root/training/occlusions/<scene>/frame_XXXX.png``,
  8-bit gray, occluded where 255).
* ``clips_per_step=k > 1`` (sintel_report, validate_sintel_mf, validate_sintel_occ_mf, validate_kitti_mf): k clips per model call
  and nothing but the accumulator leaves the GPU -- a Sintel scene goes through video.predict_video as uint8 frames (every frame
  decoded and uploaded once) and each batch's flows are scored where they are, against the .flo arrays as read, by
  ops.flow_score_batch (the sf_flow_score_batch kernel); KITTI sequences of one frame size are collected k at a time, each clip
  built by ops.frames_to_clips, one model call, the last pairs scored against the 16-bit PNG samples in one launch.  The
  default ``clips_per_step=1`` is the reference's loop, one clip per call, scored on the host.  ``python -m
  streamflow_amd.evaluate --dataset ..`` is the reference's ``evaluate_mf.py --dataset`` switch.

``model`` is anything with the reference's test-mode call ``model(images: list of [1,3,H,W] in 0..255, iters=.., test_mode=True)
-> list of nframes - 1 flows [1,2,H,W]`` (streamflow_amd.SKFlow_MF8, or the CPU oracle wrapped the same way in the tests); with
``clips_per_step > 1`` it is called as video.predict_video calls it (``model.forward_normalised(clips, iters)``, else
``model(clips)``, clips fp32 [k, T, 3, Hp, Wp] in [-1, 1]) and must live on a GPU: there is no host fallback.
Files are read with this package's own codecs (flow_io.py: PNG, .flo, KITTI 16-bit PNG; flo5.py: Spring's .flo5).  The frame
reader, the per-clip model call (pad -> model -> unpad), the clip schedule and the walks over the three dataset trees are
datasets.py's, shared with submit.py; ``sintel_clip_schedule`` is importable from here as before.  Host-side plumbing: the
kernels launched here are the tile blend of the tiled validators (ops.tile_blend) for models without ``forward_tiled`` and the
scoring kernels (ops.flow_score, ops.flow_score_batch).
"""
from __future__ import annotations

import glob
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import flow_io
from .datasets import (batched_call, frame_tensor, kitti_mf_clip, kitti_mf_sequences, model_device, padded_flows, read_clip,
                       read_frame, run_clip, sintel_clip_schedule, sintel_scenes, spring_clips, spring_flow_file)
from .utils import InputPadder

_image = frame_tensor                                                    # a PNG frame as float [3, H, W] in 0..255


def _occlusion(path: str, hw: Tuple[int, int]) -> np.ndarray:
    m = flow_io.read_png(path)
    if m.ndim != 2 or m.dtype != np.uint8 or tuple(m.shape) != tuple(hw):
        raise RuntimeError(f"{path}: an occlusion map is an 8-bit gray PNG of {hw[0]} x {hw[1]}, got {m.dtype} {m.shape}")
    return np.ascontiguousarray(m)


def _check_png_decode(png_decode: str) -> None:
    if png_decode not in ("host", "gpu"):
        raise ValueError(f"png_decode {png_decode!r} ('host' or 'gpu')")


def _check_flo5_decode(flo5_decode: str) -> None:
    if flo5_decode not in ("host", "gpu"):
        raise ValueError(f"flo5_decode must be 'host' or 'gpu' (got {flo5_decode!r})")


def _need_gpu(what: str, dev: torch.device) -> torch.device:
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"{what}: clips_per_step > 1 runs on the GPU (device {dev}, GPU available: {torch.cuda.is_available()}); "
                           "there is no CPU fallback -- clips_per_step=1 is the host-side path")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


@torch.no_grad()
def sintel_report(model: Callable, iters: int = 6, root: str = "/data/Sintel", nframes: int = 3,
                  dstypes: Sequence[str] = ("clean", "final"), device: Optional[torch.device] = None, clips_per_step: int = 1,
                  occ: bool = False, png_decode: str = "host") -> Dict[str, Dict[str, float]]:
    """Per render pass: {'epe', '1px', '3px', '5px', 'pairs'} over every scored pair of every scene.  clips_per_step > 1: that many
    clips per model call, scored on the GPU (adds 'pixels'); occ: also 'epe_occ', 'epe_noc', 'occ_pixels' from the scenes'
    occlusion maps.

    Two scorers, which differ in the last digits.  clips_per_step == 1 without occ is the reference's: the flows go to the host,
    the per-pixel EPE of every pair is kept and flow_io.sintel_metrics reduces the lot, pass by pass.  Everything else goes
    through the EVAL accumulator (scoring.py), one row per scored pair: device flows by ops.flow_score_batch, host flows (a CPU
    model) by scoring.score_host_fields with the same arithmetic; the device rows are copied to the host once, at the end of the
    report.  clips_per_step > 1: per scene, the uint8 frames (each decoded once) go through video.predict_video and every batch's
    flows are scored as they arrive (its `sink`), so neither a flow nor a whole scene's flows leave the GPU or stay on it.
    png_decode="gpu" (with clips_per_step > 1): a scene's frames are inflated on the host and unfiltered on the GPU
    (png_gpu.decode_frames) and reach predict_video as one device tensor; the same bytes, so the same report."""
    from . import ops, png_gpu, scoring, video
    _check_png_decode(png_decode)
    dev = device or model_device(model, torch.device("cpu"))
    clips_per_step, occ = int(clips_per_step), bool(occ)
    per_pixel = clips_per_step == 1 and not occ
    if clips_per_step < 1:
        raise ValueError(f"clips_per_step must be at least 1, got {clips_per_step}")
    if clips_per_step > 1:
        dev = _need_gpu("sintel_report", dev)
    report = {}
    rows = {d: [] for d in dstypes}                  # per pass: per-pixel EPE arrays, or [k, EVAL_LEN] arrays (host) / tensors (device)
    for dstype in dstypes:
        for scene, imgs, flos, occs in sintel_scenes(root, "training", dstype, flow=True, occ=occ):

            def truth(pairs: Sequence[int]):
                gts = [flow_io.read_flo(flos[j]) for j in pairs]
                return gts, ([_occlusion(occs[j], gts[0].shape[:2]) for j in pairs] if occ else None)

            if clips_per_step > 1:
                acc = torch.zeros(len(flos), scoring.EVAL_LEN, dtype=torch.float64, device=dev)

                def score(first_pair: int, flows: torch.Tensor, acc=acc, truth=truth) -> None:
                    gts, masks = truth(range(first_pair, first_pair + flows.shape[0]))
                    g = torch.from_numpy(np.stack(gts)).to(flows.device)
                    m = None if masks is None else list(torch.from_numpy(np.stack(masks)).to(flows.device))
                    ops.flow_score_batch(list(flows), list(g), acc[first_pair:first_pair + flows.shape[0]], "flo", m)

                frames = png_gpu.decode_frames(imgs, dev) if png_decode == "gpu" else [read_frame(p) for p in imgs]
                video.predict_video(model, frames, T=nframes, iters=iters, clips_per_step=clips_per_step, mode="sintel", device=dev,
                                    sink=score)
                rows[dstype].append(acc)
                continue
            for first, ids in sintel_clip_schedule(len(imgs), nframes):
                flows = run_clip(model, imgs[first:first + nframes], dev, iters)
                keep = [i for i in range(nframes - 1) if ids[i] != -1]
                if per_pixel:
                    flows = [f.float().cpu() for f in flows]
                    for i in keep:
                        gt = torch.from_numpy(flow_io.read_flo(flos[first + i])).permute(2, 0, 1).float()
                        rows[dstype].append(torch.sum((flows[i] - gt) ** 2, dim=0).sqrt().view(-1).numpy())
                    continue
                preds = [flows[i].float() for i in keep]
                gts, masks = truth([first + i for i in keep])
                if preds[0].is_cuda:
                    d = preds[0].device
                    acc = torch.zeros(len(keep), scoring.EVAL_LEN, dtype=torch.float64, device=d)
                    ops.flow_score_batch(preds, [torch.from_numpy(g).to(d) for g in gts], acc, "flo",
                                         None if masks is None else [torch.from_numpy(m).to(d) for m in masks])
                else:
                    acc = np.zeros((len(keep), scoring.EVAL_LEN), np.float64)
                    for j, pred in enumerate(preds):
                        scoring.score_host_fields(pred.numpy(), gts[j], acc[j], "flo", None if masks is None else masks[j])
                rows[dstype].append(acc)
        if per_pixel:
            m = flow_io.sintel_metrics(np.concatenate(rows[dstype]))
            m["pairs"] = len(rows[dstype])
            print("Validation (%s) EPE: %f, 1px: %f, 3px: %f, 5px: %f" % (dstype, m["epe"], m["1px"], m["3px"], m["5px"]))
            report[dstype] = m
    if per_pixel:
        return report
    on_dev = [r for d in dstypes for r in rows[d] if isinstance(r, torch.Tensor)]
    if on_dev:                                                          # one copy to the host for the whole report
        host = torch.cat([r.to(on_dev[0].device) for r in on_dev]).cpu().numpy()
        parts = iter(np.split(host, np.cumsum([r.shape[0] for r in on_dev])[:-1]))
        rows = {d: [next(parts) if isinstance(r, torch.Tensor) else r for r in rows[d]] for d in dstypes}
    for dstype in dstypes:
        if not rows[dstype]:
            raise RuntimeError(f"sintel_report: no pairs scored under {os.path.join(root, 'training', dstype)}")
        m = scoring.sintel_from(np.concatenate(rows[dstype]))
        print("Validation (%s) EPE: %f, 1px: %f, 3px: %f, 5px: %f" % (dstype, m["epe"], m["1px"], m["3px"], m["5px"]))
        if occ:
            print("Occ epe: %f, Noc epe: %f" % (m["epe_occ"], m["epe_noc"]))
        else:
            for k in ("epe_occ", "epe_noc", "occ_pixels"):
                del m[k]
        report[dstype] = m
    return report


@torch.no_grad()
def validate_sintel_mf(model: Callable, iters: int = 6, root: str = "/data/Sintel", tqdm_miniters: int = 1, nframes: int = 3,
                       device: Optional[torch.device] = None, clips_per_step: int = 1, png_decode: str = "host") -> Dict[str, float]:
    """The reference's return value: {'clean': mean EPE, 'final': mean EPE}  (evaluate_mf.py:468-503)."""
    return {k: v["epe"] for k, v in sintel_report(model, iters, root, nframes, device=device, clips_per_step=clips_per_step,
                                                  png_decode=png_decode).items()}


@torch.no_grad()
def validate_sintel_occ_mf(model: Callable, iters: int = 6, root: str = "/data/Sintel", tqdm_miniters: int = 1, nframes: int = 3,
                           clips_per_step: int = 1, device: Optional[torch.device] = None, png_decode: str = "host") -> Dict[str, float]:
    """The reference's validate_sintel_occ_mf (evaluate_mf.py:549-592): the passes albedo, clean and final, per pass the line of
    validate_sintel_mf and "Occ epe: .., Noc epe: .."; returns {pass: mean EPE}.  `tqdm_miniters` is accepted and ignored."""
    if hasattr(model, "eval"):
        model.eval()
    rep = sintel_report(model, iters, root, nframes, dstypes=("albedo", "clean", "final"), device=device,
                        clips_per_step=clips_per_step, occ=True, png_decode=png_decode)
    return {k: v["epe"] for k, v in rep.items()}


@torch.no_grad()
def validate_kitti_mf(model: Callable, iters: int = 6, multi_root: Optional[str] = None, nframes: int = 3,
                      device: Optional[torch.device] = None, clips_per_step: int = 1, png_decode: str = "host") -> Dict[str, float]:
    """{'kitti_epe', 'kitti_f1'} over the sequences present under multi_root/training (the reference walks 000000 .. 000199).
    clips_per_step > 1: up to that many sequences of one frame size per model call, scored on the GPU (_kitti_batched); with
    png_decode="gpu" their frames and flow_occ files are unfiltered on the GPU too."""
    _check_png_decode(png_decode)
    if multi_root is None:
        raise ValueError("validate_kitti_mf: multi_root (the multi-frame KITTI-2015 tree) is required")
    dev = device or model_device(model, torch.device("cpu"))
    image_root, flow_root, seqs = kitti_mf_sequences(multi_root, "training")
    if int(clips_per_step) != 1:
        return _kitti_batched(model, iters, image_root, flow_root, seqs, nframes, dev, int(clips_per_step), png_decode)

    def pairs():
        for seq in seqs:
            images = read_clip(kitti_mf_clip(image_root, seq, nframes), dev)
            gt, valid = _kitti_gt(os.path.join(flow_root, seq + "_10.png"))
            flows = padded_flows(model, images, iters, mode="kitti")
            yield flows[nframes - 2].float().cpu(), gt, valid             # only the last pair (frames 10 -> 11) has ground truth

    epe, f1 = _kitti_scores(pairs())
    return {"kitti_epe": epe, "kitti_f1": f1}


def _kitti_batched(model: Callable, iters: int, image_root: str, flow_root: str, seqs: Sequence[str], nframes: int,
                   dev: torch.device, clips_per_step: int, png_decode: str = "host") -> Dict[str, float]:
    """validate_kitti_mf, `clips_per_step` sequences per model call: consecutive sequences whose frames have one size (KITTI has
    five widths) are collected, each one's uint8 frames become a clip by ops.frames_to_clips (a video of n = T frames, 'kitti'
    padding), the clips run as one batch, and the last pair of every clip is scored in one ops.flow_score_batch call against the
    16-bit PNG samples as read (decoded in the kernel).  A size change and the end of the list flush the batch.  One accumulator
    row per sequence; scoring.kitti_from forms the reference's mean of per-image means and the F1-all rate.
    png_decode="gpu": a batch's frame files and its flow_occ files are inflated on the host and unfiltered on the GPU when the
    batch is flushed (png_gpu: one launch for the frames, one for the ground truth); the scoring call takes the decoded uint16
    samples where they are, nothing is uploaded but the scanlines."""
    from . import ops, png_gpu, scoring, video
    _check_png_decode(png_decode)
    if clips_per_step < 1:
        raise ValueError(f"clips_per_step must be at least 1, got {clips_per_step}")
    dev = _need_gpu("validate_kitti_mf", dev)
    T = int(nframes)
    call = batched_call(model, iters)
    rows, pending = [], []                                              # device rows [k, EVAL_LEN]; (frames [T, H, W, 3], samples)

    def flush() -> None:
        if not pending:
            return
        k = len(pending)
        if png_decode == "gpu":                                          # pending: (frame files, flow_occ file, (H, W))
            H, W = pending[0][2]
            frames = png_gpu.decode_frames([p for clip, _, _ in pending for p in clip], dev).view(k, T, H, W, 3)
            smp = png_gpu.decode_batch([g for _, g, _ in pending], dev)
            if smp.dtype == torch.uint8 or smp.shape[3] < 3:
                raise IOError(f"{pending[0][1]}: KITTI flow needs a 16-bit RGB PNG, got {smp.dtype} {tuple(smp.shape[1:])}")
            if tuple(smp.shape[1:3]) != (H, W):
                raise RuntimeError(f"{pending[0][1]}: ground truth {tuple(smp.shape[1:3])} for frames {(H, W)}")
            # (as int16, the same bits: the dtype the host path hands over, and one every torch build can slice and copy)
            gts = smp.view(torch.int16)[..., :3].contiguous()
        else:
            H, W = pending[0][0].shape[1:3]
            frames = torch.from_numpy(np.stack([f for f, _ in pending])).to(dev)
            # (the 16-bit samples travel as int16: the same bits, a dtype every torch build can copy to the device)
            gts = torch.from_numpy(np.stack([g for _, g in pending]).view(np.int16)).to(dev)
        pad = InputPadder((H, W), mode="kitti")._pad                     # [left, right, top, bottom]
        clips = torch.empty(k, T, 3, H + pad[2] + pad[3], W + pad[0] + pad[1], dtype=torch.float32, device=dev)
        for i in range(k):
            ops.frames_to_clips(frames[i], T, T, 0, 1, pad, channels_last=True, out=clips[i:i + 1])
        flows = list(call(clips))
        if len(flows) != T - 1:
            raise RuntimeError(f"validate_kitti_mf: the model returned {len(flows)} flows for clips of T = {T}")
        last = flows[T - 2].float()                                      # only the last pair (frames 10 -> 11) has ground truth
        preds = [last[i][:, pad[2]:pad[2] + H, pad[0]:pad[0] + W] for i in range(k)]
        acc = torch.zeros(k, scoring.EVAL_LEN, dtype=torch.float64, device=dev)
        ops.flow_score_batch(preds, list(gts), acc, "kitti")
        rows.append(acc)
        pending.clear()

    with torch.cuda.device(dev):
        for seq in seqs:
            path = os.path.join(flow_root, seq + "_10.png")
            if png_decode == "gpu":                                      # only the headers now: the files are read at the flush
                clip = kitti_mf_clip(image_root, seq, T)
                hw = video._png_size(clip[0])
                if pending and (len(pending) == clips_per_step or pending[0][2] != hw):
                    flush()
                pending.append((clip, path, hw))
                continue
            frames = np.stack([read_frame(p) for p in kitti_mf_clip(image_root, seq, T)])
            smp = flow_io.read_png(path)
            if smp.ndim != 3 or smp.shape[2] < 3 or smp.dtype != np.uint16:
                raise IOError(f"{path}: KITTI flow needs a 16-bit RGB PNG, got {smp.dtype} {smp.shape}")
            if smp.shape[:2] != frames.shape[1:3]:
                raise RuntimeError(f"{path}: ground truth {smp.shape[:2]} for frames {frames.shape[1:3]}")
            if pending and (len(pending) == clips_per_step or pending[0][0].shape != frames.shape):
                flush()
            pending.append((frames, np.ascontiguousarray(smp[:, :, :3])))
        flush()
        epe, f1 = scoring.kitti_from(torch.cat(rows))
    print("Validation KITTI: %f, %f" % (epe, f1))
    return {"kitti_epe": epe, "kitti_f1": f1}


# ---- Spring (evaluate_mf.py:50-102, core/mf_datasets.py:99-213) ---------------------------------------------------------------
@torch.no_grad()
def spring_report(model: Callable, iters: int = 6, root: str = "/data/Sintel", nframes: int = 3, device: Optional[torch.device] = None,
                  scenes: Optional[Sequence[str]] = ("0041",), flo5_decode: str = "host") -> Dict[str, float]:
    """The Spring validation of the reference (validate_spring_mf over SpringEval) as a dictionary: 'epe', '1px', '3px', '5px',
    'spring_1px', 'spring_1px_s0_10', 'spring_1px_s10_40', 'spring_1px_s40' (what the reference prints), plus 'epe_valid',
    'pixels', 'valid_pixels' and 'pairs'.

    Walks root/train/<scene>/frame_{left,right}/*.png: per scene (sorted), per camera (left, right), the forward clips, then the
    backward clips (the same frames reversed), both on sintel_clip_schedule; pair k of a clip starting at a is scored against
    ground-truth file a + k (datasets.spring_flow_file), subsampled [::2, ::2] as the reference does; pairs with frame id -1 are
    skipped.  Flows on the GPU are scored where they are by ops.flow_score into one device accumulator (one copy to the host at the end);
    host flows (a CPU model) by scoring.score_host, with the same arithmetic (scoring.py states how both relate to the reference).
    Reference quirks kept: only scene 0041 by default (the hard-coded train / val split, mf_datasets.py:117; scenes=None scores
    every scene); the dataset's |flow| < 1000 valid maps are not used; 'epe' is NaN as soon as one ground-truth pixel is NaN.
    flo5_decode="gpu": the ground truth of a clip's scored pairs is read by ONE flo5_gpu.read_batch call (chunks inflated and put
    together on the device, csrc/flo5_decode.hip) and handed to ops.flow_score as it is: the same bits as flo5.read_flo5's array, so
    the report is the host run's, key for key.  It needs the flows on the GPU; "host" (the default) is flo5.read_flo5 + an upload."""
    from . import flo5, flo5_gpu, ops, scoring
    _check_flo5_decode(flo5_decode)
    dev = device or model_device(model, torch.device("cpu"))
    if flo5_decode == "gpu" and (dev.type != "cuda" or not torch.cuda.is_available()):
        raise RuntimeError(f"spring_report: flo5_decode='gpu' decodes the ground truth on the GPU (device {dev}, GPU available: "
                           f"{torch.cuda.is_available()}); there is no CPU fallback -- flo5_decode='host' is the host-side path")
    train = os.path.join(root, "train")
    acc_host = np.zeros(scoring.LEN, np.float64)
    acc_dev = {}
    pairs = 0
    step = 2                                                            # SpringEval(subsample_groundtruth=True)
    for scene, cam, direction, order, n, schedule in spring_clips(root, "train", nframes, only=scenes):
        for first, ids in schedule:
            flows = run_clip(model, order[first:first + nframes], dev, iters)
            scored = [k for k in range(nframes - 1) if ids[k] != -1]
            files = {k: os.path.join(train, scene, spring_flow_file(direction, cam, n, first + k)) for k in scored}
            gts = {}
            if flo5_decode == "gpu" and scored:
                if not flows[scored[0]].is_cuda:
                    raise RuntimeError("spring_report: flo5_decode='gpu' needs the model's flows on the GPU; there is no CPU fallback")
                gts = dict(zip(scored, flo5_gpu.read_batch([files[k] for k in scored], flows[scored[0]].device)))
            for k in scored:
                pred = flows[k]
                if k in gts:
                    gt = gts[k]
                    if gt.dtype != torch.float32:
                        gt = gt.float()
                else:
                    gt = flo5.read_flo5(files[k])
                if pred.is_cuda:
                    acc = acc_dev.get(pred.device)
                    if acc is None:
                        acc = acc_dev[pred.device] = torch.zeros(scoring.LEN, dtype=torch.float64, device=pred.device)
                    if not isinstance(gt, torch.Tensor):
                        gt = torch.from_numpy(np.ascontiguousarray(gt, np.float32)).to(pred.device)
                    ops.flow_score(pred.float(), gt, acc, step)
                else:
                    scoring.score_host(pred.float().numpy(), gt, acc_host, step)
                pairs += 1
    if pairs == 0:
        raise RuntimeError(f"spring_report: no pairs scored under {train} (scenes={scenes})")
    for acc in acc_dev.values():
        acc_host = acc_host + acc.cpu().numpy()
    rep = scoring.report(acc_host)
    rep["pairs"] = pairs
    print("Validation EPE: %f, 1px: %f, 3px: %f, 5px: %f" % (rep["epe"], rep["1px"], rep["3px"], rep["5px"]))
    print("Spring 1px: %f, 1px(s0~10): %f, 1px(s10~40): %f, 1px(s40+): %f" % (
        rep["spring_1px"], rep["spring_1px_s0_10"], rep["spring_1px_s10_40"], rep["spring_1px_s40"]))
    return rep


@torch.no_grad()
def validate_spring_mf(model: Callable, iters: int = 6, root: str = "/data/Sintel", tqdm_miniters: int = 1, nframes: int = 3,
                       split: bool = False, device: Optional[torch.device] = None, scenes: Optional[Sequence[str]] = ("0041",),
                       flo5_decode: str = "host") -> float:
    """The reference's return value: the mean EPE over every scored pixel (evaluate_mf.py:50-102).  `split` and `tqdm_miniters`
    are accepted and ignored (the reference's SpringEval applies its 0041 split whatever `split` says; there is no progress bar).
    flo5_decode: as for spring_report."""
    _check_flo5_decode(flo5_decode)
    if hasattr(model, "eval"):
        model.eval()
    return spring_report(model, iters, root, nframes, device=device, scenes=scenes, flo5_decode=flo5_decode)["epe"]


# ---- tiled inference (evaluate_mf.py:858-1053) ------------------------------------------------------------------------------
def _tiled_flows(model: Callable, images: List[torch.Tensor], padder, tile: Tuple[int, int], iters: Optional[int],
                 dev: torch.device) -> List[torch.Tensor]:
    """Blended flows [2, h, w] (padding removed) of one clip of padded frames [1,3,Hp,Wp].  A model with `forward_tiled` runs all
    its crops in one batch; any other model (the CPU oracle, a stub) is called once per DISTINCT crop with the reference's
    test-mode call and the crops are blended by the same HIP kernel on `dev`.  `iters=None`: the model's own default (the
    reference's validate_kitti_tile calls the model without iters)."""
    from . import ops, tiling
    kw = {} if iters is None else {"iters": iters}
    if hasattr(model, "forward_tiled"):
        flows = model.forward_tiled(images, tile=tile, sigma=tiling.TILE_SIGMA, min_overlap=20, **kw)
        return [padder.unpad(f[0]).float() for f in flows]
    plan = tiling.make_plan(images[0].shape[-2:], tile, 20, pad=padder._pad)
    crops = []
    for (y, x) in plan.distinct:
        pred = model([im[:, :, y:y + tile[0], x:x + tile[1]] for im in images], test_mode=True, **kw)
        crops.append(torch.stack([f[0].float().to(dev) for f in pred]))
    out = ops.tile_blend(torch.stack(crops).contiguous(), tiling.tile_weights(tile, tiling.TILE_SIGMA, dev), plan)
    return [out[0, i] for i in range(out.shape[1])]


def _kitti_scores(pairs) -> Tuple[float, float]:
    """Mean of the per-frame EPE and the F1-all rate (epe > 3 px and > 5 % of |gt|) over pixels with valid >= 0.5, the
    reference's scoring of every KITTI validator; `pairs` yields (flow [2,H,W], gt [2,H,W], valid [H,W]) on the host."""
    out_list, epe_list = [], []
    for flow, gt, valid in pairs:
        epe = torch.sum((flow - gt) ** 2, dim=0).sqrt().view(-1)
        mag = torch.sum(gt ** 2, dim=0).sqrt().view(-1)
        val = valid.view(-1) >= 0.5
        out = ((epe > 3.0) & ((epe / mag) > 0.05)).float()
        epe_list.append(epe[val].mean().item())
        out_list.append(out[val].numpy())
    epe = float(np.mean(np.array(epe_list)))
    f1 = float(100 * np.mean(np.concatenate(out_list)))
    print("Validation KITTI: %f, %f" % (epe, f1))
    return epe, f1


def _kitti_gt(path: str):
    gt_np, valid_np = flow_io.read_flow_kitti(path)
    return torch.from_numpy(gt_np).permute(2, 0, 1).float(), torch.from_numpy(valid_np)


@torch.no_grad()
def validate_kitti_mf_tile(model: Callable, iters: int = 6, multi_root: Optional[str] = None, nframes: int = 3,
                           device: Optional[torch.device] = None) -> Dict[str, float]:
    """The reference's tiled multi-frame KITTI protocol (evaluate_mf.py:985-1053): the clip of validate_kitti_mf, replicate-padded
    at the bottom to 432 rows, cut into 432 x 960 crops (the grid follows the frame width: KITTI has 1242, 1241, 1238, 1226 and
    1224), blended with sigma = 0.05; scored on the last pair.  Returns {'kitti_epe', 'kitti_f1'}."""
    from .tiling import KITTI_MF_TILE, FixedHeightPadder
    if multi_root is None:
        raise ValueError("validate_kitti_mf_tile: multi_root (the multi-frame KITTI-2015 tree) is required")
    dev = device or model_device(model, torch.device("cpu"))
    image_root, flow_root, seqs = kitti_mf_sequences(multi_root, "training")

    def pairs():
        for seq in seqs:
            images = read_clip(kitti_mf_clip(image_root, seq, nframes), dev)
            padder = FixedHeightPadder(images[0].shape, KITTI_MF_TILE[0], mode="replicate")
            flows = _tiled_flows(model, padder.pad_list(images), padder, KITTI_MF_TILE, iters, dev)
            gt, valid = _kitti_gt(os.path.join(flow_root, seq + "_10.png"))
            yield flows[nframes - 2].cpu(), gt, valid                      # only the last pair (frames 10 -> 11) has ground truth

    epe, f1 = _kitti_scores(pairs())
    return {"kitti_epe": epe, "kitti_f1": f1}


@torch.no_grad()
def validate_kitti_tile(model: Callable, iters: int = 6, root: Optional[str] = None,
                        device: Optional[torch.device] = None) -> Dict[str, float]:
    """The reference's tiled two-frame KITTI protocol (evaluate_mf.py:919-982) over ``root/training/image_2/*_10.png``,
    ``*_11.png`` and ``flow_occ/*_10.png`` (core/datasets.py:229-245): zero-padded at the bottom to 376 rows, 376 x 720 crops,
    sigma = 0.05.  As in the reference, the model is called WITHOUT `iters` (its own default applies; `iters` is accepted and
    ignored) and needs T = 2.  Returns {'kitti-epe', 'kitti-f1'} (the reference's hyphenated keys)."""
    from .tiling import KITTI_TILE, FixedHeightPadder
    if root is None:
        raise ValueError("validate_kitti_tile: root (the KITTI-2015 tree) is required")
    dev = device or model_device(model, torch.device("cpu"))
    images1 = sorted(glob.glob(os.path.join(root, "training", "image_2", "*_10.png")))
    images2 = sorted(glob.glob(os.path.join(root, "training", "image_2", "*_11.png")))
    flows_gt = sorted(glob.glob(os.path.join(root, "training", "flow_occ", "*_10.png")))
    if not flows_gt or len(images1) != len(flows_gt) or len(images2) != len(flows_gt):
        raise RuntimeError(f"{root}: {len(images1)} / {len(images2)} frame pairs for {len(flows_gt)} ground-truth files")

    def pairs():
        for im1, im2, fl in zip(images1, images2, flows_gt):
            images = read_clip((im1, im2), dev)
            padder = FixedHeightPadder(images[0].shape, KITTI_TILE[0], mode="zeros")
            flows = _tiled_flows(model, padder.pad(*images), padder, KITTI_TILE, None, dev)
            gt, valid = _kitti_gt(fl)
            yield flows[-1].cpu(), gt, valid

    epe, f1 = _kitti_scores(pairs())
    return {"kitti-epe": epe, "kitti-f1": f1}


# ---- command line (the reference's evaluate_mf.py --dataset switch) -----------------------------------------------------------
def load_model(ckpt: str, T: int = 4, preset: Optional[str] = None, device: Optional[torch.device] = None,
               corr: Optional[str] = None):
    """SKFlow_MF8 for clips of T frames with the checkpoint loaded strictly, as StreamFlowT4 loads it ({'model': state_dict} or a
    bare dict, keys optionally prefixed 'module.'), on `device` (default: the current GPU) in eval mode."""
    from .model import SKFlow_MF8, default_args
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("evaluate: the model runs on the GPU; there is no CPU fallback")
        device = torch.device("cuda", torch.cuda.current_device())
    obj = torch.load(ckpt, map_location="cpu")
    sd = obj["model"] if isinstance(obj, dict) and "model" in obj else obj
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    model = SKFlow_MF8(default_args(T=T, preset=preset, corr=corr))
    model.load_state_dict(sd, strict=True)
    for p in model.parameters():
        p.requires_grad = False
    return model.to(device).eval()


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m streamflow_amd.evaluate",
                                 description="Validate a StreamFlow checkpoint on a dataset tree (the reference's evaluate_mf.py)")
    ap.add_argument("--dataset", required=True, choices=("sintel", "sintel_occ", "kitti", "kitti_tile", "spring"))
    ap.add_argument("--ckpt", required=True, help="StreamFlow checkpoint")
    ap.add_argument("--root", required=True, help="dataset tree (Sintel, multi-frame KITTI-2015 or Spring layout)")
    ap.add_argument("--T", type=int, default=4, help="frames per clip")
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--clips-per-step", type=int, default=8,
                    help="clips per model call (sintel, sintel_occ, kitti; 1 = the reference's per-clip loop scored on the host)")
    ap.add_argument("--png-decode", default="gpu", choices=("gpu", "host"),
                    help="where PNG rows are unfiltered when clips-per-step > 1 (the same bytes either way; 1 always decodes on the host)")
    ap.add_argument("--flo5-decode", default="gpu", choices=("gpu", "host"),
                    help="where Spring's .flo5 ground truth is inflated and put together (--dataset spring; the same bits either way)")
    ap.add_argument("--preset", default=None, help="arithmetic preset (streamflow_amd.presets); default: fp32_class")
    ap.add_argument("--corr", default=None, choices=("volume", "direct"),
                    help="correlation route: the all-pairs volume (default) or on-demand lookups from features (no N x N buffer)")
    a = ap.parse_args(argv)
    png_decode = a.png_decode if a.clips_per_step > 1 else "host"
    model = load_model(a.ckpt, T=a.T, preset=a.preset, corr=a.corr)
    if a.dataset == "sintel":
        res = validate_sintel_mf(model, iters=a.iters, root=a.root, nframes=a.T, clips_per_step=a.clips_per_step, png_decode=png_decode)
    elif a.dataset == "sintel_occ":
        res = validate_sintel_occ_mf(model, iters=a.iters, root=a.root, nframes=a.T, clips_per_step=a.clips_per_step,
                                     png_decode=png_decode)
    elif a.dataset == "kitti":
        res = validate_kitti_mf(model, iters=a.iters, multi_root=a.root, nframes=a.T, clips_per_step=a.clips_per_step, png_decode=png_decode)
    elif a.dataset == "kitti_tile":
        res = validate_kitti_mf_tile(model, iters=a.iters, multi_root=a.root, nframes=a.T)
    else:
        res = {"spring": validate_spring_mf(model, iters=a.iters, root=a.root, nframes=a.T, flo5_decode=a.flo5_decode)}
    print(" ".join("%s: %f" % (k, v) for k, v in res.items()))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
