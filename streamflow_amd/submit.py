"""Leaderboard writers with the reference's signatures and file names (SURVEY.md row f3's last step).

* ``create_sintel_submission_mf(args, model, iters, output_path, nframes)`` -- reference evaluate_mf.py:252-282 over
  ``args.sintel_root/test/{clean,final}/<scene>/*.png``: the clip schedule of ``datasets.sintel_clip_schedule``, pad -> model ->
  unpad (``datasets.run_clip``), and for every pair whose frame id is not -1 the flow as
  ``output_path/<dstype>/<scene>/frame%04d.flo`` (id + 1) and its colour-wheel image as ``output_path/<dstype>/<scene>-<id + 1>.png``.
* ``create_sintel_submission_mf_warmup`` -- evaluate_mf.py:286-323: the same, every clip warm-started from the previous clip's
  low-resolution flows (``demo.predict_clips_warm_start``, one chain per scene).
* ``create_kitti_submission_mf(args, model, iters, output_path, nframes, vis_path)`` -- submit_mf.py:700-728 over
  ``args.multi_root/testing/image_2/000NNN_FF.png``, frames 12 - nframes .. 11, the padder in its default ('sintel') mode as the
  reference has it there, the LAST flow as the 16-bit PNG ``output_path/000NNN_10.png``; the colour image goes to
  ``vis_path/flow/000NNN_10.png`` when `vis_path` is given (the reference always writes ``vis_kitti2/`` into the working directory).
* ``create_spring_submission_mf(args, model, iters, output_path, nframes)`` -- evaluate_mf.py:25-48 over
  ``args.spring_root/test/<scene>/frame_{left,right}/*.png``: forward and backward clips of every scene and camera, each flow as
  ``output_path/<scene>/flow_<FW|BW>_<cam>/flow_<FW|BW>_<cam>_%04d.flo5`` (flo5.write_flo5, gzip level 5; ``flo5_encode="gpu"``:
  flo5_gpu.write_batch, compressed on the device); no colour images.

``model`` is the reference's test-mode call (see evaluate.py); the tree walks, the frame reader and the per-clip model call are
datasets.py's, shared with evaluate.py.  The colour images of one clip are made on the device by ONE
``ops.flow_to_image`` call before the flows are copied to the host; ``vis=False`` launches no kernel, which lets the writers run
with a CPU model.
"""
from __future__ import annotations

import os
from typing import Callable, List, Optional

import torch

from . import flow_io
from .datasets import (kitti_mf_clip, kitti_mf_sequences, model_device, read_clip, run_clip, sintel_clip_schedule, sintel_scenes,
                       spring_clips, spring_flow_file)
from .utils import InputPadder


def _eval_mode(model) -> None:
    if hasattr(model, "eval"):
        model.eval()


def _colour(flows: List[torch.Tensor], keep: List[int]) -> dict:
    """{pair index: uint8 [H, W, 3]} of the kept pairs of one clip: one kernel call on the device flows."""
    from . import ops
    if not keep:
        return {}
    imgs = ops.flow_to_image(torch.stack([flows[i].float() for i in keep]).contiguous()).cpu().numpy()
    return {i: imgs[k] for k, i in enumerate(keep)}


def _write_sintel_clip(flows: List[torch.Tensor], ids: List[int], output_path: str, dstype: str, scene: str, vis: bool,
                       png_encode: str = "host") -> None:
    """flows: nframes - 1 unpadded fields [2, H, W]; ids: the clip's frame ids (-1: pair already written by an earlier clip).
    png_encode="gpu": the colour images are encoded on the device (png_gpu.encode_batch: the same pixels, other file bytes)."""
    assert len(flows) == len(ids) - 1
    if png_encode not in ("host", "gpu"):
        raise ValueError(f"png_encode must be 'host' or 'gpu', got {png_encode!r}")
    output_dir = os.path.join(output_path, dstype, scene)
    os.makedirs(output_dir, exist_ok=True)
    keep = [i for i in range(len(flows)) if ids[i] != -1]
    pngs = {i: os.path.join(output_path, dstype, "%s-%d.png" % (scene, ids[i] + 1)) for i in keep}
    if vis and keep and png_encode == "gpu":
        from . import ops, png_gpu
        png_gpu.encode_batch(ops.flow_to_image(torch.stack([flows[i].float() for i in keep]).contiguous()), [pngs[i] for i in keep])
    images = _colour(flows, keep) if vis and png_encode == "host" else {}
    for i in keep:
        flow_io.write_flo(os.path.join(output_dir, "frame%04d.flo" % (ids[i] + 1)), flows[i].permute(1, 2, 0).float().cpu().numpy())
        if i in images:
            flow_io.write_png(pngs[i], images[i])


@torch.no_grad()
def create_sintel_submission_mf(args, model: Callable, iters: int, output_path: str = "sintel_submission", nframes: int = 3,
                                vis: bool = True, device: Optional[torch.device] = None, png_encode: str = "host") -> None:
    """Create the submission tree for the Sintel leaderboard (every clip from a cold start).  png_encode: see _write_sintel_clip."""
    _eval_mode(model)
    dev = device or model_device(model, torch.device("cpu"))
    for dstype in ("clean", "final"):
        for scene, imgs, _, _ in sintel_scenes(args.sintel_root, "test", dstype):
            for first, ids in sintel_clip_schedule(len(imgs), nframes):
                _write_sintel_clip(run_clip(model, imgs[first:first + nframes], dev, iters), ids, output_path, dstype, scene, vis,
                                   png_encode)


@torch.no_grad()
def create_sintel_submission_mf_warmup(args, model: Callable, iters: int, output_path: str = "sintel_submission",
                                       nframes: int = 3, vis: bool = True, device: Optional[torch.device] = None,
                                       png_encode: str = "host") -> None:
    """Create the submission tree for the Sintel leaderboard with the warm-start chain: inside a scene every clip starts from the
    previous clip's low-resolution flows pushed forward along themselves; the chain restarts with every scene (the reference's
    `flow_prev = None`, which `demo.predict_clips_warm_start` spells as zero flows so that the model also returns the
    low-resolution fields).  Clips are read one at a time; the files of a scene are written when its chain is done."""
    from .demo import predict_clips_warm_start
    _eval_mode(model)
    dev = device or model_device(model, torch.device("cpu"))
    for dstype in ("clean", "final"):
        for scene, imgs, _, _ in sintel_scenes(args.sintel_root, "test", dstype):
            schedule = sintel_clip_schedule(len(imgs), nframes)
            padder = InputPadder(flow_io.read_png(imgs[0]).shape[:2])

            def clips():
                for first, _ in schedule:
                    yield padder.pad_list(read_clip(imgs[first:first + nframes], dev))

            for (_, ids), flows in zip(schedule, predict_clips_warm_start(model, clips(), iters=iters)):
                _write_sintel_clip([padder.unpad(f[0]) for f in flows], ids, output_path, dstype, scene, vis, png_encode)


@torch.no_grad()
def create_spring_submission_mf(args, model: Callable, iters: int, output_path: str = "sintel_submission", nframes: int = 4,
                                device: Optional[torch.device] = None, flo5_encode: str = "host") -> None:
    """Create the submission tree for the Spring leaderboard (evaluate_mf.py:25-48 over SpringSubmission, mf_datasets.py:47-97):
    every scene of ``args.spring_root/test`` (sorted), both cameras, the forward clips and then the backward clips (the frames
    reversed), every clip from a cold start on sintel_clip_schedule.  Each pair whose frame id is not -1 is written with
    flo5.write_flo5 (gzip level 5, the reference's) as ``output_path/<scene>/flow_<FW|BW>_<cam>/flow_<FW|BW>_<cam>_%04d.flo5`` with
    the 1-based id j + 1 forward and n - j backward (j: the source frame's index in the forward or reversed list).  As in the
    reference there are no colour images, and the default output_path is the reference's 'sintel_submission'.
    flo5_encode="gpu": the kept pairs of a clip are compressed on the device and written by ONE flo5_gpu.write_batch call (the same
    dataset bit for bit; another filter pipeline, shuffle + Huffman-only deflate, which h5py undoes on reading)."""
    from . import flo5
    if flo5_encode not in ("host", "gpu"):
        raise ValueError(f"flo5_encode must be 'host' or 'gpu', got {flo5_encode!r}")
    _eval_mode(model)
    dev = device or model_device(model, torch.device("cpu"))
    for scene, cam, direction, order, n, schedule in spring_clips(args.spring_root, "test", nframes):
        os.makedirs(os.path.join(output_path, scene, f"flow_{direction}_{cam}"), exist_ok=True)
        for first, ids in schedule:
            flows = run_clip(model, order[first:first + nframes], dev, iters)
            assert len(flows) == len(ids) - 1
            if flo5_encode == "gpu":
                from . import flo5_gpu
                keep = [k for k, j in enumerate(ids[:-1]) if j != -1]
                if keep:                                    # one field: the unpadded view itself; more: one batch tensor
                    fields = [flows[k].float() for k in keep]
                    flo5_gpu.write_batch(fields[0][None] if len(fields) == 1 else torch.stack(fields),
                                         [os.path.join(output_path, scene, spring_flow_file(direction, cam, n, ids[k])) for k in keep])
                continue
            for k, j in enumerate(ids[:-1]):
                if j != -1:
                    flo5.write_flo5(os.path.join(output_path, scene, spring_flow_file(direction, cam, n, j)),
                                    flows[k].permute(1, 2, 0).float().cpu().numpy(), compression_level=5)


@torch.no_grad()
def create_kitti_submission_mf(args, model: Callable, iters: int, output_path: str = "kitti_submission", nframes: int = 3,
                               vis_path: Optional[str] = None, device: Optional[torch.device] = None, png_encode: str = "host") -> None:
    """Create the submission folder for the KITTI-2015 leaderboard from the multi-frame test split: one 16-bit PNG per sequence
    (the flow of frames 10 -> 11).  Sequences are those present under ``testing/image_2`` (the reference walks 000000 .. 000199).
    png_encode="gpu": the codes come from ops.flow_to_kitti16 and both files from png_gpu.encode_batch (the same pixels as the host
    writers', other file bytes)."""
    if png_encode not in ("host", "gpu"):
        raise ValueError(f"png_encode must be 'host' or 'gpu', got {png_encode!r}")
    _eval_mode(model)
    dev = device or model_device(model, torch.device("cpu"))
    image_root, _, seqs = kitti_mf_sequences(args.multi_root, "testing")
    os.makedirs(output_path, exist_ok=True)
    if vis_path is not None:
        os.makedirs(os.path.join(vis_path, "flow"), exist_ok=True)
    for seq in seqs:
        flow = run_clip(model, kitti_mf_clip(image_root, seq, nframes), dev, iters)[-1]       # default mode, not 'kitti': submit_mf.py:711
        frame_name = seq + "_10.png"
        if png_encode == "gpu":
            from . import ops, png_gpu
            field = flow.float()[None].contiguous()
            png_gpu.encode_batch(ops.flow_to_kitti16(field), [os.path.join(output_path, frame_name)])
            if vis_path is not None:
                png_gpu.encode_batch(ops.flow_to_image(field), [os.path.join(vis_path, "flow", frame_name)])
            continue
        image = _colour([flow], [0])[0] if vis_path is not None else None
        flow_io.write_flow_kitti(os.path.join(output_path, frame_name), flow.permute(1, 2, 0).float().cpu().numpy())
        if image is not None:
            flow_io.write_png(os.path.join(vis_path, "flow", frame_name), image)
