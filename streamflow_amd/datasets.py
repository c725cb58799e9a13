"""What the dataset loops of evaluate.py and submit.py share: the PNG frame reader, the per-clip model call, the
walks over the Sintel, multi-frame KITTI-2015 and Spring trees, and two model helpers.  Host only: nothing here launches a kernel.

The clip schedule is video.py's closed form (`clip_count`, `clip_start`); `sintel_clip_schedule` is its view with the reference's
frame ids.  ``model`` is the reference's test-mode call, see evaluate.py.
"""
from __future__ import annotations

import glob
import os
from typing import Callable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import flow_io
from .utils import InputPadder


# ---- model helpers ------------------------------------------------------------------------------------------------------------
def model_device(model, default: Optional[torch.device] = None) -> Optional[torch.device]:
    """The device of the model's first parameter; `default` for a model without parameters (a function, a stub)."""
    try:
        return next(model.parameters()).device
    except (AttributeError, StopIteration, TypeError):
        return default


def batched_call(model: Callable, iters: Optional[int]) -> Callable:
    """clips fp32 [k, T, 3, Hp, Wp] in [-1, 1] -> T - 1 flows [k, 2, Hp, Wp]: `model.forward_normalised(clips, iters)` when the
    model has one (SKFlow_MF8, StreamFlowT4), else `model(clips)`."""
    return (lambda x: model.forward_normalised(x, iters)) if hasattr(model, "forward_normalised") else model


# ---- frames and clips ---------------------------------------------------------------------------------------------------------
def read_frame(path: str) -> np.ndarray:
    """A PNG frame as uint8 [H, W, 3]: grey (with or without alpha) replicated to three channels, alpha dropped."""
    img = flow_io.read_png(path)
    if img.ndim == 2 or img.shape[2] == 2:
        img = np.repeat((img if img.ndim == 2 else img[:, :, 0])[:, :, None], 3, axis=2)
    return np.ascontiguousarray(img[:, :, :3]).astype(np.uint8)


def frame_tensor(path: str) -> torch.Tensor:
    """read_frame as float [3, H, W] in 0..255, what the reference's test-mode call takes."""
    return torch.from_numpy(read_frame(path)).permute(2, 0, 1).float()


def read_clip(paths: Sequence[str], dev: torch.device) -> List[torch.Tensor]:
    return [frame_tensor(p)[None].to(dev) for p in paths]


def padded_flows(model: Callable, images: List[torch.Tensor], iters: int, mode: str = "sintel") -> List[torch.Tensor]:
    """pad -> model in test mode -> unpad: the clip's flows [2, H, W], on the model's device and in the model's dtype."""
    padder = InputPadder(images[0].shape, mode=mode)
    return [padder.unpad(f[0]) for f in model(padder.pad_list(images), iters=iters, test_mode=True)]


def run_clip(model: Callable, paths: Sequence[str], dev: torch.device, iters: int, mode: str = "sintel") -> List[torch.Tensor]:
    """The flows [2, H, W] of one clip of frame files, every clip from a cold start."""
    return padded_flows(model, read_clip(paths, dev), iters, mode)


def sintel_clip_schedule(n_images: int, nframes: int) -> List[Tuple[int, List[int]]]:
    """[(first frame, frame ids)] of one scene (core/mf_datasets.py:1125-1149): the clips of video.clip_count / clip_start; a
    frame of the tail clip whose outgoing pair an earlier clip has produced gets id -1 (the reference's flag)."""
    from .video import clip_count, clip_start
    T = int(nframes)
    if n_images < T or T < 2:
        raise ValueError(f"a scene needs at least nframes = {T} >= 2 images, got {n_images}")
    firsts = [clip_start(c, n_images, T) for c in range(clip_count(n_images, T))]
    return [(first, [j if j >= c * (T - 1) else -1 for j in range(first, first + T)]) for c, first in enumerate(firsts)]


# ---- dataset trees ------------------------------------------------------------------------------------------------------------
def scenes(root: str) -> List[str]:
    return sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))


def sintel_scenes(root: str, split: str, dstype: str, flow: bool = False, occ: bool = False) -> Iterator[tuple]:
    """(scene, frames, .flo files, occlusion maps) of ``root/<split>/<dstype>/<scene>/*.png``, sorted; `flow` / `occ` ask for
    ``root/<split>/flow/<scene>/*.flo`` / ``occlusions/<scene>/*.png`` (else None) and check that there is one per pair."""
    image_root = os.path.join(root, split, dstype)
    occ_root = os.path.join(root, split, "occlusions")
    for scene in scenes(image_root):
        imgs = sorted(glob.glob(os.path.join(image_root, scene, "*.png")))
        flos = occs = None
        if flow:
            flos = sorted(glob.glob(os.path.join(root, split, "flow", scene, "*.flo")))
            if len(flos) != len(imgs) - 1:
                raise RuntimeError(f"{scene}: {len(imgs)} frames need {len(imgs) - 1} .flo files, found {len(flos)}")
        if occ:
            occs = sorted(glob.glob(os.path.join(occ_root, scene, "*.png")))
            if len(occs) != len(flos):
                raise RuntimeError(f"{scene}: {len(flos)} .flo files need as many occlusion maps under {occ_root}, found {len(occs)}")
        yield scene, imgs, flos, occs


def kitti_mf_sequences(multi_root: str, split: str) -> Tuple[str, str, List[str]]:
    """(image_2 directory, flow_occ directory, sequence names 000NNN) of the multi-frame KITTI-2015 tree: 'training' lists the
    sequences with ground truth, 'testing' those with a frame 10 (the reference walks 000000 .. 000199)."""
    image_root = os.path.join(multi_root, split, "image_2")
    flow_root = os.path.join(multi_root, split, "flow_occ")
    listed = flow_root if split == "training" else image_root
    seqs = sorted(os.path.basename(p)[:6] for p in glob.glob(os.path.join(listed, "??????_10.png")))
    if not seqs:
        raise RuntimeError(f"no ground truth under {flow_root}" if split == "training" else f"no sequences under {image_root}")
    return image_root, flow_root, seqs


def kitti_mf_clip(image_root: str, seq: str, nframes: int) -> List[str]:
    """The clip of a sequence: frames 12 - nframes .. 11 (core/mf_datasets.py:946-952); its last pair is 10 -> 11."""
    return [os.path.join(image_root, "%s_%02d.png" % (seq, i)) for i in range(12 - nframes, 12)]


def spring_clips(root: str, split: str, nframes: int, only: Optional[Sequence[str]] = None) -> Iterator[tuple]:
    """(scene, camera, direction, frames in clip order, n, clip schedule) over ``root/<split>/<scene>/frame_{left,right}/*.png``:
    per scene (sorted; `only`: these scenes), per camera, the forward list and then the same frames reversed."""
    for scene in [s for s in scenes(os.path.join(root, split)) if only is None or s in only]:
        for cam in ("left", "right"):
            frames = sorted(glob.glob(os.path.join(root, split, scene, f"frame_{cam}", "*.png")))
            for direction, order in (("FW", frames), ("BW", frames[::-1])):
                yield scene, cam, direction, order, len(frames), sintel_clip_schedule(len(frames), nframes)


def spring_flow_file(direction: str, cam: str, n: int, index: int) -> str:
    """``flow_<FW|BW>_<cam>/flow_<FW|BW>_<cam>_NNNN.flo5`` of the pair that starts at `index` of the forward or reversed list of
    n frames: number index + 1 forward, n - index backward (mf_datasets.py:126-127, :148-149)."""
    number = index + 1 if direction == "FW" else n - index
    return os.path.join(f"flow_{direction}_{cam}", f"flow_{direction}_{cam}_{number:04d}.flo5")
