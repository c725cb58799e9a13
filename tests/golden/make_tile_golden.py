#!/usr/bin/env python3
"""Generate tile_kitti.npz by EXECUTING THE REFERENCE's own tiled-evaluation helpers on the CPU.

Run in the build container only (needs /root/reference; the GPU box never sees it):

    python tests/golden/make_tile_golden.py

It imports the reference's ``evaluate_mf.py`` through in-memory stand-ins that are this repo's own code (nothing from the
reference is copied into the repo): empty modules for what that file imports but the tile helpers never use (``h5py``,
``datasets``, ``models``, ``imageio``, ``matplotlib``, ``utils.flow_viz``), a ``cv2`` with the two calls ``frame_utils`` makes
at import time, and an ``mf_datasets`` whose ``KITTIMultiFrameEval`` serves the synthetic sequences of tests/tile_cases.py.
``torch.Tensor.cuda`` is the identity, so the reference's blend runs in fp32 on the CPU.

Recorded: ``compute_grid_indices`` at every case of tile_cases.GRID_CASES (duplicates and order included), weight patches of
``compute_weight`` (whole small patches; sampled pixels of the KITTI crops, the corners among them), the ``_pad`` of
``InputPadder2`` in the 'kitti432' / 'kitti376' modes, and the ``kitti_epe`` / ``kitti_f1`` that the reference's own
``validate_kitti_mf_tile`` returns for tile_cases.StubModel on the synthetic sequences.  Inputs are rebuilt from seeds.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = "/root/reference"

from tests import tile_cases as tc  # noqa: E402


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _KITTIMultiFrameEval:
    """mf_datasets.KITTIMultiFrameEval over the synthetic sequences: (frames [3,H,W] float, flows, valids, name) with ground
    truth on the last pair only (core/mf_datasets.py:945-1017)."""

    def __init__(self, split="training", multi_root=None, nframes=3, aug_params=None):
        assert nframes == tc.NFRAMES
        self.nframes = nframes

    def __len__(self):
        return len(tc.SEQ_SHAPES)

    def __getitem__(self, i):
        frames, gt, valid = tc.sequence(i)
        imgs = [torch.from_numpy(f).permute(2, 0, 1).float() for f in frames]
        flows = [None] * (self.nframes - 2) + [torch.from_numpy(gt).permute(2, 0, 1).float()]
        valids = [None] * (self.nframes - 2) + [torch.from_numpy(valid)]
        return imgs, flows, valids, "%06d_10.png" % i


def load_reference():
    cv2 = _module("cv2", setNumThreads=lambda n: None)
    cv2.ocl = types.SimpleNamespace(setUseOpenCL=lambda flag: None)
    for name in ("h5py", "datasets", "models", "imageio", "matplotlib", "matplotlib.pyplot"):
        _module(name)
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    _module("mf_datasets", KITTIMultiFrameEval=_KITTIMultiFrameEval)
    sys.path.insert(0, os.path.join(REF, "core"))
    import utils  # noqa: F401  (the reference's core/utils package)
    _module("utils.flow_viz")
    torch.Tensor.cuda = lambda self, *a, **k: self
    spec = importlib.util.spec_from_file_location("ref_evaluate_mf", os.path.join(REF, "evaluate_mf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    out = {}
    for i, (H, W, th, tw, mo) in enumerate(tc.GRID_CASES):
        out[f"grid{i}"] = np.array(ref.compute_grid_indices([H, W], [th, tw], mo), np.int32).reshape(-1, 2)
    for i, (th, tw, sigma) in enumerate(tc.WEIGHT_FULL):
        w = ref.compute_weight([(0, 0)], [th, tw], [th, tw], sigma)[0]
        out[f"wfull{i}"] = w.reshape(th, tw).numpy()
    for i, (th, tw, sigma) in enumerate(tc.WEIGHT_SAMPLED):
        w = ref.compute_weight([(0, 0)], [th, tw], [th, tw], sigma)[0].reshape(th, tw).numpy()
        ys, xs = tc.sampled_pixels(th, tw)
        out[f"wsamp{i}"] = w[ys, xs]
        assert out[f"wsamp{i}"][:4].max() < np.finfo(np.float32).tiny          # the corners are subnormal
    for i, (mode, h, w) in enumerate(tc.PAD_CASES):
        out[f"pad{i}"] = np.array(ref.InputPadder2((3, h, w), mode=mode)._pad, np.int32)
    res = ref.validate_kitti_mf_tile(tc.StubModel(), iters=tc.ITERS, multi_root="(synthetic)", nframes=tc.NFRAMES)
    out["kitti_epe"] = np.float64(res["kitti_epe"])
    out["kitti_f1"] = np.float64(res["kitti_f1"])
    path = os.path.join(HERE, "tile_kitti.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote tile_kitti.npz  {os.path.getsize(path) / 1024:.0f} KiB  (kitti_epe {res['kitti_epe']:.6f}, "
          f"kitti_f1 {res['kitti_f1']:.6f})")


if __name__ == "__main__":
    main()
