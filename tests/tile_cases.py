"""Seeded cases of the tiled-inference fixture (tests/golden/make_tile_golden.py -> tile_kitti.npz), shared by the generator and
the tests so that both see identical inputs: crop grids, weight patches, the fixed-height padders and a two-sequence synthetic
multi-frame KITTI tree scored by a stub model."""
import os

import numpy as np
import torch

KITTI_WIDTHS = (1242, 1241, 1238, 1226, 1224)
# (image H, W, tile h, w, min_overlap)
GRID_CASES = ([(432, w, 432, 960, 20) for w in KITTI_WIDTHS] + [(376, w, 376, 720, 20) for w in KITTI_WIDTHS]
              + [(64, 96, 48, 64, 20), (100, 130, 40, 56, 8),           # the reference's grid puts a crop past the edge here
                 (48, 64, 48, 64, 20), (75, 203, 24, 40, 5), (96, 160, 64, 96, 16), (120, 200, 64, 96, 20),
                 (64, 176, 64, 96, 20)])                                   # (the last: every crop twice, as at the KITTI shapes)
WEIGHT_FULL = ((48, 64, 0.05), (40, 56, 0.3))                  # tile h, w, sigma: whole patch recorded
WEIGHT_SAMPLED = ((432, 960, 0.05), (376, 720, 0.05))          # sampled pixels, the four corners among them
PAD_CASES = [("kitti432", h, w) for h, w in ((375, 1242), (370, 1224), (432, 1241))] + \
            [("kitti376", h, w) for h, w in ((375, 1242), (374, 1238), (376, 1226))]
# the synthetic multi-frame sequences: (H, W); two widths so that the grid is recomputed between them
SEQ_SHAPES = ((375, 1242), (370, 1224))
SEQ_SEED, NFRAMES, ITERS = 2015, 3, 4


def sampled_pixels(th, tw, seed=5, n=60):
    rng = np.random.default_rng(seed)
    ys = np.concatenate([[0, 0, th - 1, th - 1, th // 2], rng.integers(0, th, n)])
    xs = np.concatenate([[0, tw - 1, 0, tw - 1, tw // 2], rng.integers(0, tw, n)])
    return ys.astype(np.int64), xs.astype(np.int64)


def sequence(s):
    """Frames (nframes x uint8 [H, W, 3]), ground truth of the last pair quantised to 1/64 px (float32 [H, W, 2], exact through
    the KITTI 16-bit PNG codec) and its validity (float32 [H, W] of 0 / 1) of synthetic sequence s."""
    H, W = SEQ_SHAPES[s]
    rng = np.random.default_rng(SEQ_SEED + s)
    frames = [rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in range(NFRAMES)]
    gt = (np.round(rng.normal(0, 6, size=(H, W, 2)) * 64) / 64).astype(np.float32)
    valid = (rng.random((H, W)) < 0.5).astype(np.float32)
    return frames, gt, valid


def write_kitti_mf_tree(root):
    """multi_root/training/image_2/000NNN_FF.png (frames 12 - nframes .. 11) + flow_occ/000NNN_10.png of the sequences above."""
    from streamflow_amd import flow_io
    os.makedirs(os.path.join(root, "training", "image_2"), exist_ok=True)
    os.makedirs(os.path.join(root, "training", "flow_occ"), exist_ok=True)
    for s in range(len(SEQ_SHAPES)):
        frames, gt, valid = sequence(s)
        for i, img in zip(range(12 - NFRAMES, 12), frames):
            flow_io.write_png(os.path.join(root, "training", "image_2", "%06d_%02d.png" % (s, i)), img)
        enc = flow_io.kitti_encode(gt)
        enc[..., 2] = valid.astype(np.uint16)
        flow_io.write_png(os.path.join(root, "training", "flow_occ", "%06d_10.png" % s), enc)


class StubModel:
    """Test-mode call of the reference (list of T frames [1,3,h,w] in 0..255 -> T-1 flows [1,2,h,w]) whose flow depends on the
    position inside the crop (a ramp) and on the frames, so that the blend of overlapping crops is visible in the scores.  Only
    + - * by powers of two: the same bits on the CPU and on the GPU."""

    def eval(self):
        return self

    def __call__(self, images, iters=12, test_mode=True):
        _, _, h, w = images[0].shape
        dev = images[0].device
        xs = torch.arange(w, dtype=torch.float32, device=dev).view(1, 1, 1, w)
        ys = torch.arange(h, dtype=torch.float32, device=dev).view(1, 1, h, 1)
        ramp = torch.cat([(xs - 0.5 * w) * 0.015625 + ys * 0.0, (ys - 0.5 * h) * 0.0078125 + xs * 0.0], dim=1)
        out = []
        for j in range(len(images) - 1):
            a, b = images[j].float(), images[j + 1].float()
            out.append(ramp + (b[:, :2] - a[:, 1:]) * 0.03125 + float(iters) * 0.25)
        return out
