"""The video path restated in torch, step by step as the reference's read_video_and_group_predict does it (demo.py:501-534), for the
tests of streamflow_amd.video / ops.frames_to_clips / ops.clips_to_flows to compare against BITWISE:

* byte values -> `2 * (x.float() / 255.0) - 1.0` on the frames' device (demo.py:510; the model's own line, streamflow.py:100);
* -> `F.pad(..., mode="replicate")` by InputPadder's amounts (demo.py:511-512, utils.py:7-23);
* -> clips stacked by `demo.group_clips` (the window / flag loop of demo.py:517-532);
* -> after the model, `unpad` and the keep flags (demo.py:527-528).

This is the project's own code: nothing here is taken from the reference's text."""
import numpy as np
import torch
import torch.nn.functional as F

from streamflow_amd.demo import group_clips
from streamflow_amd.utils import InputPadder


def random_frames(seed: int, n: int, h: int, w: int) -> torch.Tensor:
    """uint8 [n, h, w, 3] on the host: noise with every byte value present, the four corners of every frame distinct (so that a wrong
    replicate clamp shows) and frame k tagged with k in its first pixel (so that a wrong frame shows)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    a[:, 0, 0], a[:, 0, -1], a[:, -1, 0], a[:, -1, -1] = 11, 77, 143, 209
    a[:, 0, 0, 0] = np.arange(n) % 256
    return torch.from_numpy(a)


def normalise(x_u8: torch.Tensor) -> torch.Tensor:
    return 2 * (x_u8.float() / 255.0) - 1.0


def padded_frames(frames_hwc: torch.Tensor, mode: str):
    """uint8 [n, H, W, 3] (any device) -> (fp32 [n, 3, Hp, Wp] normalised and replicate-padded on that device, the padder)."""
    x = normalise(frames_hwc.permute(0, 3, 1, 2).contiguous())
    padder = InputPadder(x.shape, mode=mode)
    return F.pad(x, padder._pad, mode="replicate"), padder


def clips(frames_hwc: torch.Tensor, T: int, mode: str) -> torch.Tensor:
    """All clips of the video: fp32 [nc, T, 3, Hp, Wp]."""
    x, _ = padded_frames(frames_hwc, mode)
    return torch.stack([x[s:s + T] for s, _ in group_clips(frames_hwc.shape[0], T)])


def kept(outs, first_clip: int, n: int, T: int, padder) -> list:
    """The kept, unpadded fields [2, H, W] of a batch's per-pair outputs (T - 1 tensors [B, 2, Hp, Wp]), in video order."""
    sched = group_clips(n, T)
    B = outs[0].shape[0]
    return [padder.unpad(outs[k][b]) for b in range(B) for k in range(T - 1) if sched[first_clip + b][1][k]]


def flows(call, frames_hwc: torch.Tensor, T: int, mode: str, clips_per_step: int) -> torch.Tensor:
    """[n - 1, 2, H, W]: `call(imgs[B, T, 3, Hp, Wp]) -> T - 1 x [B, 2, Hp, Wp]` over the clips in batches of `clips_per_step`."""
    n = frames_hwc.shape[0]
    all_clips = clips(frames_hwc, T, mode)
    _, padder = padded_frames(frames_hwc[:1], mode)
    fields = []
    for first in range(0, all_clips.shape[0], clips_per_step):
        outs = call(all_clips[first:first + clips_per_step].contiguous())
        fields += kept(outs, first, n, T, padder)
    return torch.stack(fields)


def stub_model(imgs: torch.Tensor) -> list:
    """A fixed function of the clip batch with the model's output shapes: pair k = (frame k + 1 - frame k) of the first two colour
    planes, so every output pixel names its clip, pair, plane and position."""
    return [(imgs[:, k + 1, :2] - imgs[:, k, :2]).contiguous() for k in range(imgs.shape[1] - 1)]
