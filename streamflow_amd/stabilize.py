"""Video stabilisation from the flows of a video: a camera motion per frame pair, a smoothed camera path, frames re-rendered on the GPU.

Pass 1 fits a global motion to every flow field (ops.motion_fit, csrc/stabilize.hip: iteratively reweighted least squares with
Tukey's biweight, a translation, similarity or affine model; with `occlusion` the forward-backward consistency classes keep occluded
and outside pixels out of the fit) and keeps six numbers per pair.  The camera path is their running product; it is smoothed on the
host in float64 with a Gaussian over RELATIVE transforms (no drift, no dependence on the position of frame 0), or frozen to frame 0
(tripod mode).  Pass 2 reads the frames again and renders each through its inverse map (ops.warp_affine).

Limits: the scale of the reweighting is the RMS residual, not a median, so a region that moves on its own may cover about a
quarter of the frame, not much more; one global affine motion per pair, so no parallax, no rolling shutter;
bilinear sampling.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np
import torch

MAX_ZOOM = 1.25


def _mat3(m23: np.ndarray) -> np.ndarray:
    """[..., 2, 3] -> [..., 3, 3] with the row (0, 0, 1)."""
    m23 = np.asarray(m23, np.float64)
    out = np.zeros(m23.shape[:-2] + (3, 3), np.float64)
    out[..., :2, :] = m23
    out[..., 2, 2] = 1.0
    return out


def corners(hw: Sequence[int]) -> np.ndarray:
    h, w = int(hw[0]), int(hw[1])
    return np.array([[0.0, 0.0], [w - 1.0, 0.0], [0.0, h - 1.0], [w - 1.0, h - 1.0]])


def auto_zoom(inv_maps: np.ndarray, hw: Sequence[int], max_zoom: float = MAX_ZOOM) -> float:
    """The smallest zoom in [1, max_zoom] about the frame centre that keeps the four corners of every output frame inside the source
    frame [0, w - 1] x [0, h - 1]; max_zoom when none does.  A corner q of a frame zoomed by z reads the source at B (c + (q - c) / z)
    = B c + t A (q - c), t = 1 / z: every bound is linear in t, so the answer is the largest feasible t."""
    h, w = int(hw[0]), int(hw[1])
    B = np.asarray(inv_maps, np.float64).reshape(-1, 2, 3)
    c = np.array([(w - 1) * 0.5, (h - 1) * 0.5])
    base = B[:, :, :2] @ c + B[:, :, 2]                                   # [n, 2]: where the centre reads
    slope = np.einsum("nij,qj->nqi", B[:, :, :2], corners(hw) - c)       # [n, 4, 2]
    t_lo, t_hi = 1.0 / float(max_zoom), 1.0
    hi_bound = np.array([w - 1.0, h - 1.0])
    for k in range(B.shape[0]):
        for axis in range(2):
            a = base[k, axis]
            if not 0.0 <= a <= hi_bound[axis]:
                return float(max_zoom)                                   # the centre itself reads outside: no zoom helps
            for b in slope[k, :, axis]:
                if b > 0:
                    t_hi = min(t_hi, (hi_bound[axis] - a) / b)
                elif b < 0:
                    t_hi = min(t_hi, (0.0 - a) / b)
    if not t_hi >= t_lo:
        return float(max_zoom)
    return 1.0 / t_hi


def camera_path(models, sigma: Optional[float] = 15.0, zoom=1.0, hw: Optional[Sequence[int]] = None, max_zoom: float = MAX_ZOOM):
    """models [n, 2, 3] (ops.motion_fit: M_k takes a pixel of frame k to frame k + 1) -> the inverse maps of the n + 1 frames,
    float64 numpy [n + 1, 2, 3]: output pixel -> source coordinate in that frame; and the zoom used.
    C_0 = I, C_{k+1} = M_k C_k (frame 0 -> frame k).  sigma (frames): R_k = sum_j g(j - k) C_j C_k^-1 / sum_j g(j - k), g a Gaussian
    whose window (4 sigma) is cut at the video's ends and renormalised; B_k = R_k^-1.  sigma None: tripod mode, B_k = C_k (every frame
    rendered in frame 0's coordinates).  zoom: a float >= 1 about the frame centre, or "auto" (auto_zoom); both need `hw`."""
    M = _mat3(models.detach().cpu().numpy() if isinstance(models, torch.Tensor) else models)
    if M.ndim != 3:
        raise ValueError(f"camera_path: models must be [n, 2, 3], got {M.shape[:-2] + (2, 3)}")
    n = M.shape[0]
    C = np.empty((n + 1, 3, 3), np.float64)
    C[0] = np.eye(3)
    for k in range(n):
        C[k + 1] = M[k] @ C[k]
    if sigma is None:
        B = C.copy()
    else:
        if not sigma > 0:
            raise ValueError(f"camera_path: sigma must be > 0 frames (None: tripod mode), got {sigma!r}")
        Cinv = np.linalg.inv(C)
        radius = int(np.ceil(4.0 * sigma))
        B = np.empty_like(C)
        for k in range(n + 1):
            lo, hi = max(0, k - radius), min(n, k + radius)
            j = np.arange(lo, hi + 1)
            g = np.exp(-0.5 * ((j - k) / float(sigma)) ** 2)
            # (the mean of the differences from I: a video that does not move gives R = I exactly)
            R = np.eye(3) + np.einsum("j,jab->ab", g, C[lo:hi + 1] @ Cinv[k] - np.eye(3)) / g.sum()
            B[k] = np.linalg.inv(R)
    if zoom == "auto":
        if hw is None:
            raise ValueError("camera_path: zoom='auto' needs hw")
        zoom = auto_zoom(B[:, :2], hw, max_zoom)
    zoom = float(zoom)
    if not zoom >= 1.0:
        raise ValueError(f"camera_path: zoom must be >= 1 or 'auto', got {zoom!r}")
    if zoom != 1.0:
        if hw is None:
            raise ValueError("camera_path: a zoom needs hw")
        cx, cy, t = (int(hw[1]) - 1) * 0.5, (int(hw[0]) - 1) * 0.5, 1.0 / zoom
        B = B @ np.array([[t, 0.0, cx - t * cx], [0.0, t, cy - t * cy], [0.0, 0.0, 1.0]])
    return B[:, :2].copy(), zoom


class MotionSink:
    """A predict_video sink (either form: `sink(first, flows)` or the bidirectional `sink(first, fwd, bwd, frames)`) that fits every
    batch's fields and keeps only the n x 6 models and three numbers per field, on the device; with `occlusion` (bidirectional
    only) consistency.check_pairs' forward class map weighs the fit.  models() / info() copy to the host: the one synchronisation."""

    def __init__(self, kind: str = "similarity", rounds: int = 6, step: int = 1, occlusion: bool = False, **fit):
        self.kind, self.rounds, self.step, self.occlusion, self.fit = kind, rounds, step, occlusion, fit
        self._models, self._status, self._share, self._c = [], [], [], []

    def __call__(self, first_pair: int, fwd: torch.Tensor, bwd: Optional[torch.Tensor] = None, frames=None) -> None:
        from . import consistency, ops
        cls = None
        if self.occlusion:
            if bwd is None:
                raise RuntimeError("stabilize.MotionSink: occlusion=True needs predict_video(..., bidirectional=True)")
            cls = consistency.check_pairs(fwd, bwd)[0][0]
        models, info = ops.motion_fit(fwd, cls=cls, kind=self.kind, rounds=self.rounds, step=self.step, **self.fit)
        self._models.append(models)
        self._status.append(info["status"])
        self._share.append(info["inlier_share"])
        self._c.append(info["c"])

    def models(self) -> np.ndarray:
        if not self._models:
            raise RuntimeError("stabilize.MotionSink: no batch has been seen")
        return torch.cat(self._models).cpu().numpy()

    def info(self) -> dict:
        if not self._models:
            raise RuntimeError("stabilize.MotionSink: no batch has been seen")
        return {"status": torch.cat(self._status).cpu().numpy(), "inlier_share": torch.cat(self._share).cpu().numpy(),
                "c": torch.cat(self._c).cpu().numpy()}


class Stabilized:
    """What stabilize_video did: `models` [N - 1, 2, 3], `inv_maps` [N, 2, 3], `zoom`, and report()."""

    def __init__(self, models, fit_info, inv_maps, zoom, hw, outside):
        self.models, self.fit_info, self.inv_maps, self.zoom, self.hw, self.outside = models, fit_info, inv_maps, zoom, hw, outside

    def report(self) -> dict:
        """frames; mean / max over frames of the largest distance (px) a frame corner is moved; zoom; the mean inlier weight share
        of the fits; the share of output pixels whose source lay outside the frame; the number of fields with status != 0."""
        q = np.concatenate([corners(self.hw), np.ones((4, 1))], axis=1)  # [4, 3]
        moved = np.linalg.norm(np.einsum("nij,qj->nqi", self.inv_maps, q) - q[None, :, :2], axis=-1).max(axis=1)
        n, (h, w) = self.inv_maps.shape[0], self.hw
        return {"frames": int(n), "mean_correction": float(moved.mean()), "max_correction": float(moved.max()), "zoom": float(self.zoom),
                "inlier_share": float(self.fit_info["inlier_share"].mean()), "outside": float(self.outside) / (n * h * w),
                "bad_fields": int((self.fit_info["status"] != 0).sum())}

    def report_line(self) -> str:
        r = self.report()
        return ("Stabilisation frames: %d, corner correction mean: %f, max: %f, zoom: %f, inlier share: %f, outside: %f, bad fields: %d"
                % (r["frames"], r["mean_correction"], r["max_correction"], r["zoom"], r["inlier_share"], r["outside"], r["bad_fields"]))


def stabilize_video(model: Callable, frames, emit: Callable, kind: str = "similarity", sigma: Optional[float] = 15.0, zoom="auto",
                    border: str = "replicate", fill: Sequence[int] = (0, 0, 0), occlusion: bool = False,
                    size: Optional[Sequence[int]] = None, step: int = 1, T: int = 4, iters: Optional[int] = None,
                    clips_per_step: int = 8, mode: str = "sintel", device=None, rounds: int = 6, max_zoom: float = MAX_ZOOM,
                    **predict) -> Stabilized:
    """The video with its camera shake taken out, in two passes over `frames` (anything predict_video takes that can be read twice).
    Pass 1: video.predict_video (bidirectional with `occlusion`; `size`, `predict`: its other arguments) through a MotionSink.
    camera_path(sigma, zoom) on the host.  Pass 2: the frames batch by batch through ops.warp_affine (`border`: "replicate" or
    "constant" with `fill`), each batch to `emit(first_frame, uint8 [k, H, W, 3])` in order.  Returns a Stabilized."""
    from . import ops, video
    sink = MotionSink(kind=kind, rounds=rounds, step=step, occlusion=occlusion)
    video.predict_video(model, frames, T=T, iters=iters, clips_per_step=clips_per_step, mode=mode, device=device, sink=sink,
                        bidirectional=bool(occlusion), size=size, **predict)
    models, fit_info = sink.models(), sink.info()
    src = video._Source(frames)
    inv_maps, used = camera_path(models, sigma=sigma, zoom=zoom, hw=src.hw, max_zoom=max_zoom)
    dev = sink._models[0].device
    maps = torch.from_numpy(inv_maps).to(dev)
    per_batch = max(1, int(clips_per_step) * (T - 1))
    outside = torch.zeros((), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        for lo in range(0, src.n, per_batch):
            hi = min(src.n, lo + per_batch)
            buf, channels_last, frame0 = src.device_frames(lo, hi, dev)
            out, cnt = ops.warp_affine(buf[lo - frame0:hi - frame0], maps[lo:hi], border=border, fill=fill, channels_last=channels_last)
            outside += cnt.sum()
            emit(lo, out)
    return Stabilized(models, fit_info, inv_maps, used, src.hw, int(outside.item()))
