"""Point tracking through a video: the flows of consecutive pairs chained into long-range correspondences, and tracks drawn on frames.

For each step a point moves by the forward flow sampled bilinearly where it stands, p <- p + bilinear(fwd_j, p); with the backward
flows the forward-backward test of streamflow_amd.consistency (Sundaram et al. 2010, UnFlow's constants) decides per step whether
the point is VISIBLE or OCCLUDED; a point that leaves the frame or meets a non-finite value is LOST for good.  The whole
composition is one kernel (csrc/track.hip, ops.track_advance): a thread per point walks a batch's fields, and TrackSink carries the
state from one predict_video batch to the next on the device -- nothing crosses to the host per batch.

Points are tracked FORWARD in time only: frames before a query's own frame are PENDING.  Chained bilinear sampling accumulates the
model's error from step to step and nothing re-detects a point after an occlusion: long tracks drift.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np
import torch

VISIBLE, OCCLUDED, LOST, PENDING = range(4)
STATUS_NAMES = ("visible", "occluded", "lost", "pending")
DEFAULT_BUDGET = 8 << 30                                                 # dense_tracks: bytes of results it may allocate


def grid_queries(hw: Sequence[int], step: int, frame: int = 0) -> np.ndarray:
    """float32 [P, 3] rows (t, x, y): a regular grid of spacing `step` pixels, centred in the frame, all starting at `frame`."""
    h, w, step = int(hw[0]), int(hw[1]), int(step)
    if step < 1 or h < 1 or w < 1:
        raise ValueError(f"grid_queries: hw {tuple(hw)}, step {step} (all >= 1)")
    xs = np.arange((w - 1) % step // 2, w, step, dtype=np.float32)
    ys = np.arange((h - 1) % step // 2, h, step, dtype=np.float32)
    gx, gy = np.meshgrid(xs, ys)
    return np.stack([np.full(gx.size, float(frame), np.float32), gx.ravel(), gy.ravel()], axis=1).astype(np.float32)


def _check_queries(q, what: str) -> np.ndarray:
    q = np.asarray(q)
    if q.ndim == 1 and q.size == 3:
        q = q[None]
    if q.ndim != 2 or q.shape[1] != 3 or q.shape[0] < 1:
        raise ValueError(f"{what}: queries must be [P, 3] rows (t, x, y), got shape {q.shape}")
    q = q.astype(np.float32)
    t = q[:, 0]
    if not np.all(np.isfinite(t)) or np.any(t < 0) or np.any(t != np.floor(t)) or np.any(t > 2 ** 30):
        raise ValueError(f"{what}: the first column is the frame number, a whole number >= 0")
    return np.ascontiguousarray(q)


def load_queries(path: str) -> np.ndarray:
    """Queries from a file: `.npy` holding [P, 3], or text with `t x y` per line (blank lines and lines starting with # skipped)."""
    if str(path).lower().endswith(".npy"):
        return _check_queries(np.load(path, allow_pickle=False), f"load_queries({path})")
    rows = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            line = line.split("#", 1)[0].replace(",", " ").split()
            if not line:
                continue
            if len(line) != 3:
                raise ValueError(f"load_queries({path}): line {no} has {len(line)} fields, expected `t x y`")
            try:
                rows.append([float(v) for v in line])
            except ValueError:
                raise ValueError(f"load_queries({path}): line {no} is not three numbers") from None
    if not rows:
        raise ValueError(f"load_queries({path}): no queries")
    return _check_queries(np.array(rows, np.float64), f"load_queries({path})")


def parse_track_arg(text: str, hw: Sequence[int]) -> np.ndarray:
    """The command line's --track value: `grid:STEP` or a file for load_queries."""
    if text.startswith("grid:"):
        try:
            step = int(text[5:])
        except ValueError:
            raise ValueError(f"--track {text!r}: grid:STEP needs a whole number") from None
        return grid_queries(hw, step)
    return load_queries(text)


class Tracks:
    """The tracks of a video: `xy` [N, P, 2] (x, y in pixels of the frames' own grid) and `status` [N, P] (VISIBLE, OCCLUDED, LOST,
    PENDING), row n describing frame n, and `queries` [P, 3].  Device tensors or numpy arrays; numpy() copies to the host."""

    def __init__(self, xy, status, queries):
        if tuple(xy.shape[:2]) != tuple(status.shape) or xy.shape[2] != 2 or xy.shape[1] != len(queries):
            raise ValueError(f"Tracks: xy {tuple(xy.shape)}, status {tuple(status.shape)}, {len(queries)} queries")
        self.xy, self.status, self.queries = xy, status, queries

    @property
    def n_frames(self) -> int:
        return int(self.xy.shape[0])

    @property
    def n_points(self) -> int:
        return int(self.xy.shape[1])

    def numpy(self) -> "Tracks":
        host = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        return Tracks(host(self.xy), host(self.status), host(self.queries))

    def planar(self):
        """(xy [N, 2, P] contiguous, status [N, P]): the layout ops.draw_tracks and the kernels use."""
        xy = self.xy if isinstance(self.xy, torch.Tensor) else torch.from_numpy(np.asarray(self.xy))
        st = self.status if isinstance(self.status, torch.Tensor) else torch.from_numpy(np.asarray(self.status))
        return xy.permute(0, 2, 1).contiguous(), st.contiguous()

    def lengths(self) -> np.ndarray:
        """Frames each point was active (VISIBLE or OCCLUDED), int64 [P]."""
        st = self.numpy().status
        return (st <= OCCLUDED).sum(axis=0).astype(np.int64)

    def report(self) -> dict:
        """Shares of visible, occluded and lost points at the last frame, and the median track length in frames."""
        st = self.numpy().status
        last = st[-1]
        P = float(last.size)
        return {"frames": int(st.shape[0]), "points": int(last.size), "visible": float((last == VISIBLE).sum()) / P,
                "occluded": float((last == OCCLUDED).sum()) / P, "lost": float((last == LOST).sum()) / P,
                "median_length": float(np.median(self.lengths()))}

    def report_line(self) -> str:
        r = self.report()
        return ("Tracks points: %d, frames: %d, visible at the end: %f, occluded: %f, lost: %f, median length: %.1f"
                % (r["points"], r["frames"], r["visible"], r["occluded"], r["lost"], r["median_length"]))

    def save(self, path: str) -> None:
        """`.npz` with the arrays xy [N, P, 2], status [N, P] and queries [P, 3]."""
        t = self.numpy()
        np.savez(path, xy=t.xy, status=t.status, queries=t.queries)


def _need_gpu(what: str) -> None:
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what} runs on the GPU; there is no CPU fallback")


class TrackSink:
    """A predict_video sink (either form: `sink(first_pair, fwd)` or the bidirectional `sink(first_pair, fwd, bwd, frames)`) that
    carries P points through every batch's fields with one ops.track_advance call and keeps the state on the device between batches.
    It fills `xy` [N, P, 2] and `status` [N, P] (row n = frame n; row 0 is the queries themselves).  With `emit` it keeps only the state
    and hands every batch's rows on: `emit(first_frame, xy [k, 2, P], status [k, P])`, rows first_frame .. first_frame + k - 1
    (the first call holds row 0 too).  occlusion=True needs the bidirectional form; sticky: once OCCLUDED, always."""

    def __init__(self, queries, hw: Sequence[int], n_frames: int, occlusion: bool = True, sticky: bool = False,
                 emit: Optional[Callable] = None):
        from . import _track_lib
        self.queries = _check_queries(queries, "TrackSink")
        self.hw, self.n_frames, self.occlusion, self.sticky, self.emit = (int(hw[0]), int(hw[1])), int(n_frames), bool(occlusion), bool(sticky), emit
        if self.n_frames < 2:
            raise ValueError(f"TrackSink: n_frames = {n_frames} (at least 2)")
        _need_gpu("TrackSink")
        _track_lib.load()
        self._state = None
        self._next = 0                                                   # the pair the next batch must start with
        self.xy = self.status = None
        self._planar = None

    @property
    def n_points(self) -> int:
        return int(self.queries.shape[0])

    def _begin(self, dev) -> None:
        from . import ops
        q = torch.from_numpy(self.queries).to(dev)
        self._start = q[:, 0].to(torch.int32).contiguous()
        xy0 = q[:, 1:].t().contiguous()                                  # [2, P]
        st0 = torch.full((self.n_points,), PENDING, dtype=torch.uint8, device=dev)
        # row 0 = frame 0: a zero field applied from frame -1 would move nothing, but no field is needed: a point that starts at
        # frame 0 is VISIBLE (or LOST) at its query, every other PENDING -- the entry rule of the kernel, restated on four lines
        h, w = self.hw
        inside = (xy0[0] >= 0) & (xy0[0] <= float(w - 1)) & (xy0[1] >= 0) & (xy0[1] <= float(h - 1))
        started = self._start <= 0
        st0 = torch.where(started, torch.where(inside, torch.full_like(st0, VISIBLE), torch.full_like(st0, LOST)), st0)
        self._state = (xy0, st0)
        if self.emit is None:
            self._planar = (torch.empty(self.n_frames, 2, self.n_points, dtype=torch.float32, device=dev),
                            torch.empty(self.n_frames, self.n_points, dtype=torch.uint8, device=dev))
            self._planar[0][0].copy_(xy0)
            self._planar[1][0].copy_(st0)
        self._ops = ops

    def __call__(self, first_pair: int, fwd: torch.Tensor, bwd: Optional[torch.Tensor] = None, frames=None) -> None:
        if first_pair != self._next:
            raise RuntimeError(f"TrackSink: batches must come in video order (expected pair {self._next}, got {first_pair})")
        if self.occlusion and bwd is None:
            raise RuntimeError("TrackSink: occlusion=True needs predict_video(..., bidirectional=True)")
        if tuple(fwd.shape[-2:]) != self.hw:
            raise RuntimeError(f"TrackSink: fields of {tuple(fwd.shape[-2:])}, built for {self.hw}")
        first = self._state is None
        if first:
            self._begin(fwd.device)
        k = int(fwd.shape[0])
        if first_pair + k > self.n_frames - 1:
            raise RuntimeError(f"TrackSink: pair {first_pair + k - 1} of a video of {self.n_frames} frames")
        row0 = self._state
        xy, status, self._state = self._ops.track_advance(fwd, bwd if self.occlusion else None, state=self._state, start=self._start,
                                                          frame0=first_pair, sticky=self.sticky)
        self._next = first_pair + k
        if self.emit is None:
            self._planar[0][first_pair + 1:first_pair + 1 + k].copy_(xy)
            self._planar[1][first_pair + 1:first_pair + 1 + k].copy_(status)
        elif first:
            self.emit(0, torch.cat([row0[0][None], xy]), torch.cat([row0[1][None], status]))
        else:
            self.emit(first_pair + 1, xy, status)

    def tracks(self) -> Tracks:
        if self._planar is None or self._next != self.n_frames - 1:
            raise RuntimeError("TrackSink: the video is not complete" if self.emit is None else "TrackSink: with `emit` nothing is kept")
        return Tracks(self._planar[0].permute(0, 2, 1), self._planar[1], self.queries)


def track_points(model: Callable, frames, queries, T: int = 4, iters: Optional[int] = None, clips_per_step: int = 8,
                 occlusion: bool = True, sticky: bool = False, size: Optional[Sequence[int]] = None, mode: str = "sintel", device=None,
                 **predict) -> Tracks:
    """The tracks of `queries` ([P, 3] rows (t, x, y)) through the video: video.predict_video with a TrackSink.  occlusion=True runs
    predict_video(bidirectional=True) -- TWO model calls per batch -- and marks points OCCLUDED by the forward-backward test;
    occlusion=False is forward only, one model call per batch, every active point VISIBLE.  size=(h, w) goes through to
    predict_video: the model runs at that size and the flows come back on the frames' own grid, so tracks are in original pixels.
    Returns Tracks (device tensors)."""
    from . import _track_lib, video
    queries = _check_queries(queries, "track_points")
    _need_gpu("track_points")
    _track_lib.load()
    src = video._Source(frames)
    sink = TrackSink(queries, src.hw, src.n, occlusion=occlusion, sticky=sticky)
    video.predict_video(model, frames, T=T, iters=iters, clips_per_step=clips_per_step, mode=mode, device=device, sink=sink,
                        bidirectional=bool(occlusion), size=size, **predict)
    return sink.tracks()


class DenseTracks:
    """dense_tracks' result: `xy` fp32 [n, 2, H, W] (where the anchor frame's pixels are in frames anchor + 1 .. anchor + n) and
    `status` uint8 [n, H, W]."""

    def __init__(self, xy: torch.Tensor, status: torch.Tensor, anchor: int):
        self.xy, self.status, self.anchor = xy, status, anchor

    def long_range_flow(self) -> torch.Tensor:
        """fp32 [n, 2, H, W]: the flow from the anchor frame to every later frame (positions minus the pixel grid)."""
        n, _, H, W = self.xy.shape
        gy, gx = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=self.xy.device),
                                torch.arange(W, dtype=torch.float32, device=self.xy.device), indexing="ij")
        return self.xy - torch.stack([gx, gy])[None]


class _DenseSink:
    def __init__(self, anchor: int, last: int, hw, occlusion: bool, sticky: bool):
        self.anchor, self.last, self.hw, self.occlusion, self.sticky = anchor, last, hw, occlusion, sticky
        self.xy = self.status = self.state = None

    def __call__(self, first_pair: int, fwd: torch.Tensor, bwd: Optional[torch.Tensor] = None, frames=None) -> None:
        from . import ops
        lo, hi = max(first_pair, self.anchor), min(first_pair + int(fwd.shape[0]), self.last)
        if lo >= hi:
            return
        if self.xy is None:
            n, (H, W) = self.last - self.anchor, self.hw
            self.xy = torch.empty(n, 2, H * W, dtype=torch.float32, device=fwd.device)
            self.status = torch.empty(n, H * W, dtype=torch.uint8, device=fwd.device)
        f = fwd[lo - first_pair:hi - first_pair]
        b = bwd[lo - first_pair:hi - first_pair] if self.occlusion else None
        xy, st, self.state = ops.track_advance(f, b, state=self.state, frame0=lo, sticky=self.sticky)
        self.xy[lo - self.anchor:hi - self.anchor].copy_(xy)
        self.status[lo - self.anchor:hi - self.anchor].copy_(st)


def dense_tracks(model: Callable, frames, anchor: int = 0, last: Optional[int] = None, T: int = 4, iters: Optional[int] = None,
                 clips_per_step: int = 8, occlusion: bool = True, sticky: bool = False, size: Optional[Sequence[int]] = None,
                 mode: str = "sintel", device=None, budget_bytes: int = DEFAULT_BUDGET, **predict) -> DenseTracks:
    """Every pixel of frame `anchor` tracked to frame `last` (default: the video's last): dense mode of the kernel, a point per pixel.
    The results take 9 bytes per pixel and frame ([n, 2, H, W] fp32 + [n, H, W] uint8, n = last - anchor) plus one batch's rows again
    while they are copied; a request above `budget_bytes` is refused with the byte count in the message."""
    from . import _track_lib, video
    src = video._Source(frames)
    last = src.n - 1 if last is None else int(last)
    anchor = int(anchor)
    if not 0 <= anchor < last <= src.n - 1:
        raise ValueError(f"dense_tracks: anchor {anchor}, last {last} in a video of {src.n} frames (0 <= anchor < last <= {src.n - 1})")
    H, W = src.hw
    per_batch = min(last - anchor, max(1, int(clips_per_step)) * (T - 1))
    need = 9 * H * W * (last - anchor + per_batch)
    if need > int(budget_bytes):
        raise MemoryError(f"dense_tracks: {last - anchor} frames of {H} x {W} need {need} bytes of results, the budget is "
                          f"{int(budget_bytes)} bytes (budget_bytes=, or a shorter range)")
    _need_gpu("dense_tracks")
    _track_lib.load()
    sink = _DenseSink(anchor, last, (H, W), bool(occlusion), bool(sticky))
    video.predict_video(model, frames, T=T, iters=iters, clips_per_step=clips_per_step, mode=mode, device=device, sink=sink,
                        bidirectional=bool(occlusion), size=size, **predict)
    n = last - anchor
    return DenseTracks(sink.xy.view(n, 2, H, W), sink.status.view(n, H, W), anchor)


def default_palette(n: int = 55) -> np.ndarray:
    """uint8 [n, 3]: flow_viz' colour wheel (55 hues), sampled in an order that keeps neighbouring point indices apart in hue."""
    from .flow_viz import make_colorwheel
    wheel = make_colorwheel().astype(np.uint8)
    order = (np.arange(n) * 21) % wheel.shape[0]                         # 21 and 55 are coprime: a permutation for n = 55
    return np.ascontiguousarray(wheel[order])


def alpha_fade(trail: int, newest: int = 255, oldest: int = 48) -> np.ndarray:
    """uint8 [trail]: alpha by age, linear from `newest` at age 0 to `oldest` at age trail - 1."""
    trail = int(trail)
    if trail < 1:
        raise ValueError(f"alpha_fade: trail = {trail}")
    if trail == 1:
        return np.array([newest], np.uint8)
    a = np.arange(trail, dtype=np.int64)
    return ((newest * (trail - 1 - a) + oldest * a + (trail - 1) // 2) // (trail - 1)).astype(np.uint8)


def draw(frames: torch.Tensor, tracks: Tracks, first_frame: int = 0, trail: int = 16, radius: int = 3, trail_radius: int = 1,
         draw_occluded: bool = False, palette: Optional[np.ndarray] = None) -> torch.Tensor:
    """frames uint8 [n, H, W, 3] (or [n, 3, H, W]) on the GPU, frames[j] = frame first_frame + j of the video `tracks` describes ->
    uint8 [n, H, W, 3] with the tracks drawn (ops.draw_tracks; colours from flow_viz' wheel, a linear alpha fade along the trail)."""
    _need_gpu("track.draw")
    xy, status = tracks.planar()
    dev = frames.device
    pal = torch.from_numpy(default_palette() if palette is None else np.ascontiguousarray(palette, dtype=np.uint8)).to(dev)
    from . import ops
    return ops.draw_tracks(frames, xy.to(dev), status.to(dev), first_frame, trail=trail, radius=radius, trail_radius=trail_radius,
                           palette=pal, draw_occluded=draw_occluded, alpha_table=torch.from_numpy(alpha_fade(trail)).to(dev))


def draw_video(frames, tracks: Tracks, emit: Callable, trail: int = 16, radius: int = 3, trail_radius: int = 1, draw_occluded: bool = False,
               device=None, frames_per_step: int = 24) -> None:
    """The whole video with its tracks drawn, batch by batch: `frames` is anything predict_video takes, every batch goes to
    `emit(first_frame, uint8 [k, H, W, 3])` in order.  The palette and the alpha table are made once."""
    from . import ops, video
    _need_gpu("track.draw_video")
    src = video._Source(frames)
    if src.n != tracks.n_frames:
        raise ValueError(f"draw_video: {src.n} frames, tracks of {tracks.n_frames}")
    dev = torch.device(device) if device is not None else (tracks.xy.device if isinstance(tracks.xy, torch.Tensor) and tracks.xy.is_cuda
                                                           else torch.device("cuda", torch.cuda.current_device()))
    xy, status = (t.to(dev) for t in tracks.planar())
    pal, fade = torch.from_numpy(default_palette()).to(dev), torch.from_numpy(alpha_fade(trail)).to(dev)
    with torch.cuda.device(dev):
        for lo in range(0, src.n, max(1, int(frames_per_step))):
            hi = min(src.n, lo + max(1, int(frames_per_step)))
            buf, channels_last, frame0 = src.device_frames(lo, hi, dev)
            emit(lo, ops.draw_tracks(buf[lo - frame0:hi - frame0], xy, status, lo, trail=trail, radius=radius, trail_radius=trail_radius,
                                     palette=pal, draw_occluded=draw_occluded, alpha_table=fade, channels_last=channels_last))
