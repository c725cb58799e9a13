#!/usr/bin/env python3
"""Frame and flow resizing on the GPU: sf_resize_u8 / sf_resize_f32 (csrc/resize.hip) pass by pass against the HBM roof, against
what a user would write today (torch.nn.functional.interpolate with antialias=True on the same GPU in the same run; a PIL loop on
the host plus one upload), and the cost of video.predict_video(size=...) around a stub model.

    python tools/resize_bench.py [--batches 20] [--calls 5] [--frames 50] [--runs 3] [--no-video] [--no-host]

(a) sf_resize_u8, bilinear, at 24 frames 436 x 1024 -> 224 x 512 and -> 872 x 2048, 3 frames 2160 x 3840 -> 1080 x 1920 and 3 frames
    1088 x 1920 -> 544 x 960: the whole call, and each pass alone (the horizontal pass as a call whose height does not change, the
    vertical pass as a call on the packed intermediate whose width does not change: the same kernels with the same arguments).  HIP
    events around batches of --calls calls after warming every shape up, the median over --batches batches; operands and outputs
    rotate through more than 256 MB.  Per pass the bytes it MUST move (its input once plus its output once) over the time, as a
    fraction of 8 TB/s.
(b) sf_resize_f32 on the matching flow sizes (the model's flows on their way back to the frames' grid), the same way.
(c) the same results as torch expressions: frames as permute -> float -> F.interpolate(mode="bilinear", antialias=True) -> round ->
    clamp -> uint8 -> permute; flows as F.interpolate times the scale factors.  How far their values are from the kernels' is
    reported (torch's weights are float32 and its u8 path rounds once, so the bytes differ by at most 1 almost everywhere).
(d) a PIL loop over host frames plus one upload of the result, against ops.resize_frames on frames that are already on the GPU, and
    against an upload of the full-size frames followed by ops.resize_frames.
(e) video.predict_video on --frames frames of 1088 x 1920 with a stub model (a difference of planes: its time is negligible) at
    size=None and at half size, wall clock per video: the cost of the resizing itself.  The MODEL's speed-up at the smaller size is
    not measured here: it is the existing Spring-shape and Sintel-shape rows of the README table.
One JSON line per measurement, appended to profiles/resize_bench.jsonl."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
import torch.nn.functional as F

from streamflow_amd import _lib, ops, resize

ROOF = 8.0e12                       # HBM bytes per second
OUT = os.path.join(REPO, "profiles", "resize_bench.jsonl")
FILTER = "bilinear"
U8_CASES = [(24, (436, 1024), (224, 512)), (24, (436, 1024), (872, 2048)), (3, (2160, 3840), (1080, 1920)), (3, (1088, 1920), (544, 960))]
F32_CASES = [(24, (224, 512), (436, 1024)), (24, (872, 2048), (436, 1024)), (3, (1080, 1920), (2160, 3840)), (3, (544, 960), (1088, 1920))]


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


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


class Rotor:
    """Buffer sets that take turns, more than 256 MB in all, so that no call finds its operands in the Infinity Cache."""

    def __init__(self, make, set_bytes):
        self.n = max(2, int(np.ceil(320e6 / set_bytes)))
        self.sets = [make(i) for i in range(self.n)]
        self.turn = 0

    def next(self):
        s = self.sets[self.turn % self.n]
        self.turn += 1
        return s


def tables(H, W, h, w, dev, kind):
    """The six table arguments of an entry point (None / 0 for an axis without a pass); the tensors stay cached in resize."""
    a = []
    for i, o in ((W, w), (H, h)):
        if i == o:
            a += [None, None, 0]
        else:
            tb, tk, ks = resize.device_table(i, o, FILTER, dev, kind)
            a += [tb.data_ptr(), tk.data_ptr(), ks]
    return a


def u8_call(lib, src, out, ws, n, H, W, h, w, tab):
    _lib.check(lib.sf_resize_u8(src.data_ptr(), 3 * H * W, 3 * W, 3, 1, n, H, W, h, w, *tab, out.data_ptr(), None if ws is None else ws.data_ptr(),
                                0 if ws is None else ws.numel(), _lib.stream()), "sf_resize_u8")


def f32_call(lib, src, out, ws, n, H, W, h, w, tab, sx, sy):
    _lib.check(lib.sf_resize_f32(src.data_ptr(), 2 * H * W, H * W, W, n, H, W, h, w, *tab, sx, sy, out.data_ptr(),
                                 None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), _lib.stream()), "sf_resize_f32")


def torch_frames(x, hw):
    y = F.interpolate(x.permute(0, 3, 1, 2).float(), size=hw, mode="bilinear", antialias=True)
    return torch.floor(y + 0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def torch_flows(x, hw):
    y = F.interpolate(x, size=hw, mode="bilinear", antialias=True)
    s = torch.tensor([hw[1] / x.shape[3], hw[0] / x.shape[2]], dtype=torch.float32, device=x.device)
    return y * s[None, :, None, None]


def passes(kind, lib, dev, n, HW, hw, a):
    (H, W), (h, w) = HW, hw
    el, planes = (1, 3) if kind == "u8" else (4, 2)
    torch.manual_seed(H * 7 + w)
    if kind == "u8":
        make = lambda size: (lambda i: torch.randint(0, 256, (n, size[0], size[1], 3), dtype=torch.uint8, device=dev))
        empty = lambda size: (lambda i: torch.empty(n, size[0], size[1], 3, dtype=torch.uint8, device=dev))
    else:
        make = lambda size: (lambda i: 5 * torch.randn(n, 2, size[0], size[1], device=dev))
        empty = lambda size: (lambda i: torch.empty(n, 2, size[0], size[1], dtype=torch.float32, device=dev))
    px = lambda size: n * size[0] * size[1] * planes * el
    src, mid, out = Rotor(make((H, W)), px((H, W))), Rotor(make((H, w)), px((H, w))), Rotor(empty((h, w)), px((h, w)))
    mid_out = Rotor(empty((H, w)), px((H, w)))
    need = int((lib.sf_resize_u8_ws_bytes if kind == "u8" else lib.sf_resize_f32_ws_bytes)(n, H, W, h, w))
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    sx, sy = w / W, h / H
    if kind == "u8":
        run = lambda s, o, wsp, A, B, C, D: u8_call(lib, s, o, wsp, n, A, B, C, D, tables(A, B, C, D, dev, "u8"))
        form = lambda: torch_frames(src.next(), (h, w))
    else:
        run = lambda s, o, wsp, A, B, C, D: f32_call(lib, s, o, wsp, n, A, B, C, D, tables(A, B, C, D, dev, "f32"), sx, sy)
        form = lambda: torch_flows(src.next(), (h, w))
    shape = {"kind": kind, "filter": FILTER, "n": n, "from": [H, W], "to": [h, w], "batches": a.batches, "calls_per_batch": a.calls,
             "buffer_sets": src.n, "workspace_bytes": need}
    res = {}
    for name, fn, moved in (("both passes", lambda: run(src.next(), out.next(), ws, H, W, h, w), px((H, W)) + 2 * px((H, w)) + px((h, w))),
                            ("horizontal pass", lambda: run(src.next(), mid_out.next(), None, H, W, H, w), px((H, W)) + px((H, w))),
                            ("vertical pass", lambda: run(mid.next(), out.next(), None, H, w, h, w), px((H, w)) + px((h, w)))):
        t = median_us(fn, a.batches, a.calls)
        res[name] = t["median"]
        emit({"kernel": f"sf_resize_{kind}", "part": name, **shape, "us": t, "bytes_it_must_move": moved,
              "bytes_per_s": moved / (t["median"] * 1e-6), "fraction_of_8TBs_roof": moved / (t["median"] * 1e-6) / ROOF})
    t = median_us(form, a.batches, max(1, a.calls // 2))
    # how far the torch form's values are from the kernel's, on one set
    x = src.sets[0]
    if kind == "u8":
        mine = ops.resize_frames(x, (h, w), FILTER)
        diff = (mine.int() - torch_frames(x, (h, w)).int()).abs()
        agree = {"bytes_differing": int((diff > 0).sum()), "of": int(diff.numel()), "largest_difference": int(diff.max())}
    else:
        mine = ops.resize_flows(x, (h, w), FILTER)
        agree = {"largest_abs_difference": float((mine - torch_flows(x, (h, w))).abs().max()), "largest_abs_value": float(mine.abs().max())}
    emit({"path": "torch.nn.functional.interpolate(antialias=True) form", **shape, "us": t, "torch_over_kernel": t["median"] / res["both passes"],
          "kernel_beats_torch_form": bool(res["both passes"] < t["median"]), "agreement_with_torch_form": agree})
    del src, mid, out, mid_out
    torch.cuda.empty_cache()


def wall_ms(fn, runs):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median": float(np.median(times)), "min": float(np.min(times)), "max": float(np.max(times))}


def host_loop(dev, a):
    from PIL import Image
    n, (H, W), (h, w) = U8_CASES[0]
    host = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    arr = host.numpy()
    on_dev = host.to(dev)

    def pil():
        small = np.stack([np.asarray(Image.fromarray(f, "RGB").resize((w, h), Image.BILINEAR)) for f in arr])
        return torch.from_numpy(small).to(dev)

    same = bool(torch.equal(pil(), ops.resize_frames(on_dev, (h, w), FILTER)))
    emit({"path": "PIL loop on the host + one upload, against ops.resize_frames", "n": n, "from": [H, W], "to": [h, w], "runs": a.runs,
          "pil_loop_and_upload_ms": wall_ms(pil, a.runs), "resize_frames_on_device_frames_ms": wall_ms(lambda: ops.resize_frames(on_dev, (h, w), FILTER), a.runs),
          "upload_full_size_then_resize_frames_ms": wall_ms(lambda: ops.resize_frames(host.to(dev), (h, w), FILTER), a.runs),
          "bytes_equal_to_pil": same})


def video_cost(dev, a):
    from streamflow_amd import video
    H, W, T, n = 1088, 1920, 4, a.frames
    stub = lambda imgs: [(imgs[:, k + 1, :2] - imgs[:, k, :2]).contiguous() for k in range(imgs.shape[1] - 1)]
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(dev)
    size = resize.scaled_size((H, W), scale=0.5)
    full = wall_ms(lambda: video.predict_video(stub, frames, T=T, clips_per_step=8), a.runs)
    half = wall_ms(lambda: video.predict_video(stub, frames, T=T, clips_per_step=8, size=size), a.runs)
    emit({"path": "predict_video around a stub model, device frames, 8 clips per call", "frames": n, "shape": [H, W], "size": list(size), "T": T,
          "runs": a.runs, "size_none_ms_per_video": full, "half_size_ms_per_video": half,
          "note": "the stub model's time is negligible: this is the cost of the video path with and without resizing; the model's own "
                  "speed-up at the smaller size is the README's existing Spring-shape and Sintel-shape rows, not measured here"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-video", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    assert a.batches >= 20, "the median needs at least 20 batches"
    assert torch.cuda.is_available(), "resize_bench.py needs an MI355X"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    for n, HW, hw in U8_CASES:
        passes("u8", lib, dev, n, HW, hw, a)
    for n, HW, hw in F32_CASES:
        passes("f32", lib, dev, n, HW, hw, a)
    if not a.no_host:
        host_loop(dev, a)
    if not a.no_video:
        video_cost(dev, a)


if __name__ == "__main__":
    main()
