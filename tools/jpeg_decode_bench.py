#!/usr/bin/env python3
"""JPEG / Motion-JPEG input on the GPU against a PIL (libjpeg-turbo) loop on the host, on frames of the demo's sizes.

    python tools/jpeg_decode_bench.py [--launches 20] [--windows 5] [--runs 5] [--quality 90] [--iters 4] [--out profiles/jpeg_decode_bench.jsonl]

24 frames of 436 x 1024 x 3 and three of 1088 x 1920 x 3 (colour wheels of smooth synthetic fields, tests/png_encode_cases.smooth_field,
with a little noise so that the files are not trivially small), encoded once per layout:
  rows       the project's own files (jpeg_gpu.encode_batch: 4:4:4, one restart interval per MCU row) -- the layout the decoder is
             parallel on: a wave per interval
  nodri444   PIL's file of the same pixels and tables, 4:4:4, no DRI: ONE interval, so one wave decodes the whole image (if PIL is there)
  nodri420   PIL's 4:2:0 file, no DRI, as cameras and ffmpeg write them (if PIL is there)
Per set and layout, in one run on one box:
  kernel_ms          sf_jpeg_decode alone for the whole batch (a memset and four launches; inputs on the device, output and
                     workspace allocated once): device events around --launches calls after a warm-up, the median of --windows windows
  split_kernel_ms    the same for sf_jpeg_decode_split with every interval split (split_min_bytes = 0), per segment_bytes in 64, 128,
                     256: {segment_bytes: ms}; split_over_wave = kernel_ms / the best of them
  decode_batch_ms    jpeg_gpu.decode_batch(split="never") -- a wave per interval, the route before the split route existed -- end to
                     end from the files' bytes in memory (parse in the thread pool, one upload, the call, the read of the status words,
                     synchronised), the median of --runs; decode_batch_split_ms the same with split="always", the two taken in turn
                     in the same loop; decode_batch_spread the largest (max - min) / median of the two run lists
  sync               for the first file at each segment size, from the sanitized host program that runs the kernels' functions
                     (csrc/host/jpeg_sync_host_main.cpp): segments, rounds and re-decodes beyond the speculative pass
  pil_loop_ms        PIL's decode of every file, one thread, np.stack and one upload of the batch; the median of --runs; "skipped"
                     where PIL is absent
and for the `rows` layout of the first set the whole from a file to flows:
  predict_video_reader_ms / predict_video_tensor_ms   video.predict_video (the tiny synthetic-weight model of the video tests,
                     T = 4, 8 clips per call, --iters) on an avi.MjpegReader over the written AVI file, and on the decoded frames
                     already on the device; the median of --runs
Before anything is timed every layout's pixels are compared: decode_batch against PIL's bit for bit where PIL is there, and the
first frame of `rows` against tests/jpeg_decode_cases.decode_ref; split="always" against split="never" bit for bit.  The numbers are reported, not gated.  One JSON line per set and
layout, written to --out.  Needs no dataset; a GPU is required (no fallback)."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from streamflow_amd import _lib, avi, jpeg_gpu, ops, png_gpu, video
from tests import jpeg_decode_cases as dc
from tests import jpeg_sync_cases as sc
from tests import png_encode_cases as ec

SETS = [("frames_436x1024", 24, 436, 1024), ("frames_1088x1920", 3, 1088, 1920)]
SEGMENT_BYTES = (64, 128, 256)


def median_ms(fn, runs):
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times)), 2), [round(x, 2) for x in times]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "jpeg_decode_bench.jsonl"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("jpeg_decode_bench needs the GPU; there is no CPU fallback")
    if a.launches < 10 or a.windows < 1 or a.runs < 1:
        raise ValueError("--launches at least 10, --windows and --runs at least 1")
    from bench import usable_cores
    torch.set_num_threads(min(usable_cores(), 64))
    try:
        from PIL import Image
    except ImportError:
        Image = None
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    q = jpeg_gpu.quant_tables(a.quality)
    pil_q = [[int(v) for v in t] for t in q]
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        host = sc.host_program(tmp)
        for name, n, h, w in SETS:
            flows = torch.from_numpy(np.stack([ec.smooth_field(h, w, 100 + i) for i in range(n)])).to(dev)
            clean = ops.flow_to_image(flows).cpu().numpy().astype(np.int16)
            noise = np.random.default_rng(7).integers(-6, 7, size=clean.shape, dtype=np.int16)
            source = np.clip(clean + noise, 0, 255).astype(np.uint8)
            layouts = {"rows": jpeg_gpu.encode_batch(torch.from_numpy(source).to(dev), quality=a.quality)}
            if Image is not None:
                for tag, sub in (("nodri444", 0), ("nodri420", 2)):
                    layouts[tag] = []
                    for img in source:
                        buf = io.BytesIO()
                        Image.fromarray(img).save(buf, "JPEG", qtables=pil_q, subsampling=sub, optimize=False)
                        layouts[tag].append(buf.getvalue())
            assert np.array_equal(jpeg_gpu.decode_batch(layouts["rows"][:1], dev)[0].cpu().numpy(), dc.decode_ref(layouts["rows"][0])), name
            for tag, files in layouts.items():
                rec = {"set": name, "layout": tag, "images": n, "shape": [h, w, 3], "quality": a.quality, "pool_threads": png_gpu.pool_threads(),
                       "file_bytes": sum(len(f) for f in files), "raw_bytes": n * h * w * 3}
                parsed = [jpeg_gpu.parse(f) for f in files]
                rec["intervals_per_image"] = len(parsed[0].intervals)
                got = jpeg_gpu.decode_batch(files, dev, split="never")
                assert torch.equal(jpeg_gpu.decode_batch(files, dev, split="always"), got), (name, tag)

                def pil_loop():
                    return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files])).to(dev)

                if Image is not None:
                    assert torch.equal(got, pil_loop()), (name, tag)
                    rec["equals_pil"] = True
                never, always = [], []
                for _ in range(a.runs):                                 # in turn, so that drift hits both alike
                    never += median_ms(lambda: jpeg_gpu.decode_batch(files, dev, split="never"), 1)[1]
                    always += median_ms(lambda: jpeg_gpu.decode_batch(files, dev, split="always"), 1)[1]
                rec["decode_batch_ms"], rec["decode_batch_ms_runs"] = round(float(np.median(never)), 2), never
                rec["decode_batch_split_ms"], rec["decode_batch_split_ms_runs"] = round(float(np.median(always)), 2), always
                rec["decode_batch_spread"] = round(max((max(r) - min(r)) / np.median(r) for r in (never, always)), 3)
                if Image is not None:
                    rec["pil_loop_ms"], rec["pil_loop_ms_runs"] = median_ms(pil_loop, a.runs)
                    rec["pil_loop_over_decode_batch"] = round(rec["pil_loop_ms"] / rec["decode_batch_ms"], 2)
                else:
                    rec["pil_loop_ms"] = "skipped"
                data, desc, tables = (torch.from_numpy(x.copy()).to(dev) for x in jpeg_gpu.pack(parsed, files))
                geom = parsed[0][:5]
                out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
                status = torch.empty(n, dtype=torch.int32, device=dev)
                head = (data.data_ptr(), data.numel(), desc.data_ptr(), desc.shape[0], tables.data_ptr(), tables.shape[0], n, *geom, out.data_ptr(),
                        h * w * 3, w * 3, 3, status.data_ptr())

                def timed(segment_bytes):
                    """ms per call of sf_jpeg_decode (segment_bytes None) or sf_jpeg_decode_split with every interval split."""
                    ws_bytes = lib.sf_jpeg_decode_ws_bytes(n, *geom) if segment_bytes is None else \
                        lib.sf_jpeg_decode_split_ws_bytes(n, *geom, data.numel(), desc.shape[0], segment_bytes)
                    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

                    def call():
                        if segment_bytes is None:
                            _lib.check(lib.sf_jpeg_decode(*head, ws.data_ptr(), ws_bytes, _lib.stream()), "sf_jpeg_decode")
                        else:
                            _lib.check(lib.sf_jpeg_decode_split(*head, segment_bytes, 0, ws.data_ptr(), ws_bytes, _lib.stream()), "sf_jpeg_decode_split")

                    out.zero_()
                    for _ in range(3):
                        call()
                    torch.cuda.synchronize()
                    assert not status.any() and torch.equal(out, got), (name, tag, segment_bytes)
                    windows = []
                    for _ in range(a.windows):
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        for _ in range(a.launches):
                            call()
                        e.record()
                        e.synchronize()
                        windows.append(s.elapsed_time(e) / a.launches)
                    return float(np.median(windows)), [round(x, 4) for x in windows], ws_bytes

                kernel_ms, windows, ws_bytes = timed(None)
                rec.update({"kernel_ms": round(kernel_ms, 4), "kernel_ms_windows": windows,
                            "kernel_MPix_per_s": round(n * h * w / kernel_ms / 1e3, 1), "workspace_bytes": ws_bytes})
                split = {S: timed(S) for S in SEGMENT_BYTES}
                rec["split_kernel_ms"] = {str(S): round(v[0], 4) for S, v in split.items()}
                rec["split_kernel_ms_windows"] = {str(S): v[1] for S, v in split.items()}
                rec["split_workspace_bytes"] = {str(S): v[2] for S, v in split.items()}
                rec["split_over_wave"] = round(kernel_ms / min(v[0] for v in split.values()), 2)
                rec["interval_bytes_max"] = int(desc[:, 1].max())
                first = [parsed[0]], [files[0]]
                rec["sync"] = {}
                for S in SEGMENT_BYTES:
                    c = object.__new__(sc.Call)
                    c.h, c.w, c.nc, c.hs, c.vs = geom
                    c.n, c.names = 1, [name]
                    c.data, c.desc, c.tables = jpeg_gpu.pack(*first)
                    c.segment_bytes, c.split_min_bytes = S, 0
                    r = sc.run_host(host, [c], tmp, "sync")[0]
                    rec["sync"][str(S)] = {"segments": int(r["segments"].sum()), "rounds_max": int(r["rounds"].max()),
                                           "redecodes": int(r["redecodes"].sum())}
                if tag == "rows" and name == SETS[0][0]:
                    from streamflow_amd import synthetic as syn
                    from streamflow_amd.model import SKFlow_MF8, default_args
                    path = os.path.join(tmp, name + ".avi")
                    with avi.MjpegWriter(path, w, h, 24) as v:
                        for f in files:
                            v.add(f)
                    model = SKFlow_MF8(default_args(T=4, Encoder="PatchEncoder")).to(dev)
                    model.load_state_dict(dict(syn.make_params(41, 4)), strict=True)
                    run = lambda frames: video.predict_video(model, frames, T=4, iters=a.iters, clips_per_step=8)
                    assert torch.equal(run(avi.MjpegReader(path)), run(got))
                    rec["predict_video_iters"] = a.iters
                    rec["predict_video_reader_ms"], rec["predict_video_reader_ms_runs"] = median_ms(lambda: run(avi.MjpegReader(path)), a.runs)
                    rec["predict_video_tensor_ms"], rec["predict_video_tensor_ms_runs"] = median_ms(lambda: run(got), a.runs)
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
