#!/usr/bin/env python3
"""Spring .flo5 input, the host reader against the device reader, at the size of Spring's ground truth.

    python tools/flo5_decode_bench.py [--launches 10] [--windows 5] [--runs 5] [--out profiles/flo5_decode_bench.jsonl]

Three ground-truth fields of 2160 x 3840 x 2 float32.  The data is SYNTHETIC (tests/flo5_encode_cases.bench_field -- a seeded bilinear
upsampling of coarse Gaussian noise plus 0.01 px of noise -- with NaN holes); no Spring file exists here, and real ground truth
compresses differently.  The same fields in three layouts, one JSON line each:
  h5py         h5py's layout for this shape: chunks (68, 240, 1) at gzip 5, 1024 zlib streams of 65 280 bytes per file
               (tests/flo5_decode_cases.tiled_file with 64 entries per B-tree node)
  write_flo5   flo5.write_flo5: 32 chunks of (68, 3840, 2) at gzip 5
  write_batch  flo5_gpu.write_batch: the same chunks, shuffled, Huffman-only deflate
and per layout, in one run on one box, files in the page cache:
  host_loop_ms          what spring_report(flo5_decode="host") runs per clip: flo5.read_flo5 + torch.from_numpy(...).to(device) per file
  read_batch_gpu_ms     flo5_gpu.read_batch(inflate="gpu") end to end, HOST_INFLATE_CHUNK_BYTES lifted so that sf_inflate does run
  read_batch_host_ms    flo5_gpu.read_batch(inflate="host") end to end
  read_batch_default_ms flo5_gpu.read_batch as shipped (its default `inflate` and threshold)
                        -- each the median of --runs after one warm-up, with min and max (the run-to-run spread)
  inflate_ms / assemble_ms   sf_inflate and sf_flo5_assemble alone (buffers allocated once): device events around --launches calls
                        after a warm-up, the median of --windows windows, with bytes/s of inflated output
Then `row_chunks`: one field in chunks of (r, 3840, 2) for a range of r, device inflate against host inflate end to end: where the
two cross is where flo5_gpu.HOST_INFLATE_CHUNK_BYTES belongs.  Every result is compared bit for bit with flo5.read_flo5 before
anything is timed.  A GPU is required (no fallback)."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tests import flo5_decode_cases as dc
from tests import flo5_encode_cases as fc

N_FIELDS, H, W = 3, 2160, 3840


def field(seed):
    f = np.ascontiguousarray(fc.bench_field(H, W, seed).transpose(1, 2, 0))
    rng = np.random.default_rng(seed)
    for _ in range(40):                                                   # NaN holes: occluded / invalid regions
        cy, cx, ry, rx = rng.integers(0, H), rng.integers(0, W), rng.integers(4, 120), rng.integers(4, 200)
        f[max(0, cy - ry):cy + ry, max(0, cx - rx):cx + rx] = np.nan
    return f


def timed(fn, runs, sync):
    fn()
    sync()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(float(np.median(ms)), 2), "min": round(min(ms), 2), "max": round(max(ms), 2)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("flo5_decode_bench needs the GPU; there is no CPU fallback")
    from bench import usable_cores
    from streamflow_amd import flo5, flo5_gpu, ops, png_gpu
    torch.set_num_threads(min(usable_cores(), 64))
    dev = torch.device("cuda", torch.cuda.current_device())
    sync = torch.cuda.synchronize
    shipped = flo5_gpu.HOST_INFLATE_CHUNK_BYTES
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    def kernels(paths):
        """sf_inflate and sf_flo5_assemble alone on the chunks of `paths` (one geometry)."""
        tables = [flo5.chunk_table(p) for p in paths]
        (Hh, Ww, _), cs, shuffle = tables[0]["shape"], tables[0]["chunk_shape"], 2 in tables[0]["filters"]
        size = 4 * cs[0] * cs[1] * cs[2]
        comp, desc, grid = bytearray(), [], np.full((len(paths), -(-Hh // cs[0]), -(-Ww // cs[1]), 2 // cs[2]), -1, np.int32)
        for i, t in enumerate(tables):
            for offs, addr, nbytes, _ in t["chunks"]:
                grid[(i,) + tuple(o // c for o, c in zip(offs, cs))] = len(desc)
                desc.append((len(comp), nbytes, len(desc) * size, size, 0))
                comp += t["data"][addr:addr + nbytes]
        c = torch.from_numpy(np.frombuffer(bytes(comp), np.uint8).copy()).to(dev)
        d = torch.tensor(desc, dtype=torch.int64, device=dev)
        out = torch.empty(len(desc) * size, dtype=torch.uint8, device=dev)
        g = torch.from_numpy(grid).to(dev)
        res = {}
        for name, call in (("inflate", lambda: ops.inflate(c, d, out)),
                           ("assemble", lambda: ops.flo5_assemble(out.view(len(desc), size), g, Hh, Ww, cs, shuffle))):
            for _ in range(2):
                r = call()
            sync()
            if name == "inflate":
                assert not bool(r.any())
            win = []
            for _ in range(a.windows):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.launches):
                    call()
                e.record()
                e.synchronize()
                win.append(s.elapsed_time(e) / a.launches)
            ms = float(np.median(win))
            res[name + "_ms"] = round(ms, 3)
            res[name + "_ms_windows"] = [round(x, 3) for x in win]
            res[name + "_GBps_out"] = round(len(desc) * size / ms / 1e6, 2)
        res["streams"], res["compressed_bytes"], res["chunk_bytes"] = len(desc), len(comp), size
        return res

    def measure(paths, with_kernels=True):
        want = [flo5.read_flo5(p).view(np.uint32) for p in paths[:1]]
        res = {}
        for key, kw, thresh in (("read_batch_gpu_ms", {"inflate": "gpu"}, 1 << 40), ("read_batch_host_ms", {"inflate": "host"}, shipped),
                                ("read_batch_default_ms", {}, shipped)):
            flo5_gpu.HOST_INFLATE_CHUNK_BYTES = thresh
            got = flo5_gpu.read_batch(paths, dev, **kw)
            assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0]), key
            del got
            res[key] = timed(lambda: flo5_gpu.read_batch(paths, dev, **kw), a.runs, sync)
        flo5_gpu.HOST_INFLATE_CHUNK_BYTES = shipped
        res["host_loop_ms"] = timed(lambda: [torch.from_numpy(flo5.read_flo5(p)).to(dev) for p in paths], max(2, a.runs // 2), sync)
        if with_kernels:
            res.update(kernels(paths))
        return res

    fields = [field(300 + i) for i in range(N_FIELDS)]
    common = {"bench": "flo5_decode", "data": "synthetic (bilinear upsampling of coarse Gaussian noise + 0.01 px noise, NaN holes)",
              "fields": N_FIELDS, "shape": [H, W, 2], "raw_bytes": N_FIELDS * H * W * 8, "pool_threads": png_gpu.pool_threads(),
              "default_inflate": flo5_gpu.DEFAULT_INFLATE, "host_inflate_chunk_bytes": shipped}
    with tempfile.TemporaryDirectory() as tmp:
        layouts = {}
        for name in ("h5py", "write_flo5", "write_batch"):
            layouts[name] = [os.path.join(tmp, f"{name}_{i}.flo5") for i in range(N_FIELDS)]
        for i, f in enumerate(fields):
            with open(layouts["h5py"][i], "wb") as fo:
                fo.write(dc.tiled_file(f, (68, 240, 1), 5, leaf_k=64))
            flo5.write_flo5(layouts["write_flo5"][i], f, compression_level=5)
        flo5_gpu.write_batch(torch.from_numpy(np.stack(fields)).permute(0, 3, 1, 2).contiguous().to(dev), layouts["write_batch"])
        for name, paths in layouts.items():
            rec = dict(common, layout=name, file_bytes=sum(map(os.path.getsize, paths)))
            rec.update(measure(paths))
            rec["host_loop_over_default"] = round(rec["host_loop_ms"]["median"] / rec["read_batch_default_ms"]["median"], 2)
            rec["host_inflate_over_gpu_inflate"] = round(rec["read_batch_host_ms"]["median"] / rec["read_batch_gpu_ms"]["median"], 2)
            emit(rec)
        rows = []
        for r in (2, 4, 8, 17, 34, 68):                                       # one field in row chunks: 61 KB .. 2 MB per chunk
            p = os.path.join(tmp, f"rows_{r}.flo5")
            with open(p, "wb") as fo:
                fo.write(dc.tiled_file(fields[0], (r, W, 2), 5, leaf_k=64))
            m = measure([p], with_kernels=False)
            rows.append({"rows": r, "chunk_bytes": r * W * 8, "chunks": -(-H // r), "gpu_ms": m["read_batch_gpu_ms"],
                         "host_ms": m["read_batch_host_ms"]})
        emit(dict(common, layout="row_chunks", fields=1, raw_bytes=H * W * 8, row_chunks=rows))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
