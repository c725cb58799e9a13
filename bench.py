#!/usr/bin/env python3
"""Headline benchmark: flow-fields/sec of the StreamFlow hot path at Sintel shape (436x1024 padded to
440x1024 -> 55x128 feature grid), T=4 frames (3 flow fields per clip), iters=15, one clip per GPU per step.

    python bench.py [--gpus N] [--steps K] [--warmup W]          (N > 1: the ranks are spawned by this process)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...   (N > 1, external launcher)
    python bench.py ... --dump-outputs DIR                        (+ the flows of the last timed step as DIR/*.npy)
    python bench.py ... --full                                     (+ power, clock, kernel table, rooflines, CPU baseline, EPE, ...)

A plain run sets up, warms up, times K steps and prints the headline JSON line; everything else the record can hold is
measured with --full only, after the timed steps.

A "step" = one full pass of the hot path over one clip per rank: corr volumes + pyramids for the 3 pairs,
context split, GMA attention matrix, 15 refinement iterations (lookup, motion encoder, aggregate, temporal
block, gru, flow head), mask head + convex 8x upsampling of the final flows.  Inputs (encoder features,
random-init weights of the reference architecture) are synthetic and already resident in HBM.  Clips are
independent, so N GPUs run N replicas with no data-path collective (torch.distributed is used only for the
barrier and the max-over-ranks timing the contract asks for).
"""
import argparse
import datetime
import glob
import json
import os
import socket
import statistics
import subprocess
import sys
import time
from dataclasses import replace

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _load_launch():
    # streamflow_amd/launch.py by path: importing the package would import torch, and the placement below must happen first
    import importlib.util
    spec = importlib.util.spec_from_file_location("sf_launch", os.path.join(ROOT, "streamflow_amd", "launch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


launch = _load_launch()


def _argv_option(name: str, default: str) -> str:
    for a, b in zip(sys.argv[1:], sys.argv[2:] + [""]):
        if a == name:
            return b
        if a.startswith(name + "="):
            return a.split("=", 1)[1]
    return default


def _place_this_rank():
    """Placement of a rank of an N > 1 run (spawned by this file or by torch.distributed.run), BEFORE torch / the HIP runtime are
    loaded and before OpenMP sizes its pools from the affinity mask: first remember the OUTER device list (the NUMA
    lookup maps the local rank through it), then take the rank's share of the host cores -- the cores of its GPU's NUMA node split
    between the ranks OF THIS NODE (LOCAL_WORLD_SIZE under a multi-node launcher) -- then restrict the rank to its device.
    Only when this file is the program: `import bench` (tests, tools) must not change the importer's affinity or devices."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    pin_device = (world > 1 and "SF_BENCH_DEVICE" not in os.environ and "--share-device" not in sys.argv
                  and _argv_option("--pin", os.environ.get("SF_BENCH_PIN", "visible")) == "visible")
    if pin_device:
        os.environ["SF_BENCH_OUTER_VISIBLE"] = os.environ.get("HIP_VISIBLE_DEVICES", "")
    cpus = launch.pin_rank_cpus(local_rank, local_world if world > 1 else 1)
    if pin_device:
        # a rank under an external launcher (torch.distributed.run): restricted to ITS device before the HIP runtime is even loaded
        os.environ.update(launch.pinned_device_env(local_rank, os.environ.get("HIP_VISIBLE_DEVICES")))
    return cpus


RANK_CPUS = _place_this_rank() if __name__ == "__main__" else (sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else [])

import torch
import torch.distributed as dist

WORKLOADS = {
    # name: (H, W, T, iters)
    "sintel": (440, 1024, 4, 15),
    "demo256": (256, 256, 4, 4),
    "kitti": (376, 1248, 2, 15),
    "kitti_w160": (376, 1280, 2, 15),  # experiment: KITTI with a 160-cell grid row (640-byte volume rows = whole cache lines)
    "spring": (1088, 1920, 4, 15),     # 1080p padded to /8: 136x240 grid, N = 32640 (use --clips 1; 17 GB of volumes)
}
PEAK_FP32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: exact-fp32 MFMA = fp32 vector peak
PEAK_F16_MFMA_TFLOPS = 2500.0      # dense f16/bf16 MFMA; the split path spends 3 MFMA flops per algorithmic flop
PEAK_HBM_GBPS = 8000.0             # MI355X_MICROARCH.md: 8 TB/s spec (6.3 TB/s achievable)
PEAK_CLOCK_MHZ = 2400.0            # MI355X_MICROARCH.md: max clock (the dense peaks above are quoted at it)


def log(msg: str) -> None:
    print(f"[bench +{time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


_T0 = time.perf_counter()


def usable_cores() -> int:
    """Host cores this process may actually use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except OSError:
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
                q = int(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                p = int(f.read())
            if q > 0:
                n = min(n, max(1, q // p))
        except OSError:
            pass
    return max(1, n)


def shard(n_items: int, world: int, rank: int):
    """Round-robin partition of independent clips over ranks."""
    return list(range(rank, n_items, world))


def batches(n_clips: int, per_launch: int):
    """Launch sizes of one rank's step in the strong-scaling mode: its clips in batches of at most `per_launch` (the last one
    may be smaller; a rank without clips runs nothing and only takes part in the barriers)."""
    full, rest = divmod(n_clips, per_launch)
    return [per_launch] * full + ([rest] if rest else [])


def timed_steps(step_fn, steps: int, warmup: int, world: int, sync_fn, barrier_fn, allreduce_max_fn, own=None) -> float:
    """W untimed warm-up steps, then exactly K steps bracketed by barrier + device sync; MAX over ranks.
    own (optional list): receives this rank's own time up to its device sync, BEFORE the closing barrier (diagnosis of a
    scaling run: which rank was the slow one)."""
    for _ in range(warmup):
        step_fn()
    sync_fn()
    barrier_fn()
    t0 = time.perf_counter()
    host, host_cpu = 0.0, 0.0
    for _ in range(steps):
        th, tc = time.perf_counter(), time.thread_time()
        step_fn()
        host += time.perf_counter() - th               # wall time the HOST thread spends inside the step (input staging + graph launch /
        host_cpu += time.thread_time() - tc            # enqueues; includes blocking on a full hardware queue) and its CPU time alone
    sync_fn()
    if own is not None:
        own.append(time.perf_counter() - t0)
        own.append(host)
        own.append(host_cpu)
    barrier_fn()
    dt = time.perf_counter() - t0
    return allreduce_max_fn(dt)


DUMP_BYTES = 48_000_000


def dump_outputs(outs, out_dir: str, budget_bytes: int = DUMP_BYTES):
    """--dump-outputs: the flows a caller of the timed path receives from one step, `outs` = the (flows_up, flows_lowres) of each
    forward of that step, as out_dir/flow_up_<pair>.npy [clips, 2, 8h, 8w] and flow_low_<pair>.npy [clips, 2, h, w] in float32
    (the clips of all forwards of the step concatenated).  At most `budget_bytes` of data in all: the smallest arrays are written
    whole, and an array that does not fit its share of the rest is replaced by a sample of its flattened elements, at indices
    drawn from a fixed seed (the same in every run with the same arguments, so that two builds compare element for element).
    Returns the names written."""
    import numpy as np
    arrays = {}
    for i in range(len(outs[0][0])):
        arrays[f"flow_up_{i}"] = torch.cat([o[0][i] for o in outs])
        arrays[f"flow_low_{i}"] = torch.cat([o[1][i] for o in outs])
    os.makedirs(out_dir, exist_ok=True)
    left = budget_bytes // 4
    names = sorted(arrays, key=lambda k: arrays[k].numel())
    for k, name in enumerate(names):
        x = arrays[name].detach().to("cpu", torch.float32)
        share = left // (len(names) - k)
        if x.numel() > share:
            idx = torch.randperm(x.numel(), generator=torch.Generator().manual_seed(0))[:share].sort().values
            x = x.reshape(-1)[idx]
        left -= x.numel()
        np.save(os.path.join(out_dir, name + ".npy"), x.numpy())
    return names


class PowerSampler:
    """Package power of every GPU of the node (amdgpu hwmon) every 20 ms from a thread, for the `power` object of the JSON line: the step is
    bound by the package power cap, so watts x time = joules per step is the quantity a kernel change has to lower.
    The box shows all GPUs of its node; ours is the one whose power rises most over its first sample.  Any failure -> `power: null`."""

    def __init__(self):
        import glob
        import threading
        self.dirs = sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*"))
        self.files = [d + ("/power1_average" if os.path.exists(d + "/power1_average") else "/power1_input") for d in self.dirs]
        self.rows, self.on, self.stop = [], False, False
        self.first = self._read()
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def _read(self):
        out = []
        for f in self.files:
            try:
                with open(f) as fh:
                    out.append(int(fh.read().strip()) / 1e6)
            except (OSError, ValueError):
                out.append(None)
        return out

    def _run(self):
        while not self.stop:
            if self.on:
                self.rows.append(self._read())
            time.sleep(0.02)

    def summary(self, ms_per_step: float):
        self.stop = True
        try:
            if not self.files or len(self.rows) < 4:
                return None
            rows = self.rows[len(self.rows) // 4:]                 # (the sensor settles over the first samples)
            mean = [None if any(r[i] is None for r in rows) else sum(r[i] for r in rows) / len(rows) for i in range(len(self.files))]
            rise = [(-1.0 if (m is None or f0 is None) else m - f0) for m, f0 in zip(mean, self.first)]
            g = max(range(len(rise)), key=lambda i: rise[i])
            if mean[g] is None:
                return None
            cap = None
            try:
                with open(self.dirs[g] + "/power1_cap") as fh:
                    cap = int(fh.read().strip()) / 1e6
            except (OSError, ValueError):
                pass
            idle = self.first[g]
            return {"watts_under_step": round(mean[g], 1), "watts_idle_before_the_run": round(idle, 1), "cap_watts": cap,
                    "joules_per_step": round(mean[g] * ms_per_step / 1e3, 2),
                    "joules_per_step_above_idle": round((mean[g] - idle) * ms_per_step / 1e3, 2), "samples": len(rows),
                    "source": self.files[g],
                    "note": "package power sampled every 20 ms over the timed region; the step's energy above idle equals the sum of its launches' "
                            "energies measured alone (tools/energy_table.py, DESIGN.md 12.11): on this power-capped part a kernel change pays "
                            "in the step only if it lowers joules"}
        except Exception:                                          # measurement aid only: never fatal
            return None


def cpu_baseline(samples, iters: int, pairs: int):
    """The CPU oracle (PyTorch-CPU restatement of the reference path, kind='port') on the host cores: a WHOLE clip (setup + all
    `iters` iterations, mask head, upsampling) per timed run, after one short warm-up pass; the median is reported (SURVEY.md
    8d).  `samples` = [(fmaps [1,T,..], cnets, params)]: every timed run works on a DIFFERENT sample (another weight seed,
    feature seed and clip position) -- the time does not depend on the values, and each run's flows check the HIP path on
    another input (epe_vs_oracle).  Returns (record, [upsampled flows per sample])."""
    from oracle import streamflow_oracle as orc
    cores = min(usable_cores(), 64)
    torch.set_num_threads(cores)
    log(f"cpu baseline: oracle on {cores} host threads (os.cpu_count()={os.cpu_count()})")
    orc.hotpath_forward(samples[0][0], samples[0][1], samples[0][2], 1)    # untimed: thread pool start-up, first-touch page faults
    log("cpu baseline: warm-up pass done")
    times, ups = [], []
    for r, (fm, cn, prm) in enumerate(samples):
        t0 = time.perf_counter()
        u, _ = orc.hotpath_forward(fm, cn, prm, iters)
        times.append(time.perf_counter() - t0)
        ups.append(u)
        log(f"cpu baseline: run {r + 1}/{len(samples)}: {times[-1]:.1f}s for one clip, {iters} iterations")
    clip = statistics.median(times)
    return {"value": pairs / clip, "unit": "flow-fields/s", "cores": cores, "kind": "port",
            "sample": f"oracle on one whole clip per run ({pairs} flow fields, all {iters} iterations), 1 warm-up pass + "
                      f"{len(samples)} timed runs on different inputs ({', '.join('%.1f' % t for t in times)} s), median {clip:.1f} s/clip",
            "s_per_clip": clip}, ups


HARD_SEEDS = (21, 11, 12, 13, 31, 32)      # == tests/cases.py HARD_SEEDS (seed 21: hot params 21, frames 24, Twins 22 / 23)


def hard_case_epe(preset_cfg, dev, seeds=HARD_SEEDS, iters_list=(15, 4)):
    """frames -> random-init Twins_CSC features -> loop at 128 x 192 (tests/test_gpu_parity.py::test_hard_case_sweep_vs_oracle:
    ill-conditioned inputs, flows of 4-40 px) against the chained CPU oracles, on SIX weight / frame seeds, at the
    15 iterations the reference deploys (scripts/infer.sh:17) and at the 4 of the earlier rounds' reports.
    The acceptance criterion of the config-2 (fp16-activation) arithmetic class is RELATIVE -- EPE <= 1e-3 of max(1, mean flow) --
    not the absolute 1e-3 px of `fp32_class`; it is stated in the record.  `worst_absolute` and `worst_relative` are each ONE
    seed's self-consistent numbers; `value` = worst_absolute at 15 iterations."""
    from oracle import streamflow_oracle as orc, twins_oracle as two
    from streamflow_amd import synthetic as syn
    from streamflow_amd.engine import HotPathEngine
    B, T, H, W = 1, 4, 128, 192
    per = {it: [] for it in iters_list}
    for seed in seeds:
        ps, fs, a, b = (21, 24, 22, 23) if seed == 21 else (seed, 100 + seed, 200 + seed, 300 + seed)
        hot = syn.make_params(ps, T)
        frames = torch.stack([(syn.randn(fs, f"frame{t}", (B, 3, H, W)).sigmoid() * 255.0) for t in range(T)], dim=1)
        imgs = 2 * (frames / 255.0) - 1.0
        fm = two.twins_csc_forward(imgs, syn.make_twins_params(a))
        cn = two.twins_csc_forward(imgs[:, :-1], syn.make_twins_params(b))
        eng = HotPathEngine(hot, device=dev, T=T, **preset_cfg)
        for it in iters_list:
            ups_o, _ = orc.hotpath_forward(fm, cn, hot, it)
            ups, _ = eng.forward(fm.to(dev).contiguous(), cn.to(dev).contiguous(), iters=it)
            e = max(orc.epe(u.cpu(), o) for u, o in zip(ups, ups_o))
            mag = float(torch.stack([o.norm(dim=1).mean() for o in ups_o]).mean())
            per[it].append({"seed": seed, "epe_px": e, "mean_flow_px": round(mag, 2), "relative_to_flow": e / max(mag, 1e-9)})
        del eng

    def summary(rows):
        wa = max(rows, key=lambda p: p["epe_px"])
        wr = max(rows, key=lambda p: p["relative_to_flow"])
        return {"worst_absolute": wa, "worst_relative": wr,
                "within_1e-3_of_max(1,flow)": all(p["epe_px"] <= 1e-3 * max(1.0, p["mean_flow_px"]) for p in rows),
                "within_1e-3_px_absolute": all(p["epe_px"] <= 1e-3 for p in rows), "seeds": rows}

    first = summary(per[iters_list[0]])
    out = {"value": first["worst_absolute"]["epe_px"], "unit": "px", "iterations": iters_list[0],
           "criterion": "config-2 presets (fp16 activations in every product): EPE <= 1e-3 x max(1, mean flow px) per seed -- a RELATIVE "
                        "bound, weaker than north_star's absolute 1e-3 px, which only the fp32_class preset meets on this input class",
           **first}
    for it in iters_list[1:]:
        out[f"at_{it}_iterations"] = summary(per[it])
    out["note"] = ("six weight / frame seeds: exact (oracle) Twins_CSC features of random frames, 128 x 192; HIP loop vs the CPU oracle loop; "
                   "worst_absolute / worst_relative are each one seed's own numbers")
    return out


def mfma_busy_from_profiles(kernel_family):
    """SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE x 128 SIMD-cycles per count) of the dominant family from the newest
    committed profiles/rNN*mfma_busy*.json (written by tools/pmc_mfma_json.py from a rocprofv3 --pmc pass), or None."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*mfma_busy*.json")))
    if not files:
        return None
    try:
        with open(files[-1]) as f:
            d = json.load(f)
        v = d.get(kernel_family)
        if v is None:
            return None
        if d.get("_csrc_sha") != csrc_sha():
            return {"value": None, "source": os.path.relpath(files[-1], ROOT),
                    "note": f"taken on other kernel sources (csrc hash {d.get('_csrc_sha')} != {csrc_sha()}): not quoted"}
        return {"value": v, "source": os.path.relpath(files[-1], ROOT)}
    except (OSError, ValueError):
        return None


def csrc_sha() -> str:
    """Hash of the kernel sources (streamflow_amd/csrc/*.hip, *.h): PMC traffic files are only valid for the sources they were
    profiled on (tools/traffic_json.py stores it as _csrc_sha)."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "streamflow_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "streamflow_amd", "csrc", "*.h"))):
        with open(f, "rb") as fh:
            h.update(os.path.basename(f).encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def newest_traffic_file(workload=None):
    """profiles/rNN*traffic*.json of the latest round (names sort by round), preferring the file taken on `workload`;
    None if there is none."""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]*traffic*.json")))
    if workload:
        mine = [f for f in files if workload in os.path.basename(f)]
        newest = files[-1][len(os.path.join(ROOT, "profiles", "")):][:3] if files else ""
        mine = [f for f in mine if os.path.basename(f).startswith(newest)]
        if mine:
            return mine[-1]
    return files[-1] if files else None


pinned_device_env = launch.pinned_device_env


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n: int, argv, script: str = None) -> int:
    """`python bench.py --gpus N` typed directly: start one child process per GPU (RANK/LOCAL_RANK/WORLD_SIZE/
    MASTER_* in its environment, exactly what torch.distributed.run would set) BEFORE this process has touched the
    GPU, wait for them, return the worst exit code.  Rank 0 inherits stdout and prints the one JSON line."""
    port = _free_port()
    procs = []
    # pin = visible (default; --pin / SF_BENCH_PIN): every child sees exactly ONE device (HIP_VISIBLE_DEVICES = its local rank,
    # set before the child initialises the GPU: SURVEY.md 8e) and uses device index 0; index: all devices visible, device index
    # = LOCAL_RANK.  Each child also takes its own share of the host cores when it starts (launch.pin_rank_cpus above).
    pin = os.environ.get("SF_BENCH_PIN", "visible")
    for a, b in zip(argv, list(argv)[1:] + [""]):
        if a == "--pin":
            pin = b
        elif a.startswith("--pin="):
            pin = a.split("=", 1)[1]
    if "--share-device" in argv:
        pin = "index"                               # (dry runs on fewer devices than ranks)
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        if pin == "visible":
            env.update(pinned_device_env(r, os.environ.get("HIP_VISIBLE_DEVICES")))
            env["SF_BENCH_OUTER_VISIBLE"] = os.environ.get("HIP_VISIBLE_DEVICES", "")
        procs.append(subprocess.Popen([sys.executable, script or os.path.abspath(__file__)] + list(argv), env=env))
    rc = 0
    try:
        pending = list(procs)
        while pending:
            for p in list(pending):
                code = p.poll()
                if code is None:
                    continue
                pending.remove(p)
                if code != 0:                      # one rank failed: the others would hang in the next barrier
                    rc = rc or code
                    for q in pending:
                        q.terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc


def corr_only(args, dev, cfg, H, W, T, iters):
    """BASELINE.json config 3: the all-pairs volume + pyramid build and the pyramid lookups alone.
    One step = one build of every (clip, pair) volume + `iters` lookups at fresh sub-pixel coordinates (the ratio of the
    real loop).  Bytes are the algorithmic ones of section 8(d): build = both feature maps read once + every pyramid cell
    written once; lookup = 4 levels x 10 x 10 footprint cells + coordinates + 324 fp32 output channels per pixel."""
    from streamflow_amd import ops, synthetic as syn
    from streamflow_amd.ops import Planes
    h, w, B, pairs, D = H // 8, W // 8, args.clips, T - 1, 256
    N, n = h * w, args.clips * (T - 1)
    f16 = cfg["corr_dtype"] == "f16"
    cx = ops.Ctx(precision=ops._PRECISION_NAMES[cfg["precision"]], shadows=False)
    fmaps = syn.make_features(1000, B, T, h, w)[0].to(dev)
    pitch = None if f16 else ops.corr_pitch(h, w)             # fp32 maps: line-aligned rows (KITTI), as the engine lays them out
    if args.dense_volumes:
        pitch = None
    strides = [N * (h >> l) * (pitch[l] if pitch else (w >> l)) for l in range(4)]
    blocked32 = (not f16) and args.corr_layout == "blocked"
    if f16:                # the shipped fp16 path: blocked volumes, features handed over as fp16 k-octets only (engine.py)
        vol = ops.new_blocked_volume(n, h, w, dev)
        ws = torch.empty(max(ops.corr_build_blocked_ws_bytes(n, D, h, w), 16), dtype=torch.uint8, device=dev)
    elif blocked32:        # fp32 cells in 4-row x 8-column cache-line blocks (csrc/corr_blocked32.hip)
        vol = ops.new_blocked_volume(n, h, w, dev, f32=True)
        ws = torch.empty(max(ops.corr_build_blocked_ws_bytes(n, D, h, w, True), 16), dtype=torch.uint8, device=dev)
        pitch = None
    else:
        lvls = [torch.empty(n * s, dtype=torch.float32, device=dev) for s in strides]
        ws = torch.empty(max(ops.corr_build_ws_bytes(B, pairs, D, h, w), 16), dtype=torch.uint8, device=dev)
    g = torch.Generator().manual_seed(7)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys])[None]                                        # (x, y) like coords_grid (utils.py)
    if args.corr_lookups >= 0:                      # experiments: a different build : lookup ratio (0 = builds alone)
        iters = args.corr_lookups
    coords = [Planes.of((grid + 4.0 * torch.randn(n, 2, h, w, generator=g)).reshape(n, 2, N).contiguous().to(dev))
              for _ in range(iters)]
    out = Planes.of(torch.empty(n, 324, N, device=dev))
    out_k = ops.new_shadow(out, dev) if f16 else None

    def step():
        if f16:
            ops.corr_build_blocked(fmaps.data_ptr(), fmaps.data_ptr() + 4 * D * N, T * D * N, D * N, vol, B, pairs, D, ws=ws)
            for c in coords:
                ops.corr_lookup_blocked(vol, c, None, out_k, B, pairs)
            return
        if blocked32:
            ops.corr_build_blocked(fmaps.data_ptr(), fmaps.data_ptr() + 4 * D * N, T * D * N, D * N, vol, B, pairs, D, ws=ws)
            for c in coords:
                ops.corr_lookup_blocked(vol, c, out, None, B, pairs)
            return
        ops.corr_build(fmaps.data_ptr(), fmaps.data_ptr() + 4 * D * N, T * D * N, D * N, lvls, strides, B, pairs, D, h, w,
                       ws=ws, cx=cx, pitch=pitch)
        for c in coords:
            ops.corr_lookup(lvls, strides, c, out, B, pairs, h, w, cx=cx, pitch=pitch)

    # a 2-ms step is short against the one-off ~50-ms stall the HIP runtime takes somewhere in a process's first few hundred launches
    # (tools/corr32_probe.py: GPU time per step unchanged, the wait sits on the host): let it happen before the W warm-up steps
    settle = 30
    for _ in range(settle):
        step()
    torch.cuda.synchronize()
    dt = timed_steps(step, args.steps, args.warmup, 1, torch.cuda.synchronize, lambda: None, lambda x: x)
    ops.PROFILER = ops.Profiler()
    step()
    prof = ops.PROFILER.summary()
    ops.PROFILER = None
    b, l = prof["corr_build"], prof.get("corr_lookup", {"bytes": 0.0, "ms": 0.0, "launches": 1})
    gb = lambda d: d["bytes"] / d["ms"] / 1e6 if d["ms"] else 0.0
    tot_bytes, tot_ms = b["bytes"] + l["bytes"], b["ms"] + l["ms"]
    cell = 2 if f16 else 4
    return {
        "metric": "corr_build_lookup_gbps", "value": tot_bytes / (1e3 * dt / args.steps) / 1e6, "unit": "GB/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": ("fp16 cells (blocked layout, k-octet feature hand-over), single f16 product" if f16 else
                                        "fp32 cells (cache-line blocks of 4 rows x 8 columns), f16x3 arithmetic" if blocked32 else f"fp32 cells, {cfg['precision']} arithmetic"),
        "data": "synthetic",
        "config": {"workload": f"{args.workload}_{H}x{W}_T{T}_corr_only", "clips_per_step": B, "pairs_per_clip": pairs,
                   "feature_grid": [h, w], "lookups_per_step": iters, "untimed_settle_steps_before_warmup": settle,
                   "volume_bytes_per_pair": vol.img_stride if (f16 or blocked32) else cell * sum(strides),
                   "map_row_pitch_cells": ("blocked" if (f16 or blocked32) else list(pitch) if pitch else "dense (the reference's [N, h_l, w_l])"),
                   "preset": args.preset or "default"},
        "roofline": {"kernel": "corr_build + corr_lookup", "bound": "hbm", "achieved": tot_bytes / tot_ms / 1e6,
                     "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": tot_bytes / tot_ms / 1e6 / PEAK_HBM_GBPS, "traffic": None,
                     "build": {"avg_us": 1e3 * b["ms"] / b["launches"], "gbps": gb(b), "tflops": b["flops"] / b["ms"] / 1e9,
                               "algorithmic_bytes": b["bytes"] / b["launches"]},
                     "lookup": {"avg_us": 1e3 * l["ms"] / l["launches"], "gbps": gb(l),
                                "algorithmic_bytes": l["bytes"] / l["launches"]},
                     "method": "HIP events around every launch of one instrumented step on the launch stream; bytes of SURVEY.md "
                               "section 8(d) at the element size of the stored volume"},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="sintel", choices=list(WORKLOADS))
    ap.add_argument("--total-clips", type=int, default=0,
                    help="STRONG scaling: this many clips in total per step at every --gpus N (BASELINE.json config 4: 64), "
                         "round-robined over the ranks and run in launches of --clips; 0 (default) = weak scaling, "
                         "--clips per GPU per step")
    ap.add_argument("--pin", default=os.environ.get("SF_BENCH_PIN", "visible"), choices=["index", "visible"],
                    help="how a rank takes its GPU: visible (default) = HIP_VISIBLE_DEVICES restricted to its one device "
                         "before the runtime starts (SURVEY.md 8e); index = cuda:LOCAL_RANK with every device visible")
    ap.add_argument("--clips", type=int, default=8,
                    help="clips per GPU per step, batched through every launch (default 8 = the per-GPU share of "
                         "BASELINE.json's 8-GPU 'Sintel-shape batch=64' configuration; 1 = single-clip latency)")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of HIP-graph replay")
    ap.add_argument("--all-masks", action="store_true",
                    help="run the mask head every iteration as the reference literally does (outputs identical; "
                         "the default skips the 14 mask heads whose results test_mode discards)")
    ap.add_argument("--preset", default=None, choices=["config2_mixed", "config2_fp16", "fp32_class"],
                    help="named arithmetic configuration (streamflow_amd/presets.py); default = presets.BENCH_PRESET.  config2_fp16 = "
                         "BASELINE.json configuration 2 ('bf16'): activations fp16 into split-precision weights, fp16 correlation "
                         "volumes, fused fp16 GMA aggregation, fp32 accumulation everywhere; config2_mixed = the same with single "
                         "fp16 weights in the layers where that was measured invisible; fp32_class = the library default (split "
                         "precision everywhere, fp32 volumes).  --precision / --corr-dtype / --gma override")
    ap.add_argument("--precision", default=None, choices=["f16x3", "fp32", "f16x2", "f16"],
                    help="f16x3: split-fp16 MFMA with fp32 accumulation (fp32-class accuracy); fp32: exact fp32 MFMA; "
                         "f16x2: weights split, activations rounded once to fp16")
    ap.add_argument("--gma", default=None, choices=["auto", "matrix", "flash", "stored", "hybrid"], help="GMA aggregation path (engine gma_mode)")
    ap.add_argument("--flash-qkp", type=int, default=None, choices=[1, 2, 3], help="MFMA products per logit of the fused GMA kernel")
    ap.add_argument("--corr-dtype", default=None, choices=["f16", "f32"],
                    help="storage of the correlation pyramids: f16 = fp16 cells built with single f16 MFMA products "
                         "(BASELINE.json config 2: 'bf16 corr build+lookup'); f32 = fp32 cells as the reference keeps "
                         "them, built in --precision arithmetic")
    ap.add_argument("--gemm-shapes", action="store_true", help="per-shape GEMM rows in the kernel table")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend for the barrier / max-over-ranks (nccl = RCCL; gloo for dry runs)")
    ap.add_argument("--share-device", action="store_true",
                    help="dry-run aid: map every rank to cuda:LOCAL_RANK %% device_count (use with --dist-backend gloo)")
    ap.add_argument("--serial-branches", action="store_true",
                    help="enqueue the independent chains of an iteration on one stream (profiling aid: kernel-trace "
                         "durations are then free of cross-branch contention and match the HIP-event table)")
    ap.add_argument("--streams", type=int, default=1,
                    help="experiment: split the clips of a step over S engines replayed concurrently on S streams "
                         "(fills the partial last round of one engine's launches with the other's workgroups)")
    ap.add_argument("--corr-only", action="store_true",
                    help="BASELINE.json config 3: ONLY the correlation build (all-pairs volume + 4-level pyramid) and the "
                         "pyramid lookups of the workload (one build + `iters` lookups per step), reported in GB/s against "
                         "the HBM roof; use with --workload kitti --preset fp32_class for the full-resolution fp32 volume")
    ap.add_argument("--placement-only", default=None, metavar="DIR",
                    help="dry run of the rank placement: every rank writes {rank, device environment, host cores} to DIR/rankN.json "
                         "and exits before touching the GPU (tests/test_distributed_cpu.py)")
    ap.add_argument("--dense-volumes", action="store_true",
                    help="--corr-only, fp32 volumes: keep the reference's dense [N, h_l, w_l] maps instead of line-aligned row pitches")
    ap.add_argument("--corr-lookups", type=int, default=-1, help="--corr-only: lookups per step (default: the workload's iterations)")
    ap.add_argument("--corr-layout", default="blocked", choices=["blocked", "rows"],
                    help="fp32 volumes (--corr-only and the fp32_class engine): cache-line blocks (csrc/corr_blocked32.hip) or the "
                         "reference's row-major maps with line-aligned row pitches (csrc/corr.hip)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline steps, also measure everything else of the JSON record: package power, the sustained "
                         "clock, the per-kernel table and rooflines, the CPU oracle baseline and EPE checks, the other presets, the "
                         "single-clip latency and frames -> flows (a plain run times the steps and prints the headline line only)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the flows the last timed step returned as DIR/<name>.npy (float32; a fixed, "
                         "seeded sample of the larger fields, at most 48 MB in all) to compare two builds output for output")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU oracle baseline and the EPE checks")
    ap.add_argument("--cpu-runs", type=int, default=3, help="timed whole-clip runs of the CPU oracle (median reported)")
    ap.add_argument("--no-kernel-breakdown", action="store_true",
                    help="--full: skip the clock probe, the per-kernel table, the other presets, single clip and frames -> flows")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and args.corr_only:
        ap.error("--dump-outputs writes the flows of the hot path; --corr-only has none")
    if not args.full:
        args.no_kernel_breakdown = args.no_cpu_baseline = True

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # typed as `python bench.py --gpus N`: this process becomes the launcher.  Nothing above has initialised the
        # GPU (importing torch does not), and nothing below runs here: the ranks are children, never an exec.
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))
    if args.gpus > 1 and world == 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE=1")
    if args.placement_only:
        with open(os.path.join(args.placement_only, f"rank{rank}.json"), "w") as f:
            json.dump({"rank": rank, "local_rank": local_rank, "world": world, "cpus": sorted(os.sched_getaffinity(0)),
                       "HIP_VISIBLE_DEVICES": os.environ.get("HIP_VISIBLE_DEVICES"), "SF_BENCH_DEVICE": os.environ.get("SF_BENCH_DEVICE"),
                       "torch_threads": torch.get_num_threads()}, f)
        return
    if args.pin == "visible" and world > 1 and "SF_BENCH_DEVICE" not in os.environ and not args.share_device:
        # under an external launcher: restrict this rank to its device now -- nothing has initialised the GPU yet
        os.environ["SF_BENCH_OUTER_VISIBLE"] = os.environ.get("HIP_VISIBLE_DEVICES", "")
        os.environ.update(pinned_device_env(local_rank, os.environ.get("HIP_VISIBLE_DEVICES")))
    if "SF_BENCH_DEVICE" in os.environ and not args.share_device:
        local_rank = int(os.environ["SF_BENCH_DEVICE"])
    # (first power reading = the idle draw: before this process touches the GPU)
    power = PowerSampler() if (world == 1 and not args.corr_only and args.full) else None
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs"
    if args.share_device:
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        if args.dist_backend == "nccl":
            # RCCL carries only the barrier and the max-over-ranks of the timing (no data-path collective)
            dist.init_process_group("nccl", device_id=dev, timeout=datetime.timedelta(seconds=600))
        else:
            # gloo announces its connections on stdout; rank 0's stdout must carry exactly one JSON line
            sys.stdout.flush()
            keep = os.dup(1)
            os.dup2(2, 1)
            try:
                dist.init_process_group("gloo")
                dist.barrier()
            finally:
                sys.stdout.flush()
                os.dup2(keep, 1)
                os.close(keep)

    from streamflow_amd import ops, presets, synthetic as syn
    from streamflow_amd.engine import HotPathEngine
    cfg = presets.engine_kwargs(args.preset or presets.BENCH_PRESET)
    if args.precision:
        cfg["precision"] = args.precision
    if args.corr_dtype:
        cfg["corr_dtype"] = args.corr_dtype
    if args.gma:
        cfg["gma_mode"] = args.gma
    if args.flash_qkp:
        cfg["flash_qk_products"] = args.flash_qkp
    if cfg["precision"] == "fp32" and cfg["gma_mode"] == "flash":
        cfg["gma_mode"] = "auto"                       # the exact fp32 mode keeps the materialised attention path
    args.precision, args.corr_dtype = cfg["precision"], cfg["corr_dtype"]
    if args.corr_layout == "rows":                      # fp32 volumes as the reference's row-major maps (A/B of csrc/corr_blocked32.hip)
        from dataclasses import replace as _replace
        from streamflow_amd.engine import EngineOptions
        cfg["options"] = _replace(cfg.get("options") or EngineOptions(), corr_blocked32=False)

    H, W, T, iters = WORKLOADS[args.workload]
    h, w, B = H // 8, W // 8, args.clips
    pairs = T - 1
    if args.corr_only:
        assert world == 1, "--corr-only is a single-GPU line"
        print(json.dumps(corr_only(args, dev, cfg, H, W, T, iters)), flush=True)
        return
    params = syn.make_params(0, T)
    strong = args.total_clips > 0
    my_batches = batches(len(shard(args.total_clips, world, rank)), B) if strong else [B]
    fmaps_c, cnets_c = syn.make_features(1000 + rank, B, T, h, w)
    fmaps, cnets = fmaps_c.to(dev), cnets_c.to(dev)
    eng = HotPathEngine(params, device=dev, T=T, use_graph=not args.no_graph, **cfg)
    if args.serial_branches:
        eng.parallel_branches = False
    if strong:
        args.no_kernel_breakdown = args.no_cpu_baseline = True          # (the N = 1 weak-scaling line carries those)
        assert args.streams == 1, "--total-clips and --streams exclude each other"

    # what the forwards of the latest step returned (views into engine buffers; --dump-outputs reads them after the timed steps)
    last = []
    if args.streams > 1:
        assert B % args.streams == 0, "--clips must be a multiple of --streams"
        args.no_kernel_breakdown = args.no_cpu_baseline = True
        bs = B // args.streams
        engs = [HotPathEngine(params, device=dev, T=T, use_graph=not args.no_graph, **cfg) for _ in range(args.streams)]
        strs = [torch.cuda.Stream(device=dev) for _ in range(args.streams)]
        parts = [(fmaps[i * bs:(i + 1) * bs].contiguous(), cnets[i * bs:(i + 1) * bs].contiguous()) for i in range(args.streams)]

        def step():
            cur = torch.cuda.current_stream()
            outs = []
            for e, st, (f, c) in zip(engs, strs, parts):
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    outs.append(e.forward(f, c, iters=iters, all_masks=args.all_masks))
            for st in strs:
                cur.wait_stream(st)
            last[:] = outs
    elif strong:
        # one input set per distinct launch size (the same synthetic clips every launch: timing does not depend on the values)
        feats = {b: (fmaps[:b].contiguous(), cnets[:b].contiguous()) for b in set(my_batches)}

        def step():
            last[:] = [eng.forward(*feats[b], iters=iters, all_masks=args.all_masks) for b in my_batches]
    else:
        def step():
            last[:] = [eng.forward(fmaps, cnets, iters=iters, all_masks=args.all_masks)]

    def barrier():
        if world > 1:
            dist.barrier()

    def allreduce_max(x: float) -> float:
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev if args.dist_backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    log(f"rank {rank}/{world}: engine ready, workload {args.workload}, graph={not args.no_graph}")
    step()
    torch.cuda.synchronize()
    log("first step done (includes graph capture)")
    own = []
    if power is not None:
        power.on = True
    dt = timed_steps(step, args.steps, args.warmup, world, torch.cuda.synchronize, barrier, allreduce_max, own=own)
    if power is not None:
        power.on = False
    log(f"timed region: {args.steps} steps in {dt:.3f}s (this rank: {own[0]:.3f}s)")
    if args.dump_outputs and rank == 0:
        # before anything else runs on these engines: their returned flows are views into buffers the next forward overwrites
        log(f"outputs of the last timed step: {', '.join(dump_outputs(last, args.dump_outputs))} -> {args.dump_outputs}")
    per_rank, rank_cores, rank_host, rank_host_cpu = [own[0]], [len(RANK_CPUS)], [own[1]], [own[2]]
    pl0 = next(reversed(eng._plans.values())) if eng._plans else None
    graph_calls = [int(getattr(pl0, "graph_calls", 0) or 0)]
    if world > 1:
        t_own = torch.tensor([own[0], float(len(RANK_CPUS)), own[1], float(graph_calls[0]), own[2]], dtype=torch.float64,
                             device=dev if args.dist_backend == "nccl" else "cpu")
        t_all = [torch.zeros_like(t_own) for _ in range(world)]
        dist.all_gather(t_all, t_own)
        per_rank = [float(t[0].item()) for t in t_all]
        rank_cores = [int(t[1].item()) for t in t_all]
        rank_host = [float(t[2].item()) for t in t_all]
        graph_calls = [int(t[3].item()) for t in t_all]
        rank_host_cpu = [float(t[4].item()) for t in t_all]
    if pl0 is not None and getattr(pl0, "auto_stored", False):
        gma_note = (" -> softmax weights stored once per clip and streamed (engine default for grids of >= %d px and for split-precision "
                    "logits; same results)" % eng.options.stored_auto_px)
    else:
        gma_note = ""
    clips_all = args.total_clips if strong else world * B
    fields = clips_all * pairs * args.steps
    result = {
        "metric": "flow_fields_per_sec", "value": fields / dt, "unit": "flow-fields/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
        "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
        "per_rank_ms_per_step": [round(1e3 * t / args.steps, 3) for t in per_rank],
        # spread of the ranks' own times (each up to its device sync, before the closing barrier) relative to their mean: what
        # the slowest rank costs the job
        "imbalance": round((max(per_rank) - min(per_rank)) / (sum(per_rank) / len(per_rank)), 4),
        # SCALE diagnostics: the WALL time each rank's host thread spends inside a step (input staging copies + ONE graph
        # launch, or the eager enqueues; the runtime launches a graph's nodes from the calling thread and blocks while the hardware
        # queues are full, so this follows the GPU time) and its CPU time alone -- if host_cpu approaches ms_per_step at N = 8 the
        # ranks are host-bound, not GPU-bound -- and the size of the replayed graph (launch calls captured per forward)
        "power": power.summary(1e3 * dt / args.steps) if power is not None else None,
        "host_ms_per_step": [round(1e3 * t / args.steps, 3) for t in rank_host],
        "host_cpu_ms_per_step": [round(1e3 * t / args.steps, 3) for t in rank_host_cpu],
        "graph_launch_calls": graph_calls,
        "dtype": {"fp32": "fp32", "f16x3": "f16x3-split (fp32 accumulate)",
                  "f16x2": ("f16x2 (weights hi+lo, activations fp16; fp32 accumulate)" if not cfg.get("single_layers") else
                            f"f16x2 / f16 mixed (activations fp16; weights fp16 in {len(cfg['single_layers'])} of the 45 "
                            f"contraction / depthwise layers, hi+lo in the rest; fp32 accumulate)"),
                  "f16": "f16 (weights and activations fp16; fp32 accumulate)"}[args.precision] +
                 ("; fp16 correlation volumes" if args.corr_dtype == "f16" else ""), "data": "synthetic",
        "config": {"workload": f"{args.workload}_{H}x{W}_T{T}_iters{iters}",
                   "clips_per_gpu_per_step": (B if not strong else None), "clips_per_launch": B,
                   "clips_per_step_all_gpus": clips_all,
                   "clips_per_rank": ([len(shard(args.total_clips, world, r)) for r in range(world)] if strong else [B] * world),
                   "device_pinning": args.pin if world > 1 else "single device",
                   "host_cores_per_rank": rank_cores,
                   "flow_fields_per_clip": pairs, "feature_grid": [h, w], "parallelism": f"replicas{world}",
                   "hip_graph": not args.no_graph, "mask_head_every_iteration": bool(args.all_masks),
                   "preset": args.preset or presets.BENCH_PRESET,
                   "corr_volume": {"f16": "fp16 cells, single f16 MFMA product, fp32 accumulate",
                                   "f32": "fp32 cells"}[args.corr_dtype],
                   "gma": f"{eng.gma_mode}" + (f" (fused recompute, {eng.flash_qk_products} MFMA product(s) per logit)"
                                                if eng.gma_mode == "flash" else
                                                f" (softmax weights stored once per clip as fp16, {eng.flash_qk_products} MFMA product(s) per "
                                                f"logit; streamed every iteration)" if eng.gma_mode == "stored" else "") + gma_note,
                   "precision": {"fp32": "exact fp32 (v_mfma_f32_32x32x2_f32)",
                                 "f16x3": "split fp16x3 (x=hi+lo, 3x v_mfma_f32_32x32x16_f16, fp32 accumulate)",
                                 "f16x2": "weights hi+lo fp16, activations fp16 (2x v_mfma_f32_32x32x16_f16)" +
                                          (f"; single fp16 weights (1x) in {len(cfg['single_layers'])} of 45 layers"
                                           if cfg.get("single_layers") else ""),
                                 "f16": "weights fp16, activations fp16 (1x v_mfma_f32_32x32x16_f16)"}[args.precision]},
    }

    # The clock the chip SUSTAINS under this step (MI355X clocks to its power budget): a second engine with the same configuration
    # forks a one-wave probe (sf_clock_probe: shader-cycle counter against the constant 100 MHz counter) as a BRANCH of its captured
    # graph for 80 % of the step (a probe launched from another stream beside a graph replay shared a hardware queue with it and ran
    # before or after it); the same probe on the idle device next to it.  Quoted beside the roofline, which prices the matrix-core
    # roof at the guide's 2.4 GHz.
    clock = None
    if rank == 0 and not args.no_kernel_breakdown and args.streams == 1 and not strong:
        from streamflow_amd.engine import EngineOptions
        t_step = dt / args.steps
        peng = HotPathEngine(params, device=dev, T=T, use_graph=not args.no_graph,
                             **dict(cfg, options=replace(cfg.get("options") or EngineOptions(), clock_probe_us=int(1e6 * 0.8 * t_step))))
        for _ in range(3):
            peng.forward(fmaps, cnets, iters=iters, all_masks=args.all_masks)
        torch.cuda.synchronize()
        t_sec = time.perf_counter()
        reads = []
        for _ in range(4):
            peng.forward(fmaps, cnets, iters=iters, all_masks=args.all_masks)
            torch.cuda.synchronize()
            c = [int(v) for v in peng.clock_counts.tolist()]
            reads.append(100.0 * c[0] / max(c[1], 1))
        t_sec = (time.perf_counter() - t_sec) / 4
        time.sleep(0.5)
        idle = torch.zeros(2, dtype=torch.int64, device=dev)
        ops.clock_probe(idle, 20000)
        torch.cuda.synchronize()
        ci = [int(v) for v in idle.tolist()]
        clock = {"sustained_mhz": round(statistics.median(reads), 1), "reads_mhz": [round(r, 1) for r in reads],
                 "idle_probe_mhz": round(100.0 * ci[0] / max(ci[1], 1), 1), "max_mhz": PEAK_CLOCK_MHZ,
                 "probed_step_ms": round(1e3 * t_sec, 2),
                 "method": "sf_clock_probe (shader cycles / 100 MHz ticks) as a branch of the step's own graph for 80 % of the step, 4 "
                           "steps, median; probed_step_ms = that engine's step (the timed engine has no probe); idle = the same probe alone "
                           "for 20 ms after 0.5 s of rest"}
        del peng
        log(f"clock under the step: {clock['sustained_mhz']} MHz (idle probe {clock['idle_probe_mhz']} MHz)")

    if rank == 0 and not args.no_kernel_breakdown:
        # instrumented eager pass: HIP events around every launch on the launch stream
        eager = HotPathEngine(params, device=dev, T=T, use_graph=False, **cfg)
        eager._plans = eng._plans                       # reuse buffers
        eager.parallel_branches = False                 # serial launches: clean per-kernel durations
        ops.PROFILE_SHAPES = True                          # GEMM launches by layer shape (folded into one family row below)
        eager.forward(fmaps, cnets, iters=iters, all_masks=args.all_masks)
        reps = 2
        ops.PROFILER = ops.Profiler()
        for _ in range(reps):
            eager.forward(fmaps, cnets, iters=iters, all_masks=args.all_masks)
        summ = ops.PROFILER.summary()
        ops.PROFILER = None
        log("instrumented pass done")
        kern = {}
        for name, d in summ.items():
            ms = d["ms"] / reps
            kern[name] = {"launches_per_step": d["launches"] // reps, "ms_per_step": round(ms, 4),
                          "avg_us": round(1e3 * ms / max(d["launches"] // reps, 1), 2),
                          "tflops": round(d["flops"] / reps / (ms * 1e-3) / 1e12, 2) if d["flops"] else None,
                          "gbps_algorithmic": round(d["bytes"] / reps / (ms * 1e-3) / 1e9, 1) if d["bytes"] else None}
        result["kernels"] = kern
        # fold the per-shape rows into one family row (the per-shape rows stay in `kernels` with --gemm-shapes only)
        famk = [k for k in kern if k.startswith("gemm M")]
        if famk:
            ms = sum(kern[k]["ms_per_step"] for k in famk)
            fl = sum(summ[k]["flops"] for k in famk) / reps
            by = sum(summ[k]["bytes"] for k in famk) / reps
            nl = sum(kern[k]["launches_per_step"] for k in famk)
            kern["gemm"] = {"launches_per_step": nl, "ms_per_step": round(ms, 4), "avg_us": round(1e3 * ms / max(nl, 1), 2),
                            "tflops": round(fl / (ms * 1e-3) / 1e12, 2), "gbps_algorithmic": round(by / (ms * 1e-3) / 1e9, 1)}
            if not args.gemm_shapes:
                for k in famk:
                    del kern[k]
        dom = max((k for k in kern if not k.startswith("gemm M")), key=lambda k: kern[k]["ms_per_step"])
        # HBM traffic of every family from the committed rocprofv3 PMC passes (bench.py cannot run the profiler on itself): newest
        # profiles/rNN*traffic.json -- used ONLY when it was taken on this configuration AND on this kernel source (csrc hash)
        traffic, tfile, traffic_why = {}, newest_traffic_file(args.workload), None
        if tfile:
            try:
                with open(tfile) as f:
                    traffic = json.load(f)
            except (OSError, ValueError):
                traffic = {}
        same = bool(traffic) and (
            traffic.get("_workload", "sintel") == args.workload and int(traffic.get("_clips", 8)) == B and
            traffic.get("_corr_dtype", "f32") == args.corr_dtype and traffic.get("_precision", "f16x3") == args.precision and
            traffic.get("_preset", args.preset or presets.BENCH_PRESET) == (args.preset or presets.BENCH_PRESET))
        if not traffic:
            traffic_why = "no profiles/r*traffic*.json for this workload"
        elif not same:
            traffic_why = f"{os.path.relpath(tfile, ROOT)} was taken on another configuration"
        elif traffic.get("_csrc_sha") != csrc_sha():
            same, traffic_why = False, (f"{os.path.relpath(tfile, ROOT)} was taken on other kernel sources (csrc hash "
                                        f"{traffic.get('_csrc_sha')} != {csrc_sha()}): re-run tools/r05/profiles.sh")

        def pmc_bytes_of(name):
            fam = traffic.get(name) if same else None
            return int((fam["fetch_kib_per_launch"] + fam["write_kib_per_launch"]) * 1024) if fam else None

        def row(name, members):
            """Both time floors of one kernel (or family): HBM at the bytes it must move (PMC bytes where valid, else the
            algorithmic ones) and the matrix cores at the MFMA products it really ISSUES (3 / 2 / 1 per algorithmic product, per
            layer: a single-product layer is priced as one)."""
            ms = sum(summ[k]["ms"] for k in members) / reps
            n = sum(summ[k]["launches"] for k in members) // reps
            by = sum(summ[k]["bytes"] for k in members) / reps
            fl = sum(summ[k]["flops"] for k in members) / reps
            mf = sum(summ[k]["mfma_flops"] for k in members) / reps
            peak = PEAK_FP32_MFMA_TFLOPS if args.precision == "fp32" else PEAK_F16_MFMA_TFLOPS
            pmc = pmc_bytes_of(name)
            t_hbm = (pmc * n if pmc else by) / (PEAK_HBM_GBPS * 1e9)
            t_mfma = mf / (peak * 1e12)
            t = ms * 1e-3
            return {"kernel": name, "launches_per_step": n, "ms_per_step": round(ms, 4), "avg_us": round(1e3 * ms / max(n, 1), 2),
                    "algorithmic_bytes_per_launch": int(by / max(n, 1)), "algorithmic_flops_per_launch": int(fl / max(n, 1)),
                    "mfma_flops_issued_per_launch": int(mf / max(n, 1)),
                    "frac_hbm": round(by / (PEAK_HBM_GBPS * 1e9) / t, 4) if t else None,
                    "frac_mfma": round(t_mfma / t, 4) if (t and mf) else None,
                    "bound": "mfma" if t_mfma > t_hbm else "hbm",
                    "floor_us": {"hbm": round(1e6 * t_hbm / max(n, 1), 2), "mfma": round(1e6 * t_mfma / max(n, 1), 2)},
                    "traffic": pmc, "_t_hbm": t_hbm, "_t_mfma": t_mfma, "_bytes": by, "_mf": mf, "_fl": fl}

        members = {k: [k] for k in summ if not k.startswith("gemm M")}
        shape_rows = [k for k in summ if k.startswith("gemm M")]
        if shape_rows:
            members["gemm"] = shape_rows
        fam = row(dom, members[dom])
        peak_tf = PEAK_FP32_MFMA_TFLOPS if args.precision == "fp32" else PEAK_F16_MFMA_TFLOPS
        t = fam["ms_per_step"] * 1e-3
        if fam["bound"] == "mfma":
            ach = fam["_mf"] / t / 1e12
            result["roofline"] = {"kernel": dom, "bound": "mfma", "achieved": round(ach, 1), "peak": peak_tf, "unit": "TFLOP/s",
                                  "frac": round(ach / peak_tf, 4)}
        else:
            ach = fam["_bytes"] / t / 1e9
            result["roofline"] = {"kernel": dom, "bound": "hbm", "achieved": round(ach, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                                  "frac": round(ach / PEAK_HBM_GBPS, 4)}
        # the five most expensive kernels of the step, one row each (GEMM launches by layer shape): name, time, algorithmic
        # bytes / flops, the fraction of BOTH roofs
        rows = [row(k, [k]) for k in summ if k != "gemm"]
        rows.sort(key=lambda r: -r["ms_per_step"])
        strip = lambda r: {k: v for k, v in r.items() if not k.startswith("_")}
        result["roofline"].update({
            "frac_hbm": fam["frac_hbm"], "frac_mfma": fam["frac_mfma"],
            "algorithmic_tflops": round(fam["_fl"] / t / 1e12, 1), "mfma_tflops_issued": round(fam["_mf"] / t / 1e12, 1),
            "mfma_busy": mfma_busy_from_profiles(dom),
            "clock": clock,
            "frac_mfma_at_sustained_clock": (round(fam["frac_mfma"] * PEAK_CLOCK_MHZ / clock["sustained_mhz"], 4)
                                             if (clock and fam["frac_mfma"] and clock["sustained_mhz"]) else None),
            "traffic": fam["traffic"], "traffic_note": traffic_why if fam["traffic"] is None else (
                f"bytes per launch, mean over the family: 2 x FETCH_SIZE + WRITE_SIZE from separate rocprofv3 --pmc passes of this "
                f"workload on these kernel sources ({os.path.relpath(tfile, ROOT)})"),
            "launches_per_step": fam["launches_per_step"], "avg_launch_us": fam["avg_us"],
            "algorithmic_bytes_per_launch": fam["algorithmic_bytes_per_launch"],
            "floor_ms_per_step": {"mfma": round(1e3 * fam["_t_mfma"], 2), "hbm": round(1e3 * fam["_t_hbm"], 2)},
            "per_kernel": [strip(r) for r in rows[:5]],
            "method": "one instrumented step (HIP events around every launch on the launch stream), family totals: HBM floor = bytes "
                      "(PMC where valid for this source, else algorithmic: operands read once + result written once) / 8 TB/s; MFMA "
                      "floor = issued MFMA flops (algorithmic flops x products of each layer: 1 for single-weight layers, 2 for hi+lo, "
                      "3 for f16x3) / dense f16 peak; bound = the larger floor; achieved / frac are stated against that roof"})
        # north-star sub-metric: corr build + lookup against the HBM roofline (algorithmic bytes)
        cb, cl = kern.get("corr_build"), kern.get("corr_lookup")
        if cb and cl:
            tot_b = (summ["corr_build"]["bytes"] + summ["corr_lookup"]["bytes"]) / reps
            tot_ms = cb["ms_per_step"] + cl["ms_per_step"]
            result["roofline_corr"] = {"bound": "hbm", "unit": "GB/s", "peak": PEAK_HBM_GBPS,
                                       "build_gbps": cb["gbps_algorithmic"], "lookup_gbps": cl["gbps_algorithmic"],
                                       "build_tflops": cb["tflops"], "build_plus_lookup_ms_per_step": round(tot_ms, 4),
                                       "achieved": round(tot_b / (tot_ms * 1e-3) / 1e9, 1),
                                       "frac": round(tot_b / (tot_ms * 1e-3) / 1e9 / PEAK_HBM_GBPS, 4),
                                       "bytes": "SURVEY.md section 8(d), element size of the stored volume: per pair build = 2 N 256 4 + N cells e, "
                                                "lookup = N (4 100 e + 8 + 324 4) -- the k-octet hand-over and the blocked layout's padding "
                                                "are NOT counted"}
            # ... and on the bytes THIS design has to move: the blocked fp16 path hands the looked-up features
            # over as fp16 k-octets only, so its lookup writes 324 x 2 B per pixel, not section 8(d)'s 324 x 4 B; `needed` = footprints
            # (4 levels x 100 cells x e) + coordinates + the output at the size it is stored, build = features read once + cells once
            e_sz = 2 if args.corr_dtype == "f16" else 4
            out_sz = 2 if (args.corr_dtype == "f16" and eng.corr_blocked) else 4
            npx = B * pairs * h * w
            lookup_moved = npx * (4 * 100 * e_sz + 8 + 324 * out_sz) * cl["launches_per_step"]
            moved = summ["corr_build"]["bytes"] / reps + lookup_moved
            result["roofline_corr"]["moved_bytes_per_step"] = int(moved)
            result["roofline_corr"]["frac_on_moved_bytes"] = round(moved / (tot_ms * 1e-3) / 1e9 / PEAK_HBM_GBPS, 4)
            result["roofline_corr"]["moved_bytes"] = ("what this design must move: build as section 8(d); lookup = N (4 100 e + 8 + 324 x "
                                                      f"{out_sz}) -- the output at the element size it is stored in")
            if not same:
                result["roofline_corr"]["traffic"], result["roofline_corr"]["traffic_note"] = None, traffic_why
            if same and traffic.get("corr_build") and traffic.get("corr_lookup"):
                real = 1024.0 * ((traffic["corr_build"]["fetch_kib_per_launch"] + traffic["corr_build"]["write_kib_per_launch"]) * cb["launches_per_step"] +
                                 (traffic["corr_lookup"]["fetch_kib_per_launch"] + traffic["corr_lookup"]["write_kib_per_launch"]) * cl["launches_per_step"])
                result["roofline_corr"]["traffic"] = int(real)
                result["roofline_corr"]["traffic_gbps"] = round(real / (tot_ms * 1e-3) / 1e9, 1)
                result["roofline_corr"]["traffic_over_algorithmic"] = round(real / tot_b, 3)
                result["roofline_corr"]["traffic_over_needed"] = round(real / moved, 3)

    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import streamflow_oracle as orc
        # bounded sample: ONE clip per timed oracle run, each on another input: (weights, features) seeds 0 / 1 / 2 and the
        # last / first / last clip of the 8-clip batch (the last one exercises the highest image indices of the batched
        # launches).  Seed 0 is the timed workload itself.
        plan = [(0, B - 1), (1, 0), (2, B - 1)][: max(1, args.cpu_runs)]
        sets = {}
        for sd, _ in plan:
            prm = params if sd == 0 else syn.make_params(sd, T)
            fm, cn = (fmaps_c, cnets_c) if sd == 0 else syn.make_features(1000 + 17 * sd, B, T, h, w)
            sets[sd] = (fm, cn, prm)
        base, ups_cpu = cpu_baseline([(sets[sd][0][c:c + 1], sets[sd][1][c:c + 1], sets[sd][2]) for sd, c in plan], iters, pairs)
        result["cpu_baseline"] = base
        per = []
        for (sd, c), uc in zip(plan, ups_cpu):
            # seed 0: the SAME engine, plan and (graph) launch sequence the timed region used; the other seeds: the same
            # configuration with their own weights; all `iters` iterations, the whole 8-clip batch in the launch
            e_sd = eng if sd == 0 else HotPathEngine(sets[sd][2], device=dev, T=T, use_graph=not args.no_graph, **cfg)
            ups_gpu, _ = e_sd.forward(sets[sd][0].to(dev), sets[sd][1].to(dev), iters=iters, all_masks=args.all_masks)
            mag = float(torch.stack([o.norm(dim=1).mean() for o in uc]).mean())
            per.append({"seed": sd, "clip": c, "epe_px": max(orc.epe(a[c:c + 1].cpu(), b_) for a, b_ in zip(ups_gpu, uc)),
                        "mean_flow_px": round(mag, 2)})
            if sd != 0:
                del e_sd
                torch.cuda.empty_cache()
        result["epe_vs_oracle"] = {"value": max(p_["epe_px"] for p_ in per), "unit": "px", "iters": iters, "clips_in_launch": B,
                                   "samples": per,
                                   "note": "max over the samples (weight / feature seeds x first and last clip of the batch) of the "
                                           "max over the pairs of the mean EPE: HIP path (batched launch sequence; seed 0 = the "
                                           "timed engine itself) vs CPU oracle, full shape, all iterations"}
        try:
            result["epe_hard_case"] = hard_case_epe(cfg, dev)
        except RuntimeError as e:
            result["epe_hard_case"] = {"error": str(e)[:200]}

    if rank == 0 and world == 1 and not args.no_kernel_breakdown and cfg == presets.engine_kwargs(presets.BENCH_PRESET):
        for other in ("config2_fp16",):
            # the all-split-weights form of the same arithmetic class (round 2's headline preset), same run, same box
            try:
                o_eng = HotPathEngine(params, device=dev, T=T, use_graph=not args.no_graph, **presets.engine_kwargs(other))
                for _ in range(2):
                    o_eng.forward(fmaps, cnets, iters=iters, all_masks=args.all_masks)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(5):
                    o_eng.forward(fmaps, cnets, iters=iters, all_masks=args.all_masks)
                torch.cuda.synchronize()
                dto = (time.perf_counter() - t0) / 5
                result[other + "_mode"] = {"value": B * pairs / dto, "unit": "flow-fields/s", "ms_per_step": 1e3 * dto,
                                           "note": "same workload, split (hi + lo) weights in every layer"}
                del o_eng
                torch.cuda.empty_cache()
            except RuntimeError as e:
                result[other + "_mode"] = {"error": str(e)[:200]}
        # the same workload in the library's fp32-class arithmetic (split precision everywhere, fp32 volumes), so that
        # both named configurations are on record from one run on one box
        try:
            ref_eng = HotPathEngine(params, device=dev, T=T, use_graph=not args.no_graph, **presets.engine_kwargs("fp32_class"))
            for _ in range(2):
                ref_eng.forward(fmaps, cnets, iters=iters, all_masks=args.all_masks)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                ref_eng.forward(fmaps, cnets, iters=iters, all_masks=args.all_masks)
            torch.cuda.synchronize()
            dtr = (time.perf_counter() - t0) / 5
            result["fp32_class_mode"] = {"value": B * pairs / dtr, "unit": "flow-fields/s", "ms_per_step": 1e3 * dtr,
                                         "config": presets.engine_kwargs("fp32_class"),
                                         "note": "same workload, split precision f16x3 in every contraction, fp32 volumes, fused GMA "
                                                 "with fp16 q / k / v (EPE vs oracle ~2e-5 px)"}
            del ref_eng
            torch.cuda.empty_cache()
        except RuntimeError as e:
            result["fp32_class_mode"] = {"error": str(e)[:200]}

    if rank == 0 and world == 1 and args.clips != 1 and not args.no_kernel_breakdown:
        # single-clip latency: the same engine and kernels with one clip per launch (tails and launch gaps show)
        try:
            f1, c1 = fmaps[:1].contiguous(), cnets[:1].contiguous()
            for _ in range(3):
                eng.forward(f1, c1, iters=iters, all_masks=args.all_masks)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                eng.forward(f1, c1, iters=iters, all_masks=args.all_masks)
            torch.cuda.synchronize()
            dt1 = (time.perf_counter() - t0) / 10
            result["single_clip"] = {"clips_per_step": 1, "value": pairs / dt1, "unit": "flow-fields/s",
                                     "ms_per_clip": 1e3 * dt1}
        except RuntimeError as e:
            result["single_clip"] = {"error": str(e)[:200]}

    if rank == 0 and world == 1 and not args.no_kernel_breakdown and args.workload != "spring":
        # frames -> flows: the reference's forward runs the encoder inside the call (streamflow.py:105-108); random frames,
        # random-init Twins_CSC weights of the reference's architecture (fnet on T frames, cnet on T - 1), then the same
        # engine.  Secondary numbers: `value` above starts at the features (BASELINE.json's hot path).
        try:
            from streamflow_amd.encoders import Twins_CSC
            fnet, cnet = Twins_CSC().to(dev), Twins_CSC().to(dev)
            fnet.svt.load_state_dict({k[4:]: v for k, v in syn.make_twins_params(1).items()}, strict=True)
            cnet.svt.load_state_dict({k[4:]: v for k, v in syn.make_twins_params(2).items()}, strict=True)
            frames = (torch.rand(B, T, 3, H, W, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
            if True:
                def encode():
                    return (fnet(frames, precision=cfg["precision"]).float().contiguous(),
                            cnet(frames[:, :-1], precision=cfg["precision"]).float().contiguous())
                for _ in range(2):
                    fm, cn = encode()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(3):
                    fm, cn = encode()
                torch.cuda.synchronize()
                t_enc = (time.perf_counter() - t0) / 3
                eng.forward(fm, cn, iters=iters, all_masks=args.all_masks)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(3):
                    fm, cn = encode()
                    eng.forward(fm, cn, iters=iters, all_masks=args.all_masks)
                torch.cuda.synchronize()
                t_all = (time.perf_counter() - t0) / 3
            result["encoder_ms_per_clip"] = round(1e3 * t_enc / B, 3)
            result["frames_to_flows_per_sec"] = {"value": B * pairs / t_all, "unit": "flow-fields/s", "ms_per_step": 1e3 * t_all,
                                                 "encoder_share": round(t_enc / t_all, 3),
                                                 "note": "Twins_CSC fnet + cnet (random-init weights of the reference architecture) on "
                                                         "random frames, then the timed hot path; same clips per step"}
            del fnet, cnet, frames
            torch.cuda.empty_cache()
        except RuntimeError as e:
            result["frames_to_flows_per_sec"] = {"error": str(e)[:200]}

    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        barrier()                           # rank 0 may still be in its instrumented pass: leave together
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
