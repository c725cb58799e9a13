"""The media entry points held to the rule of tests/test_gpu_engine_state.py -- a result is a function of its inputs only: what a
buffer held before, what the previous call left behind and which stream or graph replay runs the call must not matter.  Through the
C ABI, for every record of tests/media_state_cases.py (sf_flow_consistency, sf_warp_frames, sf_frame_interp, sf_resize_u8 / _f32,
sf_jpeg_encode, sf_jpeg_decode(_split), sf_flo5_encode, sf_inflate, sf_flo5_assemble, sf_motion_moments / _solve / _fit,
sf_warp_affine_u8, sf_flow_to_kitti16, sf_png_encode, sf_png_unfilter, sf_frames_to_clips, sf_clips_to_flows, sf_tile_blend):

  (a) USED BUFFERS.  Every buffer -- workspace, outputs, status, stats, descriptor tables -- is allocated once at case A's size between
      guard bands.  A runs, then B in the same buffers with nothing cleared but the stats rows (the header: they are ADDED to); then
      the reverse order in new buffers.  The second call's bytes equal the call's in fresh buffers BITWISE and meet the pinned
      reference of its module; everything outside its extent is what the first call left; guards and inputs are untouched.  The
      leftovers of a VALID call pass every range check that junk fails: counts, offsets, segment tables, error keys, partial sums of
      another image set are what a long-running video or dataset loop hands the next call.  Nothing is sized below A, so a stale index
      wrongly followed lands inside the allocation and shows as a changed byte.
  (b) SIDE STREAM, CAPTURE, REPLAY.  One eager call on a side stream; one capture of the call on that stream in torch's default (global)
      capture mode -- a host synchronisation, an allocation or a launch on another stream inside the entry point makes the capture
      raise: the check for "on `stream`, no host synchronisation"; three replays, each with new content of the same geometry in the
      static inputs, each compared with an eager call on fresh buffers and with the reference.  A test per entry point.

Integer fields of the workspaces, read in the kernels before the first run -- who writes each before who reads it in the same call:
  sf_jpeg_decode        first_error / covered [n]: cleared by the entry point, atomicMax / atomicAdd by jpeg_entropy_kernel, read by
                        jpeg_status_kernel.  coef: every block of an interval's MCUs is stored whole (64 lanes) by the wave before
                        jpeg_idct_kernel reads it; planes: written by jpeg_idct_kernel before jpeg_colour_kernel.
  sf_jpeg_decode_split  first_wg, u_off [intervals]: written for EVERY interval by jpeg_plan_kernel (-1: the wave route) before any
                        reader.  err_key [intervals] and wg_interval [workgroups]: cleared to 0xFF by the entry point, then
                        jpeg_plan_kernel names the split intervals' workgroups.  u_len, u_err: written by jpeg_unstuff_kernel for every
                        split interval, read (seg_work) only through a split interval.  ustream: written up to u_len, read below it.
                        ex_bit, ex_sk, nblk [segment slots]: written by jpeg_spec_kernel for the segments below nseg of every named
                        workgroup, read by jpeg_sync_kernel for the same slots, which writes first_blk; jpeg_write_kernel reads its own
                        slot and its predecessor's (same interval, below nseg).  A specification that is no table ends all three
                        kernels before any of those reads.  coef: cleared by the entry point (two segments may write one block).
  sf_jpeg_encode        ibits [intervals]: written by jpeg_pack_kernel (after it has cleared exactly the words it ORs into), read by
                        jpeg_count_kernel, which writes ilen; jpeg_offsets_kernel reads ilen and writes ioff; jpeg_gather_kernel reads
                        ibits and ioff.  Every interval's word is written: the grids are (block rows, images) throughout.
  sf_png_encode         scanlines and table records by the first three kernels before the fourth (tests/test_gpu_engine_state.py).
  sf_flo5_encode        the byte planes whole (padding included) by flo5_shuffle_kernel; a block's record (code tables, bit length,
                        Adler sums) by flo5_table_kernel, its start by flo5_offsets_kernel, before flo5_pack_kernel reads them.
  The other workspaces hold no integer a kernel follows: per-block floating-point partials written by the main launch before the finish
  launch sums the same blocks (sf_flow_consistency, sf_warp_frames, the sf_motion_* calls, sf_warp_affine_u8's counts, sf_frame_interp's
  rows), sf_frame_interp's accumulators (cleared by the entry point), the intermediate image of the resizers.
No field read before it is written turned up by reading.  What the RUNS turned up: the entry points' per-call clears were
hipMemsetAsync calls, and a memset node of a captured graph cleared only part of its bytes from the second replay on, so under replay
sf_frame_interp blended into stale sums and sf_jpeg_decode(_split) met stale status words, keys and workgroup maps.  The clears are
kernels now (sf::fill_async, csrc/sf_common.h); test_flow_to_image_replay_clears_the_maximum is the same finding for
sf_flow_to_image, whose older capture test replays with growing flows only.

The wrappers' table caches: ops.norm_lut (first use inside a capture: refused, nothing cached; first use outside: complete for every
stream when it returns), resize.device_table and tiling.tile_weights (first use inside a capture: the same refusal, no entry)."""
import numpy as np
import pytest
import torch

from tests import media_state_cases as mc
from tests import video_cases as vc
from tests.guarded import GuardedBytes

pytestmark = pytest.mark.gpu

FILL = 0x7F
REFUSAL = "first time inside a graph capture"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def lib():
    from streamflow_amd import _lib
    return _lib.load()


class Buffers:
    """Every buffer of a call, allocated once at `sizes` between guard bands and filled with FILL."""

    def __init__(self, dev, sizes):
        self.g = {name: GuardedBytes(dev, size, fill=FILL) for name, size in sizes.items()}

    def load(self, bound):
        """The caller's part before a call: the inputs' bytes, and zeros in the stats rows (the header: rows are ADDED to)."""
        for name, b in bound.bufs.items():
            if b.role == mc.IN:
                self.g[name].view()[:b.nbytes].copy_(torch.from_numpy(b.data))
            elif b.role == mc.STATS:
                self.g[name].view()[:b.nbytes].zero_()

    def launch(self, bound, stream=None):
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        rc = bound.call(lib(), lambda name: self.g[name].ptr, s)
        assert rc == 0, (bound.entry, rc, lib().sf_last_error())

    def whole(self):
        return {name: g.buf.clone() for name, g in self.g.items()}

    def read(self, bound):
        torch.cuda.synchronize()
        return {name: self.g[name].view()[:b.nbytes].cpu().numpy() for name, b in bound.bufs.items() if b.role != mc.IN}

    def guards_unchanged(self):
        return all(g.guards_unchanged() for g in self.g.values())


_FRESH = {}


def fresh(dev, rec, which, v=0):
    """(the Bound, what the call writes into NEW buffers of exactly its own sizes on the current stream), computed once per case and
    held to the module's pinned reference there."""
    key = (rec.entry, which, v)
    if key not in _FRESH:
        bound = rec.bind(which, v)
        bufs = Buffers(dev, bound.sizes())
        bufs.load(bound)
        bufs.launch(bound)
        outs = bufs.read(bound)
        assert bufs.guards_unchanged()
        bound.check(outs)
        _FRESH[key] = (bound, outs)
    return _FRESH[key]


def regions_of(bound, want):
    """name -> (extent, free) for every output, status and stats buffer of the call (a workspace is scratch throughout)."""
    special = bound.regions(want)
    out = {}
    for name, b in bound.bufs.items():
        if b.role not in (mc.IN, mc.WS):
            out[name] = special.get(name, (np.ones(b.nbytes, bool), np.zeros(b.nbytes, bool)))
    return out


def compare(bound, got, want, what):
    for name, (extent, _) in regions_of(bound, want).items():
        bad = int((got[name][extent] != want[name][extent]).sum())
        kept = int((got[name][extent] == FILL).sum())
        assert bad == 0, (f"{what}: {bad} of {int(extent.sum())} bytes of `{name}` differ from the call in fresh buffers "
                          f"({kept} hold the fill byte)")


@pytest.mark.parametrize("order", ["A-then-B", "B-then-A"])
@pytest.mark.parametrize("entry", mc.ENTRIES)
def test_used_buffers(dev, entry, order):
    """Property (a): every buffer allocated once at A's size; the first case runs, then the second in the same buffers with nothing
    cleared in between but the stats rows.  The second call's outputs, status and stats are bitwise those of the call in fresh
    buffers and meet the pinned reference; every byte outside the second call's extent is what the first call left; the guard bands
    are intact; the inputs come back unchanged."""
    rec = mc.record(entry)
    first, second = (fresh(dev, rec, w)[0] for w in (("A", "B") if order == "A-then-B" else ("B", "A")))
    want = fresh(dev, rec, "B" if order == "A-then-B" else "A")[1]
    bufs = Buffers(dev, rec.bind("A").sizes())
    bufs.load(first)
    bufs.launch(first)
    torch.cuda.synchronize()
    bufs.load(second)
    before = {name: t.cpu().numpy() for name, t in bufs.whole().items()}
    bufs.launch(second)
    got = bufs.read(second)
    after = {name: t.cpu().numpy() for name, t in bufs.whole().items()}
    assert bufs.guards_unchanged(), f"{entry} {order}: a guard band was written"
    compare(second, got, want, f"{entry} {order}")
    regions = regions_of(second, want)
    for name, b in second.bufs.items():
        lo = bufs.g[name].guard
        a, z = after[name][lo:lo + bufs.g[name].size], before[name][lo:lo + bufs.g[name].size]
        if b.role == mc.IN:
            keep = np.ones(a.size, bool)
        else:
            keep = np.ones(a.size, bool)
            keep[:b.nbytes] = False if b.role == mc.WS else ~(regions[name][0] | regions[name][1])
        bad = int((a[keep] != z[keep]).sum())
        assert bad == 0, f"{entry} {order}: {bad} bytes of `{name}` ({b.role}) outside the call's extent changed"
    second.check(got)


@pytest.mark.parametrize("entry", mc.ENTRIES)
def test_side_stream_capture_and_replay(dev, entry):
    """Property (b), after tests/test_gpu_flow_viz.py::test_inside_graph_capture: case A's inputs in static buffers; one eager call
    on a side stream; one capture of the call on that stream in torch's default (global) capture mode, in which a host
    synchronisation, an allocation or a launch on another stream inside the entry point makes the capture raise; three replays, each
    after new content of the same geometry has been copied into the static inputs and the stats rows zeroed, each compared with the
    eager call on fresh buffers and with the pinned reference.  The graph is a single-stream chain."""
    rec = mc.record(entry)
    bound, want = fresh(dev, rec, "A", 0)
    bufs = Buffers(dev, bound.sizes())
    bufs.load(bound)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bufs.launch(bound, side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    compare(bound, bufs.read(bound), want, f"{entry} eager on a side stream")
    bufs.load(bound)
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph, stream=side):
            bufs.launch(bound, side.cuda_stream)
    finally:
        torch.cuda.synchronize()                                        # (after a capture error: nothing of it reaches the next test)
    for v in range(1, mc.VARIANTS):
        other, want = fresh(dev, rec, "A", v)
        assert other.sizes() == bound.sizes()
        for name, b in bound.bufs.items():
            if b.role not in (mc.IN, mc.WS):
                bufs.g[name].view().fill_(FILL)
        bufs.load(other)
        graph.replay()
        got = bufs.read(other)
        assert bufs.guards_unchanged(), f"{entry} replay {v}: a guard band was written"
        compare(other, got, want, f"{entry} replay {v}")
        other.check(got)


def test_flow_to_image_replay_clears_the_maximum(dev):
    """sf_flow_to_image's per-field maximum is an atomic maximum on a slot the call clears: replays with SHRINKING flows show a clear
    that does not happen (tests/test_gpu_flow_viz.py::test_inside_graph_capture replays growing flows, which a stale maximum passes)."""
    from tests import viz_cases
    n, h, w = 3, 24, 40
    flows, out, ws = torch.zeros(n, 2, h, w, device=dev), torch.zeros(n, h, w, 3, dtype=torch.uint8, device=dev), torch.zeros(n, device=dev)

    def call(src, dst, rad, stream):
        assert lib().sf_flow_to_image(src.data_ptr(), dst.data_ptr(), rad.data_ptr(), n, h, w, -1.0, -1.0, 0, stream) == 0, lib().sf_last_error()

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph, stream=side):
            call(flows, out, ws, side.cuda_stream)
    finally:
        torch.cuda.synchronize()
    for r, scale in enumerate((50.0, 5.0, 0.5, 0.05)):
        new = torch.from_numpy(viz_cases.gaussian_fields(n, h, w, [scale, 2 * scale, 0.5 * scale], seed=30 + r)).to(dev)
        flows.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_ws = torch.empty_like(out), torch.empty_like(ws)
        call(new, eager, eager_ws, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(ws, eager_ws), (r, ws.tolist(), eager_ws.tolist())
        assert torch.equal(out, eager), r


# ---- the table caches of the wrappers -----------------------------------------------------------------------------------------------
def _video_call(dev, which="B"):
    """(uint8 frames on the device, frames_to_clips's arguments, the restatement on the device) of a table case."""
    frames, (n, H, W, T), (left, top, Hp, Wp), nc = mc._video(which, 0)
    frames = frames.to(dev)
    kw = dict(n=n, T=T, first_clip=0, n_clips=nc, pad=(left, Wp - W - left, top, Hp - H - top))
    return frames, kw, vc.clips(frames, T, "sintel"), (nc, T, 3, Hp, Wp)


def _poison_the_small_blocks(dev):
    """NaN into the blocks a 1 KiB table will be carved from next: a table that is read before it is built then shows, instead of
    being saved by the bytes of the table freed a moment ago."""
    junk = [torch.full((256,), float("nan"), device=dev) for _ in range(256)]
    torch.cuda.synchronize()
    del junk


def test_first_frames_to_clips_inside_a_capture_is_refused_and_caches_nothing(dev):
    from streamflow_amd import ops
    frames, kw, want, shape = _video_call(dev)
    out = torch.zeros(shape, device=dev)
    ops._NORM_LUT.clear()
    _poison_the_small_blocks(dev)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    try:
        with pytest.raises(RuntimeError, match=REFUSAL):
            with torch.cuda.graph(graph, stream=side):
                ops.frames_to_clips(frames, out=out, **kw)
        torch.cuda.synchronize()
        assert not ops._NORM_LUT, "a table requested inside a capture was cached"
        got = ops.frames_to_clips(frames, **kw)                          # the following eager call builds it and is right
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        again = torch.cuda.CUDAGraph()
        with torch.cuda.graph(again, stream=side):                       # ... after which a capture is fine
            ops.frames_to_clips(frames, out=out, **kw)
        again.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    finally:
        torch.cuda.synchronize()
        ops._NORM_LUT.clear()                                            # (whatever happened, no later test reads this table)


STALL_CYCLES = 20_000_000        # torch.cuda._sleep: device clock ticks; the test prints the stall's length in milliseconds


def test_first_use_on_a_stalled_stream_then_at_once_on_another(dev):
    """The table's first use on a stream that is still busy, then at once, with no wait, a call on a second stream: the second call
    must read a complete table."""
    from streamflow_amd import ops
    frames, kw, want, shape = _video_call(dev)
    ops._NORM_LUT.clear()
    _poison_the_small_blocks(dev)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    out1, out2 = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(s1):
            t0.record()
            torch.cuda._sleep(STALL_CYCLES)
            t1.record()
            ops.frames_to_clips(frames, out=out1, **kw)
        with torch.cuda.stream(s2):
            ops.frames_to_clips(frames, out=out2, **kw)
        torch.cuda.synchronize()
        print(f"stall of {STALL_CYCLES} ticks: {t0.elapsed_time(t1):.2f} ms")
        wrong = int((out2.view(torch.int32) != want.view(torch.int32)).sum())
        print(f"second stream: {wrong} of {out2.numel()} values differ from the restatement")
        assert wrong == 0, f"the call on the second stream read the table before it was built: {wrong} of {out2.numel()} values differ"
        assert torch.equal(out1.view(torch.int32), want.view(torch.int32))
    finally:
        torch.cuda.synchronize()
        ops._NORM_LUT.clear()


def test_later_uses_of_the_table_do_not_synchronise(dev):
    """Only the first use per device may wait: with the table built, a capture in global mode (which a synchronisation breaks) records
    the call."""
    from streamflow_amd import ops
    frames, kw, want, shape = _video_call(dev)
    ops.norm_lut(dev)
    out = torch.zeros(shape, device=dev)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.graph(graph, stream=side):
            ops.frames_to_clips(frames, out=out, **kw)
    finally:
        torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


def _refused_in_a_capture(dev, first_use, cache, key_count):
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    try:
        with pytest.raises(RuntimeError, match=REFUSAL):
            with torch.cuda.graph(graph, stream=side):
                first_use()
    finally:
        torch.cuda.synchronize()
    assert key_count(cache) == 0, "a table requested inside a capture was cached"
    return first_use()                                                   # the eager first use works


def test_resize_device_table_first_use_inside_a_capture(dev):
    from streamflow_amd import resize
    from tests import resize_cases as rc
    for kind in ("u8", "f32"):
        key = lambda cache: sum(1 for k in cache if k[:3] == (53, 24, "bicubic") and k[4] == kind)
        for k in [k for k in resize._TABLES if k[:3] == (53, 24, "bicubic")]:
            del resize._TABLES[k]
        bounds, k, ksize = _refused_in_a_capture(dev, lambda: resize.device_table(53, 24, "bicubic", dev, kind), resize._TABLES, key)
        torch.cuda.synchronize()
        want_b, want_k = rc.table(53, 24, "bicubic")
        assert key(resize._TABLES) == 1 and ksize == want_k.shape[1] and np.array_equal(bounds.cpu().numpy(), want_b)
        assert np.array_equal(k.cpu().numpy(), rc.fixed(want_k) if kind == "u8" else want_k.astype(np.float32))


def test_tile_weights_first_use_inside_a_capture(dev):
    from streamflow_amd import tiling
    th, tw, sigma = 24, 40, 0.07
    on_device = lambda cache: sum(1 for k in cache if k[:3] == (th, tw, sigma) and k[3] != "cpu")
    for k in [k for k in tiling._WEIGHTS if k[:3] == (th, tw, sigma)]:
        del tiling._WEIGHTS[k]
    w = _refused_in_a_capture(dev, lambda: tiling.tile_weights((th, tw), sigma, dev), tiling._WEIGHTS, on_device)
    torch.cuda.synchronize()
    assert on_device(tiling._WEIGHTS) == 1 and torch.equal(w.cpu(), tiling.tile_weights((th, tw), sigma))
