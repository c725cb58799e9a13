"""sf_frame_interp (csrc/frame_interp.hip) through the C ABI with raw strides; every buffer is a guard-banded allocation of
tests/guarded.py.

Criteria.  Output bytes, cover codes and the stats rows are BITWISE the numpy restatement's (tests/interp_cases.py; its agreement
with a scalar restatement and its distance from a float64 ideal are tests/test_interp_cases_cpu.py): all sums are integer, so there
is no tolerance anywhere.  Operands must come back unchanged, and so must everything outside the outputs and the workspace.  NaN,
Inf and huge flows are ordinary inputs with defined results (they contribute nothing): nothing here is meant to fault."""
import numpy as np
import pytest
import torch

from tests import interp_cases as ic
from tests.guarded import Guarded, GuardedBytes

pytestmark = pytest.mark.gpu

OUT_FILL, COVER_FILL = 0x5A, 0x77


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from streamflow_amd import _lib
    return _lib.load()


def place_frames(arr, dev, layout):
    """uint8 [n, h, w, 3] inside a guard-banded byte allocation -> (GuardedBytes, byte strides (frame, row, pixel, channel)).
    plain: dense HWC.  hwc: HWC, rows 5 bytes longer, 7 bytes between frames, the base 1 byte off the allocation's alignment.
    chw: planar, rows 3 bytes longer, 2 bytes between planes, 1 byte between frames, the base 3 bytes off."""
    n, h, w, _ = arr.shape
    if layout == "plain":
        ps, cs, rs, shift = 3, 1, 3 * w, 0
        fs = h * rs
    elif layout == "hwc":
        ps, cs, rs, shift = 3, 1, 3 * w + 5, 1
        fs = h * rs + 7
    else:
        ps, rs, shift = 1, w + 3, 3
        cs = h * rs + 2
        fs = 3 * cs + 1
    g = GuardedBytes(dev, n * fs, fill=0xEE, shift=shift)
    i, y, x, c = np.ix_(np.arange(n), np.arange(h), np.arange(w), np.arange(3))
    idx = torch.from_numpy((i * fs + y * rs + x * ps + c * cs).reshape(-1)).to(dev)
    g.view()[idx] = torch.from_numpy(arr.reshape(-1)).to(dev)
    return g, (fs, rs, ps, cs)


def place_flows(flow, dev, strided):
    """fp32 [n, 2, h, w] as 2 n planes of a NaN-filled Guarded allocation -> (Guarded, ptr, (field, channel, row) strides in floats).
    strided: rows 3 floats longer, 5 floats between planes, the base 1 float in, and the planes in the order [channel][field]."""
    n, _, h, w = flow.shape
    if strided:
        ld, off = w + 3, 1
        stride = h * ld + 5
        planes = torch.from_numpy(np.ascontiguousarray(flow.transpose(1, 0, 2, 3))).reshape(2 * n, h, w)
        strides = (stride, n * stride, ld)
    else:
        ld, off, stride = w, 0, h * w
        planes = torch.from_numpy(flow).reshape(2 * n, h, w)
        strides = (2 * stride, stride, ld)
    g = Guarded(dev, 2 * n, h, w, off, ld, stride, float("nan")).put(planes)
    return g, g.ptr, strides


class Call:
    """One case placed on the device: operands, class maps, outputs, stats rows and a workspace of exactly the size asked for."""

    def __init__(self, lib, dev, a, b, fwd, bwd, cls=None, layout="plain", start=0.0, ws_fill=0x7F, cover=True):
        self.lib, self.n, self.h, self.w = lib, fwd.shape[0], fwd.shape[2], fwd.shape[3]
        n, h, w = self.n, self.h, self.w
        strided = layout != "plain"
        self.a, self.sa = place_frames(a, dev, layout)
        self.b, self.sb = place_frames(b, dev, layout)
        self.f, self.fptr, self.sf = place_flows(fwd, dev, strided)
        self.g, self.gptr, self.sg = place_flows(bwd, dev, strided)
        self.cls = None
        if cls is not None:
            self.cls = [GuardedBytes(dev, n * h * w, shift=1 if strided else 0) for _ in range(2)]
            for g, c in zip(self.cls, cls):
                g.view().copy_(torch.from_numpy(c.reshape(-1)).to(dev))
        self.out = GuardedBytes(dev, n * h * w * 3, fill=OUT_FILL, shift=1 if strided else 0)
        self.cover = GuardedBytes(dev, n * h * w, fill=COVER_FILL, shift=3 if strided else 0) if cover else None
        self.stats = GuardedBytes(dev, n * ic.LEN * 8, guard=4096)
        self.rows().fill_(start)
        self.ws = GuardedBytes(dev, lib.sf_frame_interp_ws_bytes(n, h, w), fill=ws_fill, guard=4096)
        self.operands = [g.buf.clone() for g in self._operand_buffers()]

    def _operand_buffers(self):
        return [self.a, self.b, self.f, self.g] + (self.cls or [])

    def rows(self):
        return self.stats.view().view(torch.float64).view(self.n, ic.LEN)

    def run(self, num, den, imp=(16, 1, 16), codes=(0, 1), **kw):
        q = dict(a=self.a.ptr, b=self.b.ptr, fwd=self.fptr, bwd=self.gptr, n=self.n, h=self.h, w=self.w, num=num, den=den,
                 cls_f=None if self.cls is None else self.cls[0].ptr, cls_b=None if self.cls is None else self.cls[1].ptr, imp=imp,
                 out=self.out.ptr, cover=None if self.cover is None else self.cover.ptr, stats=self.stats.ptr, ws=self.ws.ptr,
                 ws_bytes=self.ws.size, fr=self.sf[2], rs=self.sa[1])
        q.update(kw)
        sa, sb, sf, sg = self.sa, self.sb, self.sf, self.sg
        return self.lib.sf_frame_interp(q["a"], sa[0], q["rs"], sa[2], sa[3], q["b"], sb[0], sb[1], sb[2], sb[3], q["fwd"], sf[0], sf[1],
                                        q["fr"], q["bwd"], sg[0], sg[1], sg[2], q["n"], q["h"], q["w"], q["num"], q["den"], q["cls_f"],
                                        q["cls_b"], codes[0], codes[1], q["imp"][0], q["imp"][1], q["imp"][2], q["out"], q["cover"],
                                        q["stats"], q["ws"], q["ws_bytes"], torch.cuda.current_stream().cuda_stream)

    def results(self):
        """(out, cover or None, stats) as numpy arrays, after asserting every guard and that no operand was written."""
        torch.cuda.synchronize()
        for g, snap in zip(self._operand_buffers(), self.operands):
            assert torch.equal(g.buf.view(torch.uint8), snap.view(torch.uint8)), "an operand was written"
        assert self.out.guards_unchanged() and self.stats.guards_unchanged() and self.ws.guards_unchanged()
        assert self.cover is None or self.cover.guards_unchanged()
        n, h, w = self.n, self.h, self.w
        return (self.out.view().view(n, h, w, 3).cpu().numpy(), None if self.cover is None else self.cover.view().view(n, h, w).cpu().numpy(),
                self.rows().cpu().numpy())


def check(got, want, start=0.0, calls=1):
    out, cover, stats = got
    assert np.array_equal(out, want[0]), f"{int((out != want[0]).sum())} of {out.size} output bytes differ"
    if cover is not None:
        assert np.array_equal(cover, want[1]), f"{int((cover != want[1]).sum())} of {cover.size} cover codes differ"
    assert np.array_equal(stats, start + calls * want[2]), (stats, want[2])


LAYOUTS = {(5, 260): ("plain", "hwc", "chw"), (13, 37): ("plain", "hwc")}


@pytest.mark.parametrize("variant", ic.VARIANTS, ids=["nocls", "cls-16-1-16", "cls-1-1-1"])
@pytest.mark.parametrize("case", ic.CASES, ids=ic.case_ids())
def test_kernel_matches_the_restatement_bitwise(lib, dev, case, variant):
    with_cls, imp = variant
    a, b, fwd, bwd, num, den, cls = ic.build(case, with_cls)
    want = ic.restate(a, b, fwd, bwd, num, den, cls, imp=imp)
    for layout in LAYOUTS.get(fwd.shape[2:], ("plain",)):
        call = Call(lib, dev, a, b, fwd, bwd, cls, layout)
        assert call.run(num, den, imp) == 0, lib.sf_last_error()
        check(call.results(), want)


@pytest.mark.parametrize("case", ic.BIG, ids=ic.case_ids(ic.BIG))
def test_kernel_matches_the_restatement_under_heavy_contention(lib, dev, case):
    """Where the resolve leaves its fast paths: one side's W at and above 2^31 with dark channels (2 W passes 32 bits, 2 C + W does
    not: the mean is 0), and about a hundred both-sided targets with W on both sides of 2^24 (64-bit and 128-bit blends)."""
    a, b, fwd, bwd, num, den, _ = ic.build(case)
    call = Call(lib, dev, a, b, fwd, bwd)
    assert call.run(num, den) == 0, lib.sf_last_error()
    check(call.results(), ic.restate(a, b, fwd, bwd, num, den))


def test_other_class_bytes_and_no_cover_map(lib, dev):
    """The bytes that mean visible / occluded are arguments (a mask image's 255 / 0 / 128); without `cover` the same bytes."""
    case = ic.CASES[7]
    a, b, fwd, bwd, num, den, cls = ic.build(case, True)
    want = ic.restate(a, b, fwd, bwd, num, den, cls, imp=(9, 2, 5))
    table = np.array([255, 0, 128], np.uint8)
    call = Call(lib, dev, a, b, fwd, bwd, [table[c] for c in cls], "hwc", cover=False)
    assert call.run(num, den, (9, 2, 5), codes=(255, 0)) == 0, lib.sf_last_error()
    check(call.results(), want)


def test_every_pixel_on_one_target_sums_exactly(lib, dev):
    """Maximal contention: h * w adds of weight 4096 * 16 (times the byte) meet in one accumulator; the 64-bit sums are exact."""
    a, b, fwd, bwd, num, den, _ = ic.build(ic.CASES[10])
    a[0], b[0] = 255, 254                                                 # the largest sums: 481 * 4096 * 16 * 255 > 2^32
    assert 13 * 37 * 4096 * 16 * 255 > 1 << 32
    want = ic.restate(a, b, fwd, bwd, num, den)
    call = Call(lib, dev, a, b, fwd, bwd)
    assert call.run(num, den) == 0, lib.sf_last_error()
    got = call.results()
    check(got, want)
    assert (got[0][0, 13 // 2, 37 // 2] == 255).all() and got[1][0, 13 // 2, 37 // 2] == 0 and (got[1][0] == 3).sum() == 13 * 37 - 1


def test_non_finite_and_huge_flows_contribute_nothing(lib, dev):
    h, w = 5, 8
    a = np.full((1, h, w, 3), 200, np.uint8)
    b = np.full((1, h, w, 3), 100, np.uint8)
    fwd = np.zeros((1, 2, h, w), np.float32)
    bwd = np.zeros((1, 2, h, w), np.float32)
    for x, bad in enumerate(ic.SPECIALS):
        fwd[0, 0, 0, x] = bad
        fwd[0, 1, 1, x] = bad
        bwd[0, :, 2, x] = bad
    call = Call(lib, dev, a, b, fwd, bwd, layout="hwc")
    assert call.run(1, 2) == 0, lib.sf_last_error()
    out, cover, stats = got = call.results()
    check(got, ic.restate(a, b, fwd, bwd, 1, 2))
    assert (cover[0, 0, :5] == 2).all() and (cover[0, 1, :5] == 2).all() and (cover[0, 2, :5] == 1).all()
    assert (out[0, 0, :5] == 100).all() and (out[0, 2, :5] == 200).all() and (out[0, 3] == 150).all()
    assert stats[0].tolist() == [40, 25, 5, 10, 0]


@pytest.mark.parametrize("case", [ic.CASES[10], ic.CASES[14], ic.CASES[19]], ids=lambda c: c[0])
def test_repeated_calls_and_stale_workspaces_give_the_same_bytes(lib, dev, case):
    """Two calls on the same inputs are bitwise equal; a workspace full of 0xFF gives what a zeroed one gives (the call clears its
    accumulators itself); the stats rows are ADDED to."""
    a, b, fwd, bwd, num, den, cls = ic.build(case, True)
    want = ic.restate(a, b, fwd, bwd, num, den, cls)
    results = []
    for ws_fill, start in ((0x00, 0.0), (0xFF, 0.0), (0x7F, 1000.0)):
        call = Call(lib, dev, a, b, fwd, bwd, cls, ws_fill=ws_fill, start=start)
        assert call.run(num, den) == 0, lib.sf_last_error()
        got = call.results()
        check(got, want, start=start)
        results.append(got)
    for other in results[1:]:
        assert other[0].tobytes() == results[0][0].tobytes() and other[1].tobytes() == results[0][1].tobytes()
    # a second call on the same buffers (its workspace now holds the first call's sums): the same bytes, the rows doubled
    assert call.run(num, den) == 0, lib.sf_last_error()
    again = call.results()
    check(again, want, start=1000.0, calls=2)
    assert again[0].tobytes() == results[0][0].tobytes()


def test_bad_arguments_launch_nothing(lib, dev):
    a, b, fwd, bwd, num, den, cls = ic.build(ic.CASES[7], True)
    call = Call(lib, dev, a, b, fwd, bwd, cls, "hwc")
    P = call.cls[0].ptr
    need = lib.sf_frame_interp_ws_bytes(call.n, call.h, call.w)
    for bad in (dict(a=None), dict(b=None), dict(fwd=None), dict(bwd=None), dict(out=None), dict(stats=None), dict(ws=None),
                dict(n=0), dict(n=65536), dict(h=0), dict(w=0), dict(fr=call.w - 1), dict(rs=-1), dict(num=0), dict(num=den), dict(den=65),
                dict(den=1), dict(imp=(0, 1, 1)), dict(imp=(16, 17, 16)), dict(cls_f=None), dict(cls_b=None),
                dict(fwd=call.fptr + 2), dict(stats=call.stats.ptr + 4), dict(ws=call.ws.ptr + 4), dict(ws_bytes=need - 1)):
        assert call.run(**dict(dict(num=num, den=den), **bad)) == -1, bad
        assert b"sf_frame_interp" in lib.sf_last_error(), bad
    call.results()                                                       # guards and operands
    assert bool((call.out.view() == OUT_FILL).all()) and bool((call.cover.view() == COVER_FILL).all())
    assert bool((call.ws.view() == 0x7F).all()) and bool((call.rows() == 0).all())
    assert P == call.cls[0].ptr
    # ... and the good call does write
    assert call.run(num, den) == 0, lib.sf_last_error()
    check(call.results(), ic.restate(a, b, fwd, bwd, num, den, cls))
