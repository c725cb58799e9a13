"""The correlation family through the C ABI (-m gpu): sf_corr_build_pyramid[_pitched] / sf_corr_build_ws_bytes / sf_corr_lookup[_pitched]
(csrc/corr.hip), sf_corr_blocked_geometry / _bytes / sf_corr_build_blocked_ws_bytes / sf_corr_build_blocked / sf_corr_lookup_blocked
(csrc/corr_blocked.hip) and their five blocked32 counterparts (csrc/corr_blocked32.hip) -- raw pointers and strides handed to
streamflow_amd._lib.load(), not CorrBlock or the ops wrappers (which only ever pass tight strides, offset 0, 16-byte aligned bases and
f2 = f1 + D * N), at the smallest grids at which the index arithmetic can go wrong (tests/corr_cases.py).

Features sit in NaN-filled buffers, the workspace is exactly the bytes the size function returns between guard bands, every level /
blocked volume is prefilled with 0xFF bytes (a NaN in fp16 and fp32), lookup outputs with NaN.  Every case asserts: status 0; sizes and
geometry equal to the CPU restatement; every data cell written and finite; no byte outside the spans the header lets the call write
changed (pad cells of a pitched row, padding cells and records of a blocked volume are inside); inputs and guard bands unchanged; the
placed run (bases 4 / 8 / 12 bytes off 16, clip / pair / level / volume / output strides with gaps, odd ones included) BITWISE the
contiguous one; image (b, t) of a batch bitwise the call on that pair alone; frames shared (f2 = f1 + f_pair_stride) and f2 in a buffer
of its own bitwise equal where the CPU model packs the same operands, inside the bound otherwise; cells within the derived build bound
of the float64 reference, looked-up channels within the lookup bound of the float64 lookup ON THE STORED CELLS, finite at non-finite
and far coordinates and zero where every tap is outside; the k-octet copy bitwise fp16(out) beside fp32 planes, rows 324..327 zero,
and within koct_alone_bound alone.  err / bound is printed per case ("CORR ...").  tests/test_corr_cases_cpu.py shows that these
bounds tell a wrong kernel from a right one.

Worst err / bound measured on the MI355X over the 13 cases (52 tests, 9.5 s), per entry point and arithmetic class -- a record, not a
threshold:
    sf_corr_build_pyramid      FP32 0.182   F16X3 0.495   F16 0.499          unit-normal features (test_cross_layout): F16X3 0.453, F16 0.473
    sf_corr_lookup[_pitched]   fp32 cells 0.226   fp16 cells 0.234
    sf_corr_build_blocked      0.499 (0.079 where f2 apart / a single pair folds another factor)       unit-normal features 0.473
    sf_corr_lookup_blocked     out 0.191   out_koct alone 1.000
    sf_corr_build_blocked32    0.495                                             unit-normal features 0.453
    sf_corr_lookup_blocked32   0.213
    cross-layout, unit-normal features: blocked32 cells EQUAL the pitched F16X3 cells bitwise on all ten grids (limit 2e-6), looked-up
        features differ by at most 4.8e-7 (limit 2e-5).
The builds of the classes that round operands reach 0.50 at D = 1, where the error IS the two operand roundings (the bound's factor 2
over the first-order sum); a k-octet copy asked for alone reaches 1.00 by construction: the cells are fp16 subnormals' size, the
rounding of the copy (up to 2^-25) is all of its bound and some of 300,000 values lies next to a tie."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import corr_cases as cc
from tests.guarded import Guarded, GuardedBytes

pytestmark = pytest.mark.gpu
NAN = float("nan")
CASES = cc.cases()
IDS = [c["id"] for c in CASES]
PRECISIONS = ((cc.FP32, "fp32"), (cc.F16X3, "x3"), (cc.F16, "f16"))
PLACES = ("a", "b", "c")

BUILD = ("f1", "f2", "f_clip_stride", "f_pair_stride", "lvl0", "lvl1", "lvl2", "lvl3", "lvl_pair_stride", "B", "pairs", "D", "h", "w",
         "num_levels", "precision", "split_ws", "split_ws_bytes")
BUILDP = BUILD[:9] + ("lvl_pitch",) + BUILD[9:]
LOOK = ("lvl0", "lvl1", "lvl2", "lvl3", "lvl_pair_stride", "coords", "out", "out_img_stride", "out_koct", "out_koct_img_stride", "B",
        "pairs", "h", "w", "num_levels", "radius", "vol_precision")
LOOKP = LOOK[:5] + ("lvl_pitch",) + LOOK[5:]
BBUILD = ("f1", "f2", "f_clip_stride", "f_pair_stride", "vol", "vol_img_stride_bytes", "B", "pairs", "D", "h", "w", "ws", "ws_bytes")
BLOOK = ("vol", "vol_img_stride_bytes", "coords", "out", "out_img_stride", "out_koct", "out_koct_img_stride", "B", "pairs", "h", "w")
B32LOOK = ("vol", "vol_img_stride_bytes", "coords", "out", "out_img_stride", "B", "pairs", "h", "w")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _L():
    from streamflow_amd import _lib as L
    return L


def _call(name, names, args, **over):
    a = dict(args, **over)
    status = getattr(_L().load(), name)(*[a[k] for k in names], _L().stream())
    torch.cuda.synchronize()
    return status


def _ok(status, what):
    assert status == 0, f"{what}: refused ({status}): {_L().load().sf_last_error().decode(errors='replace')}"


def _i64x4(v):
    return None if v is None else (C.c_int64 * 4)(*[int(x) for x in v])


def _i32x4(v):
    return None if v is None else (C.c_int32 * 4)(*[int(x) for x in v])


def _up(x, m):
    return -(-x // m) * m


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same(a, b):
    return a.shape == b.shape and bool(np.array_equal(_bits64(a), _bits64(b)))


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
class Frames:
    """Frame (b, j) as a [D][N] plane set at off + b * cs + j * ps floats of a NaN-filled buffer."""

    def __init__(self, dev, data, off, ps, cs):
        B, T1, D, N = data.shape
        assert ps >= D * N and cs >= T1 * ps
        self.off, self.ps, self.cs = off, ps, cs
        host = np.full(off + B * cs + 16, np.nan, np.float32)
        for b in range(B):
            for j in range(T1):
                at = off + b * cs + j * ps
                host[at: at + D * N] = data[b, j].reshape(-1)
        self.buf = torch.from_numpy(host).to(dev)
        self.snap = self.buf.clone()

    def ptr(self, b=0, j=0):
        return self.buf.data_ptr() + 4 * (self.off + b * self.cs + j * self.ps)

    def unchanged(self):
        return bool(torch.equal(self.buf.view(torch.int32), self.snap.view(torch.int32)))


def _feature_layout(case, place):
    """(off1, off2, f_pair_stride, f_clip_stride) in floats: f1 / f2 bases 0, 4, 8, 12 bytes off 16; strides tight, with gaps % 4 == 0,
    with gaps % 4 != 0."""
    DN, T1 = case["D"] * case["h"] * case["w"], case["pairs"] + 1
    if place == "tight":
        return 0, 0, DN, T1 * DN
    if place == "a":
        ps = _up(DN, 4) + 4
        return 1, 2, ps, T1 * ps + 8
    if place == "b":
        ps = _up(DN, 4) + 3
        return 3, 1, ps, T1 * ps + 6
    ps = _up(DN, 4) + 8
    return 0, 4, ps, T1 * ps + 4


@functools.lru_cache(maxsize=None)
def _host(cid, amp=cc.AMP):
    """Per case and feature scale, computed once and left unchanged: the frames, the coordinates, the float64 pyramid of every image."""
    case = dict(next(c for c in CASES if c["id"] == cid), amp=amp)
    f = cc.features(case)
    exact = [cc.pyramid(f[b, t], f[b, t + 1], case["h"], case["w"]) for b in range(case["B"]) for t in range(case["pairs"])]
    return f, cc.coords(case), exact


class Inputs:
    """f1 frames (and, shared, f2 = f1 + f_pair_stride) or f2 in a buffer of its own with the same strides; the coordinates."""

    def __init__(self, dev, case, place="tight", separate=False):
        f, xy, _ = _host(case["id"], case.get("amp", cc.AMP))
        off1, off2, self.ps, self.cs = _feature_layout(case, place)
        assert place not in ("a", "c") or (self.ps % 4 == 0 and self.cs % 4 == 0)
        assert place != "b" or self.ps % 4 != 0
        self.F1 = Frames(dev, f, off1, self.ps, self.cs)
        self.F2 = None
        if separate:
            g = np.full_like(f, np.nan)
            g[:, :-1] = f[:, 1:]                                                   # slot t holds frame t + 1; the last slot is never read
            self.F2 = Frames(dev, g, off2, self.ps, self.cs)
        coff = 0 if place == "tight" else 1
        self.xy = torch.from_numpy(np.concatenate([np.full(coff, np.nan, np.float32), xy.reshape(-1), np.full(8, np.nan, np.float32)])).to(dev)
        self.xy_snap, self.coff = self.xy.clone(), coff

    def f1(self, b=0, t=0):
        return self.F1.ptr(b, t)

    def f2(self, b=0, t=0):
        return self.F2.ptr(b, t) if self.F2 is not None else self.F1.ptr(b, t + 1)

    def coords(self, img=0, N=0):
        return self.xy.data_ptr() + 4 * (self.coff + img * 2 * N)

    def unchanged(self):
        return (self.F1.unchanged() and (self.F2 is None or self.F2.unchanged())
                and bool(torch.equal(self.xy.view(torch.int32), self.xy_snap.view(torch.int32))))


# ---- row-major volumes -------------------------------------------------------------------------------------------------------------------------
class Levels:
    """Four level buffers of 0xFF bytes.  Level l: base[l] cells off the buffer's start, pair stride ps[l], row pitch pitch[l]."""

    def __init__(self, dev, B, pairs, h, w, cell16, pitch=None, place="tight"):
        self.B, self.pairs, self.h, self.w, self.N, self.cell16 = B, pairs, h, w, h * w, cell16
        self.pitch = [w >> l for l in range(4)] if pitch is None else list(pitch)
        self.pitched = pitch is not None
        self.dtype = np.float16 if cell16 else np.float32
        self.es = 2 if cell16 else 4
        self.base, self.ps, self.buf = [], [], []
        for l in range(4):
            img = B * self.N * (h >> l) * self.pitch[l]
            if place == "tight":
                base, ps = 0, img
            elif place == "a":                                                     # 4 / 8 / 12 bytes off 16; an EVEN stride in cells
                base, ps = (1, 2, 3, 1)[l] * (2 if cell16 else 1), img + 4 + (img % 2)
            elif place == "b":                                                     # 12 / 4 / 8 / 12 bytes off 16; an ODD stride in cells
                base, ps = (3, 1, 2, 3)[l] * (2 if cell16 else 1), img + 5 + (img % 2)
            else:                                                                  # 16-byte aligned bases and strides, with gaps
                base, ps = 0, _up(img, 8) + 8
            self.base.append(base)
            self.ps.append(ps)
            self.buf.append(torch.full((base + (pairs - 1) * ps + img + 8,), -1, dtype=torch.int16 if cell16 else torch.int32, device=dev))
        self.strides = None if place == "tight" and pairs == 1 else _i64x4(self.ps)

    def ptr(self, l, b=0, t=0):
        return self.buf[l].data_ptr() + self.es * (self.base[l] + t * self.ps[l] + b * self.N * (self.h >> l) * self.pitch[l])

    def args(self, b=None, t=0):
        d = {f"lvl{l}": self.ptr(l, b or 0, t) for l in range(4)}
        d["lvl_pair_stride"] = self.strides if b is None else None
        if self.pitched:
            d["lvl_pitch"] = _i32x4(self.pitch)
        return d

    def decode(self):
        """Four levels [n_img][N][hl][wl] float64 through the decoders of tests/corr_cases.py (once per build)."""
        if getattr(self, "cells", None) is not None:
            return self.cells
        out = []
        for l in range(4):
            raw = self.buf[l].cpu().numpy().view(np.uint8)
            out.append(cc.decode_rows(raw, self.dtype, self.B, self.pairs, self.N, self.h >> l, self.w >> l, self.pitch[l], self.ps[l], self.base[l]))
        self.cells = out
        return out

    def check_written(self, what):
        """Every data cell written and finite; every cell outside the spans [base + t ps, + B N hl pitch) still 0xFF."""
        for l, cells in enumerate(self.decode()):
            assert np.isfinite(cells).all(), (what, l, "a data cell was not written or is not finite")
            img = self.B * self.N * (self.h >> l) * self.pitch[l]
            inside = torch.zeros(self.buf[l].numel(), dtype=torch.bool, device=self.buf[l].device)
            for t in range(self.pairs):
                inside[self.base[l] + t * self.ps[l]: self.base[l] + t * self.ps[l] + img] = True
            assert bool((self.buf[l][~inside] == -1).all()), (what, l, "a cell outside the level's span changed")

    def untouched(self):
        return all(bool((b == -1).all()) for b in self.buf)


def _pitches(w, kind):
    if kind == "exact":
        return [w >> l for l in range(4)]
    if kind == "line":
        return [_up(w, 32)] * 4
    return [min((w >> l) + 3, _up(w, 32)) for l in range(4)]                        # in between


def build_pyramid(dev, case, prec, place="tight", separate=False, pitch=None, only=None):
    """One sf_corr_build_pyramid[_pitched] call with every placement check.  only = (b, t): that pair alone (B = pairs = 1)."""
    h, w, D = case["h"], case["w"], case["D"]
    B, pairs = (case["B"], case["pairs"]) if only is None else (1, 1)
    I = Inputs(dev, case, place, separate)
    Lv = Levels(dev, B, pairs, h, w, prec == cc.F16, None if pitch is None else _pitches(w, pitch), place)
    lib = _L().load()
    want = cc.build_ws_bytes(B, pairs, D, h, w)
    assert lib.sf_corr_build_ws_bytes(B, pairs, D, h, w) == want
    ws = None if prec == cc.FP32 else GuardedBytes(dev, want)
    b, t = only or (0, 0)
    args = dict(f1=I.f1(b, t), f2=I.f2(b, t), f_clip_stride=I.cs, f_pair_stride=I.ps, B=B, pairs=pairs, D=D, h=h, w=w, num_levels=4,
                precision=prec, split_ws=None if ws is None else ws.ptr, split_ws_bytes=0 if ws is None else want, **Lv.args())
    what = (case["id"], prec, place, separate, pitch, only)
    _ok(_call("sf_corr_build_pyramid_pitched" if pitch else "sf_corr_build_pyramid", BUILDP if pitch else BUILD, args), what)
    Lv.check_written(what)
    assert I.unchanged() and (ws is None or ws.guards_unchanged()), (what, "an input or a guard band changed")
    return Lv, I


def _check_cells(entry, case, cls, cells, K, images=None):
    """cells: four levels [n_img][N][hl][wl]; every element within the build bound of the float64 reference."""
    f, _, exact = _host(case["id"], case.get("amp", cc.AMP))
    worst = 0.0
    for img in (range(case["B"] * case["pairs"]) if images is None else images):
        b, t = divmod(img, case["pairs"])
        bound, ex = cc.build_bound(f[b, t], f[b, t + 1], case["h"], case["w"], K)
        for l in range(4):
            r = np.abs(cells[l][img] - ex[l]) / bound[l]
            assert float(r.max()) <= 1.0, (entry, case["id"], cls, img, l, float(r.max()), np.unravel_index(int(np.argmax(r)), r.shape))
            worst = max(worst, float(r.max()))
    print(f"CORR {entry} {case['id']}: {cls} err/bound {worst:.3f}")


# ---- lookups -----------------------------------------------------------------------------------------------------------------------------------
def _outputs(dev, n_img, N, place, want_out=True, want_koct=False):
    out = ko = None
    if want_out:
        off, stride = (0, 324 * N) if place == "tight" else ((1, 324 * N + 5) if place == "a" else ((3, 324 * N + 7) if place == "b" else (4, 324 * N + 8)))
        out = Guarded(dev, n_img, 324, N, off, N, stride, NAN, tail=8)
    if want_koct:
        off, stride = (0, 41 * N * 8) if place == "tight" else (8, 41 * N * 8 + (8 if place == "a" else 24))
        ko = Guarded(dev, n_img, 328, N, off, N, stride, NAN, dtype=torch.float16, koct=True, tail=8)
        assert ko.ptr % 16 == 0
    return out, ko


def _out_args(out, ko):
    return dict(out=None if out is None else out.ptr, out_img_stride=0 if out is None else out.stride,
                out_koct=None if ko is None else ko.ptr, out_koct_img_stride=0 if ko is None else ko.stride)


def _check_outputs(what, out, ko, I):
    """Written, nothing outside the views, inputs unchanged; beside fp32 planes the k-octet copy is bitwise fp16(out), rows 324..327 zero."""
    res = res16 = None
    if out is not None:
        assert out.outside_unchanged(), (what, "an element outside out changed")
        res = out.region()
        assert bool(torch.isfinite(res).all()), (what, "out: an element was not written or is not finite")
    if ko is not None:
        assert ko.outside_unchanged(), (what, "an element outside out_koct changed")
        r = ko.region()
        assert bool(torch.isfinite(r).all()) and bool((r[:, 324:] == 0).all()), (what, "out_koct: not written, or rows 324..327 not zero")
        res16 = r[:, :324]
        if res is not None:
            assert bool(torch.equal(res16.contiguous().view(torch.int16), res.half().view(torch.int16))), (what, "out_koct is not fp16(out)")
    assert I.unchanged(), (what, "an input changed")
    return (None if res is None else res.cpu().numpy().astype(np.float64)), (None if res16 is None else res16.float().cpu().numpy().astype(np.float64))


def _check_lookup(entry, case, cls, cells, res, res16_alone=None):
    """res [n_img][324][N] against the float64 lookup on the stored cells."""
    _, xy, _ = _host(case["id"], case.get("amp", cc.AMP))
    worst = 0.0
    for img in range(res.shape[0] if res is not None else res16_alone.shape[0]):
        ref, asum, dead = cc.lookup([cells[l][img] for l in range(4)], xy[img])
        bound = cc.lookup_bound(asum)
        if res is not None:
            r = np.abs(res[img] - ref) / bound
            assert np.isfinite(res[img]).all() and not res[img][dead].any(), (entry, case["id"], cls, img, "not zero where every tap is outside")
        else:
            r = np.abs(res16_alone[img] - ref) / cc.koct_alone_bound(ref, bound)
            assert not res16_alone[img][dead].any()
        assert float(r.max()) <= 1.0, (entry, case["id"], cls, img, float(r.max()), np.unravel_index(int(np.argmax(r)), r.shape))
        worst = max(worst, float(r.max()))
    print(f"CORR {entry} {case['id']}: {cls}{'' if res is not None else ' koct alone'} err/bound {worst:.3f}")


def lookup_rows(dev, case, Lv, I, place="tight", koct=False, only=None):
    h, w, N = case["h"], case["w"], case["h"] * case["w"]
    B, pairs = (case["B"], case["pairs"]) if only is None else (1, 1)
    out, ko = _outputs(dev, B * pairs, N, place, True, koct)
    b, t = only or (0, 0)
    args = dict(coords=I.coords(b * case["pairs"] + t, N), B=B, pairs=pairs, h=h, w=w, num_levels=4, radius=4,
                vol_precision=cc.F16 if Lv.cell16 else cc.F16X3, **Lv.args(*((None,) if only is None else (b, t))), **_out_args(out, ko))
    what = (case["id"], "lookup", Lv.cell16, Lv.pitched, place, koct, only)
    _ok(_call("sf_corr_lookup_pitched" if Lv.pitched else "sf_corr_lookup", LOOKP if Lv.pitched else LOOK, args), what)
    return _check_outputs(what, out, ko, I)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pyramid_build_and_lookup(dev, case):
    n_img = case["B"] * case["pairs"]
    for k, (prec, cls) in enumerate(PRECISIONS):
        K = cc.klass(cls)
        Lv, I = build_pyramid(dev, case, prec)
        cells = Lv.decode()
        _check_cells("build_pyramid", case, cls, cells, K)
        # placed = contiguous, bitwise (the 16-byte aligned placement with gaps, "c", goes through the pitched entry below)
        placed = {}
        for place in {"fp32": ("a",), "x3": ("b",), "f16": ("a", "b")}[cls]:         # fp16 cells: an even and an odd lvl_pair_stride
            placed[place] = build_pyramid(dev, case, prec, place=place, separate=case["pairs"] > 1 and k == 1)
            for l, (a, b) in enumerate(zip(cells, placed[place][0].decode())):
                assert _same(a, b), (case["id"], cls, place, l, "placed run differs from the contiguous one")
        if case["pairs"] > 1:                                                      # f2 in a buffer of its own: the same operands, the same bits
            LvS, _ = build_pyramid(dev, case, prec, separate=True)
            assert all(_same(a, b) for a, b in zip(cells, LvS.decode())), (case["id"], cls, "separate frames differ from shared ones")
        if n_img > 1:                                                              # image (b, t) of the batch = the call on that pair alone
            for img in range(n_img):
                Lv1, _ = build_pyramid(dev, case, prec, only=divmod(img, case["pairs"]))
                for l, (a, b) in enumerate(zip(cells, Lv1.decode())):
                    assert _same(a[img], b[0]), (case["id"], cls, img, l, "batch differs from the single call")
        # pitched maps: the data cells are the dense ones, bitwise
        pitched = {}
        for kind in (("exact", "line", "between") if prec == cc.F16X3 else (("between",) if prec == cc.FP32 else ("line",))):
            LvQ, IQ = build_pyramid(dev, case, prec, place="tight" if kind == "line" else ("b" if prec == cc.FP32 else "c"), pitch=kind)
            for l, (a, b) in enumerate(zip(cells, LvQ.decode())):
                assert _same(a, b), (case["id"], cls, kind, l, "pitched data cells differ from the dense ones")
            pitched[kind] = (LvQ, IQ)
        if prec == cc.FP32:
            continue
        # lookups on the stored cells
        res, _ = lookup_rows(dev, case, Lv, I)
        _check_lookup("lookup", case, cls, cells, res)
        LvB, IB = placed["b"]                                                      # levels 12 / 4 / 8 bytes off 16, odd strides
        resP, _ = lookup_rows(dev, case, LvB, IB, place="b")
        assert _same(res, resP), (case["id"], cls, "placed lookup differs from the contiguous one")
        if Lv.cell16:
            # `out` aligned with out_img_stride > 324 N ("c": the concatenation buffer of the engine, the 16-byte-store kernel where
            # N % 4 == 0) and off 16 bytes ("a", "b": the dword kernel); the k-octet copy tight and inside a wider buffer
            for out_place, koct in (("c", False), ("tight", True), ("a", True), ("b", True), ("c", True)):
                resK, _ = lookup_rows(dev, case, Lv, I, place=out_place, koct=koct)
                assert _same(res, resK), (case["id"], cls, out_place, koct, "placed lookup / lookup with a k-octet copy differs")
        else:
            for kind, (LvQ, IQ) in pitched.items():
                resQ, _ = lookup_rows(dev, case, LvQ, IQ, place="tight" if kind == "line" else "c")
                assert _same(res, resQ), (case["id"], cls, kind, "pitched lookup differs from the dense one")
        if n_img > 1:
            for img in range(n_img):
                r1, _ = lookup_rows(dev, case, Lv, I, only=divmod(img, case["pairs"]), koct=Lv.cell16)
                assert _same(res[img], r1[0]), (case["id"], cls, img, "batched lookup differs from the single call")


# ---- blocked volumes ---------------------------------------------------------------------------------------------------------------------------
class Volume:
    """n_img images at `stride` bytes in a buffer of 0xFF bytes, the base `off` bytes past a 256-byte aligned allocation."""

    def __init__(self, dev, n_img, h, w, f32cells, off=0, extra=0):
        self.n_img, self.h, self.w, self.f32 = n_img, h, w, f32cells
        self.g = cc.blocked_geometry(h, w, f32cells)
        self.img_bytes = self.g["src_rows"] * self.g["rec_bytes"]
        self.stride, self.off = self.img_bytes + extra, off
        self.buf = torch.full((off + n_img * self.stride + 256,), 0xFF, dtype=torch.uint8, device=dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def image_ptr(self, img):
        return self.ptr + img * self.stride

    def raw(self):
        return self.buf[self.off:].cpu().numpy()

    def decode(self):
        if getattr(self, "cells", None) is None:
            self.cells = cc.decode_blocked(self.raw(), self.f32, self.n_img, self.h, self.w, self.stride)
        return self.cells

    def check_written(self, what):
        for l, cells in enumerate(self.decode()):
            assert np.isfinite(cells).all(), (what, l, "a data cell was not written or is not finite")
        inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        for img in range(self.n_img):
            inside[self.off + img * self.stride: self.off + img * self.stride + self.img_bytes] = True
        assert bool((self.buf[~inside] == 0xFF).all()), (what, "a byte outside the images changed")

    def moved(self, dev, off):
        """The built volume copied to another base (16-byte but not 128-byte aligned for off = 16)."""
        V = Volume(dev, self.n_img, self.h, self.w, self.f32, off, self.stride - self.img_bytes)
        V.buf[off: off + self.n_img * self.stride] = self.buf[self.off: self.off + self.n_img * self.stride]
        return V


def _blocked_sizes(case, f32cells, B, pairs):
    """The size and geometry functions against the restatement; returns the workspace bytes."""
    lib, h, w, D = _L().load(), case["h"], case["w"], case["D"]
    sfx = "blocked32" if f32cells else "blocked"
    rec, srows = C.c_int64(), C.c_int64()
    off, nby, nbx = (C.c_int64 * 4)(), (C.c_int32 * 4)(), (C.c_int32 * 4)()
    _ok(getattr(lib, f"sf_corr_{sfx}_geometry")(h, w, C.byref(rec), off, nby, nbx, C.byref(srows)), "geometry")
    g = cc.blocked_geometry(h, w, f32cells)
    assert (rec.value, list(off), list(nby), list(nbx), srows.value) == (g["rec_bytes"], g["lvl_off"], g["nby"], g["nbx"], g["src_rows"])
    _ok(getattr(lib, f"sf_corr_{sfx}_geometry")(h, w, None, None, None, None, None), "geometry with null outputs")
    for n in (1, B * pairs):
        assert getattr(lib, f"sf_corr_{sfx}_bytes")(n, h, w) == cc.blocked_bytes(n, h, w, f32cells)
    want = cc.blocked32_ws_bytes(B * pairs, D, h, w) if f32cells else cc.blocked_ws_bytes(B * pairs, D, h, w)
    assert getattr(lib, f"sf_corr_build_{sfx}_ws_bytes")(B * pairs, D, h, w) == want
    return want


def build_blocked(dev, case, f32cells, place="tight", separate=False, only=None):
    h, w, D = case["h"], case["w"], case["D"]
    B, pairs = (case["B"], case["pairs"]) if only is None else (1, 1)
    I = Inputs(dev, case, place, separate)
    V = Volume(dev, B * pairs, h, w, f32cells, *((0, 0) if place == "tight" else ((128, 128) if place == "a" else ((384, 384) if place == "b" else (0, 256)))))
    want = _blocked_sizes(case, f32cells, B, pairs)
    ws = GuardedBytes(dev, want)
    b, t = only or (0, 0)
    args = dict(f1=I.f1(b, t), f2=I.f2(b, t), f_clip_stride=I.cs, f_pair_stride=I.ps, vol=V.ptr, vol_img_stride_bytes=V.stride, B=B, pairs=pairs,
                D=D, h=h, w=w, ws=ws.ptr, ws_bytes=want)
    what = (case["id"], "blocked32" if f32cells else "blocked16", place, separate, only)
    _ok(_call("sf_corr_build_blocked32" if f32cells else "sf_corr_build_blocked", BBUILD, args), what)
    V.check_written(what)
    assert I.unchanged() and ws.guards_unchanged(), (what, "an input or a guard band changed")
    return V, I


def lookup_blocked(dev, case, V, I, place="tight", mode="out", only=None):
    h, w, N = case["h"], case["w"], case["h"] * case["w"]
    B, pairs = (case["B"], case["pairs"]) if only is None else (1, 1)
    out, ko = _outputs(dev, B * pairs, N, place, mode != "koct", mode != "out")
    img = 0 if only is None else only[0] * case["pairs"] + only[1]
    args = dict(vol=V.image_ptr(img), vol_img_stride_bytes=V.stride, coords=I.coords(img, N), B=B, pairs=pairs, h=h, w=w, **_out_args(out, ko))
    what = (case["id"], "lookup_blocked32" if V.f32 else "lookup_blocked", place, mode, only)
    if V.f32:
        _ok(_call("sf_corr_lookup_blocked32", B32LOOK, args), what)
    else:
        _ok(_call("sf_corr_lookup_blocked", BLOOK, args), what)
    return _check_outputs(what, out, ko, I)


def _blocked_family(dev, case, f32cells):
    n_img, pairs = case["B"] * case["pairs"], case["pairs"]
    entry, cls = ("blocked32", "x3") if f32cells else ("blocked", "b16")
    K = cc.klass(cls, case["D"], pairs, True) if pairs > 1 else cc.klass(cls, case["D"], 1, False)     # the tight run shares frames
    V, I = build_blocked(dev, case, f32cells)
    cells = V.decode()
    _check_cells("build_" + entry, case, cls, cells, K)
    # "c" keeps the four-pixel pack (N % 4 == 0) with gapped strides, shared frames included; "a" and "b" take the one-pixel pack
    for place in PLACES:
        VP, _ = build_blocked(dev, case, f32cells, place=place)
        assert all(_same(a, b) for a, b in zip(cells, VP.decode())), (case["id"], entry, place, "placed build differs from the contiguous one")
    if pairs > 1:
        # f2 in a buffer of its own: bitwise the shared run where the model packs the same operands (the model decides), else inside the bound
        KS = cc.klass(cls, case["D"], pairs, False)
        VS, _ = build_blocked(dev, case, f32cells, separate=True)
        sep = VS.decode()
        if (KS["pa"], KS["pb"]) == (K["pa"], K["pb"]):
            assert all(_same(a, b) for a, b in zip(cells, sep)), (case["id"], entry, "separate frames differ from shared ones")
        else:
            _check_cells("build_" + entry + " separate", case, cls, sep, KS)
        for place in ("a", "c"):                                                       # placed AND f2 in a buffer of its own
            VQ, _ = build_blocked(dev, case, f32cells, place=place, separate=True)
            assert all(_same(a, b) for a, b in zip(sep, VQ.decode())), (case["id"], entry, place, "placed separate build differs")
    if n_img > 1:
        K1 = cc.klass(cls, case["D"], 1, False)                                        # a single pair is never shared
        for img in range(n_img):
            V1, _ = build_blocked(dev, case, f32cells, only=divmod(img, pairs))
            one = V1.decode()
            if (K1["pa"], K1["pb"]) == (K["pa"], K["pb"]):
                assert all(_same(a[img], b[0]) for a, b in zip(cells, one)), (case["id"], entry, img, "batch differs from the single call")
            else:
                _check_cells("build_" + entry + " single", case, cls, [np.repeat(x, n_img, 0) for x in one], K1, images=[img])
    # lookups
    res, _ = lookup_blocked(dev, case, V, I)
    _check_lookup("lookup_" + entry, case, cls, cells, res)
    VM = V.moved(dev, 16)                                                              # 16-byte, not 128-byte aligned: the lookup asks no more
    assert VM.ptr % 128 == 16
    for place in PLACES:
        resP, _ = lookup_blocked(dev, case, VM, I, place=place)
        assert _same(res, resP), (case["id"], entry, place, "placed lookup differs from the contiguous one")
    if not f32cells:
        for place in ("tight", "a"):
            resB, _ = lookup_blocked(dev, case, VM if place == "a" else V, I, place=place, mode="both")
            assert _same(res, resB), (case["id"], entry, place, "lookup with both outputs differs")
            _, r16 = lookup_blocked(dev, case, V, I, place=place, mode="koct")
            assert _same(r16, res.astype(np.float32).astype(np.float16).astype(np.float64)), (case["id"], entry, place, "k-octet alone is not fp16(out)")
            _check_lookup("lookup_" + entry, case, cls, cells, None, r16)
    if n_img > 1:
        for img in range(n_img):
            r1, _ = lookup_blocked(dev, case, V, I, only=divmod(img, pairs))
            assert _same(res[img], r1[0]), (case["id"], entry, img, "batched lookup differs from the single call")
    return cells, res


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_blocked16_build_and_lookup(dev, case):
    _blocked_family(dev, case, False)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_blocked32_build_and_lookup(dev, case):
    _blocked_family(dev, case, True)


@pytest.mark.parametrize("case", CASES[:10], ids=IDS[:10])
def test_cross_layout(dev, case):
    """One case per grid, built from UNIT-NORMAL features (the scale the existing tolerances were written for; cells are O(1), every lo
    half of the split a normal fp16): blocked32 cells and features against the pitched F16X3 path within the existing 2e-6 / 2e-5,
    blocked fp16 cells against the dense F16 build by the one-fp16-ulp rule of test_blocked_matches_row_major_fp16_path
    (tests/test_corr_cases_cpu.py: a single-product build is beyond these limits).  Each build is also held to its derived bound at
    this scale: the normal-lo branch of the split term."""
    case = dict(case, amp=cc.CROSS_AMP)
    pairs = case["pairs"]
    V32, I = build_blocked(dev, case, True)
    LvQ, IQ = build_pyramid(dev, case, cc.F16X3, pitch="line")
    _check_cells("build_blocked32 unit", case, "x3", V32.decode(), cc.klass("x3"))
    _check_cells("build_pyramid unit", case, "x3", LvQ.decode(), cc.klass("x3"))
    worst = max(float(np.abs(a - b).max()) for a, b in zip(V32.decode(), LvQ.decode()))
    ra, _ = lookup_blocked(dev, case, V32, I)
    rb, _ = lookup_rows(dev, case, LvQ, IQ)
    print(f"CORR cross {case['id']}: cells {worst:.2e} of {cc.CROSS_CELLS:.0e}, features {float(np.abs(ra - rb).max()):.2e} of {cc.CROSS_LOOKUP:.0e}")
    assert worst < cc.CROSS_CELLS and float(np.abs(ra - rb).max()) < cc.CROSS_LOOKUP
    V16, _ = build_blocked(dev, case, False)
    Lv16, _ = build_pyramid(dev, case, cc.F16)
    _check_cells("build_blocked unit", case, "b16", V16.decode(), cc.klass("b16", case["D"], pairs, pairs > 1))
    _check_cells("build_pyramid unit", case, "f16", Lv16.decode(), cc.klass("f16"))
    for x, y in zip(Lv16.decode(), V16.decode()):
        assert (np.abs(x - y) <= cc.cross_f16_ulp(x)).all()


# ---- refusals: every one is made before any launch (SF_REQUIRE in the three files); nothing is touched --------------------------------------------
def _refused(name, names, args, objs, **over):
    status = _call(name, names, args, **over)
    msg = _L().load().sf_last_error()
    assert status < 0 and msg, (name, over, status, "not refused")
    for o in objs:
        if isinstance(o, (Levels,)):
            assert o.untouched(), (name, over, "a level buffer was touched")
        elif isinstance(o, Volume):
            assert bool((o.buf == 0xFF).all()), (name, over, "the volume was touched")
        elif isinstance(o, GuardedBytes):
            assert o.guards_unchanged() and bool((o.view() == 0x7F).all()), (name, over, "the workspace was touched")
        elif isinstance(o, Guarded):
            assert bool(torch.isnan(o.buf).all()), (name, over, "an output was touched")
        else:
            assert o.unchanged(), (name, over, "an input was touched")


def test_refusals_pyramid(dev):
    case = dict(CASES[0])                                                              # 8 x 8, D = 256, pairs = 3
    h, w, D, B, pairs, N = 8, 8, 256, 1, 3, 64
    I = Inputs(dev, case)
    for prec in (cc.F16X3, cc.F16):
        Lv = Levels(dev, B, pairs, h, w, prec == cc.F16, place="c")
        wsb = cc.build_ws_bytes(B, pairs, D, h, w)
        ws = GuardedBytes(dev, wsb)
        objs = (I, Lv, ws)
        args = dict(f1=I.f1(), f2=I.f2(), f_clip_stride=I.cs, f_pair_stride=I.ps, B=B, pairs=pairs, D=D, h=h, w=w, num_levels=4, precision=prec,
                    split_ws=ws.ptr, split_ws_bytes=wsb, **Lv.args())
        for p in ("f1", "f2", "lvl0", "lvl1", "lvl2", "lvl3", "split_ws", "lvl_pair_stride"):
            _refused("sf_corr_build_pyramid", BUILD, args, objs, **{p: None})
        for over in (dict(h=7), dict(w=7), dict(num_levels=3), dict(num_levels=5), dict(precision=2), dict(precision=4),
                     dict(split_ws_bytes=wsb - 1), dict(split_ws=ws.ptr + 8)):
            _refused("sf_corr_build_pyramid", BUILD, args, objs, **over)
        for l in range(4):
            lo, hi = [8 >> k for k in range(4)], [8 >> k for k in range(4)]
            lo[l] -= 1
            hi[l] = 33
            for p in (lo, hi):
                _refused("sf_corr_build_pyramid_pitched", BUILDP, args, objs, lvl_pitch=_i32x4(p))
        out, ko = _outputs(dev, B * pairs, N, "tight", True, True)
        objs = (I, Lv, out, ko)
        largs = dict(coords=I.coords(), B=B, pairs=pairs, h=h, w=w, num_levels=4, radius=4, vol_precision=prec, **Lv.args(),
                     **_out_args(out, ko if prec == cc.F16 else None))
        for p in ("lvl0", "lvl1", "lvl2", "lvl3", "coords", "out", "lvl_pair_stride"):
            _refused("sf_corr_lookup", LOOK, largs, objs, **{p: None})
        for over in (dict(num_levels=3), dict(radius=3), dict(radius=5)):
            _refused("sf_corr_lookup", LOOK, largs, objs, **over)
        if prec == cc.F16:
            _refused("sf_corr_lookup_pitched", LOOKP, largs, objs, lvl_pitch=_i32x4([8, 4, 2, 1]))          # a pitched lookup of fp16 cells
            _refused("sf_corr_lookup", LOOK, largs, objs, out_koct=ko.ptr + 8)
            _refused("sf_corr_lookup", LOOK, largs, objs, out_koct_img_stride=ko.stride + 4)
        else:
            _refused("sf_corr_lookup", LOOK, largs, objs, out_koct=ko.ptr, out_koct_img_stride=ko.stride)    # out_koct with fp32 cells
            _refused("sf_corr_lookup_pitched", LOOKP, largs, objs, lvl_pitch=_i32x4([8, 4, 1, 1]))          # a pitch below w >> l


@pytest.mark.parametrize("f32cells", [False, True], ids=["blocked16", "blocked32"])
def test_refusals_blocked(dev, f32cells):
    case = dict(CASES[0])
    h, w, D, B, pairs, N = 8, 8, 256, 1, 3, 64
    I = Inputs(dev, case)
    V = Volume(dev, B * pairs, h, w, f32cells, 0, 128)
    wsb = cc.blocked32_ws_bytes(3, D, h, w) if f32cells else cc.blocked_ws_bytes(3, D, h, w)
    ws = GuardedBytes(dev, wsb)
    objs = (I, V, ws)
    name = "sf_corr_build_blocked32" if f32cells else "sf_corr_build_blocked"
    args = dict(f1=I.f1(), f2=I.f2(), f_clip_stride=I.cs, f_pair_stride=I.ps, vol=V.ptr, vol_img_stride_bytes=V.stride, B=B, pairs=pairs, D=D,
                h=h, w=w, ws=ws.ptr, ws_bytes=wsb)
    for p in ("f1", "f2", "vol", "ws"):
        _refused(name, BBUILD, args, objs, **{p: None})
    for over in (dict(h=7), dict(w=7), dict(ws_bytes=wsb - 1), dict(ws=ws.ptr + 8), dict(vol=V.ptr + 64), dict(vol=V.ptr + 16),
                 dict(vol_img_stride_bytes=V.img_bytes - 128), dict(vol_img_stride_bytes=V.stride + 64)):
        _refused(name, BBUILD, args, objs, **over)
    if not f32cells:
        _refused(name, BBUILD, args, objs, D=257)
    out, ko = _outputs(dev, B * pairs, N, "tight", True, not f32cells)
    objs = (I, V, out) + (() if ko is None else (ko,))
    largs = dict(vol=V.ptr, vol_img_stride_bytes=V.stride, coords=I.coords(), B=B, pairs=pairs, h=h, w=w, **_out_args(out, ko))
    name, names = ("sf_corr_lookup_blocked32", B32LOOK) if f32cells else ("sf_corr_lookup_blocked", BLOOK)
    for p in ("vol", "coords"):
        _refused(name, names, largs, objs, **{p: None})
    for over in (dict(h=7), dict(w=7), dict(vol=V.ptr + 8), dict(vol_img_stride_bytes=V.stride + 8)):
        _refused(name, names, largs, objs, **over)
    if f32cells:
        _refused(name, names, largs, objs, out=None)
    else:
        _refused(name, names, largs, objs, out=None, out_koct=None)                                           # both outputs null
        _refused(name, names, largs, objs, out_koct=ko.ptr + 8)
        _refused(name, names, largs, objs, out_koct_img_stride=ko.stride + 4)
    lib = _L().load()
    sfx = "blocked32" if f32cells else "blocked"
    for hh, ww in ((7, 8), (8, 7)):
        assert getattr(lib, f"sf_corr_{sfx}_geometry")(hh, ww, None, None, None, None, None) < 0 and lib.sf_last_error()
