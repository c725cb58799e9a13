"""The volume-free correlation route through the C ABI (-m gpu): sf_corr_direct_ws_bytes / sf_corr_direct_pack / sf_corr_direct_lookup
(csrc/corr_direct.hip) -- raw pointers and strides handed to streamflow_amd._lib.load(), at the shapes of tests/corr_cases.py and the
four coordinate sets of tests/corr_direct_cases.py (noise + the 20 fixed edge / NaN / inf pixels; uniformly random: the box is the
whole level; a whole tile dead; one pixel of a tile in the opposite corner).

Features sit in NaN-filled buffers, the workspace is exactly the bytes the size function returns between guard bands and is filled
with 0xFF bytes (NaN halves) before the pack, outputs sit in sentinel-filled buffers.  Asserted: status 0; every channel finite and
within the DERIVED bound of the float64 reference (both classes); exactly zero where every tap is outside; out_koct bitwise fp16(out),
rows 324..327 zero; nothing outside the views and the workspace written, the features unchanged; out alone / out_koct alone / both
bitwise the same; the placed run (bases off 16 bytes, strides with gaps) bitwise the contiguous one; image (b, t) of a batch bitwise
the call on that pair alone; a shared frame bitwise separate buffers; a pixel's channels bitwise unchanged when only OTHER pixels'
coordinates change; the workspace's earlier contents (zeros, NaN, 3e38) without influence; bad arguments refused with the documented
codes.  err / bound is printed per case ("CORRD ...").

Worst err / bound measured on the MI355X over the 13 cases and four coordinate sets (99 tests, 12 s) -- a record, not a threshold:
F16 0.451, F16X3 0.462 (both at D = 1, where the error IS the two operand roundings and the bound's factor 2 is the margin)."""
import numpy as np
import pytest
import torch

from tests import corr_cases as cc
from tests import corr_direct_cases as dc
from tests.guarded import SENTINEL, Guarded, GuardedBytes

pytestmark = pytest.mark.gpu
CASES = dc.cases()
IDS = [c["id"] for c in CASES]
KL = list(dc.KLASSES)
BAD_ARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _L():
    from streamflow_amd import _lib as L
    return L


def _ok(status, what):
    assert status == 0, f"{what}: refused ({status}): {_L().load().sf_last_error().decode(errors='replace')}"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a.view(np.int16)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(_bits(a), _bits(b)))


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


def run(dev, F, xy, h, w, precision, placed=False, outs=("out", "koct"), separate=False, ws_fill=0xFF, ws_f32=None):
    """Pack + lookup of the frames F [B][pairs + 1][D][N] at coordinates xy [n][2][N].  Returns (out [n][324][N] fp32 or None,
    koct [n][328][N] fp16 or None); asserts the statuses, the guard bands and that the inputs are unchanged."""
    lib = _L().load()
    B, T1, D, N = F.shape
    pairs, n = T1 - 1, B * (T1 - 1)
    DN = D * N
    ps = DN + (7 if placed else 0)
    cs = T1 * ps + (5 if placed else 0)
    fr1 = Frames(dev, F, 1 if placed else 0, ps, cs)
    fr2 = Frames(dev, np.concatenate([F[:, 1:], F[:, :1]], 1), 3 if placed else 0, ps, cs) if separate else None
    f1, f2 = fr1.ptr(0, 0), (fr2.ptr(0, 0) if separate else fr1.ptr(0, 1))
    need = lib.sf_corr_direct_ws_bytes(B, pairs, D, h, w, precision)
    assert need == dc.ws_bytes(B, pairs, D, h, w, precision)
    ws = GuardedBytes(dev, need, fill=ws_fill)
    if ws_f32 is not None:
        ws.view().view(torch.float32).fill_(ws_f32)
    coff = 1 if placed else 0
    cbuf = torch.full((coff + n * 2 * N + 3,), float("nan"), dtype=torch.float32, device=dev)
    cbuf[coff: coff + n * 2 * N] = torch.from_numpy(np.array(xy, np.float32).reshape(-1)).to(dev)
    csnap = cbuf.clone()
    O = Guarded(dev, n, 324, N, 3 if placed else 0, N, 324 * N + (5 if placed else 0), SENTINEL) if "out" in outs else None
    K = (Guarded(dev, n, 328, N, 8 if placed else 0, N, 41 * N * 8 + (24 if placed else 0), SENTINEL, dtype=torch.float16, koct=True)
         if "koct" in outs else None)
    _ok(lib.sf_corr_direct_pack(f1, f2, cs, ps, ws.ptr, need, B, pairs, D, h, w, precision, _L().stream()), "sf_corr_direct_pack")
    _ok(lib.sf_corr_direct_lookup(ws.ptr, cbuf.data_ptr() + 4 * coff, None if O is None else O.ptr, 0 if O is None else O.stride,
                                  None if K is None else K.ptr, 0 if K is None else K.stride, B, pairs, D, h, w, precision,
                                  _L().stream()), "sf_corr_direct_lookup")
    torch.cuda.synchronize()
    assert ws.guards_unchanged(), "a byte outside the workspace was written"
    assert fr1.unchanged() and (fr2 is None or fr2.unchanged()), "features were written"
    assert torch.equal(cbuf.view(torch.int32), csnap.view(torch.int32)), "coordinates were written"
    assert O is None or O.outside_unchanged(), "out: written outside the view"
    assert K is None or K.outside_unchanged(), "out_koct: written outside the view"
    return (None if O is None else O.region().cpu().numpy(), None if K is None else K.region().cpu().numpy())


def _precision(k):
    return dc.KLASSES[k]["precision"]


# ---- the values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KL)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_channel_within_the_derived_bound(dev, case, k):
    h, w = case["h"], case["w"]
    for cs in dc.COORD_SETS:
        ref = dc.reference(case["id"], cs)
        out, koct = run(dev, ref["F"], ref["xy"], h, w, _precision(k))
        assert np.isfinite(out).all() and np.isfinite(koct.astype(np.float32)).all(), cs
        assert (out[ref["dead"]] == 0).all(), f"{cs}: not exactly zero where every tap is outside"
        ratio = np.abs(out.astype(np.float64) - ref["out"]) / ref["bound"][k]
        print(f"CORRD {case['id']} {k} {cs}: err / bound {ratio.max():.3f}  (bound max {ref['bound'][k].max():.3g})")
        assert ratio.max() <= 1.0, (cs, float(ratio.max()))
        assert _same(koct[:, :324], out.astype(np.float16)), f"{cs}: out_koct is not fp16(out)"
        assert (_bits(koct[:, 324:]) == 0).all(), f"{cs}: rows 324..327 not zero"


@pytest.mark.parametrize("k", KL)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_outputs_alone_and_placed_runs_are_bitwise_the_same(dev, case, k):
    ref = dc.reference(case["id"], "noise")
    args = (dev, ref["F"], ref["xy"], case["h"], case["w"], _precision(k))
    out, koct = run(*args)
    o1, _ = run(*args, outs=("out",))
    _, k1 = run(*args, outs=("koct",))
    op, kp = run(*args, placed=True)
    assert _same(out, o1) and _same(koct, k1), "one output alone differs from both"
    assert _same(out, op) and _same(koct, kp), "the placed run differs from the contiguous one"


BATCHES = [c for c in CASES if c["B"] * c["pairs"] > 1]


@pytest.mark.parametrize("k", KL)
@pytest.mark.parametrize("case", BATCHES, ids=[c["id"] for c in BATCHES])
def test_batch_equals_the_single_pair_and_shared_equals_separate(dev, case, k):
    h, w = case["h"], case["w"]
    for cs in ("noise", "uniform"):
        ref = dc.reference(case["id"], cs)
        out, koct = run(dev, ref["F"], ref["xy"], h, w, _precision(k))
        osep, ksep = run(dev, ref["F"], ref["xy"], h, w, _precision(k), separate=True)
        assert _same(out, osep) and _same(koct, ksep), f"{cs}: f2 in a buffer of its own differs from the shared frames"
        for b in range(case["B"]):
            for t in range(case["pairs"]):
                img = b * case["pairs"] + t
                o1, k1 = run(dev, ref["F"][b: b + 1, t: t + 2], ref["xy"][img: img + 1], h, w, _precision(k))
                assert _same(out[img: img + 1], o1) and _same(koct[img: img + 1], k1), f"{cs}: image ({b}, {t}) alone differs"


@pytest.mark.parametrize("k", KL)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_pixel_does_not_depend_on_its_neighbours_coordinates(dev, case, k):
    """Every third pixel keeps its coordinates, all the others move (noise -> uniform, corner, dead): other boxes, other chunks, other
    positions of its cells inside a chunk -- the kept pixels' 324 values stay bitwise the same."""
    ref = dc.reference(case["id"], "noise")
    h, w = case["h"], case["w"]
    keep = np.arange(h * w) % 3 == 0
    out, _ = run(dev, ref["F"], ref["xy"], h, w, _precision(k), outs=("out",))
    for cs in ("uniform", "corner", "dead_tile"):
        xy = dc.coords(ref["case"], cs).copy()
        xy[:, :, keep] = ref["xy"][:, :, keep]
        o2, _ = run(dev, ref["F"], xy, h, w, _precision(k), outs=("out",))
        assert _same(out[:, :, keep], o2[:, :, keep]), cs


@pytest.mark.parametrize("k", KL)
def test_earlier_contents_of_the_workspace_have_no_influence(dev, k):
    case = [c for c in CASES if c["id"] == "15x17-D24-B1p1"][0]
    ref = dc.reference(case["id"], "noise")
    args = (dev, ref["F"], ref["xy"], case["h"], case["w"], _precision(k))
    runs = [run(*args, ws_fill=0x00), run(*args, ws_fill=0xFF), run(*args, ws_f32=3.0e38)]
    for o, ko in runs[1:]:
        assert _same(o, runs[0][0]) and _same(ko, runs[0][1])


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_the_documented_codes(dev):
    lib, st = _L().load(), _L().stream()
    B, pairs, D, h, w = 1, 1, 8, 8, 9
    N = h * w
    f = torch.zeros(2 * D * N, dtype=torch.float32, device=dev)
    xy = torch.zeros(2 * N, dtype=torch.float32, device=dev)
    out = torch.full((324 * N,), SENTINEL, dtype=torch.float32, device=dev)
    koct = torch.full((41 * N * 8 + 16,), SENTINEL, dtype=torch.float16, device=dev)
    out0, koct0 = out.clone(), koct.clone()
    need = lib.sf_corr_direct_ws_bytes(B, pairs, D, h, w, cc.F16)
    ws = GuardedBytes(dev, need)
    f1, f2 = f.data_ptr(), f.data_ptr() + 4 * D * N
    pack = lambda **o: lib.sf_corr_direct_pack(*[{**dict(f1=f1, f2=f2, cs=2 * D * N, ps=D * N, ws=ws.ptr, wsb=need, B=B, pairs=pairs,
                                                         D=D, h=h, w=w, prec=cc.F16), **o}[x]
                                                 for x in ("f1", "f2", "cs", "ps", "ws", "wsb", "B", "pairs", "D", "h", "w", "prec")], st)
    look = lambda **o: lib.sf_corr_direct_lookup(*[{**dict(ws=ws.ptr, xy=xy.data_ptr(), out=out.data_ptr(), os=324 * N, ko=koct.data_ptr(),
                                                           ks=41 * N * 8, B=B, pairs=pairs, D=D, h=h, w=w, prec=cc.F16), **o}[x]
                                                   for x in ("ws", "xy", "out", "os", "ko", "ks", "B", "pairs", "D", "h", "w", "prec")], st)
    assert pack(prec=cc.FP32) == UNSUPPORTED and look(prec=cc.FP32) == UNSUPPORTED and pack(prec=2) == UNSUPPORTED
    assert lib.sf_corr_direct_ws_bytes(B, pairs, D, h, w, cc.FP32) == 0
    assert pack(h=7) == BAD_ARG and look(w=7) == BAD_ARG                                    # a grid below 8 x 8
    assert pack(wsb=need - 1) == BAD_ARG and pack(ws=ws.ptr + 4) == BAD_ARG and pack(f1=None) == BAD_ARG
    assert look(out=None, ko=None) == BAD_ARG                                               # both outputs NULL
    assert look(ko=koct.data_ptr() + 2) == BAD_ARG and look(ko=koct.data_ptr() + 8) == BAD_ARG and look(ks=41 * N * 8 + 4) == BAD_ARG
    assert look(D=257) == UNSUPPORTED
    torch.cuda.synchronize()
    assert ws.guards_unchanged() and bool((ws.view() == 0x7F).all()), "a refused call wrote the workspace"
    assert torch.equal(out, out0) and torch.equal(koct, koct0), "a refused call wrote an output"
    assert pack() == 0 and look() == 0 and look(out=None) == 0 and look(ko=None) == 0
    torch.cuda.synchronize()
