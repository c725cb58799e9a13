"""sft_track_advance and sft_draw_tracks on the GPU, through the raw C ABI of libstreamflow_track with guard bands around every
buffer, BITWISE against the numpy float32 restatements of tests/track_cases.py (advance32, draw32).

Shapes: fields of 1 x 1, 2 x 2, 5 x 7 and 3 x 300 (a row longer than a block), 1 .. 1000 points (one wave less one, one wave, one
more, more than a block, several blocks), dense mode where h * w is no multiple of 64, 1, 2 and 7 steps; fields as views with row,
channel and field strides larger than dense, NaN in the gaps.  Content: smooth flows of about 2 px, and the special set (NaN, +-Inf,
1e30, -0.0 in flows and queries, points on x = w - 1 / y = h - 1, flows that land exactly on the border and one ulp beyond).

Both entry points are also held to the two properties tests/test_gpu_media_state.py holds the main ABI to: (a) a case run in
buffers another case used is bitwise the fresh-buffer result and changes no byte outside its extent; (b) an eager call on a side
stream, a capture in torch's default capture mode and three replays with changed static inputs are each bitwise the eager result."""
import numpy as np
import pytest
import torch

from tests import track_cases as tc
from tests.guarded import GuardedBytes

pytestmark = pytest.mark.gpu

FILL = 0x7F
IN, OUT, WS = "in", "out", "ws"
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def lib():
    from streamflow_amd import _track_lib
    return _track_lib.load()


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Bound:
    """One call: its buffers (name -> (role, input bytes or output size)), how to make it, and what it must write."""

    def __init__(self, entry, bufs, call, want):
        self.entry, self.bufs, self.call, self.want = entry, bufs, call, want

    def sizes(self):
        return {n: (len(v) if r == IN else int(v)) for n, (r, v) in self.bufs.items()}

    def nbytes(self, name):
        return self.sizes()[name]


class Buffers:
    def __init__(self, dev, sizes):
        self.g = {n: GuardedBytes(dev, max(s, 4), fill=FILL) for n, s in sizes.items()}

    def load(self, bound):
        for n, (r, v) in bound.bufs.items():
            if r == IN and len(v):
                self.g[n].view()[:len(v)].copy_(torch.from_numpy(v))

    def launch(self, bound, stream=None):
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        rc = bound.call(lib(), lambda n: self.g[n].ptr, s)
        assert rc == 0, (bound.entry, rc, lib().sft_last_error())

    def read(self, bound):
        torch.cuda.synchronize()
        return {n: self.g[n].view()[:bound.nbytes(n)].cpu().numpy() for n, (r, _) in bound.bufs.items() if r == OUT}

    def whole(self):
        torch.cuda.synchronize()
        return {n: g.view().cpu().numpy() for n, g in self.g.items()}

    def guards_unchanged(self):
        return all(g.guards_unchanged() for g in self.g.values())


def check(bound, got, what=""):
    for n, w in bound.want.items():
        bad = int((got[n] != w).sum())
        assert bad == 0, f"{bound.entry} {what}: {bad} of {w.size} bytes of `{n}` differ from the restatement"


def fresh(dev, bound, repeat=False):
    bufs = Buffers(dev, bound.sizes())
    bufs.load(bound)
    bufs.launch(bound)
    got = bufs.read(bound)
    assert bufs.guards_unchanged(), f"{bound.entry}: a guard band was written"
    check(bound, got)
    if repeat:
        bufs.launch(bound)
        again = bufs.read(bound)
        assert all(np.array_equal(again[n], got[n]) for n in got) and bufs.guards_unchanged()
    return got


# ---- sft_track_advance --------------------------------------------------------------------------------------------------------------

def advance_bound(fwd, bwd=None, queries=None, frame0=0, alpha=tc.ALPHA, beta=tc.BETA, sticky=False, views=True, state=None,
                  dense_null=False, in_place=False, use_start=True):
    """fwd / bwd float32 [K, 2, h, w].  queries [P, 3] (state PENDING) or `state` = (xy, status, start); dense_null: NULL state."""
    K, _, h, w = fwd.shape
    if dense_null:
        sxy = sst = start = None
        P = h * w
    elif state is not None:
        sxy, sst, start = state
        P = sxy.shape[1]
    else:
        sxy, sst, start = tc.initial_state(queries, h, w)
        P = sxy.shape[1]
    if not use_start:
        start = None
    want_xy, want_st, want_counts = tc.advance32(fwd, bwd, sxy, sst, start, frame0, alpha, beta, sticky)
    bufs, strides = {}, {}
    for name, f in (("fwd", fwd), ("bwd", bwd)):
        if f is None:
            strides[name] = (0, 0, 0, None)
            continue
        if views:
            buf, view = tc.strided(f, row_pad=3 if name == "fwd" else 1, ch_pad=2, field_pad=5)
            off = 16
        else:
            buf, view, off = np.ascontiguousarray(f), np.ascontiguousarray(f), 0
        bufs[name] = (IN, raw(buf))
        strides[name] = tuple(s // 4 for s in view.strides[:3]) + (off,)
    if sxy is not None:
        bufs["sxy"], bufs["sst"] = (IN, raw(sxy.astype(F32))), (IN, raw(sst))
        if start is not None:
            bufs["start"] = (IN, raw(start.astype(np.int32)))
    bufs["oxy"], bufs["ost"], bufs["counts"] = (OUT, K * 2 * P * 4), (OUT, K * P), (OUT, K * 16)
    want = {"oxy": raw(want_xy), "ost": raw(want_st), "counts": raw(want_counts.astype(np.uint32))}
    if not in_place:
        bufs["sxo"], bufs["sso"] = (OUT, 2 * P * 4), (OUT, P)
        want["sxo"], want["sso"] = raw(want_xy[-1]), raw(want_st[-1])

    def call(lb, ptr, stream):
        f, b = strides["fwd"], strides["bwd"]
        sxo = ptr("sxy") if in_place else ptr("sxo")
        sso = ptr("sst") if in_place else ptr("sso")
        return lb.sft_track_advance(ptr("fwd") + f[3], f[0], f[1], f[2], None if bwd is None else ptr("bwd") + b[3], b[0], b[1], b[2], K, h, w,
                                    frame0, None if sxy is None else ptr("sxy"), None if sxy is None else ptr("sst"),
                                    None if start is None else ptr("start"), P, alpha, beta, int(sticky), ptr("oxy"), ptr("ost"), sxo, sso,
                                    ptr("counts"), None, 0, stream)

    b = Bound("sft_track_advance", bufs, call, want)
    b.rows = (want_xy, want_st)
    return b


FIELDS = [(1, 1), (2, 2), (5, 7), (3, 300)]
POINTS = [1, 63, 64, 65, 257, 1000]


@pytest.mark.parametrize("K", [1, 2, 7])
@pytest.mark.parametrize("hw", FIELDS)
def test_advance_is_bitwise_the_restatement(dev, hw, K):
    h, w = hw
    seen = set()
    for P in POINTS:
        seed = 100 * K + P
        fwd, bwd = tc.smooth_flows(seed, K, h, w), -tc.smooth_flows(seed + 1, K, h, w)
        q = tc.random_queries(seed, P, h, w, n_frames=K + 1)
        fresh(dev, advance_bound(fwd, bwd, q, sticky=bool(P % 2)), repeat=P == 65)
        sf, sb, sq = tc.special_case(seed + 2, K, h, w, P)
        got = fresh(dev, advance_bound(sf, sb, sq, beta=4.0, frame0=3 if P == 64 else 0))
        seen |= set(np.unique(got["ost"]).tolist())
        # bwd = NULL: the restatement without the visibility test; a poisoned bwd is nowhere in the call
        got = fresh(dev, advance_bound(sf, None, sq, views=P != 257))
        assert not (got["ost"] == tc.OCCLUDED).any()
    assert tc.LOST in seen and (tc.VISIBLE in seen or h * w == 1)      # (on 1 x 1 every flow but zero leaves the frame)


@pytest.mark.parametrize("hw", [(5, 7), (3, 300)])
def test_dense_mode_equals_explicit_grid_points(dev, hw):
    h, w = hw
    for K, seed in ((1, 0), (7, 1)):
        sf, sb, _ = tc.special_case(seed + 30, K, h, w, 16)
        fwd = sf if K == 1 else tc.smooth_flows(seed, K, h, w, amp=1.0)
        bwd = sb if K == 1 else -tc.smooth_flows(seed, K, h, w, amp=1.0)
        null = fresh(dev, advance_bound(fwd, bwd, dense_null=True), repeat=True)
        gx, gs = tc.grid_state(h, w)
        explicit = fresh(dev, advance_bound(fwd, bwd, state=(gx, gs, None)))
        assert all(np.array_equal(null[n], explicit[n]) for n in ("oxy", "ost", "counts", "sxo", "sso"))


def test_carried_state_split_and_in_place(dev):
    h, w, K, P = 5, 7, 7, 65
    sf, sb, q = tc.special_case(77, K, h, w, P)
    q[:, 0] = np.arange(P) % (K + 1)                                     # starts in both halves
    whole = advance_bound(sf, sb, q, sticky=True, beta=4.0)
    got = fresh(dev, whole)
    sxy, sst, start = tc.initial_state(q, h, w)
    a = fresh(dev, advance_bound(sf[:3], sb[:3], state=(sxy, sst, start), sticky=True, beta=4.0))
    carried = (a["sxo"].view(F32).reshape(2, P), a["sso"], start)
    b = fresh(dev, advance_bound(sf[3:], sb[3:], state=carried, frame0=3, sticky=True, beta=4.0))
    for n in ("oxy", "ost", "counts"):
        assert np.array_equal(np.concatenate([a[n], b[n]]), got[n]), n
    assert np.array_equal(b["sxo"], got["sxo"]) and np.array_equal(b["sso"], got["sso"])
    # state written over the inputs: the same rows, and the state buffers hold the last row afterwards
    bound = advance_bound(sf, sb, q, sticky=True, beta=4.0, in_place=True)
    bufs = Buffers(dev, bound.sizes())
    bufs.load(bound)
    bufs.launch(bound)
    inp = bufs.read(bound)
    check(bound, inp)
    left = bufs.whole()
    assert bufs.guards_unchanged()
    assert np.array_equal(left["sxy"][:8 * P], got["sxo"]) and np.array_equal(left["sst"][:P], got["sso"])


def advance_cases(which, v=0):
    """Case A: 7 steps of 1000 points on 3 x 300 with bwd; case B: 2 steps of 65 points on 5 x 7 without.  v: other content, same geometry."""
    if which == "A":
        sf, sb, q = tc.special_case(200 + v, 7, 3, 300, 1000)
        return advance_bound(sf, sb, q, beta=4.0, sticky=True)
    sf, _, q = tc.special_case(300 + v, 2, 5, 7, 65)
    return advance_bound(sf, None, q, frame0=1)


# ---- sft_draw_tracks ----------------------------------------------------------------------------------------------------------------

def draw_bound(seed, P, trail, h=13, w=70, n=2, n_rows=6, first_frame=3, first_row=0, occ=False, planar=False, radius=3, trail_radius=1):
    xy, status = tc.draw_case(seed, n_rows, P, h, w)
    rng = np.random.default_rng(seed + 1000)
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    pal = tc.small_palette()
    alpha = np.linspace(255, 60, trail).astype(np.uint8)
    want = tc.draw32(frames, first_frame, xy, status, first_row, trail, radius, trail_radius, pal, alpha, occ)
    src = np.ascontiguousarray(frames.transpose(0, 3, 1, 2)) if planar else frames
    s = (h * w * 3, w, 1, h * w) if planar else (h * w * 3, w * 3, 3, 1)
    bufs = {"src": (IN, raw(src)), "xy": (IN, raw(xy)), "st": (IN, raw(status)), "pal": (IN, raw(pal)), "at": (IN, raw(alpha)),
            "out": (OUT, n * h * w * 3), "ws": (WS, n * h * w * 4)}

    def call(lb, ptr, stream):
        return lb.sft_draw_tracks(ptr("src"), s[0], s[1], s[2], s[3], n, h, w, first_frame, ptr("xy"), ptr("st"), n_rows, P, first_row, trail,
                                  radius, trail_radius, int(occ), ptr("pal"), len(pal), ptr("at"), ptr("out"), ptr("ws"), n * h * w * 4, stream)

    b = Bound("sft_draw_tracks", bufs, call, {"out": raw(want)})
    b.frames = frames
    return b


@pytest.mark.parametrize("trail", [1, 4])
@pytest.mark.parametrize("P", [1, 65])
def test_draw_is_bitwise_the_restatement(dev, P, trail):
    assert lib().sft_draw_tracks_ws_bytes(2, 13, 70) == 2 * 13 * 70 * 4
    first = draw_bound(P, P, trail)
    got = fresh(dev, first, repeat=True)
    assert (got["out"] != raw(first.frames)).any()
    fresh(dev, draw_bound(P + 1, P, trail, first_frame=2, first_row=1, occ=True, planar=True, radius=16 if P == 1 else 2, trail_radius=0))
    # a second call in the same workspace, with other tracks: the key image is cleared by the call itself
    second = draw_bound(P + 2, P, trail, first_frame=1, first_row=0, occ=True)
    bufs = Buffers(dev, first.sizes())
    for b in (first, second):
        bufs.load(b)
        bufs.launch(b)
        check(b, bufs.read(b), "in a used workspace")
    assert bufs.guards_unchanged()


def draw_cases(which, v=0):
    if which == "A":
        return draw_bound(40 + v, 65, 4, h=13, w=70, n=2, n_rows=6)
    return draw_bound(50 + v, 7, 1, h=6, w=9, n=1, n_rows=3, first_frame=1)


# ---- the two properties of tests/test_gpu_media_state.py ------------------------------------------------------------------------------

ENTRIES = {"sft_track_advance": advance_cases, "sft_draw_tracks": draw_cases}


@pytest.mark.parametrize("order", ["A-then-B", "B-then-A"])
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_used_buffers(dev, entry, order):
    """Every buffer allocated once at the larger of the two cases' sizes; the first case runs, then the second in the same buffers
    with nothing cleared in between.  The second call's outputs are bitwise the restatement (= the call in fresh buffers), every
    byte outside its extent is what the first call left, the inputs come back unchanged, the guard bands are intact."""
    A, B = ENTRIES[entry]("A"), ENTRIES[entry]("B")
    first, second = (A, B) if order == "A-then-B" else (B, A)
    want = fresh(dev, second)
    sa, sb = A.sizes(), B.sizes()
    bufs = Buffers(dev, {n: max(sa.get(n, 0), sb.get(n, 0)) for n in set(sa) | set(sb)})
    bufs.load(first)
    bufs.launch(first)
    torch.cuda.synchronize()
    bufs.load(second)
    before = bufs.whole()
    bufs.launch(second)
    got = bufs.read(second)
    after = bufs.whole()
    assert bufs.guards_unchanged(), f"{entry} {order}: a guard band was written"
    check(second, got, order)
    assert all(np.array_equal(got[n], want[n]) for n in want)
    for n in after:
        role = second.bufs.get(n, (IN, b""))[0]
        keep = np.ones(after[n].size, bool)
        if role != IN:
            keep[:second.nbytes(n)] = False
        bad = int((after[n][keep] != before[n][keep]).sum())
        assert bad == 0, f"{entry} {order}: {bad} bytes of `{n}` ({role}) outside the call's extent changed"


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_side_stream_capture_and_replay(dev, entry):
    """Case A's inputs in static buffers; one eager call on a side stream; one capture of the call on that stream in torch's default
    (global) capture mode, in which a host synchronisation, an allocation or a launch on another stream inside the entry point makes
    the capture raise; three replays, each after new content of the same geometry has been copied into the static inputs and the
    outputs refilled, each bitwise the restatement."""
    bound = ENTRIES[entry]("A", 0)
    bufs = Buffers(dev, bound.sizes())
    bufs.load(bound)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bufs.launch(bound, side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    check(bound, bufs.read(bound), "eager on a side stream")
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph, stream=side):
            bufs.launch(bound, side.cuda_stream)
    finally:
        torch.cuda.synchronize()                                        # (after a capture error: nothing of it reaches the next test)
    for v in range(1, 4):
        other = ENTRIES[entry]("A", v)
        assert other.sizes() == bound.sizes()
        for n, (r, _) in bound.bufs.items():
            if r == OUT:
                bufs.g[n].view().fill_(FILL)
        bufs.load(other)
        graph.replay()
        got = bufs.read(other)
        assert bufs.guards_unchanged(), f"{entry} replay {v}: a guard band was written"
        check(other, got, f"replay {v}")
