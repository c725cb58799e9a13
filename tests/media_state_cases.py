"""The case table of tests/test_gpu_media_state.py: one record per media entry point of include/streamflow_hip.h, each with two
cases, A and B, taken from the modules whose references are already pinned (interp_cases, consistency_cases, resize_cases, jpeg_cases,
jpeg_decode_cases, jpeg_sync_cases, png_cases, png_encode_cases, flo5_encode_cases, flo5_decode_cases, stabilize_cases, video_cases
and the blend restatement of the tile tests).  A and B differ in content and in geometry (image count and size) and A needs at
least as many bytes as B in EVERY buffer the call takes (tests/test_media_state_cases_cpu.py checks that from the *_ws_bytes and
bound functions), so that B can run in buffers A has used and the reverse.  The shapes are the small ones of each module's own GPU
test.  Importing this module launches nothing and needs no GPU; bind() loads the library for its size functions only.

A record's bind(which, variant) gives a Bound: the host bytes of every input (descriptor, table and grid arrays included), the size
of every output, status, stats and workspace buffer, the call through the C ABI on given device addresses, and check(), which holds
the outputs to the module's own reference (the numpy restatement, the PIL fixture or the float64 bound).  `variant` 0 .. 3 is other
content of the SAME geometry and the same byte counts (what a graph replay may change in its static inputs).

COVERED_ELSEWHERE names, for every other entry point of streamflow_amd._lib.SIGNATURES, the test that already runs it on used
buffers or replays it; a new entry point has to be put on one side or the other (tests/test_media_state_cases_cpu.py)."""
import ctypes as C

import numpy as np

IN, OUT, STATUS, STATS, WS = "in", "out", "status", "stats", "ws"
VARIANTS = 4
NOT_ENTRY_POINTS = ("_ws_bytes", "_bound", "_geometry", "_frags", "_layout", "_ok")


def lib():
    from streamflow_amd import _lib
    return _lib.load()


def raw(a):
    """The bytes of an array as uint8 [bytes]."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()


class Buf:
    def __init__(self, role, data=None, nbytes=None):
        self.role, self.data = role, data
        self.nbytes = int(len(data) if data is not None else nbytes)


class Bound:
    """One case of one entry point bound to host data.  bufs: name -> Buf in argument order; call(lib, p, stream) -> the return
    code, p(name) the device address of a buffer; check(outs), outs: name -> uint8 bytes of every buffer that is no input.
    regions(outs) -> name -> (extent, free): boolean masks over a buffer's bytes, for the outputs whose written extent depends on
    the data: `extent` is what the call defines (compared bitwise), `free` what the header leaves unspecified; every other byte
    must stay what it was.  Without an entry a buffer's extent is all its bytes; a workspace is free throughout."""

    def __init__(self, entry):
        self.entry, self.bufs, self.call, self.check, self.regions = entry, {}, None, None, lambda outs: {}

    def add(self, name, role, data=None, nbytes=None):
        self.bufs[name] = Buf(role, None if data is None else raw(data), nbytes)
        return self

    def sizes(self):
        return {k: b.nbytes for k, b in self.bufs.items()}


def vary_u8(a, v):
    """Other bytes of the same shape: rolled along the row axis and shifted in value."""
    return a if v == 0 else ((np.roll(a, v, axis=-2).astype(np.int64) + 37 * v) & 255).astype(np.uint8)


def vary_f32(a, v):
    return a if v == 0 else (np.roll(a, v, axis=-1) * np.float32(1 + 0.25 * v)).astype(np.float32)


def rotate(seq, v):
    seq = list(seq)
    return seq[v % len(seq):] + seq[:v % len(seq)]


def hwc_strides(h, w):
    return (3 * h * w, 3 * w, 3, 1)


def sums_close(got, want, terms, what):
    assert abs(got - want) <= terms * 2.0 ** -52 * abs(want), (what, got, want, terms)


# ---- forward-backward consistency, warping, interpolation --------------------------------------------------------------------------
CONSISTENCY = {"A": (150, 3, 17, 65), "B": (120, 2, 13, 37)}                 # (seed, n, h, w): more than one block a field / one block


def _consistency_inputs(which, v):
    from tests import consistency_cases as cc
    seed, n, h, w = CONSISTENCY[which]
    return cc.make_case(seed + 1000 * v, n, h, w)


def bind_flow_consistency(which, v=0):
    from tests import consistency_cases as cc
    fwd, bwd, _, _ = _consistency_inputs(which, v)
    n, _, h, w = fwd.shape
    b = Bound("sf_flow_consistency").add("fwd", IN, fwd).add("bwd", IN, bwd).add("cls", OUT, nbytes=n * h * w)
    b.add("stats", STATS, nbytes=n * cc.LEN * 8).add("ws", WS, nbytes=lib().sf_flow_consistency_ws_bytes(n, h, w))
    ws_bytes = b.bufs["ws"].nbytes
    b.call = lambda L, p, s: L.sf_flow_consistency(p("fwd"), 2 * h * w, h * w, w, p("bwd"), 2 * h * w, h * w, w, n, h, w, cc.ALPHA, cc.BETA,
                                                   0, 1, 2, p("cls"), p("stats"), p("ws"), ws_bytes, s)

    def check(outs):
        want_cls, want, _, _ = cc.restate32(fwd, bwd)
        assert np.array_equal(outs["cls"].reshape(n, h, w), want_cls)
        stats = outs["stats"].view(np.float64).reshape(n, cc.LEN)
        for i in range(n):
            for k in (cc.PIXELS, cc.VISIBLE, cc.OCCLUDED, cc.OUTSIDE, cc.FINITE):
                assert stats[i, k] == want[i, k], (i, k, stats[i], want[i])
            sums_close(stats[i, cc.SUM_FB], want[i, cc.SUM_FB], want[i, cc.VISIBLE], "SUM_FB")
            sums_close(stats[i, cc.SUM_MAG], want[i, cc.SUM_MAG], want[i, cc.FINITE], "SUM_MAG")
    b.check = check
    return b


def bind_warp_frames(which, v=0):
    """With the class map, the reference frames and the stats rows (the optional arguments, which come together)."""
    from tests import consistency_cases as cc
    fwd, bwd, src, ref = _consistency_inputs(which, v)
    n, _, h, w = fwd.shape
    cls = cc.restate32(fwd, bwd)[0]
    b = Bound("sf_warp_frames").add("src", IN, src).add("flows", IN, fwd).add("out", OUT, nbytes=n * h * w * 3).add("cls", IN, cls)
    b.add("ref", IN, ref).add("stats", STATS, nbytes=n * 2 * 8).add("ws", WS, nbytes=lib().sf_warp_frames_ws_bytes(n, h, w))
    ws_bytes, st = b.bufs["ws"].nbytes, hwc_strides(h, w)
    b.call = lambda L, p, s: L.sf_warp_frames(p("src"), *st, p("flows"), 2 * h * w, h * w, w, n, h, w, p("out"), p("cls"), 0, p("ref"), *st,
                                              p("stats"), p("ws"), ws_bytes, s)

    def check(outs):
        want, want_stats = cc.warp32(src, fwd, cls, ref, visible=0)
        assert np.array_equal(outs["out"].reshape(n, h, w, 3), want)
        stats = outs["stats"].view(np.float64).reshape(n, 2)
        for i in range(n):
            assert stats[i, 1] == want_stats[i, 1]
            sums_close(stats[i, 0], want_stats[i, 0], want_stats[i, 1], "SUM_ABS")
    b.check = check
    return b


INTERP = {"A": "5x260-special-3/4", "B": "13x37-holes"}      # 3 pairs, rows longer than one 256-pixel unit, NaN / Inf flows; 2 pairs


def bind_frame_interp(which, v=0):
    """With class maps, the cover map and the stats rows."""
    from tests import consistency_cases as cc
    from tests import interp_cases as ic
    case = next(c for c in ic.CASES if c[0] == INTERP[which])
    a, bb, fwd, bwd, num, den, _ = ic.build(case)
    a, bb, fwd, bwd = vary_u8(a, v), vary_u8(bb, 2 * v), vary_f32(fwd, v), vary_f32(bwd, v)
    cls = (cc.restate32(fwd, bwd)[0], cc.restate32(bwd, fwd)[0])
    n, _, h, w = fwd.shape
    imp = (16, 1, 16)
    b = Bound("sf_frame_interp").add("a", IN, a).add("b", IN, bb).add("fwd", IN, fwd).add("bwd", IN, bwd)
    b.add("cls_f", IN, cls[0]).add("cls_b", IN, cls[1]).add("out", OUT, nbytes=n * h * w * 3).add("cover", OUT, nbytes=n * h * w)
    b.add("stats", STATS, nbytes=n * ic.LEN * 8).add("ws", WS, nbytes=lib().sf_frame_interp_ws_bytes(n, h, w))
    ws_bytes, st, fs = b.bufs["ws"].nbytes, hwc_strides(h, w), (2 * h * w, h * w, w)
    b.call = lambda L, p, s: L.sf_frame_interp(p("a"), *st, p("b"), *st, p("fwd"), *fs, p("bwd"), *fs, n, h, w, num, den, p("cls_f"),
                                               p("cls_b"), 0, 1, *imp, p("out"), p("cover"), p("stats"), p("ws"), ws_bytes, s)

    def check(outs):
        want = ic.restate(a, bb, fwd, bwd, num, den, cls, imp=imp)
        assert np.array_equal(outs["out"].reshape(n, h, w, 3), want[0])
        assert np.array_equal(outs["cover"].reshape(n, h, w), want[1])
        assert np.array_equal(outs["stats"].view(np.float64).reshape(n, ic.LEN), want[2])
    b.check = check
    return b


# ---- resize -----------------------------------------------------------------------------------------------------------------------
RESIZE_U8 = {"A": (((150, 530), (75, 265), 3), "bicubic"), "B": (((37, 53), (16, 24), 1), "bicubic")}       # both passes, several blocks
RESIZE_F32 = {"A": (((55, 128), (109, 255)), 2, "bicubic"), "B": (((37, 53), (16, 24)), 1, "lanczos")}
F32_SCALE = (1.75, 0.4)


def _resize_tables(b, H, W, h, w, name, kind):
    from tests import resize_cases as rc
    ks = []
    for axis, (a, o) in (("x", (W, w)), ("y", (H, h))):
        bounds, k = rc.table(a, o, name)
        b.add("bounds_" + axis, IN, bounds.astype(np.int32)).add("k" + axis, IN, rc.fixed(k) if kind == "u8" else k.astype(np.float32))
        ks.append(int(k.shape[1]))
    return ks


def bind_resize_u8(which, v=0):
    from tests import resize_cases as rc
    case, name = RESIZE_U8[which]
    (H, W), (h, w), n = case
    img = vary_u8(rc.u8_input(case, "noise"), v)
    b = Bound("sf_resize_u8").add("src", IN, img)
    kx, ky = _resize_tables(b, H, W, h, w, name, "u8")
    b.add("out", OUT, nbytes=n * h * w * 3).add("ws", WS, nbytes=lib().sf_resize_u8_ws_bytes(n, H, W, h, w))
    ws_bytes = b.bufs["ws"].nbytes
    b.call = lambda L, p, s: L.sf_resize_u8(p("src"), *hwc_strides(H, W), n, H, W, h, w, p("bounds_x"), p("kx"), kx, p("bounds_y"), p("ky"),
                                            ky, p("out"), p("ws"), ws_bytes, s)

    def check(outs):
        assert np.array_equal(outs["out"].reshape(n, h, w, 3), rc.resize_u8(img, (h, w), name))
    b.check = check
    return b


def bind_resize_f32(which, v=0):
    from tests import resize_cases as rc
    case, n, name = RESIZE_F32[which]
    (H, W), (h, w) = case
    flow = vary_f32(rc.f32_input(case, n), v)
    b = Bound("sf_resize_f32").add("src", IN, flow)
    kx, ky = _resize_tables(b, H, W, h, w, name, "f32")
    b.add("out", OUT, nbytes=n * 2 * h * w * 4).add("ws", WS, nbytes=lib().sf_resize_f32_ws_bytes(n, H, W, h, w))
    ws_bytes, (sx, sy) = b.bufs["ws"].nbytes, F32_SCALE
    b.call = lambda L, p, s: L.sf_resize_f32(p("src"), 2 * H * W, H * W, W, n, H, W, h, w, p("bounds_x"), p("kx"), kx, p("bounds_y"), p("ky"),
                                             ky, sx, sy, p("out"), p("ws"), ws_bytes, s)

    def check(outs):
        got = outs["out"].view(np.float32).reshape(n, 2, h, w).astype(np.float64)
        err = np.abs(got - rc.resize_f64(flow, (h, w), name, sx, sy))
        assert (err <= rc.bound_f32(flow, (h, w), name, sx, sy)).all()
    b.check = check
    return b


# ---- encoders: one slot per image or chunk and its length ---------------------------------------------------------------------------
def _slots(b, n_slots, stride, specified_tail):
    """regions() of an encoder's `out`: slot k's extent is its first lengths[k] bytes; the rest of the slot is unspecified where the
    header says so (sf_png_encode, sf_flo5_encode) and must stay untouched where it says that (sf_jpeg_encode)."""
    def regions(outs):
        lengths = outs["lengths"].view(np.int64)
        extent = np.zeros(n_slots * stride, bool)
        for k in range(n_slots):
            extent[k * stride:k * stride + int(lengths[k])] = True
        return {"out": (extent, np.zeros_like(extent) if specified_tail else ~extent)}
    b.regions = regions


def _streams(outs, n_slots, stride):
    lengths = outs["lengths"].view(np.int64)
    return [outs["out"][k * stride:k * stride + int(lengths[k])].tobytes() for k in range(n_slots)]


JPEG_ENCODE = {"A": (37, 45, 3, 90, (("wheel", 31), ("noise", 32), ("const", 33))), "B": (17, 23, 3, 75, (("mixed", 5), ("noise", 6)))}


def bind_jpeg_encode(which, v=0):
    from tests import jpeg_cases as jc
    h, w, c, quality, kinds = JPEG_ENCODE[which]
    images = [vary_u8(jc.make(kind, h, w, c, seed), v) for kind, seed in kinds]
    n, q = len(images), np.ascontiguousarray(jc.tables(quality), np.uint16)
    bound = lib().sf_jpeg_encode_bound(h, w, c)
    b = Bound("sf_jpeg_encode").add("img", IN, np.stack(images)).add("out", OUT, nbytes=n * bound).add("lengths", OUT, nbytes=8 * n)
    b.add("ws", WS, nbytes=lib().sf_jpeg_encode_ws_bytes(n, h, w, c))
    ws_bytes = b.bufs["ws"].nbytes
    b.call = lambda L, p, s: L.sf_jpeg_encode(p("img"), h * w * c, w * c, n, h, w, c, q.ctypes.data, p("out"), bound, p("lengths"), p("ws"),
                                              ws_bytes, s)
    _slots(b, n, bound, specified_tail=True)

    def check(outs):
        assert _streams(outs, n, bound) == [jc.encode_ref(img, q) for img in images]
    b.check = check
    return b


PNG_ENCODE = {"A": (37, 45, 3, 0, (("smooth", 31), ("noise", 32), ("zeros", 33))), "B": (33, 20, 6, 1, (("smooth", 34), ("noise", 35)))}


def bind_png_encode(which, v=0):
    from tests import png_encode_cases as ec
    h, w, bpp, swap16, kinds = PNG_ENCODE[which]
    images = [vary_u8(ec.make(kind, h, w, bpp, seed), v) for kind, seed in kinds]
    n, bound = len(images), lib().sf_png_encode_bound(h, w, bpp)
    b = Bound("sf_png_encode").add("img", IN, np.stack(images)).add("out", OUT, nbytes=n * bound).add("lengths", OUT, nbytes=8 * n)
    b.add("ws", WS, nbytes=lib().sf_png_encode_ws_bytes(n, h, w, bpp))
    ws_bytes = b.bufs["ws"].nbytes
    b.call = lambda L, p, s: L.sf_png_encode(p("img"), h * w * bpp, w * bpp, n, h, w, bpp, swap16, p("out"), bound, p("lengths"), p("ws"),
                                             ws_bytes, s)
    _slots(b, n, bound, specified_tail=False)

    def check(outs):
        assert _streams(outs, n, bound) == [ec.encode_ref(img, bool(swap16)) for img in images]
    b.check = check
    return b


FLO5_ENCODE = {"A": (37, 53, 8, ((2, True), (3, False))), "B": (9, 20, 4, ((4, True),))}         # (h, w, rows per chunk, (seed, special))


def bind_flo5_encode(which, v=0):
    from tests import flo5_encode_cases as fc
    h, w, rpc, kinds = FLO5_ENCODE[which]
    fields = [fc.make(h, w, seed + 100 * v, special) for seed, special in kinds]
    n, nchunks, bound = len(fields), -(-h // rpc), lib().sf_flo5_chunk_bound(rpc, w)
    slots = n * nchunks
    b = Bound("sf_flo5_encode").add("flow", IN, np.stack(fields)).add("out", OUT, nbytes=slots * bound)
    b.add("lengths", OUT, nbytes=8 * slots).add("ws", WS, nbytes=lib().sf_flo5_encode_ws_bytes(n, h, w, rpc))
    ws_bytes = b.bufs["ws"].nbytes
    b.call = lambda L, p, s: L.sf_flo5_encode(p("flow"), 2 * h * w, h * w, w, n, h, w, rpc, p("out"), bound, p("lengths"), p("ws"), ws_bytes, s)
    _slots(b, slots, bound, specified_tail=False)

    def check(outs):
        assert _streams(outs, slots, bound) == [fc.chunk_stream_ref(f, c, rpc) for f in fields for c in range(nchunks)]
    b.check = check
    return b


KITTI16 = {"A": (3, 17, 65), "B": (2, 13, 37)}


def bind_flow_to_kitti16(which, v=0):
    from tests import png_encode_cases as ec
    n, h, w = KITTI16[which]
    flow = np.stack([ec.smooth_field(h, w, 10 * v + i) * np.float32(40 * (i + 1)) for i in range(n)]).astype(np.float32)
    flow[0, 0, 0, :5] = [np.nan, np.inf, -np.inf, 600.0, -600.0]                # 0, 65535, 0, clamped above and below
    b = Bound("sf_flow_to_kitti16").add("flow", IN, flow).add("out", OUT, nbytes=n * h * w * 3 * 2)
    b.call = lambda L, p, s: L.sf_flow_to_kitti16(p("flow"), p("out"), n, h, w, s)

    def check(outs):
        assert np.array_equal(outs["out"].view(np.uint16).reshape(n, h, w, 3), np.stack([ec.kitti16_ref(f) for f in flow]))
    b.check = check
    return b


# ---- decoders ---------------------------------------------------------------------------------------------------------------------
PNG_UNFILTER = {"A": (37, 53, 3, 8, 3, 0), "B": (11, 13, 3, 16, 2, 1)}            # (h, w, channels, depth, images, swap16)


def bind_png_unfilter(which, v=0):
    from tests import png_cases as pc
    h, w, ch, depth, n, swap16 = PNG_UNFILTER[which]
    bpp = ch * depth // 8
    images = [pc.image(h, w, ch, depth, 50 + 10 * v + i) for i in range(n)]
    blocks = [pc.encode(img, pc.filter_types("mixed", h, 7 * v + i), None, depth) for i, img in enumerate(images)]
    line, row = 1 + w * bpp, w * bpp
    b = Bound("sf_png_unfilter").add("scan", IN, np.stack(blocks)).add("out", OUT, nbytes=n * h * row)
    b.call = lambda L, p, s: L.sf_png_unfilter(p("scan"), h * line, n, h, w, bpp, p("out"), h * row, row, swap16, s)

    def check(outs):
        rows = np.stack([pc.raw_rows(img, depth)[0] for img in images])
        if swap16:
            rows = np.ascontiguousarray(rows.reshape(n, h, -1, 2)[..., ::-1]).reshape(n, h, row)
        assert np.array_equal(outs["out"].reshape(n, h, row), rows)
    b.check = check
    return b


JPEG_DECODE = {"A": ("420-33x33", "420-33x33-rst1", "420-33x33-rst3", "420-33x33-rst3-fill"),        # no DRI, DRI 1, DRI 3 (own tables)
               "B": ("444-16x17", "444-16x17-nodht", "444-16x17-q100-noise")}
# both routes in one call: the threshold lies between the interval sizes of the batch
JPEG_SPLIT = {"A": (JPEG_DECODE["A"], 16), "B": (("444-73x9-rows",), 16)}


def split_threshold(desc):
    """A split_min_bytes with intervals on both sides of it: the median of the distinct interval lengths."""
    sizes = sorted({int(x) for x in desc[:, 1]})
    assert len(sizes) >= 2
    return sizes[len(sizes) // 2]


def _bind_jpeg_decode(entry, names, segment_bytes, v):
    from tests import jpeg_decode_cases as dc
    from tests import jpeg_sync_cases as sc
    names = rotate(names, v)
    call = sc.Call(names)
    n, h, w = call.n, call.h, call.w
    geom = (n, h, w, call.nc, call.hs, call.vs)
    data = np.concatenate([call.data, np.zeros(1, np.uint8)])               # (never empty; the call is given len(call.data))
    b = Bound(entry).add("data", IN, data).add("desc", IN, np.ascontiguousarray(call.desc, np.int64))
    b.add("tables", IN, np.ascontiguousarray(call.tables, np.uint8)).add("out", OUT, nbytes=n * h * w * 3).add("status", STATUS, nbytes=4 * n)
    head = lambda p: (p("data"), len(call.data), p("desc"), len(call.desc), p("tables"), len(call.tables), *geom, p("out"), h * w * 3,
                      w * 3, 3, p("status"))
    if entry == "sf_jpeg_decode":
        ws_bytes = lib().sf_jpeg_decode_ws_bytes(*geom)
        b.call = lambda L, p, s: L.sf_jpeg_decode(*head(p), p("ws"), ws_bytes, s)
    else:
        smin = split_threshold(call.desc)
        ws_bytes = lib().sf_jpeg_decode_split_ws_bytes(*geom, len(call.data), len(call.desc), segment_bytes)
        b.call = lambda L, p, s: L.sf_jpeg_decode_split(*head(p), segment_bytes, smin, p("ws"), ws_bytes, s)
        b.split_min_bytes, b.interval_bytes = smin, [int(x) for x in call.desc[:, 1]]
    b.add("ws", WS, nbytes=ws_bytes)

    def check(outs):
        assert not outs["status"].view(np.int32).any()
        got = outs["out"].reshape(n, h, w, 3)
        for i, name in enumerate(names):
            assert np.array_equal(got[i], dc.decode_ref(sc.load(name))), name
    b.check = check
    return b


def bind_jpeg_decode(which, v=0):
    return _bind_jpeg_decode("sf_jpeg_decode", JPEG_DECODE[which], 0, v)


def bind_jpeg_decode_split(which, v=0):
    names, seg = JPEG_SPLIT[which]
    return _bind_jpeg_decode("sf_jpeg_decode_split", names, seg, v)


INFLATE = {"A": ("text-l5-default", "chunk-l5", "run-l9", "n64-l0-fixed", "writer-37x53-c0", "empty-l9-default", "far-l9", "text-flushes"),
           "B": ("n65-l9-huffman", "text-l1-rle", "one-l5-default", "n64-l5-default")}


def bind_inflate(which, v=0):
    """Streams at unaligned input offsets with junk between them; one of them is handed over as stored bytes (SF_INFLATE_STORED)."""
    from tests import flo5_decode_cases as dc
    names = rotate(INFLATE[which], v)
    comp, desc, slots, at = bytearray(b"\xEE" * 3), [], [], 5
    for k, name in enumerate(names):
        s, d = dc.good(name)
        stored = name == INFLATE[which][3]
        src = d if stored else s
        desc.append((len(comp), len(src), at, len(d), 1 if stored else 0))
        slots.append((at, d))
        comp += bytes(src) + b"\xEE" * 3
        at += len(d) + 7
    n, out_bytes = len(names), at
    b = Bound("sf_inflate").add("in", IN, np.frombuffer(bytes(comp), np.uint8)).add("desc", IN, np.array(desc, np.int64))
    b.add("out", OUT, nbytes=out_bytes).add("status", STATUS, nbytes=4 * n)
    b.call = lambda L, p, s: L.sf_inflate(p("in"), len(comp), p("desc"), n, p("out"), out_bytes, p("status"), s)

    def regions(outs):
        extent = np.zeros(out_bytes, bool)
        for o, d in slots:
            extent[o:o + len(d)] = True
        return {"out": (extent, np.zeros_like(extent))}
    b.regions = regions

    def check(outs):
        assert not outs["status"].view(np.int32).any()
        for (o, d), name in zip(slots, names):
            assert outs["out"][o:o + len(d)].tobytes() == d, name
    b.check = check
    return b


ASSEMBLE = {"A": ((136, 240), (34, 60, 1), False, 3), "B": ((33, 40), (8, 16, 2), True, 1)}


def bind_flo5_assemble(which, v=0):
    """Raw chunks in shuffled slot order, one chunk of every file missing (file 1: a slot index out of range)."""
    from tests import flo5_decode_cases as dc
    (h, w), (ch, cw, cc), shuffle, n = ASSEMBLE[which]
    gy, gx, gc = -(-h // ch), -(-w // cw), 2 // cc
    size = 4 * ch * cw * cc
    stride = size + 8
    cells = [(i, y, x, c) for i in range(n) for y in range(gy) for x in range(gx) for c in range(gc)]
    order = np.random.default_rng(h * 7 + n + v).permutation(len(cells))
    slots = np.full((len(cells), stride), 0xC3, np.uint8)
    grid = np.full((n, gy, gx, gc), -1, np.int32)
    want = []
    for i in range(n):
        f = dc.smooth_field(h, w, 10 + i + 50 * v)
        chunks = {}
        for (j, y, x, c) in cells:
            if j != i:
                continue
            if (y, x, c) == ((i + 1) % gy, i % gx, i % gc):
                grid[i, y, x, c] = -1 if i != 1 else len(cells) + 5
                continue
            buf = np.zeros((ch, cw, cc), "<f4")
            part = f[y * ch:(y + 1) * ch, x * cw:(x + 1) * cw, c * cc:(c + 1) * cc]
            buf[:part.shape[0], :part.shape[1]] = part
            data = np.frombuffer(buf.tobytes(), np.uint8)
            if shuffle:
                data = np.ascontiguousarray(data.reshape(-1, 4).T).reshape(-1)
            k = int(order[cells.index((i, y, x, c))])
            slots[k, :size] = data
            grid[i, y, x, c] = k
            chunks[(y, x, c)] = data.tobytes()
        want.append(dc.assemble_ref((h, w, 2), (ch, cw, cc), shuffle, chunks))
    b = Bound("sf_flo5_assemble").add("chunks", IN, slots).add("grid", IN, grid).add("out", OUT, nbytes=n * h * w * 2 * 4)
    b.call = lambda L, p, s: L.sf_flo5_assemble(p("chunks"), stride, len(cells), p("grid"), n, h, w, ch, cw, cc, int(shuffle), p("out"), s)

    def check(outs):
        assert np.array_equal(outs["out"].view(np.uint32).reshape(n, h, w, 2), np.stack(want))
    b.check = check
    return b


# ---- stabilisation ------------------------------------------------------------------------------------------------------------------
MOTION = {"A": (31, 3, 33, 130), "B": (41, 2, 13, 37)}                      # (seed, n, h, w): five blocks of moments units / one
CODES, CLASS_WEIGHTS = (0, 1, 2), (1.0, 0.25, 0.0)
FIT_KIND, FIT_ROUNDS, FIT_KAPPA, FIT_FLOOR = 2, 3, 2.0, 1e-3


def _motion_inputs(which, v):
    from tests import stabilize_cases as sc
    seed, n, h, w = MOTION[which]
    flows = sc.make_fields(seed + 100 * v, n, h, w, noise=0.5)[0]
    flows[0, 0, 0, :3] = [np.nan, np.inf, 1e30]                              # weight 0
    return flows, sc.make_cls(seed + 1 + 100 * v, n, h, w, CODES)


def check_moments(got, want, mag, cnt):
    from tests import stabilize_cases as sc
    assert np.array_equal(got[:, sc.N], want[:, sc.N])
    assert (np.abs(got - want) <= cnt * 2.0 ** -52 * mag).all()


def bind_motion_moments(which, v=0):
    """With the class map and a previous model (the robust weights)."""
    from tests import stabilize_cases as sc
    flows, cls = _motion_inputs(which, v)
    n, _, h, w = flows.shape
    rng = np.random.default_rng(70 + w + v)
    model, inv_c2 = rng.uniform(-3, 3, (n, 6)).astype(np.float32), rng.uniform(0.01, 0.2, n).astype(np.float32)
    max_mag = 4.0 * max(h, w)
    b = Bound("sf_motion_moments").add("flows", IN, flows).add("cls", IN, cls).add("model", IN, model).add("inv_c2", IN, inv_c2)
    b.add("moments", OUT, nbytes=n * sc.LEN * 8).add("ws", WS, nbytes=lib().sf_motion_moments_ws_bytes(n, h, w, 1))
    ws_bytes = b.bufs["ws"].nbytes
    b.call = lambda L, p, s: L.sf_motion_moments(p("flows"), 2 * h * w, h * w, w, n, h, w, p("cls"), *CODES, *CLASS_WEIGHTS, 1, max_mag,
                                                 p("model"), p("inv_c2"), p("moments"), p("ws"), ws_bytes, s)

    def check(outs):
        wt = sc.weights32(flows, cls=cls, codes=CODES, class_weights=CLASS_WEIGHTS, step=1, model=model, inv_c2=inv_c2)
        check_moments(outs["moments"].view(np.float64).reshape(n, sc.LEN), *sc.moments64(*wt))
    b.check = check
    return b


def check_solution(m, a, kind):
    """A device model against numpy.linalg.solve on the normal equations of the moments it was solved from, within Cholesky's backward
    error (the criterion of tests/test_gpu_stabilize.py)."""
    from tests import stabilize_cases as sc
    M, rhs = sc.normal_matrix(m, kind)
    cond = np.linalg.cond(M)
    for got, r in zip(sc.unknowns(a, kind), rhs):
        want = np.linalg.solve(M, r)
        assert np.abs(got - want).max() <= 64 * 2.0 ** -53 * cond * np.abs(want).max(), (got, want)


def bind_motion_solve(which, v=0):
    from tests import stabilize_cases as sc
    flows, cls = _motion_inputs(which, v)
    n = flows.shape[0]
    moments = sc.moments64(*sc.weights32(flows, cls=cls, codes=CODES, class_weights=CLASS_WEIGHTS))[0]
    b = Bound("sf_motion_solve").add("moments", IN, moments).add("model64", OUT, nbytes=n * 48).add("model32", OUT, nbytes=n * 24)
    b.add("c", OUT, nbytes=n * 8).add("inv_c2", OUT, nbytes=n * 4).add("status", STATUS, nbytes=n * 4)
    b.call = lambda L, p, s: L.sf_motion_solve(p("moments"), n, FIT_KIND, FIT_KAPPA, FIT_FLOOR, p("model64"), p("model32"), p("c"),
                                               p("inv_c2"), p("status"), s)

    def check(outs):
        m64 = outs["model64"].view(np.float64).reshape(n, 6)
        assert not outs["status"].view(np.int32).any()
        assert np.array_equal(outs["model32"].view(np.float32).reshape(n, 6), m64.astype(np.float32))
        c = outs["c"].view(np.float64)
        assert (c >= FIT_FLOOR).all() and np.isfinite(c).all()
        for i in range(n):
            check_solution(moments[i], m64[i], FIT_KIND)
            ic2 = float(outs["inv_c2"].view(np.float32)[i])
            assert abs(ic2 - 1.0 / (c[i] * c[i])) <= 2.0 ** -23 / (c[i] * c[i])
    b.check = check
    return b


def bind_motion_fit(which, v=0):
    from tests import stabilize_cases as sc
    flows, cls = _motion_inputs(which, v)
    n, _, h, w = flows.shape
    b = Bound("sf_motion_fit").add("flows", IN, flows).add("cls", IN, cls).add("trace", OUT, nbytes=n * FIT_ROUNDS * sc.TRACE_LEN * 8)
    b.add("ws", WS, nbytes=lib().sf_motion_fit_ws_bytes(n, h, w, 1))
    ws_bytes = b.bufs["ws"].nbytes
    b.call = lambda L, p, s: L.sf_motion_fit(p("flows"), 2 * h * w, h * w, w, n, h, w, p("cls"), *CODES, *CLASS_WEIGHTS, 1, 4.0 * max(h, w),
                                             FIT_KIND, FIT_ROUNDS, FIT_KAPPA, FIT_FLOOR, p("trace"), p("ws"), ws_bytes, s)

    def check(outs):
        """Link by link: every round's moments from the device's previous fp32 model and inv_c2, its model from its own moments."""
        trace = outs["trace"].view(np.float64).reshape(n, FIT_ROUNDS, sc.TRACE_LEN)
        model = inv_c2 = None
        for r in range(FIT_ROUNDS):
            wt = sc.weights32(flows, cls=cls, codes=CODES, class_weights=CLASS_WEIGHTS, step=1, model=model, inv_c2=inv_c2)
            check_moments(trace[:, r, :sc.LEN], *sc.moments64(*wt))
            for i in range(n):
                assert trace[i, r, sc.T_STATUS] == sc.OK
                check_solution(trace[i, r, :sc.LEN], trace[i, r, sc.T_MODEL:sc.T_MODEL + 6], FIT_KIND)
            model, inv_c2 = trace[:, r, sc.T_MODEL:sc.T_MODEL + 6].astype(np.float32), trace[:, r, sc.T_INV_C2].astype(np.float32)
    b.check = check
    return b


WARP_AFFINE = {"A": (17, 65, 12, 1), "B": (13, 37, 6, 0)}                     # (h, w, frames = the first maps of warp_maps, border)


def warp_maps(h, w):
    """The inverse maps of tests/test_gpu_stabilize.py: identity, shifts, a rotation, a zoom, maps that leave the frame, NaN / Inf."""
    cx, cy = (w - 1) / 2, (h - 1) / 2
    co, si = np.cos(0.3), np.sin(0.3)
    maps = [[1, 0, 0, 0, 1, 0], [1, 0, 2, 0, 1, -1], [1, 0, -3, 0, 1, 1], [1, 0, 0.25, 0, 1, -0.625],
            [co, -si, cx - co * cx + si * cy + 0.3, si, co, cy - si * cx - co * cy - 0.2],
            [0.5, 0, cx / 2, 0, 0.5, cy / 2], [1, 0, 1e4, 0, 1, 0], [1, 0, 0, 0, 1, -(h + 5.0)],
            [np.nan, 0, 0, 0, 1, 0], [1, 0, 0, 0, 1, np.inf], [1, 0, -np.inf, 0, 1, 0], [1e30, 0, 0, 0, -1e30, 0.5]]
    return np.array(maps, np.float32)


def bind_warp_affine_u8(which, v=0):
    from tests import stabilize_cases as sc
    h, w, n, border = WARP_AFFINE[which]
    maps = np.roll(warp_maps(h, w)[:n], v, axis=0)
    src = np.random.default_rng(80 + h + w + v).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    fill = (7, 130, 255)
    b = Bound("sf_warp_affine_u8").add("src", IN, src).add("maps", IN, maps).add("out", OUT, nbytes=n * h * w * 3)
    b.add("outside", OUT, nbytes=4 * n).add("ws", WS, nbytes=lib().sf_warp_affine_ws_bytes(n, h, w))
    ws_bytes = b.bufs["ws"].nbytes
    b.call = lambda L, p, s: L.sf_warp_affine_u8(p("src"), *hwc_strides(h, w), p("maps"), n, h, w, border, *fill, p("out"), p("outside"),
                                                 p("ws"), ws_bytes, s)

    def check(outs):
        want, counts = sc.warp_affine32(src, maps, border, fill)
        assert np.array_equal(outs["out"].reshape(n, h, w, 3), want)
        assert np.array_equal(outs["outside"].view(np.uint32).astype(np.int64), counts)
    b.check = check
    return b


# ---- the video path and the tile blend ----------------------------------------------------------------------------------------------
VIDEO = {"A": (8, 36, 52, 4), "B": (6, 20, 28, 3)}                            # (frames, H, W, T): the last clip overlaps its predecessor


def norm_lut():
    """The table the caller hands to sf_frames_to_clips, by video_cases.normalise (the model's expression) on the host: the kernel
    does no arithmetic on pixel values, so its output is this table's entries whatever built it."""
    import torch
    from tests import video_cases as vc
    return vc.normalise(torch.arange(256, dtype=torch.uint8)).numpy()


def _video(which, v):
    from streamflow_amd.utils import InputPadder
    from tests import video_cases as vc
    n, H, W, T = VIDEO[which]
    frames = vc.random_frames(20 + v, n, H, W)
    left, right, top, bottom = InputPadder((1, 3, H, W), mode="sintel")._pad
    return frames, (n, H, W, T), (left, top, H + top + bottom, W + left + right), -(-(n - 1) // (T - 1))


def bind_frames_to_clips(which, v=0):
    from tests import video_cases as vc
    frames, (n, H, W, T), (left, top, Hp, Wp), nc = _video(which, v)
    b = Bound("sf_frames_to_clips").add("frames", IN, frames.numpy()).add("lut", IN, norm_lut()).add("out", OUT, nbytes=nc * T * 3 * Hp * Wp * 4)
    b.call = lambda L, p, s: L.sf_frames_to_clips(p("frames"), *hwc_strides(H, W), 0, n, n, T, 0, nc, H, W, top, left, Hp, Wp, p("lut"),
                                                  p("out"), s)

    def check(outs):
        want = vc.clips(frames, T, "sintel").numpy()
        assert want.shape == (nc, T, 3, Hp, Wp)
        assert np.array_equal(outs["out"].view(np.uint32), want.reshape(-1).view(np.uint32))
    b.check = check
    return b


def bind_clips_to_flows(which, v=0):
    import torch
    from streamflow_amd import _lib
    from tests import video_cases as vc
    frames, (n, H, W, T), (left, top, Hp, Wp), nc = _video(which, v)
    outs_model = vc.stub_model(vc.clips(frames, T, "sintel"))                # T - 1 x [nc, 2, Hp, Wp]
    pair_bytes = nc * 2 * Hp * Wp * 4                                        # the T - 1 pair tensors one after the other in one buffer
    b = Bound("sf_clips_to_flows").add("pairs", IN, torch.stack(outs_model).numpy()).add("out", OUT, nbytes=(n - 1) * 2 * H * W * 4)

    def call(L, p, s):
        ptrs = _lib.SfPairPtrs()
        for k in range(T - 1):
            ptrs.p[k] = p("pairs") + k * pair_bytes
        return L.sf_clips_to_flows(C.byref(ptrs), 2 * Hp * Wp, Hp * Wp, Wp, n, T, 0, nc, 0, n - 1, H, W, top, left, p("out"), s)
    b.call = call

    def check(outs):
        _, padder = vc.padded_frames(frames[:1], "sintel")
        want = torch.stack(vc.kept(outs_model, 0, n, T, padder)).numpy()
        assert want.shape == (n - 1, 2, H, W)
        assert np.array_equal(outs["out"].view(np.uint32), np.ascontiguousarray(want).reshape(-1).view(np.uint32))
    b.check = check
    return b


# (canvas H, W, tile h, w, min_overlap, pad [left, right, top, bottom], clips, pairs): two crops / sixteen crops and an inner window
TILE = {"A": (64, 176, 64, 96, 20, (0, 0, 0, 0), 1, 3), "B": (75, 203, 24, 40, 5, (1, 2, 3, 4), 1, 1)}


def bind_tile_blend(which, v=0):
    import torch
    from streamflow_amd import _lib, tiling
    from tests.test_gpu_tile_blend import ref_blend
    H, W, th, tw, mo, pad, B, P = TILE[which]
    plan = tiling.make_plan((H, W), (th, tw), mo, pad=pad)
    flows = torch.randn(B * plan.n_distinct, P, 2, th, tw, generator=torch.Generator().manual_seed(H * W + th + v)) * 10.0
    wts = tiling.tile_weights((th, tw), tiling.TILE_SIGMA)
    y0, x0, h, w = plan.crop
    desc = _lib.SfTilePlan(n_seq=len(plan.sequence), n_distinct=plan.n_distinct, tile_h=th, tile_w=tw, img_h=H, img_w=W, out_y0=y0,
                           out_x0=x0, out_h=h, out_w=w)
    for k, ((ty, tx), d) in enumerate(zip(plan.sequence, plan.index)):
        desc.tile_y[k], desc.tile_x[k], desc.tile_id[k] = ty, tx, d
    b = Bound("sf_tile_blend").add("flows", IN, flows.numpy()).add("weights", IN, wts.numpy()).add("out", OUT, nbytes=B * P * 2 * h * w * 4)
    b.call = lambda L, p, s: L.sf_tile_blend(p("flows"), p("weights"), p("out"), C.byref(desc), B, P, s)

    def check(outs):
        want = ref_blend(flows, wts, plan, B).numpy()
        assert np.array_equal(outs["out"].view(np.uint32), np.ascontiguousarray(want).reshape(-1).view(np.uint32))
    b.check = check
    return b


class Record:
    def __init__(self, entry, bind, int_ws):
        self.entry, self.bind, self.int_ws = entry, bind, int_ws


# int_ws: the workspace holds integer fields a kernel could follow as an index (the docstring of tests/test_gpu_media_state.py says
# who writes each before who reads it)
TABLE = [Record("sf_flow_consistency", bind_flow_consistency, False), Record("sf_warp_frames", bind_warp_frames, False),
         Record("sf_frame_interp", bind_frame_interp, False), Record("sf_resize_u8", bind_resize_u8, False),
         Record("sf_resize_f32", bind_resize_f32, False), Record("sf_jpeg_encode", bind_jpeg_encode, True),
         Record("sf_jpeg_decode", bind_jpeg_decode, True), Record("sf_jpeg_decode_split", bind_jpeg_decode_split, True),
         Record("sf_flo5_encode", bind_flo5_encode, True), Record("sf_inflate", bind_inflate, False),
         Record("sf_flo5_assemble", bind_flo5_assemble, False), Record("sf_motion_moments", bind_motion_moments, False),
         Record("sf_motion_solve", bind_motion_solve, False), Record("sf_motion_fit", bind_motion_fit, False),
         Record("sf_warp_affine_u8", bind_warp_affine_u8, False), Record("sf_flow_to_kitti16", bind_flow_to_kitti16, False),
         Record("sf_png_encode", bind_png_encode, True), Record("sf_png_unfilter", bind_png_unfilter, False),
         Record("sf_frames_to_clips", bind_frames_to_clips, False), Record("sf_clips_to_flows", bind_clips_to_flows, False),
         Record("sf_tile_blend", bind_tile_blend, False)]
ENTRIES = [r.entry for r in TABLE]


def record(entry):
    return next(r for r in TABLE if r.entry == entry)


_ENGINE = "tests/test_gpu_engine_state.py"
# entry point -> the existing test that runs it on used buffers (poisoned allocations, poisoned plans, a second forward) or replays it
COVERED_ELSEWHERE = {
    **{name: _ENGINE + " (properties A, B, C: every engine kernel in poisoned and used plan buffers, eager and replayed)" for name in (
        "sf_coords_grid", "sf_bilinear_sampler", "sf_corr_build_pyramid", "sf_corr_lookup", "sf_corr_build_pyramid_pitched",
        "sf_corr_lookup_pitched", "sf_corr_build_blocked", "sf_corr_lookup_blocked", "sf_corr_build_blocked32", "sf_corr_lookup_blocked32",
        "sf_gemm", "sf_gma_flash_pack_qk", "sf_gma_flash_aggregate", "sf_gma_flash_aggregate_f16v", "sf_gma_flash_project_v",
        "sf_gma_flash_store_p", "sf_gma_stored_aggregate", "sf_ffn_pair", "sf_sk_tail", "sf_temporal_block", "sf_mask_upsample",
        "sf_softmax_rows", "sf_splitk_combine", "sf_dwconv_res_gelu", "sf_dwconv_res_gelu_f16in", "sf_layernorm_cm", "sf_temporal_attn",
        "sf_temporal_attn_f16in", "sf_pack_koct", "sf_context_split", "sf_flow_update", "sf_upsample_flow")},
    "sf_corr_direct_pack": "tests/test_gpu_engine_corr_direct.py (the engine's plans with the direct store, eager and replayed)",
    "sf_corr_direct_lookup": "tests/test_gpu_engine_corr_direct.py (the engine's plans with the direct store, eager and replayed)",
    **{name: _ENGINE + " (property A: Twins_CSC.forward in poisoned allocations)" for name in (
        "sf_window_attn", "sf_window_attn_mfma", "sf_subsample_attn", "sf_subsample_attn_mfma", "sf_dwconv3x3_res")},
    "sf_forward_interpolate": _ENGINE + " (property E: forward_interpolate in poisoned allocations)",
    "sf_flow_to_image": "tests/test_gpu_flow_viz.py::test_inside_graph_capture",
    "sf_flow_score": "tests/test_gpu_engine_state.py::test_flow_score_scratch",
    "sf_flow_score_batch": "tests/test_gpu_engine_state.py::test_flow_score_batch_scratch",
    "sf_frame_interp_phases": "tests/test_gpu_media_state.py (sf_frame_interp's record runs the same launches; the entry point itself is "
                              "the timing tool's, and the header makes its workspace the caller's to keep between the calls of a sequence)",
    "sf_gemm_route": "tests/test_gemm_packed_cases_cpu.py (no device work: a pure function of the descriptor)",
    **{name: "tests/test_abi_cpu.py (a size function under another suffix than *_ws_bytes: no device work)" for name in (
        "sf_corr_blocked_bytes", "sf_corr_blocked32_bytes", "sf_gemm_split_ws_floats", "sf_gma_stored_p_bytes")},
    "sf_version": "tests/test_abi_cpu.py (no device work)",
    "sf_last_error": "tests/test_abi_cpu.py (no device work)",
    "sf_clock_probe": "tests/test_abi_cpu.py (a measuring probe of tools/clock_probe_check.py: no product path calls it, it has no buffers to reuse)",
}
