"""CPU: the decision table of engine.resolve_skblock -- which launches one SK block makes (ffn1 as one sf_ffn_pair or two GEMMs; the back
half as one sf_sk_tail, pw + sf_ffn_pair or three GEMMs) and the format of every tensor handed over between them -- and that
engine.run_skblock issues exactly what the route says.  The resolver reads descriptors and the library's shape tables only, so the planes
here stand over an 8-float CPU tensor.  Expected routes are literals, read off run_skblock as it was before the resolver existed.

Blocks are the six of the canonical model (T = 4), inputs and outputs in the forms the engine's plan gives them: convc1 / convc2 between
k-octet-only tensors (koct_io), the GRU from fp32 planes with a k-octet copy, the flow head from the grouped view of the hidden state.
Grids: 4 x 7040 = 28160 pixels is the first launch that 'fills the chip'; the largest smaller one that keeps the fp16 hand-over (P % 4 == 0)
is 1 x 28156 -- at 28159 pixels P is odd, and the route is the all-fp32 one of P = 133 below."""
import os

import pytest
import torch

from streamflow_amd import ops, synthetic as syn
from streamflow_amd.engine import HotPathWeights, SkRoute, resolve_skblock, run_skblock
from streamflow_amd.ops import EPI_GELU, EPI_NONE, EPI_RES_GELU, EPI_RES_GELU_DW1, Planes

F16X2, F16X3, F16, FP32 = ops.PRECISION_F16X2, ops.PRECISION_F16X3, ops.PRECISION_F16, ops.PRECISION_FP32
FULL, SMALL = (4, 7040), (1, 28156)                      # (images, pixels): 28160 and 28156
# (C_in, C_out, K): update.py's SKMotionEncoder6_Deep_nopool_res (cor_planes = 4 * 9 * 9, out_dim = 128) and SKUpdateBlock_TAM_v3
# (embed_dim = 128, T = 4) with model.default_args' k_conv = [1, 15], PCUpdater_conv = [1, 7]
BLOCKS = {"convc1": (324, 256, 15), "convc2": (256, 192, 15), "convf2": (128, 64, 15), "conv": (256, 126, 15), "gru": (640, 128, 7),
          "flow_head": (384, 6, 15)}
IO = {"convc1": ("koct", "koct"), "convc2": ("koct", "koct"), "convf2": ("koct", "koct"), "conv": ("koct", "shadow"),
      "gru": ("shadow", "shadow"), "flow_head": ("grouped", "f32")}
BASE = torch.zeros(8)


@pytest.fixture(scope="module", autouse=True)
def lib():
    from streamflow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def packed():
    W = HotPathWeights(syn.make_params(3, 4), "cpu", T=4)
    assert {b: (getattr(W, b).c_in, getattr(W, b).c_out, getattr(W, b).k) for b in HotPathWeights.SK_BLOCKS} == BLOCKS
    return W


@pytest.fixture
def W(packed):
    yield packed
    packed.set_single(())


def planes(form, rows, n, P, off=0):
    koct = Planes(BASE, off + 4, (rows + 7) // 8 * 8 * P, n, rows, P, f16=True, koct=True)
    if form == "koct":
        return koct
    if form == "rows16":
        return Planes(BASE, off, rows * P, n, rows, P, f16=True)
    if form == "grouped":                                # '(B T) C -> B (T C)' over a buffer of 640-row images, with its k-octet copy
        sh = Planes(BASE, off + 4, 3 * 640 * P, n, rows, P, f16=True, koct=True, group=128, group_stride=640 * P)
        return Planes(BASE, off, 3 * 640 * P, n, rows, P, group=128, group_stride=640 * P, shadow=sh)
    return Planes(BASE, off, rows * P, n, rows, P, shadow=koct if form == "shadow" else None)


def route(W, block, grid=FULL, xin=None, yout=None, precision=F16X2, **flags):
    blk, (n, P) = getattr(W, block), grid
    X, Y = planes(xin or IO[block][0], blk.c_in, n, P, 64), planes(yout or IO[block][1], blk.c_out, n, P, 128)
    return resolve_skblock(blk, X, Y, ops.Ctx(precision, **flags))


R = SkRoute                                              # (front, back, fold, x2, x3, x4, hid1, hid2)
ALL_F32 = R("gemms", "gemms", False, "f32", "f32", "f32", "f32", "f32")
PAIR_TAIL = R("pair", "tail", True, "f16", "f16", None, None, None)
PAIR_PAIR = R("pair", "pair", True, "f16", "f16", "koct", None, None)
PAIR_GEMMS = R("pair", "gemms", True, "f16", "f16", "koct", None, "koct")
GEMMS_TAIL = R("gemms", "tail", True, "f16", "f16", None, "koct", None)
GEMMS_PAIR = R("gemms", "pair", True, "f16", "f16", "koct", "koct", None)
GEMMS_GEMMS = R("gemms", "gemms", True, "f16", "f16", "koct", "koct", "koct")


def test_koct_only_inputs_take_the_pair_and_the_tail_where_it_pays(W):
    """convc2 (256 -> 192): one launch each half when the launch fills the chip, pw + pair below (the small-launch rule).  convc1
    (324 -> 256): sf_sk_tail is built for C <= 256 shapes only and hi + lo ffn2 pairs do not pay at C >= 256, so its back half is
    three GEMMs at 28160 pixels and pw + pair below."""
    assert route(W, "convc2", FULL) == PAIR_TAIL
    assert route(W, "convc2", SMALL) == PAIR_PAIR
    assert route(W, "convc1", FULL) == PAIR_GEMMS
    assert route(W, "convc1", SMALL) == PAIR_PAIR
    assert route(W, "convf2", FULL) == PAIR_TAIL and route(W, "conv", FULL) == PAIR_TAIL
    assert route(W, "convf2", SMALL) == PAIR_PAIR and route(W, "conv", SMALL) == PAIR_PAIR
    assert route(W, "convc2", (18, 7040)) == PAIR_TAIL
    # an output in fp16 ROWS is something neither fused back half writes
    assert route(W, "convc2", FULL, yout="rows16") == PAIR_GEMMS and route(W, "convc2", SMALL, yout="rows16") == PAIR_GEMMS
    # fp32 planes without a k-octet copy (convf1's output with koct_io off): two GEMMs in front
    assert route(W, "convf2", FULL, xin="f32") == GEMMS_TAIL and route(W, "convf2", SMALL, xin="f32") == GEMMS_PAIR


def test_gru(W):
    """640 -> 128 from fp32 planes with a k-octet copy: no pair shape and no tail shape at C = 640 (W.gru.tail is not built), so five
    GEMMs at every size, with the fp16 hand-over formats in f16x2 / f16 and fp32 planes in f16x3 / fp32."""
    assert not W.gru.tail.built(2) and not W.gru.tail.built(1)
    for grid in (FULL, SMALL, (18, 7040)):
        assert route(W, "gru", grid) == GEMMS_GEMMS
        assert route(W, "gru", grid, precision=F16) == GEMMS_GEMMS
        assert route(W, "gru", grid, precision=F16X3) == ALL_F32
        assert route(W, "gru", grid, precision=FP32) == ALL_F32


def test_flow_head(W):
    """384 -> 6 on the grouped view.  sk_tail_all: sf_sk_tail is built for (384, 6) with one and with two products and the scratch x3 /
    fp32 output meet sk_tail_ok, so the back half is the tail -- asserted through W.tail.built, which is what the library says."""
    assert route(W, "flow_head", FULL) == GEMMS_GEMMS and route(W, "flow_head", SMALL) == GEMMS_GEMMS
    assert route(W, "flow_head", FULL, head_pairs=True) == PAIR_PAIR
    assert route(W, "flow_head", (18, 7040), head_pairs=True) == PAIR_PAIR
    assert route(W, "flow_head", SMALL, head_pairs=True) == GEMMS_GEMMS           # (grouped: no small-launch rule either)
    assert route(W, "flow_head", FULL, xin="f32", head_pairs=True) == GEMMS_GEMMS  # no k-octet copy to read
    built = W.flow_head.tail.built(W.flow_head.tail.products(ops.Ctx(F16X2)))
    assert built is True
    for grid in (FULL, SMALL):
        assert route(W, "flow_head", grid, sk_tail_all=True) == (GEMMS_TAIL if built else GEMMS_GEMMS)
        assert route(W, "flow_head", grid, sk_tail_all=True, sk_tail=False) == GEMMS_GEMMS
    assert route(W, "flow_head", FULL, sk_tail_all=True, head_pairs=True) == PAIR_TAIL
    # sk_tail_all elsewhere: small launches, and convc1 / the GRU stay (no built shape)
    assert route(W, "convc2", SMALL, sk_tail_all=True) == PAIR_TAIL
    assert route(W, "convc1", FULL, sk_tail_all=True) == PAIR_GEMMS and route(W, "gru", FULL, sk_tail_all=True) == GEMMS_GEMMS


# each switch off in turn, on convc2 at 28160 (PAIR_TAIL with everything on) and at 28156 (PAIR_PAIR): the fields not named stay
SWITCHES = {
    # unfolded pw: fp32 x2 / x3 (so no ffn1 pair, which writes fp16 rows), x4 as fp16 ROWS (allow_koct=False: no ffn2 pair, no tail)
    "pw_fold": (R("gemms", "gemms", False, "f32", "f32", "f16", "koct", "koct"),) * 2,
    # fp32 x2: no ffn1 pair; the back half is untouched
    "x2_f16": (R("gemms", "tail", True, "f32", "f16", None, "koct", None), R("gemms", "pair", True, "f32", "f16", "koct", "koct", None)),
    "ffn_pairs": (GEMMS_TAIL, GEMMS_GEMMS),
    "sk_tail": (PAIR_GEMMS, PAIR_PAIR),
    # fp16 rows everywhere: neither fused kernel runs without k-octet hand-over
    "hidden_koct": (R("gemms", "gemms", True, "f16", "f16", "f16", "f16", "f16"),) * 2,
    "hidden_f16": (ALL_F32,) * 2,
    # sf_ffn_pair needs the k-octet copies' switch, sf_sk_tail (fp16 rows in) does not
    "shadows": (GEMMS_TAIL, GEMMS_GEMMS),
}


@pytest.mark.parametrize("flag", list(SWITCHES))
def test_each_switch_off_in_turn(W, flag):
    assert route(W, "convc2", FULL) == PAIR_TAIL and route(W, "convc2", SMALL) == PAIR_PAIR
    assert (route(W, "convc2", FULL, **{flag: False}), route(W, "convc2", SMALL, **{flag: False})) == SWITCHES[flag]


@pytest.mark.parametrize("block", list(BLOCKS))
def test_pixel_counts_off_multiples_of_four_keep_fp32_planes(W, block):
    for n in (2, 212):                                   # 266 and 28196 pixels
        assert route(W, block, (n, 133)) == ALL_F32
        assert route(W, block, (n, 133), head_pairs=True, sk_tail_all=True) == ALL_F32


def test_mixed_single_flags(W):
    """One of pw / ffn2.0 / ffn2.2 single: the tail has no common product count (W.tail.products is None), and the ffn2 pair follows
    pair2_pays -- products (1, 1) pay at every size, (2, 1) only as a small launch, (1, 2) is no built product pair."""
    cx = ops.Ctx(F16X2)
    for names, products, full, small in [(("convc2.pw",), (2, 2), PAIR_GEMMS, PAIR_PAIR),
                                         (("convc2.ffn2_0",), (1, 2), PAIR_GEMMS, PAIR_GEMMS),
                                         (("convc2.ffn2_2",), (2, 1), PAIR_GEMMS, PAIR_PAIR),
                                         (("convc2.ffn2_0", "convc2.ffn2_2"), (1, 1), PAIR_PAIR, PAIR_PAIR)]:
        W.set_single(names)
        assert W.convc2.tail.products(cx) is None and W.convc2.pair2.products(cx) == products
        assert (route(W, "convc2", FULL), route(W, "convc2", SMALL)) == (full, small), names
        assert route(W, "convc2", FULL, sk_tail_all=True) == full
    W.set_single(("convc2.ffn1_0",))                     # (1, 2) in front: two GEMMs; the back half does not see it
    assert (route(W, "convc2", FULL), route(W, "convc2", SMALL)) == (GEMMS_TAIL, GEMMS_PAIR)


def test_all_layers_single(W):
    """set_single('all'): pair products (1, 1), so pair2_pays at every C.  The tail still goes first where it is built for one product:
    (256, 126) and (128, 64) -- not (256, 192), whose single-product form is not built."""
    W.set_single("all")
    cx = ops.Ctx(F16X2)
    assert all(getattr(W, b).pair2.products(cx) == (1, 1) and getattr(W, b).tail.products(cx) == 1 for b in BLOCKS)
    assert not W.convc2.tail.built(1) and W.conv.tail.built(1) and W.convf2.tail.built(1)
    assert route(W, "convc1", FULL) == PAIR_PAIR and route(W, "convc2", FULL) == PAIR_PAIR
    assert route(W, "conv", FULL) == PAIR_TAIL and route(W, "convf2", FULL) == PAIR_TAIL
    assert route(W, "gru", FULL) == GEMMS_GEMMS                                   # (640, 128) is no pair shape
    assert route(W, "flow_head", FULL) == GEMMS_PAIR and route(W, "flow_head", FULL, head_pairs=True) == PAIR_PAIR
    # the f16 mode has one product everywhere without any flag
    W.set_single(())
    assert route(W, "convc1", FULL, precision=F16) == PAIR_PAIR and route(W, "convc2", FULL, precision=F16) == PAIR_PAIR


def test_the_route_is_a_value_of_its_arguments_only(W):
    a = route(W, "convc2", SMALL)
    assert a == route(W, "convc2", SMALL) and hash(a) == hash(route(W, "convc2", SMALL)) and {a: 1}[PAIR_PAIR] == 1
    blk = W.convc2
    X, Y = planes("koct", 256, *SMALL), planes("koct", 192, *SMALL)
    cx = ops.Ctx(F16X2, split_ws=torch.zeros(4))
    assert resolve_skblock(blk, X, Y, cx) == resolve_skblock(blk, X, Y, cx.no_split()) == a
    # offsets, strides and image ranges of the same tensors do not matter, the pixel total does
    assert resolve_skblock(blk, planes("koct", 256, *SMALL, off=512), planes("koct", 192, *SMALL, off=1024), cx) == a
    assert resolve_skblock(blk, planes("koct", 256, 7039, 4), planes("koct", 192, 7039, 4), cx) == a
    assert resolve_skblock(blk, planes("koct", 256, 7040, 4), planes("koct", 192, 7040, 4), cx) == PAIR_TAIL


# ---- B. the executor follows the route -------------------------------------------------------------------------------------------

def _d(p):
    return ("koct" if p.koct else "f16" if p.f16 else "f32", p.rows, p.n_img, p.off, p.img_stride)


@pytest.fixture
def launches(W, monkeypatch):
    """ops.gemm / ffn_pair / sk_tail / dwconv_res_gelu replaced by recorders: (op, layer | pair | tail, epilogue | mode, gelu_out,
    residual given, (format, rows, n_img, off, img_stride) of every Planes argument)."""
    log, names = [], {}
    for b in BLOCKS:
        for n in HotPathWeights.SK_LAYERS + ("pw_res", "pair1", "pair2", "tail"):
            names[id(getattr(getattr(W, b), n))] = n
    monkeypatch.setattr(ops, "gemm", lambda A, X, Y, epilogue=EPI_NONE, R=None, dw_w=None, dw_b=None, cx=None:
                        log.append(("gemm", names[id(A)], epilogue, None, R is not None, _d(X), _d(Y)) + ((_d(R),) if R is not None else ())))
    monkeypatch.setattr(ops, "ffn_pair", lambda pair, X, Y, mode, dw_w=None, dw_b=None, gelu_out=False, cx=None:
                        log.append(("ffn_pair", names[id(pair)], mode, gelu_out, False, _d(X), _d(Y))))
    monkeypatch.setattr(ops, "sk_tail", lambda tail, X, Y, gelu_out=False, cx=None:
                        log.append(("sk_tail", names[id(tail)], None, gelu_out, False, _d(X), _d(Y))))
    monkeypatch.setattr(ops, "dwconv_res_gelu", lambda X, wgt, bias, Y, h, w, k, single=False, cx=None:
                        log.append(("dwconv", k, None, None, False, _d(X), _d(Y))))
    return log


def _run(W, block, grid, final_gelu=False, xin=None, **flags):
    """run_skblock over descriptors: X at float 64, Y at 128 (k-octet planes 4 floats further), hid / xa / xb at 1000 / 2000 / 3000."""
    blk, (n, P) = getattr(W, block), grid
    X, Y = planes(xin or IO[block][0], blk.c_in, n, P, 64), planes(IO[block][1], blk.c_out, n, P, 128)
    r8 = lambda r: (r + 7) // 8 * 8
    hid, xa, xb = (Planes(BASE, off, r8(rows) * P, n, r8(rows), P) for off, rows in ((1000, blk.c_mid), (2000, blk.c_in), (3000, blk.c_in)))
    run_skblock(blk, X, Y, hid, xa, xb, 4, P // 4, final_gelu, cx=ops.Ctx(F16X2, **flags))
    return resolve_skblock(blk, X, Y, ops.Ctx(F16X2, **flags))


def test_executor_pair_tail(W, launches):
    n, P = FULL
    assert _run(W, "convc2", FULL) == PAIR_TAIL
    X, Y, x2, x3 = ("koct", 256, n, 68, 256 * P), ("koct", 192, n, 132, 192 * P), ("f16", 256, n, 2000, 256 * P), ("f16", 256, n, 3000, 256 * P)
    assert launches == [("ffn_pair", "pair1", 1, False, False, X, x2),
                        ("dwconv", 15, None, None, False, x2, x3),
                        ("sk_tail", "tail", None, False, False, x3, Y)]


def test_executor_pair_pair_with_final_gelu(W, launches):
    n, P = SMALL
    assert _run(W, "convc1", SMALL, final_gelu=True) == PAIR_PAIR
    X, Y = ("koct", 324, n, 68, 328 * P), ("koct", 256, n, 132, 256 * P)
    x2, x3, x4 = ("f16", 324, n, 2000, 324 * P), ("f16", 324, n, 3000, 324 * P), ("koct", 324, n, 2000, 328 * P)
    assert launches == [("ffn_pair", "pair1", 1, False, False, X, x2),
                        ("dwconv", 15, None, None, False, x2, x3),
                        ("gemm", "pw_res", EPI_GELU, None, False, x3, x4),
                        ("ffn_pair", "pair2", 0, True, False, x4, Y)]


def test_executor_pair_gemms_with_final_gelu(W, launches):
    n, P = FULL
    assert _run(W, "convc1", FULL, final_gelu=True) == PAIR_GEMMS
    X, Y = ("koct", 324, n, 68, 328 * P), ("koct", 256, n, 132, 256 * P)
    x2, x3, x4 = ("f16", 324, n, 2000, 324 * P), ("f16", 324, n, 3000, 324 * P), ("koct", 324, n, 2000, 328 * P)
    hid = ("koct", 486, n, 1000, 488 * P)                # 486 rows: a partial last octet
    assert launches == [("ffn_pair", "pair1", 1, False, False, X, x2),
                        ("dwconv", 15, None, None, False, x2, x3),
                        ("gemm", "pw_res", EPI_GELU, None, False, x3, x4),
                        ("gemm", "ffn2_0", EPI_GELU, None, False, x4, hid),
                        ("gemm", "ffn2_2", EPI_GELU, None, False, hid, Y)]


def test_executor_gemms_tail(W, launches):
    n, P = FULL
    assert _run(W, "convc2", FULL, ffn_pairs=False) == GEMMS_TAIL
    X, Y, x2, x3 = ("koct", 256, n, 68, 256 * P), ("koct", 192, n, 132, 192 * P), ("f16", 256, n, 2000, 256 * P), ("f16", 256, n, 3000, 256 * P)
    hid = ("koct", 384, n, 1000, 384 * P)
    assert launches == [("gemm", "ffn1_0", EPI_GELU, None, False, X, hid),
                        ("gemm", "ffn1_2", EPI_RES_GELU_DW1, None, True, hid, x2, X),
                        ("dwconv", 15, None, None, False, x2, x3),
                        ("sk_tail", "tail", None, False, False, x3, Y)]


def test_executor_gemms_pair(W, launches):
    n, P = SMALL
    assert _run(W, "convf2", SMALL, xin="f32") == GEMMS_PAIR
    X, Y, x2, x3 = ("f32", 128, n, 64, 128 * P), ("koct", 64, n, 132, 64 * P), ("f16", 128, n, 2000, 128 * P), ("f16", 128, n, 3000, 128 * P)
    hid, x4 = ("koct", 192, n, 1000, 192 * P), ("koct", 128, n, 2000, 128 * P)
    assert launches == [("gemm", "ffn1_0", EPI_GELU, None, False, X, hid),
                        ("gemm", "ffn1_2", EPI_RES_GELU_DW1, None, True, hid, x2, X),
                        ("dwconv", 15, None, None, False, x2, x3),
                        ("gemm", "pw_res", EPI_GELU, None, False, x3, x4),
                        ("ffn_pair", "pair2", 0, False, False, x4, Y)]


def test_executor_gemms_gemms_folded_and_unfolded(W, launches):
    n, P = FULL
    assert _run(W, "gru", FULL) == GEMMS_GEMMS
    X, Y = ("f32", 640, n, 64, 640 * P), ("f32", 128, n, 128, 128 * P)
    x2, x3, x4, hid = ("f16", 640, n, 2000, 640 * P), ("f16", 640, n, 3000, 640 * P), ("koct", 640, n, 2000, 640 * P), ("koct", 960, n, 1000, 960 * P)
    assert launches == [("gemm", "ffn1_0", EPI_GELU, None, False, X, hid),
                        ("gemm", "ffn1_2", EPI_RES_GELU_DW1, None, True, hid, x2, X),
                        ("dwconv", 7, None, None, False, x2, x3),
                        ("gemm", "pw_res", EPI_GELU, None, False, x3, x4),
                        ("gemm", "ffn2_0", EPI_GELU, None, False, x4, hid),
                        ("gemm", "ffn2_2", EPI_NONE, None, False, hid, Y)]
    del launches[:]
    assert _run(W, "gru", FULL, pw_fold=False) == R("gemms", "gemms", False, "f32", "f32", "f16", "koct", "koct")
    x2, x3, x4 = ("f32", 640, n, 2000, 640 * P), ("f32", 640, n, 3000, 640 * P), ("f16", 640, n, 2000, 640 * P)
    assert launches == [("gemm", "ffn1_0", EPI_GELU, None, False, X, hid),
                        ("gemm", "ffn1_2", EPI_RES_GELU_DW1, None, True, hid, x2, X),
                        ("dwconv", 7, None, None, False, x2, x3),
                        ("gemm", "pw", EPI_RES_GELU, None, True, x3, x4, x3),
                        ("gemm", "ffn2_0", EPI_GELU, None, False, x4, hid),
                        ("gemm", "ffn2_2", EPI_NONE, None, False, hid, Y)]


def test_executor_takes_a_route(W, launches):
    """A route handed in is followed without asking the resolver: the all-GEMM route where the default is pair + tail."""
    blk, (n, P) = W.convc2, FULL
    X, Y = planes("koct", 256, n, P, 64), planes("koct", 192, n, P, 128)
    hid, xa, xb = (Planes(BASE, off, rows * P, n, rows, P) for off, rows in ((1000, 384), (2000, 256), (3000, 256)))
    run_skblock(blk, X, Y, hid, xa, xb, 4, P // 4, cx=ops.Ctx(F16X2), route=GEMMS_GEMMS)
    assert [(l[0], l[1]) for l in launches] == [("gemm", "ffn1_0"), ("gemm", "ffn1_2"), ("dwconv", 15), ("gemm", "pw_res"), ("gemm", "ffn2_0"),
                                                ("gemm", "ffn2_2")]
