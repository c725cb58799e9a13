"""Case lists of tests/test_gpu_glue_kernels.py: the per-pixel kernels between the GEMMs and the fused chains -- sf_temporal_attn /
sf_temporal_attn_f16in, sf_layernorm_cm, sf_upsample_flow, sf_bilinear_sampler, sf_context_split, sf_flow_update, sf_pack_koct,
sf_dwconv3x3_res -- through the C ABI.  Pure Python: no torch, no device; tests/test_glue_cases_cpu.py checks the coverage and holds
the float64 restatements and the draws.

A case is a dict with `kernel`, `id`, `seed` and the kernel's own sizes.  One case is one pytest case; what a case loops over
inside (input classes, eps, logit gains, output forms, destinations) is listed here as well, so that the CPU file can assert it.
Every case with more than one image is also run one image at a time (BATCHES)."""

BATCHES = (1, 3)                                          # images (clips for the attention) of a run; 1 = each image alone

# ---- sf_temporal_attn, sf_temporal_attn_f16in: workgroup = 64 pixels, channels split over 4 waves, C / 4 each (unrolled by 4) -------
ATTN_TT = (1, 2, 3, 4, 5, 6, 7)
ATTN_C = (4, 36, 32, 128)                                 # C / 4 = 1, 9 (no multiple of the unroll), 8 (one k-octet per wave), 32
ATTN_P = (1, 63, 64, 65, 130)
ATTN_GAINS = (1, 4)                                       # on q and k: at C = 128, gain 4 spreads the scores over about 16
ATTN_GRID_P = 65                                          # the full TT x C grid runs here
ATTN_PLIST_TT, ATTN_PLIST_C = (1, 3, 7), (36, 128)        # the full P list runs here
ATTN_ENTRIES = ("f32", "f16in")
ATTN_TT_REFUSED, ATTN_KOCT_C_REFUSED = 8, 36

# ---- sf_layernorm_cm: C = 128 / 256 -> the split kernel (64 pixels a workgroup), anything else one thread per pixel (256) ----------
LN_C = (128, 256, 96, 324, 1)
LN_P = (1, 63, 64, 65, 257)
LN_EPS = (1e-5, 1e-6)
LN_CLASSES = ("golden", "mean100", "tiny", "constcol")    # randn * 2 + 0.3 | randn + 100 | randn * 1e-3 | golden + a constant column
LN_KOCT_C = (128, 256)
LN_KOCT_C_REFUSED = 96
# the constant of the variance-0 column: a dyadic value whose partial sums (up to 324 copies) and whose mean are exact in fp32 in
# any order, so that x - mean is exactly 0 and the output exactly beta.  (A constant like 3.7 leaves the fp32 mean up to an ulp
# off; 1 / sqrt(eps) = 1000 then turns that ulp into 2e-4 of output in ANY fp32 LayerNorm: a property of the format, not an edge.)
LN_CONST = 3.5

# ---- sf_upsample_flow: one workgroup per (image, row, 32-pixel x segment) ---------------------------------------------------------
UP_SHAPES = ((1, 1, 1), (2, 2, 31), (1, 3, 32), (2, 3, 33), (1, 2, 65))          # (n, h, w)
UP_CLASSES = ("golden", "sharp", "equal", "onehot")       # flow 3 mask 2 | flow 100 mask 30 | equal logits | one +80 among -80s
UP_SEG = 32

# ---- sf_bilinear_sampler: grid-stride loop of 256-thread blocks ------------------------------------------------------------------
BS_IMAGES = ((1, 1, 2, 2), (3, 5, 6, 7), (2, 1, 1, 9))    # (M, C, Hi, Wi)
BS_POINTS = (20, 15)                                      # (Ho, Wo): 300 points, more than one block
INF, NAN = float("inf"), float("nan")


def bs_fixed_coords(Hi, Wi):
    """[(x, y)] written over the first points of every image: corners, half a pixel / one pixel outside, far outside, non-finite."""
    yi, xi = 0.25 * (Hi - 1), 0.5 * (Wi - 1) + 0.25       # inside (or on the only row / column)
    return [(0.0, 0.0), (Wi - 1.0, 0.0), (0.0, Hi - 1.0), (Wi - 1.0, Hi - 1.0),
            (-0.5, yi), (Wi - 0.5, yi), (xi, -1.0), (xi, float(Hi)),
            (1e7, yi), (-1e7, yi), (INF, yi), (-INF, yi), (NAN, yi), (xi, NAN), (xi, 1e7), (xi, -INF)]


BS_ZERO = slice(6, 16)                                    # of bs_fixed_coords: every tap outside the image, or a non-finite coordinate

# ---- sf_context_split, sf_flow_update, sf_pack_koct ------------------------------------------------------------------------------
CS_HDIM, CS_P = (1, 128), (1, 257)
CS_SATURATED = (20.0, -20.0)
FU_SHAPES = ((1, 1, 1), (3, 9, 20), (2, 3, 257))          # (n, h, w)
FU_DESTS = ("a", "b", "ab", "koct")                       # flow_a | flow_b | both, different strides | neither, flow_koct
FU_KOCT_ROWS = (126, 7, 0)                                # 7: x in lane 7 of octet 0, y in lane 0 of octet 1
FU_KOCT_IMAGE_ROWS = 128
FU_FAR = (3000.0, -3000.0)
PK_ROWS = (1, 7, 8, 9, 126, 324)
PK_P = (1, 255, 256, 257)
# fp32 values whose fp16 rounding is the point: overflow to infinity, fp16 subnormals, exact ties (to even: down, then up), -0.0
PK_SPECIAL = (7e4, -7e4, 1e-7, -1e-7, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24 * 1.5, 65520.0, -0.0)

# ---- sf_dwconv3x3_res: vec4 kernel (4 pixels a thread: a workgroup = 1024 pixels) when W % 4 == 0 and all is aligned, else scalar ---
DW_SHAPES = ((1, 1), (1, 4), (3, 4), (5, 9), (9, 31), (5, 260))                  # (H, W)
DW_C, DW_N = (1, 3), (1, 2)

KERNELS = ("temporal_attn", "layernorm", "upsample", "bilinear", "context_split", "flow_update", "pack_koct", "dwconv3x3")


def _mk(kernel, seed, **kw):
    c = dict(kernel=kernel, seed=seed, **kw)
    c["id"] = "-".join([kernel] + ["%s%s" % (k, "x".join(map(str, v)) if isinstance(v, tuple) else v) for k, v in kw.items()])
    return c


def attn_cases():
    keys = [(TT, C, ATTN_GRID_P) for TT in ATTN_TT for C in ATTN_C]
    keys += [(TT, C, P) for TT in ATTN_PLIST_TT for C in ATTN_PLIST_C for P in ATTN_P if P != ATTN_GRID_P]
    return [_mk("temporal_attn", 100 + i, TT=TT, C=C, P=P, B=BATCHES[-1]) for i, (TT, C, P) in enumerate(keys)]


def attn_forms(C):
    """Output requests: `out` alone, and where the k-octet copy exists (C % 32 == 0) the copy alone and both."""
    return ("out", "koct", "both") if C % 32 == 0 else ("out",)


def ln_cases():
    return [_mk("layernorm", 200 + i, C=C, P=P, n=BATCHES[-1]) for i, (C, P) in enumerate((C, P) for C in LN_C for P in LN_P)]


def ln_forms(C):
    return ("y", "koct", "both") if C in LN_KOCT_C else ("y",)


def up_cases():
    return [_mk("upsample", 300 + i, nhw=s) for i, s in enumerate(UP_SHAPES)]


def bs_cases():
    return [_mk("bilinear", 400 + i, img=s) for i, s in enumerate(BS_IMAGES)]


def cs_cases():
    return [_mk("context_split", 500 + i, hdim=hd, P=P, n=BATCHES[-1]) for i, (hd, P) in enumerate((a, b) for a in CS_HDIM for b in CS_P)]


def fu_cases():
    return [_mk("flow_update", 600 + i, nhw=s) for i, s in enumerate(FU_SHAPES)]


def pk_cases():
    return [_mk("pack_koct", 700 + i, rows=r, P=P, n=BATCHES[-1]) for i, (r, P) in enumerate((a, b) for a in PK_ROWS for b in PK_P)]


def dw_cases():
    return [_mk("dwconv3x3", 800 + i, hw=s) for i, s in enumerate(DW_SHAPES)]


def all_cases():
    return attn_cases() + ln_cases() + up_cases() + bs_cases() + cs_cases() + fu_cases() + pk_cases() + dw_cases()


# ---- placements ------------------------------------------------------------------------------------------------------------------
# These entry points take image strides only (or nothing: tight tensors), so ld = cols always.  Elements per layout, and the base
# alignment in bytes that include/streamflow_hip.h demands: k-octet planes 16 (and image strides of whole octets), fp32 4, fp16 rows
# 2; "f32x4": the alignment at which sf_dwconv3x3_res takes its vec4 kernel (16 bytes, image strides % 4 floats).
ELEM = {"f32": 4, "rows16": 2, "koct": 2, "f32x4": 4}
BASE_ALIGN = {"f32": 4, "rows16": 2, "koct": 16, "f32x4": 16}
STRIDE_MULT = {"f32": 1, "rows16": 1, "koct": 8, "f32x4": 4}


def place(layout, rows, cols, placed, strided=True, k=0):
    """(off, stride) in elements for a logical [rows][cols] image.  placed = False: offset 0, tight.  placed = True: the base the
    smallest step off the allocation's start that the layout's alignment allows, and (strided: the entry point takes an image
    stride for this operand) a stride beyond the span by a gap that differs from operand to operand (k) and is odd where the
    layout allows."""
    span = -(-rows // 8) * cols * 8 if layout == "koct" else rows * cols
    if not placed:
        return 0, span
    off = BASE_ALIGN[layout] // ELEM[layout]
    if not strided:
        return off, span
    return off, span + STRIDE_MULT[layout] * (3 + 2 * k)
