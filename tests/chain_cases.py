"""Case lists of tests/test_gpu_chain_descriptors.py: the four fused chain kernels (sf_ffn_pair, sf_sk_tail, sf_temporal_block,
sf_mask_upsample) through raw descriptors.  Pure Python: no torch, no device; tests/test_chain_cases_cpu.py checks the coverage.

A case is a dict: kernel, shape, pm (product counts), N or hw, batch, placement ("contiguous" / "aligned" / "unaligned"), seed,
plus what only one kernel has (mode, TT, x_group, r32).  Parts:
  A  placement: every shape x product combination at one ragged size, pitched / gapped / offset against contiguous;
  B  tile edges: every shape at its largest product count, sizes around the wave and workgroup widths, contiguous;
  C  product class: every shape x product combination, weights whose `lo` halves are as large as fp16 allows."""

# (K1, H, M2) by mode; (K1, M2) must be streamflow_amd.ops.PAIR_SHAPES (checked on the CPU), H = 1.5 K1 (update.py:14-16)
PAIR_MODE1 = [(128, 192, 128), (256, 384, 256), (324, 486, 324), (384, 576, 384)]
PAIR_MODE0 = [(128, 192, 64), (256, 384, 192), (256, 384, 126), (324, 486, 256), (384, 576, 6), (256, 384, 4), (128, 192, 2)]
PAIR_PM = [(1, 1), (2, 1), (2, 2)]                       # what ops.ffn_pair_ok admits
TAIL_SHAPES = [(256, 384, 192), (256, 384, 126), (384, 576, 6), (128, 192, 64)]      # tests/test_gpu_sk_tail.py::SHAPES
TAIL_UNBUILT = ((256, 384, 192), 1)                      # the one combination the project declares unbuilt (csrc/sk_tail.hip)
TEMPORAL_SHAPE = (128, 256)                              # (C, hidden)
MASK_SHAPE = (256, 576)                                  # (K, M)
R32_K1 = (128, 256, 384)                                 # mode 1 with the fp32 residual is built for the flow head's ffn1 shapes only

# pixels per wave, pixels per workgroup (ffn_pair: NW = 4 or 8 waves, chosen by shape)
WAVE = {"ffn_pair": 16, "sk_tail": 32, "temporal_block": 16, "mask_upsample": 16}
WORKGROUP = {"ffn_pair": (64, 128), "sk_tail": (128,), "temporal_block": (64,), "mask_upsample": (64,)}

A_N = {"ffn_pair": 132, "sk_tail": 132, "temporal_block": 68}
A_HW = [(4, 17), (9, 15)]
A_BATCH = 3
B_N = {"sk_tail": [1, 31, 33, 100, 128, 129, 260], "ffn_pair": [1, 15, 17, 68, 127, 129, 260], "temporal_block": [1, 15, 17, 65, 132]}
B_HW = [(1, 1), (1, 5), (5, 1), (5, 13), (2, 34), (9, 15)]
B_BATCHES = (1, 3)
# (big, small): the first `small` pixels of the run at `big` must be bitwise the run at `small` (the temporal block's list has no 129
# or 260: its pairs step over a wave and over a workgroup the same way)
B_PREFIX = {"sk_tail": [(129, 33), (260, 129)], "ffn_pair": [(129, 17), (260, 129)], "temporal_block": [(132, 65), (65, 17)]}
C_N, C_BATCH = 260, 2
D_HW, D_BATCH, D_REPEATS = (47, 156), 3, 5

# alignment the entry points require today (the SF_REQUIRE lines of csrc/ffn_pair.hip, sk_tail.hip, temporal.hip, mask_upsample.hip),
# in bytes, by operand layout: k-octet planes 16 (and image / group strides of whole octets: % 8 halves), fp32 planes 4, fp16 rows
# none stated (2: the element).  sf_mask_upsample's `out` is the one fp32 operand with 16.
BASE_ALIGN = {"koct": 16, "f32": 4, "rows16": 2, "f32_out16": 16}
ELEM = {"koct": 2, "f32": 4, "rows16": 2, "f32_out16": 4}


def _id(c):
    s = "x".join(str(v) for v in c["shape"])
    pm = "".join(str(v) for v in c["pm"]) if isinstance(c["pm"], tuple) else str(c["pm"])
    parts = [c["kernel"], s, "pm" + pm]
    if "mode" in c:
        parts.append("m%d" % c["mode"])
    if "TT" in c:
        parts.append("T%d" % c["TT"])
    if c.get("x_group"):
        parts.append("g%d" % c["x_group"])
    if c.get("r32"):
        parts.append("r32")
    parts.append("N%d" % c["N"] if "N" in c else "%dx%d" % c["hw"])
    parts.append("b%d" % c["batch"])
    if c["placement"] != "contiguous":
        parts.append(c["placement"])
    return "-".join(parts)


def _case(kernel, shape, pm, batch, placement, seed, **kw):
    c = dict(kernel=kernel, shape=shape, pm=pm, batch=batch, placement=placement, seed=seed, **kw)
    c["id"] = _id(c)
    return c


def pair_shapes():
    return [(s, 1) for s in PAIR_MODE1] + [(s, 0) for s in PAIR_MODE0]


def part_a():
    """Placement cases.  Both classes alternate over the list, so every shape meets both."""
    out, k = [], 0
    cls = lambda: ("aligned", "unaligned")[k % 2]
    for shape, mode in pair_shapes():
        for pm in PAIR_PM:
            out.append(_case("ffn_pair", shape, pm, A_BATCH, cls(), 1000 + k, N=A_N["ffn_pair"], mode=mode)); k += 1
    for K1 in (384, 256, 128):                                     # the grouped flow-head view (update.py:775), both modes
        for mode, M2 in ((1, K1), (0, 2 * K1 // 128)):
            out.append(_case("ffn_pair", (K1, K1 * 3 // 2, M2), (2, 2), A_BATCH, cls(), 1000 + k, N=A_N["ffn_pair"], mode=mode,
                             x_group=128)); k += 1
    for K1 in R32_K1:                                              # mode 1 with the residual from fp32 planes (SfFfnPair.R32)
        out.append(_case("ffn_pair", (K1, K1 * 3 // 2, K1), (2, 2), A_BATCH, cls(), 1000 + k, N=A_N["ffn_pair"], mode=1,
                         x_group=128 if K1 > 128 else 0, r32=True)); k += 1
    for shape in TAIL_SHAPES:
        for pm in (1, 2):
            out.append(_case("sk_tail", shape, pm, A_BATCH, cls(), 1000 + k, N=A_N["sk_tail"])); k += 1
    for TT in (1, 2, 3):
        for pm in (1, 2):
            out.append(_case("temporal_block", TEMPORAL_SHAPE, pm, A_BATCH, cls(), 1000 + k, N=A_N["temporal_block"], TT=TT)); k += 1
    for hw in A_HW:
        for pm in (1, 2):
            out.append(_case("mask_upsample", MASK_SHAPE, pm, A_BATCH, cls(), 1000 + k, hw=hw)); k += 1
    return out


def largest_pm(kernel, shape):
    return (2, 2) if kernel == "ffn_pair" else 2


def part_b():
    """Tile-edge groups: one list of cases per (kernel, shape[, TT]) -- the sizes of a group share their data (the first N pixels of
    one draw), so that prefixes and single images can be compared bit for bit.  Returns [(group id, [case, ...])]."""
    groups, k = [], 0
    for shape, mode in pair_shapes():
        pm = largest_pm("ffn_pair", shape)
        cs = [_case("ffn_pair", shape, pm, b, "contiguous", 2000 + k, N=N, mode=mode) for N in B_N["ffn_pair"] for b in B_BATCHES]
        groups.append(("ffn_pair-%s-m%d" % ("x".join(map(str, shape)), mode), cs)); k += 1
    for shape in TAIL_SHAPES:
        cs = [_case("sk_tail", shape, 2, b, "contiguous", 2000 + k, N=N) for N in B_N["sk_tail"] for b in B_BATCHES]
        groups.append(("sk_tail-%s" % "x".join(map(str, shape)), cs)); k += 1
    for TT in (1, 2, 3):
        cs = [_case("temporal_block", TEMPORAL_SHAPE, 2, b, "contiguous", 2000 + k, N=N, TT=TT) for N in B_N["temporal_block"]
              for b in B_BATCHES]
        groups.append(("temporal_block-T%d" % TT, cs)); k += 1
    for hw in B_HW:
        cs = [_case("mask_upsample", MASK_SHAPE, 2, b, "contiguous", 2000 + k, hw=hw) for b in B_BATCHES]
        groups.append(("mask_upsample-%dx%d" % hw, cs)); k += 1
    return groups


def part_c():
    out, k = [], 0
    for shape, mode in pair_shapes():
        for pm in PAIR_PM:
            out.append(_case("ffn_pair", shape, pm, C_BATCH, "contiguous", 3000 + k, N=C_N, mode=mode)); k += 1
    for shape in TAIL_SHAPES:
        for pm in (1, 2):
            out.append(_case("sk_tail", shape, pm, C_BATCH, "contiguous", 3000 + k, N=C_N)); k += 1
    for TT in (1, 2, 3):
        for pm in (1, 2):
            out.append(_case("temporal_block", TEMPORAL_SHAPE, pm, C_BATCH, "contiguous", 3000 + k, N=C_N, TT=TT)); k += 1
    for pm in (1, 2):
        out.append(_case("mask_upsample", MASK_SHAPE, pm, C_BATCH, "contiguous", 3000 + k, hw=(13, 20))); k += 1      # 13 * 20 = 260
    return out


def layers_of(kernel):
    """Names of the weight layers whose product class part C flips, in the order the kernel's packer takes them."""
    return {"ffn_pair": ("first", "second"), "sk_tail": ("pw", "ffn2_0", "ffn2_2"), "temporal_block": ("qkv", "proj", "fc1", "fc2"),
            "mask_upsample": ("mask2",)}[kernel]


def operands(c):
    """[(field, layout, logical rows, row group, tight)] of a case's strided operands.  tight: the ABI gives the operand no leading
    dimension or image stride (sf_mask_upsample's flow and out), only its base moves."""
    k = c["kernel"]
    if k == "ffn_pair":
        K1, _, M2 = c["shape"]
        g = c.get("x_group", 0)
        ops = [("X", "koct", K1, g, False)]
        ops += [("C", "f32", M2, 0, False), ("C16", "koct", M2, 0, False)] if c["mode"] == 0 else [("C16", "rows16", M2, 0, False)]
        if c.get("r32"):
            ops.append(("R32", "f32", M2, g, False))
        return ops
    if k == "sk_tail":
        C, _, M2 = c["shape"]
        return [("X", "rows16", C, 0, False), ("Y", "f32", M2, 0, False), ("Y16", "koct", M2, 0, False)]
    if k == "temporal_block":
        return [("X16", "koct", 128, 0, False), ("Y", "f32", 128, 0, False), ("Y16", "koct", 128, 0, False)]
    h, w = c["hw"]
    return [("X16", "koct", 256, 0, False), ("flow", "f32", 2 * h, 0, True), ("out", "f32_out16", 16 * h, 0, True)]


def cols_of(c, field):
    if c["kernel"] != "mask_upsample":
        return c["N"]
    h, w = c["hw"]
    return {"X16": h * w, "flow": w, "out": 8 * w}[field]


# ---- placements ------------------------------------------------------------------------------------------------------------------
def place(layout, placement, rows, cols, seed, group=0, tight=False):
    """(off, ld, stride, group_stride) in ELEMENTS of the layout for a logical [rows][cols] image.
    contiguous: ld = cols, tight stride, offset 0.
    aligned: ld padded up to the next multiple of 16 bytes' worth of columns beyond cols, base 16 bytes in, strides whole 16 bytes.
    unaligned: ld = cols + 1 or + 3 (fp16 rows: the odd one of them), the smallest base offset the stated alignment allows, an
    image stride with an odd gap where the layout allows one (k-octet strides stay whole octets: the entry points require it)."""
    if tight:
        off = 0 if placement == "contiguous" else (16 if placement == "aligned" else BASE_ALIGN[layout]) // ELEM[layout]
        return off, cols, rows * cols, 0
    oct_rows = -(-(group or rows) // 8)
    if layout == "koct":                                          # ld counts pixels (16 bytes each); offsets and strides halves
        if placement == "contiguous":
            ld, off, gap = cols, 0, 0
        elif placement == "aligned":
            ld, off, gap = -(-(cols + 1) // 8) * 8, 8, 64
        else:
            ld, off, gap = cols + (1, 3)[seed % 2], 8, 8
        gspan = oct_rows * ld * 8
        gs = gspan + gap if group else 0
        span = (rows // group - 1) * gs + gspan if group else gspan
        return off, ld, span + gap, gs
    q = 16 // ELEM[layout]
    if placement == "contiguous":
        ld, off, gap = cols, 0, 0
    elif placement == "aligned":
        ld, off, gap = -(-(cols + 1) // q) * q, q, 2 * q
    else:
        ld = cols + (1, 3)[seed % 2]
        if layout == "rows16" and ld % 2 == 0:
            ld += 1
        off, gap = BASE_ALIGN[layout] // ELEM[layout], 5
    grows = group or rows
    gs = grows * ld + gap if group else 0
    span = (rows // group - 1) * gs + grows * ld if group else rows * ld
    return off, ld, span + gap, gs
