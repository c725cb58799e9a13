"""Case lists of the packed-weight GEMM tests (tests/test_gpu_gemm_packed.py: sf_gemm with a_layout = SF_LAYOUT_SPLIT_F16 through raw
descriptors) and the dispatcher's rules for them restated in Python, so that a CPU test (tests/test_gemm_packed_cases_cpu.py) can hold
the restatement against sf_gemm_route -- the library's own dispatch code -- for every case, and check that the lists reach every
kernel branch.  Pure Python: no torch, no library.

A case is a dict; descriptor(case) turns it into the SfGemm fields (pointers as dummy addresses with the alignment the placement
gives them; the GPU test puts real addresses of the same alignment there) and route(descriptor) restates the dispatch:
("ok", {family, tile_rows, products, nks, res, msplit, n_main, k_splits}) or ("refused", code, message part).

`lay` = a_layout * 4 + b_layout as in csrc/gemm_split.hip: 8 = fp32 K-major planes, 12 = fp16 rows, 13 = fp16 k-octets."""

# SfGemm / SfGemmRoute constants (include/streamflow_hip.h)
K_MAJOR, SPLIT_F16, F16_K_MAJOR, F16_KOCT = 0, 2, 4, 5
F16X3, F16X2, F16 = 1, 2, 3
NONE, GELU, RELU, RES, RES_GELU, DW1, AXPY = range(7)
AUTO, TILED, BSTAT = 0, 1, 2
FP32_TILED, SPLIT_TILED, KOCT_DMA, BDIRECT, FAM_BSTAT, FAM_BSTAT_GELU = 1, 2, 3, 4, 5, 6
BAD_ARG, UNSUPPORTED = -1, -2
PREC = {"f16x3": F16X3, "f16x2": F16X2, "f16": F16}
PM = {"f16x3": 3, "f16x2": 2, "f16": 1}
NEEDS_R = (RES, RES_GELU, DW1, AXPY)
BD_MIN_M, BD_MIN_WG = 192, 384          # SF_GEMM_BD_MIN_M / SF_GEMM_BD_MIN_WG (gemm_split.hip)

# the tolerances the value checks use (tests/test_gpu_gemm_descriptors.py TOL; tests/test_gpu_gemm_bstat.py for fp16 results)
TOL = {"f16x3": 3e-5, "f16x2": 5e-5, "f16": 5e-5}


def cdiv(a, b):
    return -(-a // b)


def up(a, b):
    return cdiv(a, b) * b


# ---- placement: where a logical [batch][rows][cols] view sits in its allocation -----------------------------------------------
def place(kind, rows, cols, mode, group=0, ld=None):
    """(off, ld, stride, group_stride) in elements of `kind`:
    'f32' fp32 planes / 'h16' fp16 rows: element (r, c) at r * ld + c; 'koct' k-octet planes: ((r / 8) * ld + c) * 8 + r % 8 (halves).
    mode 'dense': base on the allocation start, ld = cols, images back to back.  'pitched': base 16 bytes in, ld > cols, a gap after
    every image (and group) -- everything still a multiple of 16 bytes.  'odd' ('f32', 'h16'): base one element in, odd ld / stride /
    group gap.  'even' ('h16'): base 4 bytes in, even ld and stride that are no multiple of 16 bytes.  `ld` given: use it (C16 shares
    C's)."""
    if kind == "koct":
        mode = "dense" if mode == "dense" else "pitched"
        off = 0 if mode == "dense" else 8
        ld = ld or (cols if mode == "dense" else cols + 3)
        gap = 0 if mode == "dense" else 24
        if group:
            gs = group // 8 * ld * 8 + gap
            return off, ld, cdiv(rows, group) * gs + gap, gs
        return off, ld, cdiv(rows, 8) * ld * 8 + gap, 0
    q = 4 if kind == "f32" else 8
    if mode == "dense":
        off, ld, gap = 0, ld or cols, 0
    elif mode == "pitched":
        off, ld, gap = q, ld or up(cols + 1, q) + q, 2 * q
    elif mode == "even":
        assert kind == "h16"
        off, ld, gap = 2, ld or cols + cols % 2 + 2, 2
    else:
        off, ld, gap = 1, ld or cols + 1 + cols % 2, 3 if kind == "f32" else 1
    if group:
        gs = group * ld + gap + (2 if mode == "odd" else 0)
        return off, ld, (cdiv(rows, group) - 1) * gs + group * ld + gap, gs
    return off, ld, rows * ld + gap, 0


def _modes(c):
    """Placement mode of B, C, R for the case's `place` ('dense' | 'pitched' | 'unaligned').  'unaligned' moves every buffer whose
    format allows an alignment below 16 bytes ON THE KERNEL FAMILY THE CASE AIMS AT off it; the others stay pitched."""
    p = c["place"]
    if p != "unaligned":
        return p, p, p
    bstat = c["algo"] == BSTAT
    b = {8: "odd", 12: "odd" if bstat else "even", 13: "pitched"}[c["lay"]]
    # tiled: c_f16 = 1 / 3 and a k-octet residual run on the vector epilogue only (16-byte C and R); B-stationary: dword stores
    free_c = (c["c_f16"] == 0 and (c["r"] != 2 or bstat)) or (c["c_f16"] == 3 and bstat)
    free_r = c["r"] == 1 and (c["c_f16"] in (0, 2) or bstat)
    return b, "odd" if free_c else "pitched", "odd" if free_r else "pitched"


_BASE = {"A_hi": 1 << 20, "A_lo": 2 << 20, "B": 1 << 28, "C": 2 << 28, "C16": 3 << 28, "R": 4 << 28, "bias": 5 << 28, "dw_w": (5 << 28) + 4096,
         "dw_b": (5 << 28) + 8192, "gamma": (5 << 28) + 12288, "split_ws": 6 << 28}


def auto_splits(M, N, K, batch):
    """gemm_split.hip auto_splits (BK = 32)."""
    bm = 128 if M > 64 else (64 if M > 32 else 32)
    wgs = cdiv(M, bm) * cdiv(N, 128) * batch
    nk = cdiv(K, 32)
    if wgs >= 96 or nk < 8:
        return 1
    ks = min(cdiv(512, wgs), nk // 3)
    ks = min(ks, 16 if (wgs <= 16 and nk >= 64) else 8)
    return 1 if ks < 2 else ks


def descriptor(c):
    """SfGemm fields of a case (dict: field -> int / float) plus '_geo': {role: (kind, rows, cols, off, ld, stride, group, group_stride)}
    for the GPU test to build its guarded buffers from.  `over`: field overrides applied last (the refusal cases)."""
    M, N, K, batch, lay = c["M"], c["N"], c["K"], c["batch"], c["lay"]
    mb, mc, mr = _modes(c)
    d = dict(M=M, N=N, K=K, batch=batch, a_layout=SPLIT_F16, b_layout={8: K_MAJOR, 12: F16_K_MAJOR, 13: F16_KOCT}[lay],
             precision=PREC[c["prec"]], epilogue=c["epi"], algo=c["algo"], c_f16=c["c_f16"], r_f16=2 if c["r"] == 2 else 0,
             a_k_pad=c.get("a_k_pad", 128), lda_h=up(M, 128) + c.get("lda_extra", 0), alpha=c.get("alpha", 0.5),
             A_hi=_BASE["A_hi"], A_lo=_BASE["A_lo"], bias=_BASE["bias"] if c.get("bias", True) else 0,
             b_group=c.get("b_group", 0), r_group=c.get("r_group", 0), conv3x3=0, h=0, w=0, k_splits=0)
    geo = {}
    conv = c.get("conv")
    brows = K // 9 if conv else K
    bkind = {8: "f32", 12: "h16", 13: "koct"}[lay]
    off, ld, st, gs = place(bkind, brows, N, mb, d["b_group"])
    geo["B"] = (bkind, brows, N, off, ld, st, d["b_group"], gs)
    d.update(B=_BASE["B"] + off * (4 if bkind == "f32" else 2), ldb=ld, strideB=st, b_group_stride=gs)
    if conv:
        d.update(conv3x3=1, h=conv[0], w=conv[1])
    ckind = {0: "f32", 1: "h16", 2: "koct", 3: "f32"}[c["c_f16"]]
    off, ld, st, _ = place(ckind, M, N, mc)
    geo["C"] = (ckind, M, N, off, ld, st, 0, 0)
    d.update(C=_BASE["C"] + off * (4 if ckind == "f32" else 2), ldc=ld, strideC=st)
    if c["c_f16"] == 3:
        o16, _, s16, _ = place("koct", M, N, "dense" if c["place"] == "dense" else "pitched", ld=ld)
        geo["C16"] = ("koct", M, N, o16, ld, s16, 0, 0)
        d.update(C16=_BASE["C16"] + 2 * o16, strideC16=s16)
    if c["r"]:
        rkind = "koct" if c["r"] == 2 else "f32"
        off, ld, st, gs = place(rkind, M, N, mr, d["r_group"])
        geo["R"] = (rkind, M, N, off, ld, st, d["r_group"], gs)
        d.update(R=_BASE["R"] + off * (4 if rkind == "f32" else 2), ldr=ld, strideR=st, r_group_stride=gs,
                 dw_w=_BASE["dw_w"], dw_b=_BASE["dw_b"], gamma=_BASE["gamma"])
    if c.get("split_ws"):
        d.update(split_ws=_BASE["split_ws"], split_ws_floats=auto_splits(M, N, K, batch) * batch * M * N)
    d.update(c.get("over", {}))
    d["_geo"] = geo
    return d


# ---- the dispatch restated ------------------------------------------------------------------------------------------------
def pick_tile(M):
    """gemm_split.hip pick_tile: 128 rows unless padding M wastes more than a quarter of the MFMAs, then 64 unless M <= 32."""
    if up(M, 128) * 4 <= M * 5:
        return 128
    return 64 if (up(M, 64) * 4 <= M * 5 or M > 32) else 32


def bdirect(d):
    """launch_cfg's B-direct rule (k-octet B on the 128-row tile)."""
    n_wg2 = cdiv(d["N"], 256) * cdiv(d["M"], 128) * d["batch"]
    bd_m = d["M"] >= BD_MIN_M or (d["M"] > 96 and d["K"] <= 192)
    return bd_m and n_wg2 >= BD_MIN_WG and d["k_splits"] <= 1 and d["ldb"] * 32 < 1 << 31


def bstat_auto(d):
    return d["c_f16"] == 2 or (d["b_layout"] == F16_KOCT and up(d["M"], 128) * 4 > d["M"] * 5)


def gemm_bstat_ok(d):
    """gemm_bstat.hip gemm_bstat_ok (without the 2^30 span limits: no case comes near them)."""
    g = lambda k: d.get(k, 0)
    if d["precision"] not in (F16X2, F16) or d["a_layout"] != SPLIT_F16 or d["conv3x3"] or d["k_splits"] > 1:
        return False
    if d["b_layout"] not in (F16_KOCT, K_MAJOR, F16_K_MAJOR):
        return False
    if d["K"] <= 64 or d["K"] > 640 or d["M"] > 1024 or d["c_f16"] == 1:
        return False
    if d["c_f16"] == 2 and d["epilogue"] not in (NONE, GELU, RES_GELU):
        return False
    if d["b_layout"] == F16_K_MAJOR and d["b_group"]:
        return False
    if d["b_group"] % 32 or d["r_group"] % 32:
        return False
    if d["a_k_pad"] < 128 or d["a_k_pad"] % 128:
        return False
    needs_r = d["epilogue"] in NEEDS_R
    if d["r_f16"] == 2 and (not needs_r or d["r_group"]):
        return False
    if needs_r and d["K"] > (512 if d["r_f16"] == 2 else 384):
        return False
    if d["c_f16"] >= 2:
        p, s = (d["C"], d["strideC"]) if d["c_f16"] == 2 else (g("C16"), g("strideC16"))
        if p & 15 or s & 7 or d["ldc"] < d["N"]:
            return False
    if d["b_layout"] == F16_KOCT and (d["B"] & 15 or d["strideB"] & 7 or g("b_group_stride") & 7 or d["ldb"] < d["N"]):
        return False
    if d["r_f16"] not in (0, 2):
        return False
    if needs_r and (not g("R") or g("ldr") < d["N"]):
        return False
    if d["epilogue"] == DW1 and not (g("dw_w") and g("dw_b")):
        return False
    if d["epilogue"] == AXPY and not g("gamma"):
        return False
    if d["r_f16"] == 2 and (g("R") & 15 or g("strideR") & 7):
        return False
    if d["c_f16"] != 2 and d["ldc"] < d["N"]:
        return False
    if d["c_f16"] == 3 and not g("C16"):
        return False
    return True


def _nks_sel(nks):
    return 8 if nks <= 8 else 16 if nks <= 16 else 24 if nks <= 24 else 32 if nks <= 32 else 40


def bstat_route(d):
    """gemm_bstat.hip gemm_bstat_launch: the instantiation (NKS, RES) and the grid shaping (msplit, n_main)."""
    pm = 1 if d["precision"] == F16 else 2
    M, K = d["M"], d["K"]
    gelu = d["epilogue"] == GELU and d["c_f16"] == 2
    wgs = cdiv(d["N"], 128) * d["batch"]
    units = cdiv(M, 32) if gelu else cdiv(M, 64)
    n_main, f = wgs, 1
    if wgs < 512:
        best = 1.0
        for cand in range(2, min(4, units) + 1):
            t = float((wgs * cand + 511) // 512) / cand + 0.04 * (cand - 1)
            if t < best - 1e-9:
                best, f = t, cand
        if f > 1:
            n_main = 0
    if gelu:
        return dict(family=FAM_BSTAT_GELU, tile_rows=0, products=pm, nks=_nks_sel(cdiv(K, 16)), res=0, msplit=f, n_main=n_main, k_splits=0)
    sk = 128 if pm == 1 else 64
    res = 0 if d["epilogue"] not in NEEDS_R else (2 if d["r_f16"] == 2 else 1)
    return dict(family=FAM_BSTAT, tile_rows=0, products=pm, nks=_nks_sel(cdiv(K, sk) * sk // 16), res=res, msplit=f, n_main=n_main, k_splits=0)


def check_output_formats(d):
    """gemm_split.hip check_output_formats: None or the refusal."""
    g = lambda k: d.get(k, 0)
    vec_c = not (d["N"] & 3 or d["ldc"] & 3 or d["strideC"] & 3 or d["C"] & 15)
    vec_r = True
    if g("R") and d["r_f16"] != 2:
        vec_r = not (g("ldr") & 3 or g("strideR") & 3 or g("r_group_stride") & 3 or g("R") & 15)
    ksp = d["k_splits"] > 1
    if d["c_f16"] == 1 and (not vec_c or not vec_r or ksp):
        return UNSUPPORTED, "c_f16 = 1 needs the vector epilogue"
    if d["c_f16"] == 3 and not (vec_c and vec_r and not ksp and not g("strideC16") & 7 and not g("C16") & 15 and d["ldc"] >= d["N"]):
        return UNSUPPORTED, "c_f16 = 3 (fp32 + k-octet output) needs the vector epilogue"
    if d["c_f16"] == 2 and (d["ldc"] < d["N"] or d["strideC"] & 7 or d["C"] & 15 or ksp or d["epilogue"] not in (NONE, GELU, RES_GELU)):
        return UNSUPPORTED, "c_f16 = 2 (k-octet output) needs ldc >= N"
    if d["r_f16"] not in (0, 2):
        return BAD_ARG, "r_f16 must be 0 or 2"
    if d["r_f16"] == 2 and not (g("R") and d["epilogue"] == DW1 and d["c_f16"] != 2 and vec_c and d["r_group"] == 0 and g("ldr") >= d["N"]
                                and not g("strideR") & 7 and not g("R") & 15 and not ksp and d["alpha"] != 0.0):
        return UNSUPPORTED, "r_f16 = 2 (k-octet residual) needs epilogue RES_GELU_DW1"
    return None


def _inner(d):
    """gemm_split.hip gemm_split_dispatch_inner, the checks in its order."""
    M, K = d["M"], d["K"]
    if d["conv3x3"] and (d["b_layout"] != K_MAJOR or (K // 9) % 32 or d["b_group"] or d["k_splits"] > 1):
        return "refused", UNSUPPORTED, "conv3x3 needs a plain K-major B with Cin % 32 == 0"
    if d["b_group"] % 32:
        return "refused", BAD_ARG, "b_group must be a multiple of 32"
    if d["lda_h"] < up(M, 128) or d["lda_h"] & 127 or (d["A_hi"] | d["A_lo"]) & 15:
        return "refused", BAD_ARG, "SPLIT_F16 A needs 16-byte aligned A_hi/A_lo and lda_h = M padded to 128"
    if d["a_k_pad"] < 0 or d["a_k_pad"] & 31:
        return "refused", BAD_ARG, "a_k_pad must be 0 or a multiple of 32"
    if (d["algo"] == BSTAT or (d["algo"] == AUTO and bstat_auto(d))) and gemm_bstat_ok(d):
        return "ok", bstat_route(d)
    if d["algo"] == BSTAT:
        return "refused", UNSUPPORTED, "SF_ALGO_BSTAT cannot run this problem"
    bad = check_output_formats(d)
    if bad:
        return ("refused",) + bad
    pm = {F16X3: 3, F16X2: 2, F16: 1}[d["precision"]]
    rows = pick_tile(M)
    tiled = dict(family=SPLIT_TILED, tile_rows=rows, products=pm, nks=0, res=0, msplit=0, n_main=0, k_splits=0)
    if d["b_layout"] == F16_KOCT:
        if (d["b_group"] & 31 or d.get("b_group_stride", 0) & 7 or d["conv3x3"] or d["strideB"] & 7 or d["B"] & 15 or d["ldb"] < d["N"]):
            return "refused", UNSUPPORTED, "SF_LAYOUT_F16_KOCT B needs F16X2 / F16, a SPLIT_F16 A, groups of a multiple of 32 rows"
        if rows != 128:
            return "refused", UNSUPPORTED, "SF_LAYOUT_F16_KOCT B needs the 128-row tile"
        return "ok", dict(tiled, family=BDIRECT if bdirect(d) else KOCT_DMA)
    if d["b_layout"] == F16_K_MAJOR:
        if d["N"] & 1 or d["ldb"] & 1 or d["strideB"] & 1 or d["b_group"] or d["conv3x3"] or d["B"] & 3:
            return "refused", UNSUPPORTED, "SF_LAYOUT_F16_K_MAJOR B needs SF_PRECISION_F16X2, a SPLIT_F16 A, even N / ldb / strideB"
    return "ok", tiled


def route(d):
    """What sf_gemm / sf_gemm_route answer for descriptor d (packed weights only)."""
    if d["b_layout"] in (F16_K_MAJOR, F16_KOCT) and d["precision"] not in (F16X2, F16):
        return "refused", BAD_ARG, "a stored-fp16 activation operand needs SF_PRECISION_F16X2 or SF_PRECISION_F16"
    if d["conv3x3"] and (d["b_layout"] != K_MAJOR or d["b_group"]):
        return "refused", BAD_ARG, "conv3x3 needs a plain K-major B"
    if d["b_group"] and d["b_layout"] not in (K_MAJOR, F16_KOCT):
        return "refused", BAD_ARG, "b_group needs a K-major or k-octet B"
    # gemm_split_dispatch: the library's own split-K through the caller's scratch
    to_bstat = d["algo"] != TILED and gemm_bstat_ok(d) and (d["algo"] == BSTAT or bstat_auto(d))
    if d["k_splits"] == 0 and d.get("split_ws") and not d["conv3x3"] and not d["c_f16"] and not d["r_f16"] and not to_bstat:
        ks = auto_splits(d["M"], d["N"], d["K"], d["batch"])
        if ks > 1 and d["split_ws_floats"] >= ks * d["batch"] * d["M"] * d["N"]:
            p = dict(d, C=d["split_ws"], ldc=d["N"], strideC=d["M"] * d["N"], bias=0, R=0, epilogue=NONE, alpha=1.0, k_splits=ks)
            r = _inner(p)
            if r[0] == "ok":
                r[1]["k_splits"] = ks
            return r
    return _inner(d)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _case(part, lay, prec, M, N, K, batch, epi=NONE, c_f16=0, r=0, algo=AUTO, place="pitched", **kw):
    """r: residual format 0 none / 1 fp32 planes / 2 k-octets (the epilogue must need it)."""
    assert (r != 0) == (epi in NEEDS_R), (epi, r)
    c = dict(part=part, lay=lay, prec=prec, M=M, N=N, K=K, batch=batch, epi=epi, c_f16=c_f16, r=r, algo=algo, place=place)
    c.update(kw)
    c["id"] = "%s-l%d-%s-M%dN%dK%db%d-e%dc%dr%d-a%d-%s" % (part, lay, prec, M, N, K, batch, epi, c_f16, r, algo, place) + \
              "".join("-%s%s" % (k, str(v).replace(" ", "")) for k, v in sorted(kw.items()) if k != "over")
    c["seed"] = 1000 + hash_id(c["id"].replace("-" + place, "")) % 100000      # (the placements of one problem share their data)
    return c


def hash_id(s):
    """A stable string hash (Python's own is salted per process)."""
    h = 0
    for ch in s:
        h = (h * 131 + ord(ch)) % 1000003
    return h


PLACES = ("pitched", "dense", "unaligned")


def _part_a():
    """Placement: every family x B layout x output form x residual form once, at one ragged size, in three placements."""
    out = []
    N, batch = 132, 3

    def add(lay, prec, M, K, epi, c_f16, r, algo):
        for p in PLACES:
            out.append(_case("A", lay, prec, M, N, K, batch, epi, c_f16, r, algo, p))

    # split tiled, fp32 planes in (lay 8) and fp16 rows in (lay 12): every precision, every output form, every residual form.
    # c_f16 = 2 stays on the tiled family only at K <= 64 or K > 640 (or forced); M = 126 takes the 128-row tile
    for lay, precs in ((8, ("f16x3", "f16x2", "f16")), (12, ("f16x2", "f16"))):
        for i, prec in enumerate(precs):
            add(lay, prec, 126, 100, NONE, 0, 0, AUTO)
            add(lay, prec, 126, 100, RES_GELU, 0, 1, AUTO)
            add(lay, prec, 126, 100, DW1, 0, 2, TILED)
            add(lay, prec, 126, 100, GELU, 1, 0, AUTO)
            add(lay, prec, 126, 100, (RES, AXPY, RES_GELU)[i], 1, 1, AUTO)
            add(lay, prec, 126, 100, DW1, 1, 2, TILED)
            add(lay, prec, 126, 48, GELU, 2, 0, AUTO)
            add(lay, prec, 126, 48, RES_GELU, 2, 1, AUTO)
            add(lay, prec, 126, 100, RELU, 3, 0, AUTO)
            add(lay, prec, 126, 100, (AXPY, RES, DW1)[i], 3, 1, AUTO)
            add(lay, prec, 126, 100, DW1, 3, 2, TILED)
    # k-octet DMA tile (N = 132 never fills the B-direct grid)
    for prec in ("f16x2", "f16"):
        add(13, prec, 126, 100, NONE, 0, 0, TILED)
        add(13, prec, 126, 100, RES, 0, 1, TILED)
        add(13, prec, 126, 100, DW1, 0, 2, TILED)
        add(13, prec, 126, 100, GELU, 1, 0, TILED)
        add(13, prec, 126, 100, NONE, 2, 0, TILED)
        add(13, prec, 126, 100, RES_GELU, 2, 1, TILED)
        add(13, prec, 126, 100, GELU, 3, 0, TILED)
        add(13, prec, 126, 100, DW1, 3, 2, TILED)
        add(13, prec, 126, 100, AXPY, 1, 1, TILED)
        add(13, prec, 126, 100, DW1, 1, 2, TILED)
        add(13, prec, 126, 100, RES_GELU, 3, 1, TILED)
    # activation-stationary: every B layout; fp32 planes / k-octets / both out; both residual formats with every residual epilogue
    for prec in ("f16x2", "f16"):
        for lay in (8, 12, 13):
            add(lay, prec, 126, 100, RELU, 0, 0, BSTAT)
            add(lay, prec, 126, 100, GELU, 2, 0, BSTAT)                 # the pipelined-GELU kernel
            add(lay, prec, 126, 100, NONE, 3, 0, BSTAT)
        add(8, prec, 126, 100, RES, 0, 1, BSTAT)
        add(12, prec, 126, 100, RES_GELU, 2, 1, BSTAT)
        add(13, prec, 126, 100, AXPY, 3, 1, BSTAT)
        add(13, prec, 126, 100, RES, 0, 2, BSTAT)
        add(8, prec, 126, 100, RES_GELU, 2, 2, BSTAT)
        add(12, prec, 126, 100, AXPY, 3, 2, BSTAT)
        add(13, prec, 126, 100, DW1, 3, 2, BSTAT)
        add(13, prec, 126, 100, NONE, 2, 0, AUTO)                       # (AUTO: k-octets out -> B-stationary, general kernel)
    return out


def _part_b():
    out = []
    # -- B-stationary edges: pixel counts below one wave, at 31 / 33, around the 128-pixel tile; M tails of the c_f16 = 3 (M % 4)
    # and c_f16 = 2 (M % 8) stores; K over every NKS instantiation.  (M, K, epilogue, c_f16, r) rotate over the list
    ms = (6, 31, 65, 126, 200)
    ks = (65, 100, 128, 324, 486, 640)
    forms = ((NONE, 0, 0), (GELU, 2, 0), (RELU, 3, 0), (RES_GELU, 3, 1), (DW1, 0, 2), (NONE, 2, 0), (RES, 2, 1), (AXPY, 0, 2))
    i = 0
    for N in (1, 31, 33, 127, 129, 260):
        for lay in (8, 12, 13):
            for prec in ("f16x2", "f16"):
                M, K = ms[i % 5], ks[(i // 2) % 6]
                epi, c_f16, r = forms[i % 8]
                if r == 1 and K > 384:
                    K = 324
                if r == 2 and K > 512:
                    K = 486
                if c_f16 == 2 and epi == RES:
                    epi = RES_GELU
                out.append(_case("B-bstat", lay, prec, M, N, K, 2, epi, c_f16, r, BSTAT, "unaligned" if i % 3 == 0 else "pitched"))
                i += 1
    # a wave owns its pixels' whole K: the first `small` pixels of the run at `big` must equal the run at `small` bitwise
    for big, small in ((129, 33), (260, 129)):
        for lay, prec, K, epi, c_f16, r in ((13, "f16x2", 324, GELU, 2, 0), (8, "f16", 640, NONE, 0, 0), (12, "f16x2", 100, DW1, 3, 2)):
            for N in (big, small):
                out.append(_case("B-prefix", lay, prec, 65, N, K, 1, epi, c_f16, r, BSTAT, "dense", pair=(big, small)))
    # every NKS instantiation: general kernel with RES 0 (all), RES 1 (<= 24), RES 2 (<= 32); pipelined GELU (all); PM 1 and 2
    for prec in ("f16x2", "f16"):
        for K in (100, 200, 324, 486, 640):
            out.append(_case("B-nks", 13, prec, 65, 130, K, 1, NONE, 3, 0, BSTAT))
            out.append(_case("B-nks", 13, prec, 65, 130, K, 1, GELU, 2, 0, BSTAT))
            if K <= 384:
                out.append(_case("B-nks", 8, prec, 65, 130, K, 1, RES_GELU, 0, 1, BSTAT))
            if K <= 512:
                out.append(_case("B-nks", 12, prec, 65, 130, K, 1, DW1, 0, 2, BSTAT))
    # grid shaping: msplit 1 .. 4 (row units of 64, of 32 for the pipelined kernel) and a grid of >= 512 workgroups (n_main > 0)
    for M in (64, 126, 192, 200):
        out.append(_case("B-msplit", 13, "f16x2", M, 260, 128, 2, RES, 0, 1, BSTAT))
    for M in (31, 64, 96, 200):
        out.append(_case("B-msplit", 13, "f16", M, 260, 128, 2, GELU, 2, 0, BSTAT))
    out.append(_case("B-msplit", 13, "f16", 31, 16284, 65, 4, GELU, 2, 0, BSTAT))
    out.append(_case("B-msplit", 8, "f16x2", 6, 16284, 65, 4, NONE, 0, 0, BSTAT))
    # -- B-direct (128 x 256 tile): ceil(N / 256) * ceil(M / 128) * batch >= 384 with a ragged last tile; N = 16284 for the vector
    # epilogue, 16283 for the scalar one.  Both arms of the row rule: M >= 192 (M = 256) and 96 < M <= 128 with K <= 192.  (ALGO_TILED
    # where SF_ALGO_AUTO hands the problem to the activation-stationary kernel: k-octets out.)
    # M = 192 itself never gets there: padded to 256 rows it wastes more than a quarter of the tile, pick_tile takes the 64-row
    # tile, which has no k-octet kernel -- SF_ALGO_AUTO runs it activation-stationary, SF_ALGO_TILED refuses (refusals()).
    shapes = ((256, 128, 3), (128, 192, 6))
    j = 0
    for prec in ("f16x2", "f16"):
        for epi, c_f16, r in ((NONE, 0, 0), (GELU, 2, 0), (RELU, 3, 0), (RES_GELU, 0, 1), (DW1, 0, 2), (GELU, 1, 0), (DW1, 3, 2),
                              (RES, 1, 1), (RES_GELU, 2, 1), (AXPY, 3, 1), (DW1, 1, 2)):
            M, K, batch = shapes[j % 2]
            out.append(_case("B-bdirect", 13, prec, M, 16284, K, batch, epi, c_f16, r, TILED, "pitched" if j % 2 else "dense"))
            j += 1
        out.append(_case("B-bdirect", 13, prec, 256, 16283, 128, 3, RES, 0, 1, TILED, "unaligned"))
        out.append(_case("B-m192", 13, prec, 192, 16284, 128, 3, NONE, 0, 0, AUTO, "dense"))
    out.append(_case("B-bdirect", 13, "f16x2", 128, 16284, 192, 6, NONE, 0, 0, AUTO, "dense"))     # (AUTO: M = 128 pads nothing)
    out.append(_case("B-below", 13, "f16x2", 256, 16284 - 256, 128, 3, NONE, 0, 0, TILED))         # 378 tiles: the DMA tile
    # -- tiled with k-octets out
    for prec in ("f16x3", "f16x2", "f16"):
        out.append(_case("B-tiledc2", 8, prec, 126, 132, 960, 2, RES_GELU, 2, 1))
        out.append(_case("B-tiledc2", 8, prec, 128, 132, 48, 2, GELU, 2, 0))
    out.append(_case("B-tiledc2", 13, "f16x2", 126, 132, 960, 2, GELU, 2, 0))
    out.append(_case("B-tiledc2", 12, "f16", 128, 132, 48, 2, NONE, 2, 0))
    # -- tile heights 32 / 64 / 128 of the register-staged kernels, every precision (pick_tile)
    for lay, precs in ((8, ("f16x3", "f16x2", "f16")), (12, ("f16x2", "f16"))):
        for prec in precs:
            for M in (31, 65, 128):
                out.append(_case("B-tile", lay, prec, M, 130, 100, 2, GELU, 0, 0, AUTO, "unaligned" if M == 65 else "pitched"))
    # -- the implicit 3 x 3 convolution with packed weights, ldb > N
    k = 0
    for h, w in ((1, 1), (1, 5), (5, 1), (5, 13)):
        for cin in (32, 64):
            M = (31, 65, 128)[k % 3]
            out.append(_case("B-conv", 8, ("f16x3", "f16x2", "f16")[k % 3], M, h * w, 9 * cin, 2, (RELU, NONE, GELU)[k % 3], 0, 0,
                             conv=(h, w)))
            k += 1
    # -- grouped rows ('(B T) C -> B (T C)' views) with a gap between the groups: B as fp32 planes and as k-octets, on the
    # activation-stationary kernel and on the tiled family; a grouped fp32 residual
    for algo in (BSTAT, TILED):
        out.append(_case("B-group", 13, "f16x2", 126, 132, 384, 2, GELU, 0, 0, algo, b_group=128))
        out.append(_case("B-group", 8, "f16", 126, 132, 384, 2, NONE, 0, 0, algo, b_group=128))
        out.append(_case("B-group", 8, "f16x2", 128, 132, 256, 2, RES, 0, 1, algo, r_group=32))
    # -- weight planes: a_k_pad = 0 / 32 (cut at K rounded up to 32) on the tiled kernels, lda_h beyond M padded to 128 everywhere
    for a_k_pad in (0, 32):
        # (K = 130: the planes end at 160 rows of k, not at 256)
        out.append(_case("B-wpad", 8, "f16x3", 126, 132, 130, 2, NONE, 0, 0, TILED, a_k_pad=a_k_pad))
        out.append(_case("B-wpad", 13, "f16x2", 126, 132, 130, 2, NONE, 0, 0, TILED, a_k_pad=a_k_pad, lda_extra=128))
        out.append(_case("B-wpad", 12, "f16", 65, 132, 130, 2, NONE, 0, 0, TILED, a_k_pad=a_k_pad, lda_extra=128))
    out.append(_case("B-wpad", 13, "f16x2", 126, 132, 100, 2, GELU, 2, 0, BSTAT, lda_extra=128))
    out.append(_case("B-wpad", 8, "f16", 200, 132, 324, 2, NONE, 0, 0, BSTAT, lda_extra=128))
    out.append(_case("B-wpad", 13, "f16", 256, 16284, 160, 3, NONE, 0, 0, TILED, lda_extra=128, a_k_pad=32))     # B-direct
    # -- the library's own split-K with packed weights
    out.append(_case("B-splitk", 8, "f16x3", 128, 300, 1024, 1, GELU, 0, 0, split_ws=True))
    out.append(_case("B-splitk", 13, "f16x2", 128, 300, 1024, 1, RES, 0, 1, split_ws=True, place="dense"))
    return out


def _part_c():
    """Determinism: one case per family, run five times."""
    return [_case("C", 8, "f16x3", 126, 1000, 200, 2, RES_GELU, 0, 1),
            _case("C", 12, "f16x2", 65, 1000, 200, 2, GELU, 1, 0),
            _case("C", 13, "f16x2", 126, 1000, 200, 2, DW1, 3, 2, TILED),
            _case("C", 13, "f16", 256, 16284, 128, 3, GELU, 2, 0, TILED, "dense"),
            _case("C", 13, "f16x2", 200, 1000, 324, 2, RES_GELU, 3, 1, BSTAT),
            _case("C", 13, "f16x2", 200, 1000, 324, 2, GELU, 2, 0, BSTAT)]


def cases():
    """Every accepted case, in run order."""
    return _part_a() + _part_b() + _part_c()


# ---- refusals: (id, case, overrides, code, message part) -----------------------------------------------------------------
def refusals():
    base13 = dict(lay=13, prec="f16x2", M=126, N=132, K=100, batch=2)
    out = []

    def add(name, code, msg, over=None, epi=NONE, c_f16=0, r=0, algo=AUTO, place="pitched", **kw):
        b = dict(base13)
        b.update({k: kw.pop(k) for k in list(kw) if k in b})
        c = _case("R", b["lay"], b["prec"], b["M"], b["N"], b["K"], b["batch"], epi, c_f16, r, algo, place, **kw)
        c["over"] = over or {}
        c["id"] = "R-" + name
        out.append((c, code, msg))

    koct_msg, c2_msg, c3_msg, r2_msg = "SF_LAYOUT_F16_KOCT B needs", "c_f16 = 2 (k-octet output) needs", "c_f16 = 3 (fp32 + k-octet output) needs", "r_f16 = 2 (k-octet residual) needs"
    bs_msg = "SF_ALGO_BSTAT cannot run this problem"
    B, C, C16, R = (_BASE[k] for k in ("B", "C", "C16", "R"))
    add("koct-M96-tiled", UNSUPPORTED, "needs the 128-row tile (M padded to 128 within 1.25 M", M=96, algo=TILED)
    add("koct-M192-tiled", UNSUPPORTED, "needs the 128-row tile (M padded to 128 within 1.25 M", M=192, N=16284, K=128, batch=3, algo=TILED)
    add("koct-f16x3", BAD_ARG, "a stored-fp16 activation operand needs", prec="f16x3")
    add("rows-f16x3", BAD_ARG, "a stored-fp16 activation operand needs", prec="f16x3", lay=12)
    # 16-byte bases and strides % 8 of the k-octet forms, on both families
    for algo, tag in ((TILED, "tiled"), (BSTAT, "bstat")):
        bs = algo == BSTAT
        add("B-base-" + tag, UNSUPPORTED, bs_msg if bs else koct_msg, dict(B=B + 8), algo=algo)
        add("B-stride-" + tag, UNSUPPORTED, bs_msg if bs else koct_msg, dict(strideB=13 * 135 * 8 + 4), algo=algo)
        add("B-ldb-" + tag, UNSUPPORTED, bs_msg if bs else koct_msg, dict(ldb=131), algo=algo)
        add("B-groupstride-" + tag, UNSUPPORTED, bs_msg if bs else koct_msg, dict(b_group_stride=32 // 8 * 135 * 8 + 4), algo=algo, K=128, b_group=32)
        add("C2-base-" + tag, UNSUPPORTED, bs_msg if bs else c2_msg, dict(C=C + 8), c_f16=2, algo=algo)
        add("C2-stride-" + tag, UNSUPPORTED, bs_msg if bs else c2_msg, dict(strideC=16 * 135 * 8 + 4), c_f16=2, algo=algo)
        add("C2-ldc-" + tag, UNSUPPORTED, bs_msg if bs else c2_msg, dict(ldc=131), c_f16=2, algo=algo)
        add("C16-base-" + tag, UNSUPPORTED, bs_msg if bs else c3_msg, dict(C16=C16 + 8), c_f16=3, algo=algo)
        add("C16-stride-" + tag, UNSUPPORTED, bs_msg if bs else c3_msg, dict(strideC16=16 * 136 * 8 + 4), c_f16=3, algo=algo)
        add("C3-ldc-" + tag, UNSUPPORTED, bs_msg if bs else c3_msg, dict(ldc=128), c_f16=3, algo=algo)
        add("R2-base-" + tag, UNSUPPORTED, bs_msg if bs else r2_msg, dict(R=R + 8), epi=DW1, r=2, algo=algo)
        add("R2-stride-" + tag, UNSUPPORTED, bs_msg if bs else r2_msg, dict(strideR=16 * 135 * 8 + 4), epi=DW1, r=2, algo=algo)
        add("R2-ldr-" + tag, UNSUPPORTED, bs_msg if bs else r2_msg, dict(ldr=131), epi=DW1, r=2, algo=algo)
        add("R2-grouped-" + tag, UNSUPPORTED, bs_msg if bs else r2_msg, dict(r_group=32, r_group_stride=32 * 135), epi=DW1, r=2, algo=algo)
        add("c2-epilogue-" + tag, UNSUPPORTED, bs_msg if bs else c2_msg, epi=RELU, c_f16=2, algo=algo)
        add("c2-dw1-" + tag, UNSUPPORTED, bs_msg if bs else c2_msg, epi=DW1, c_f16=2, r=1, algo=algo)
    add("C2-base-auto", UNSUPPORTED, c2_msg, dict(C=C + 8), c_f16=2)                # AUTO: B-stationary declines, the tiled family names it
    add("b_group-48", BAD_ARG, "b_group must be a multiple of 32", dict(b_group=48, b_group_stride=48 * 135), K=96, lay=8)
    add("b_group-48-koct", BAD_ARG, "b_group must be a multiple of 32", dict(b_group=48, b_group_stride=48 * 135), K=96)
    add("b_group-rows", BAD_ARG, "b_group needs a K-major or k-octet B", dict(b_group=32, b_group_stride=32 * 136), K=96, lay=12)
    lda_msg = "SPLIT_F16 A needs 16-byte aligned A_hi/A_lo and lda_h = M padded to 128"
    add("lda_h-small", BAD_ARG, lda_msg, dict(lda_h=128), M=200)
    add("lda_h-192", BAD_ARG, lda_msg, dict(lda_h=192))
    add("lda_h-small-bstat", BAD_ARG, lda_msg, dict(lda_h=128), M=200, algo=BSTAT)
    add("A_hi-misaligned", BAD_ARG, lda_msg, dict(A_hi=_BASE["A_hi"] + 8))
    for v in (8, 16, 100, -32):           # a padding promise below what the kernels read (added with these tests)
        add("a_k_pad%d" % v, BAD_ARG, "a_k_pad must be 0 or a multiple of 32", dict(a_k_pad=v), lay=8, algo=(AUTO, TILED, BSTAT)[v % 3])
    add("A_lo-misaligned", BAD_ARG, lda_msg, dict(A_lo=_BASE["A_lo"] + 4), lay=8)
    # c_f16 = 1 / 3 without the vector epilogue on the tiled family
    c1_msg = "c_f16 = 1 needs the vector epilogue"
    add("c1-N", UNSUPPORTED, c1_msg, N=130, c_f16=1, algo=TILED)
    add("c1-ldc", UNSUPPORTED, c1_msg, dict(ldc=134), c_f16=1, algo=TILED)
    add("c1-strideC", UNSUPPORTED, c1_msg, dict(strideC=126 * 144 + 18), c_f16=1, algo=TILED)
    add("c1-base", UNSUPPORTED, c1_msg, dict(C=C + 8), c_f16=1, algo=TILED)
    add("c1-R-base", UNSUPPORTED, c1_msg, dict(R=R + 4), epi=RES, c_f16=1, r=1, algo=TILED)
    add("c1-ldr", UNSUPPORTED, c1_msg, dict(ldr=133), epi=RES, c_f16=1, r=1, algo=TILED)
    add("c1-bstat", UNSUPPORTED, bs_msg, c_f16=1, algo=BSTAT)
    add("c3-N", UNSUPPORTED, c3_msg, N=130, c_f16=3, algo=TILED)
    add("c3-ldc", UNSUPPORTED, c3_msg, dict(ldc=134), c_f16=3, algo=TILED)
    add("c3-base", UNSUPPORTED, c3_msg, dict(C=C + 4), c_f16=3, algo=TILED)
    add("c3-strideR", UNSUPPORTED, c3_msg, dict(strideR=126 * 140 + 9), epi=AXPY, c_f16=3, r=1, algo=TILED)
    # a k-octet residual on the tiled family: RES_GELU_DW1 and the vector epilogue only
    for epi in (RES, RES_GELU, AXPY):
        add("r2-epi%d-tiled" % epi, UNSUPPORTED, r2_msg, epi=epi, r=2, algo=TILED)
    add("r2-N-tiled", UNSUPPORTED, r2_msg, N=130, epi=DW1, r=2, algo=TILED)
    add("r2-C-base-tiled", UNSUPPORTED, r2_msg, dict(C=C + 4), epi=DW1, r=2, algo=TILED)
    add("r2-no-residual-epilogue", UNSUPPORTED, bs_msg, dict(r_f16=2, R=R, ldr=135, strideR=16 * 135 * 8), epi=GELU, algo=BSTAT)
    # SF_ALGO_BSTAT outside what the kernel is built for
    add("bstat-K64", UNSUPPORTED, bs_msg, K=64, algo=BSTAT)
    add("bstat-K641", UNSUPPORTED, bs_msg, K=641, algo=BSTAT)
    add("bstat-a_k_pad32", UNSUPPORTED, bs_msg, algo=BSTAT, a_k_pad=32)
    add("bstat-a_k_pad0", UNSUPPORTED, bs_msg, algo=BSTAT, a_k_pad=0)
    add("bstat-conv3x3", UNSUPPORTED, bs_msg, lay=8, N=65, K=288, algo=BSTAT, conv=(5, 13))
    add("bstat-f16x3", UNSUPPORTED, bs_msg, lay=8, prec="f16x3", algo=BSTAT)
    add("bstat-R32-K385", UNSUPPORTED, bs_msg, K=385, epi=RES, r=1, algo=BSTAT)
    add("bstat-R16-K513", UNSUPPORTED, bs_msg, K=513, epi=DW1, r=2, algo=BSTAT)
    add("bstat-M1025", UNSUPPORTED, bs_msg, M=1025, algo=BSTAT)
    # fp16 rows with odd extents: the tiled family refuses them (the activation-stationary kernel takes them: part B)
    rows_msg = "SF_LAYOUT_F16_K_MAJOR B needs"
    add("rows-N-odd", UNSUPPORTED, rows_msg, lay=12, N=131, algo=TILED)
    add("rows-ldb-odd", UNSUPPORTED, rows_msg, dict(ldb=137), lay=12, algo=TILED)
    add("rows-strideB-odd", UNSUPPORTED, rows_msg, dict(strideB=100 * 144 + 17), lay=12, algo=TILED)
    add("rows-base-2", UNSUPPORTED, rows_msg, dict(B=B + 2), lay=12, algo=TILED)
    add("rows-N-odd-auto", UNSUPPORTED, rows_msg, lay=12, N=131)
    add("conv-Cin48", UNSUPPORTED, "conv3x3 needs a plain K-major B with Cin", lay=8, N=65, K=9 * 48, conv=(5, 13))
    return out


def accepted_forms():
    """Every (family, B layout of the register-staged tiles else 0, products, c_f16, residual format) the library accepts for packed
    weights: the combinations the GPU file must run at least once."""
    out = set()
    tiled_cr = [(cf, r) for cf in (0, 1, 2, 3) for r in (0, 1, 2) if not (cf == 2 and r == 2)]      # (a k-octet residual: c_f16 != 2)
    for cf, r in tiled_cr:
        out |= {(SPLIT_TILED, 8, pm, cf, r) for pm in (1, 2, 3)} | {(SPLIT_TILED, 12, pm, cf, r) for pm in (1, 2)}
        out |= {(fam, 0, pm, cf, r) for fam in (KOCT_DMA, BDIRECT) for pm in (1, 2)}
    out |= {(FAM_BSTAT, 0, pm, cf, r) for pm in (1, 2) for cf in (0, 2, 3) for r in (0, 1, 2)}
    out |= {(FAM_BSTAT_GELU, 0, pm, 2, 0) for pm in (1, 2)}
    return out
