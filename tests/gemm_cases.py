"""Seeded case lists of the raw-descriptor GEMM tests (tests/test_gpu_gemm_descriptors.py) and the dispatcher rules they
rely on, restated in Python so that a CPU test (tests/test_gemm_rules_cpu.py) can check the lists cover every kernel branch.

Layout pairs are (a_layout, b_layout) of SfGemm: 0 = K-major, 1 = K-minor, 3 = stored-fp16 K-minor B (the attention matrix of
sf_softmax_rows(out16), the engine's `attn16` operand)."""
from streamflow_amd._lib import LAYOUT_F16_K_MINOR, LAYOUT_K_MAJOR, LAYOUT_K_MINOR

PRECS = ("fp32", "f16x3", "f16x2", "f16")
PAIRS = ((LAYOUT_K_MAJOR, LAYOUT_K_MAJOR), (LAYOUT_K_MINOR, LAYOUT_K_MINOR), (LAYOUT_K_MAJOR, LAYOUT_K_MINOR),
         (LAYOUT_K_MINOR, LAYOUT_K_MAJOR), (LAYOUT_K_MINOR, LAYOUT_F16_K_MINOR))
N_EPI = 7


def tile_rows(prec: str, M: int, N: int, batch: int) -> int:
    """Workgroup tile height sf_gemm picks.  fp32 (gemm.hip pick_bm): the smallest makespan on 256 CUs in units of 32-row wave
    tiles, ties to the larger tile.  Split precisions (gemm_split.hip pick_tile): 128 rows unless padding M wastes more than a
    quarter, then 64 unless M <= 32."""
    if prec == "fp32":
        best, best_bm = -1, 128
        for bm in (128, 64, 32):
            wgs = -(-M // bm) * -(-N // 128) * batch
            span = -(-wgs // 256) * (bm // 32)
            if best < 0 or span < best:
                best, best_bm = span, bm
        return best_bm
    if -(-M // 128) * 128 * 4 <= M * 5:
        return 128
    return 64 if (-(-M // 64) * 64 * 4 <= M * 5 or M > 32) else 32


def refusal(prec: str, pair, M: int, N: int, batch: int):
    """The library's message when sf_gemm must refuse this descriptor, else None."""
    if pair == (LAYOUT_K_MINOR, LAYOUT_F16_K_MINOR):
        if prec == "fp32":
            return "stored-fp16 B operand needs a split precision"
        if tile_rows(prec, M, N, batch) != 128:
            return "SF_LAYOUT_F16_K_MINOR B not built for this tile"
        return None
    if prec != "fp32" and pair[0] != pair[1]:
        return "layout combination a=%d b=%d not built" % pair
    return None


# (M, N, K, batch): every list reaches all three tile heights of its precision family (tile_rows); K covers a single row, odd
# tails of the 16 / 32-deep k-tiles and a deep chain; N covers one column, odd widths and the vector epilogue (N % 4 == 0)
_SHAPES_FP32 = [(1, 17, 7, 1), (31, 129, 33, 2), (65, 11520, 33, 1), (300, 5120, 31, 2), (33, 1000, 200, 1),
                (97, 127, 1544, 1), (129, 1, 1, 3)]
_SHAPES_SPLIT = [(1, 17, 7, 1), (31, 129, 33, 2), (33, 1000, 200, 1), (65, 127, 31, 3), (128, 300, 1544, 1),
                 (129, 1, 1, 2), (300, 1000, 97, 1)]
_SHAPES_F16B = [(128, 300, 1544, 1), (103, 17, 7, 2), (128, 129, 33, 3), (256, 1000, 200, 1), (110, 127, 31, 1),
                (128, 1, 1, 2), (205, 64, 323, 1)]          # the stored-fp16 B runs on the 128-row tile only


def raw_cases():
    """[(id, dict)] of the raw-descriptor sweep: every (precision, layout pair, epilogue) once, plus a refused descriptor per
    (precision, pair) the dispatcher does not build."""
    out = []
    for pi, prec in enumerate(PRECS):
        for qi, pair in enumerate(PAIRS):
            shapes = _SHAPES_FP32 if prec == "fp32" else (_SHAPES_F16B if pair[1] == LAYOUT_F16_K_MINOR else _SHAPES_SPLIT)
            for epi in range(N_EPI):
                i = pi * 5 + qi * 3 + epi
                M, N, K, batch = shapes[(epi + qi) % len(shapes)]
                c = dict(prec=prec, pair=pair, epi=epi, M=M, N=N, K=K, batch=batch, alpha=(1.0, 0.5, -1.25)[i % 3],
                         bias=(i % 4 != 1), unaligned=(i % 3 == 2), seed=7000 + 100 * pi + 10 * qi + epi)
                c["refused"] = refusal(prec, pair, M, N, batch)
                if c["refused"] is not None and epi > 0:
                    continue                         # one refused descriptor per (precision, pair) is enough
                out.append(("%s-a%db%d-e%d-M%dN%dK%db%d" % (prec, pair[0], pair[1], epi, M, N, K, batch), c))
    # the 128-row-only form refused at a tile height it has no kernel for
    for prec in PRECS[1:]:
        c = dict(prec=prec, pair=PAIRS[4], epi=0, M=64, N=300, K=100, batch=1, alpha=1.0, bias=False, unaligned=False, seed=7999)
        c["refused"] = refusal(prec, PAIRS[4], 64, 300, 1)
        out.append(("%s-a1b3-M64-refused" % prec, c))
    return out


# library split-K (SfGemm.split_ws): (M, N, K, batch) with sf_gemm_split_ws_floats > 0 -- a 300-pixel output over K = 1024 and
# the Twins encoder's sr convolutions (K = 8192, 16 splits)
AUTO_SPLIT_SHAPES = [(128, 300, 1024, 1), (64, 196, 8192, 1), (256, 196, 8192, 1)]
# caller split-K (SfGemm.k_splits) + sf_splitk_combine: (k_splits, pair, M, N, K, n_img); K = 323 has 11 k-tiles of 32, so 16
# splits leave five slices empty; the last case has more than 2^20 floats per image (the combine grid strides its loop)
CALLER_SPLIT_CASES = [(2, PAIRS[1], 64, 300, 323, 2), (3, PAIRS[4], 128, 300, 1000, 2), (4, PAIRS[1], 33, 132, 1000, 3),
                      (16, PAIRS[4], 128, 200, 323, 2), (16, PAIRS[1], 128, 64, 1000, 2), (3, PAIRS[1], 128, 300, 1000, 2),
                      (4, PAIRS[4], 128, 1000, 323, 2), (2, PAIRS[4], 128, 8200, 323, 2)]
