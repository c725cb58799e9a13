// Shared host/device helpers for libstreamflow_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/streamflow_hip.h"

namespace sf {

// thread-local error string (sf_last_error)
char* err_buf();
int fail(int code, const char* fmt, ...);

// sf_gemm_route: while this thread-local pointer is set (by sf_gemm_route, around the ordinary sf_gemm call) every launch site of
// the GEMM dispatch reports which kernel it is there and returns SF_OK instead of launching.  One copy of the rules: the probe sits
// where the launches are.  (defined in gemm.hip)
SfGemmRoute*& gemm_route_probe();
inline int gemm_route_report(int family, int tile_rows, int products, int nks = 0, int res = 0, int msplit = 0, int n_main = 0) {
    SfGemmRoute& r = *gemm_route_probe();
    r.family = family; r.tile_rows = tile_rows; r.products = products;
    r.nks = nks; r.res = res; r.msplit = msplit; r.n_main = n_main;
    return SF_OK;
}

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SF_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return SF_OK;
}

// Clearing on the stream with a KERNEL, for every word an entry point must reset per call.  hipMemsetAsync is not used for that:
// captured into a graph it becomes a memset node, and on the ROCm 7.0 runtime a memset node clears its bytes on the first replay
// only -- later replays leave a part of them as they were (tests/test_gpu_media_state.py: sf_frame_interp's accumulators, the
// status words and the split tables of sf_jpeg_decode(_split) kept the previous replay's contents).  A kernel node replays as it
// was captured.  `rows` runs of `bytes` bytes, `pitch_bytes` apart, each byte = `byte`; p, bytes and pitch_bytes multiples of 4.
static __global__ __launch_bounds__(256) void fill_words_kernel(uint32_t* p, int64_t pitch_words, int64_t width_words, int64_t rows,
                                                                uint32_t v) {
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
        uint32_t* row = p + r * pitch_words;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < width_words; i += (int64_t)gridDim.x * 256) row[i] = v;
    }
}
inline int fill_async(const char* what, void* p, int byte, int64_t bytes, hipStream_t s, int64_t rows = 1, int64_t pitch_bytes = 0) {
    if (bytes <= 0 || rows <= 0) return SF_OK;
    if (((uintptr_t)p & 3) || (bytes & 3) || (pitch_bytes & 3)) return fail(SF_ERR_BAD_ARG, "%s: a clear that is no run of 32-bit words", what);
    const int64_t words = bytes / 4;
    const int64_t blocks = (words + 255) / 256;
    const unsigned gx = blocks > 4096 ? 4096u : (unsigned)blocks;
    const unsigned gy = rows > 65535 ? 65535u : (unsigned)rows;
    const uint32_t v = 0x01010101u * (uint32_t)(byte & 255);
    hipLaunchKernelGGL(fill_words_kernel, dim3(gx, gy), dim3(256), 0, s, static_cast<uint32_t*>(p), pitch_bytes / 4, words, rows, v);
    return check_launch(what);
}

// erf(x) in fp32 as x*P(x^2)/Q(x^2) on [-4,4] (the rational minimax fit used by Eigen/XLA's float erf):
// branch-free, 12 FMAs + one reciprocal; |error| <= 4.5e-7 absolute, the same class as libm erff's fp32
// rounding.  ocml's erff has two data-dependent branches (both taken in a wave of mixed magnitudes) and made
// the GELU epilogues VALU-bound.
__device__ __forceinline__ float erf_fast(float x) {
    x = fminf(fmaxf(x, -4.0f), 4.0f);
    const float x2 = x * x;
    float p = -2.72614225801306e-10f;
    p = fmaf(p, x2, 2.77068142495902e-08f);
    p = fmaf(p, x2, -2.10102402082508e-06f);
    p = fmaf(p, x2, -5.69250639462346e-05f);
    p = fmaf(p, x2, -7.34990630326855e-04f);
    p = fmaf(p, x2, -2.95459980854025e-03f);
    p = fmaf(p, x2, -1.60960333262415e-02f);
    float q = -1.45660718464996e-05f;
    q = fmaf(q, x2, -2.13374055278905e-04f);
    q = fmaf(q, x2, -1.68282697438203e-03f);
    q = fmaf(q, x2, -7.37332916720468e-03f);
    q = fmaf(q, x2, -1.42647390514189e-02f);
    return (x * p) * __builtin_amdgcn_rcpf(q);
}

// exact (erf-based) GELU, as F.gelu / nn.GELU default: 0.5 x (1 + erf(x / sqrt(2)))
// (x / 2 is clamped below where the erf argument saturates: 1 + erf_fast(-4) is 0 only to the fit's 4.5e-7, which times an
// unbounded |x| / 2 would be an error growing with |x|; clamped it stays <= 1.3e-6 for every x <= 4.  For larger x the fit's
// error and the fp32 roundings of the two products are relative: 3e-7 x, restated and measured in tests/test_dwconv_cases_cpu.py)
__device__ __forceinline__ float gelu_erf(float x) {
    return 0.5f * fmaxf(x, -5.6568542f) * (1.0f + erf_fast(x * 0.70710678118654752440f));
}

// a * b rounded ONCE to fp32, opaque to the optimiser.  hipcc folds "x = a * b; h = (half)x" into v_fma_mixlo_f16 (h =
// RN16 of the EXACT product) while "x - (float)h" elsewhere uses RN16(RN32(a b)): two roundings of one value that differ
// when RN32(a b) sits on an fp16 tie.  Once in ~2^13 values the hi that is multiplied is then not the hi that lo was
// computed against and a hi + lo split is off by a whole fp16 ulp (measured: csrc/encoder.hip's three-product attention,
// 4.7e-5 on two queries in 1560 instead of 4e-7; `#pragma clang fp contract(off)` does not stop the fold).
__device__ __forceinline__ float mul_rn(float a, float b) {
    float r = a * b;
    asm volatile("" : "+v"(r));
    return r;
}

// Two GELUs at a time on packed fp32 (v_pk_fma_f32 / v_pk_mul_f32): the same operations in the same order as
// gelu_erf, i.e. bit-identical results at half the VALU issue slots.  The GEMM epilogues are VALU-bound on small-K
// shapes (M384 K256: 186 us with the GELU epilogue vs 141 us without), and a lane holds its outputs in pairs anyway.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 splat2(float a) { f32x2 v; v[0] = a; v[1] = a; return v; }
__device__ __forceinline__ f32x2 erf_fast2(f32x2 x) {
    x = __builtin_elementwise_min(__builtin_elementwise_max(x, splat2(-4.0f)), splat2(4.0f));
    const f32x2 x2 = x * x;
    f32x2 p = splat2(-2.72614225801306e-10f);
    p = __builtin_elementwise_fma(p, x2, splat2(2.77068142495902e-08f));
    p = __builtin_elementwise_fma(p, x2, splat2(-2.10102402082508e-06f));
    p = __builtin_elementwise_fma(p, x2, splat2(-5.69250639462346e-05f));
    p = __builtin_elementwise_fma(p, x2, splat2(-7.34990630326855e-04f));
    p = __builtin_elementwise_fma(p, x2, splat2(-2.95459980854025e-03f));
    p = __builtin_elementwise_fma(p, x2, splat2(-1.60960333262415e-02f));
    f32x2 q = splat2(-1.45660718464996e-05f);
    q = __builtin_elementwise_fma(q, x2, splat2(-2.13374055278905e-04f));
    q = __builtin_elementwise_fma(q, x2, splat2(-1.68282697438203e-03f));
    q = __builtin_elementwise_fma(q, x2, splat2(-7.37332916720468e-03f));
    q = __builtin_elementwise_fma(q, x2, splat2(-1.42647390514189e-02f));
    f32x2 r;
    r[0] = __builtin_amdgcn_rcpf(q[0]);
    r[1] = __builtin_amdgcn_rcpf(q[1]);
    return (x * p) * r;
}
__device__ __forceinline__ f32x2 gelu_erf2(f32x2 x) {
    return splat2(0.5f) * __builtin_elementwise_max(x, splat2(-5.6568542f)) * (splat2(1.0f) + erf_fast2(x * splat2(0.70710678118654752440f)));
}

// GELU for results that leave as fp16 in the f16x2 / f16 arithmetic (kFast below: the k-octet GEMM epilogue, the fp16-row
// output of the depthwise kernel): a pure polynomial -- erf(z) ~ z Q(z^2) on |z| <= 3 (degree-8 minimax
// Q, |err| <= 2.2e-5, erf(3) = 1 - 2.2e-5 beyond), constants folded so that gelu(x) = h + h * (xc * D(xc^2)), h = x / 2,
// xc = x clamped to +-3 sqrt 2: 14 issue slots per PAIR (2 v_med3, 10 v_pk_fma / v_pk_mul, no v_rcp) against 28 for the
// rational form above.  |gelu error| <= 5.2e-5 absolute for every x <= 8 (h is clamped below at -3/sqrt 2, so that the residue of
// erf(3) != 1 stays 4.7e-5 for negative x instead of growing like 1.1e-5 |x|: ADVICE r2).  Beyond the clamp of xc the error is that
// residue times x / 2 and DOES grow: 6.6e-6 x, above 5.2e-5 from x = 8 on.  Relative to gelu(x) it is <= 1.35e-5 for x > 0 (1.2e-5
// of x) -- a fortieth of the fp16 rounding (2^-11 relative) that every activation of these modes receives on its way into the next
// contraction.  (Restated in float64 and in fp32 and measured on a grid over [-12, 12]: tests/test_dwconv_cases_cpu.py.)
__device__ __forceinline__ f32x2 gelu_poly2(f32x2 x) {
    f32x2 xc;
    xc[0] = __builtin_amdgcn_fmed3f(x[0], -4.2426405f, 4.2426405f);
    xc[1] = __builtin_amdgcn_fmed3f(x[1], -4.2426405f, 4.2426405f);
    const f32x2 t = xc * xc;
    f32x2 p = splat2(1.12535e-10f);
    p = __builtin_elementwise_fma(p, t, splat2(-1.074371e-08f));
    p = __builtin_elementwise_fma(p, t, splat2(4.5365834e-07f));
    p = __builtin_elementwise_fma(p, t, splat2(-1.12924145e-05f));
    p = __builtin_elementwise_fma(p, t, splat2(0.0001871811f));
    p = __builtin_elementwise_fma(p, t, splat2(-0.0022188f));
    p = __builtin_elementwise_fma(p, t, splat2(0.019636236f));
    p = __builtin_elementwise_fma(p, t, splat2(-0.13269384f));
    p = __builtin_elementwise_fma(p, t, splat2(0.79780626f));
    const f32x2 h = splat2(0.5f) * __builtin_elementwise_max(x, splat2(-4.2426405f));
    return __builtin_elementwise_fma(h, xc * p, h);
}
// gelu_poly2 of NP pairs at a time with the Horner chains INTERLEAVED (coefficient loop outside, pair loop inside).  Evaluated
// pair by pair an epilogue is bound by the latency of one dependent chain -- 14 packed instructions at ~11 cycles each, 160
// cycles per pair measured with the phase timers of csrc/gemm_bstat.hip, 2550 of an m-step's 3670 epilogue cycles -- because
// hipcc keeps the pairs apart to save registers; four chains in flight hide each other's latency.  Same operations per value
// as gelu_poly2 (bit-identical results).
template <int NP>
__device__ __forceinline__ void gelu_poly_n(f32x2 (&x)[NP]) {
    f32x2 xc[NP], t[NP], p[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        xc[i][0] = __builtin_amdgcn_fmed3f(x[i][0], -4.2426405f, 4.2426405f);
        xc[i][1] = __builtin_amdgcn_fmed3f(x[i][1], -4.2426405f, 4.2426405f);
        t[i] = xc[i] * xc[i];
        p[i] = splat2(1.12535e-10f);
    }
    constexpr float c[8] = {-1.074371e-08f, 4.5365834e-07f, -1.12924145e-05f, 0.0001871811f, -0.0022188f, 0.019636236f,
                            -0.13269384f, 0.79780626f};
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int i = 0; i < NP; ++i) p[i] = __builtin_elementwise_fma(p[i], t[i], splat2(c[k]));
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const f32x2 h = splat2(0.5f) * __builtin_elementwise_max(x[i], splat2(-4.2426405f));
        x[i] = __builtin_elementwise_fma(h, xc[i] * p[i], h);
    }
}
template <bool kFast>
__device__ __forceinline__ f32x2 gelu2(f32x2 x) {
    if constexpr (kFast) return gelu_poly2(x);
    else return gelu_erf2(x);
}

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// MI355X dispatches workgroup b of a 1-D grid to XCD b % 8 (8 XCDs with private 4 MiB L2s; observed, used for speed
// only).  Returns a work-item id such that every XCD walks ONE CONTIGUOUS range of ids (bijective for any grid size),
// so that consecutive ids -- which the caller orders to share operand tiles -- meet in the same L2.
__device__ __forceinline__ int xcd_linear_id(int b, int nwg) {
    constexpr int kXcd = 8;
    const int xcd = b % kXcd, local = b / kXcd;
    const int q = nwg / kXcd, r = nwg % kXcd;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
}

}  // namespace sf

#define SF_REQUIRE(cond, ...)                                         \
    do {                                                              \
        if (!(cond)) return sf::fail(SF_ERR_BAD_ARG, __VA_ARGS__);    \
    } while (0)
