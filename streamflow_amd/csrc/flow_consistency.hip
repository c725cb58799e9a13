// Forward-backward consistency of flow fields and backward warping of frames, a batch of fields per call (the check of Sundaram et
// al. 2010 as UnFlow, Meister et al. 2018, states it; include/streamflow_hip.h, "forward-backward consistency", has the contract).
//
// sf_flow_consistency: for every pixel of field i the backward field is sampled bilinearly where the forward flow points; the pixel
// is VISIBLE when |fwd + bwd(sampled)|^2 <= alpha (|fwd|^2 + |bwd|^2) + beta, OCCLUDED when it is not (a NaN tap included), OUTSIDE
// when the target leaves the frame.  Output: a class byte per pixel (the three byte values are arguments) and, ADDED into one row
// of fp64 per field, the counts and two sums.  sf_warp_frames: the same coordinates, taps of a uint8 RGB frame, rounded bytes out;
// with a class map and reference frames also the photometric error over visible pixels.
//
// Both main kernels: grid (blocks per field, n), grid-stride over the field, four pixels per thread.  The two map pixels to lanes
// differently, each as it measured faster (tools/flow_consistency_bench.py):
// * flow_consistency_kernel: a wave owns 256 consecutive pixels of a row, lane l the pixels l, l + 64, l + 128, l + 192 of them.
//   Every wave instruction -- the loads of the forward planes, the class stores and, for smooth flows, the taps of the backward
//   field -- then covers consecutive addresses.  (Four CONSECUTIVE pixels per thread with float4 loads and one word of class bytes
//   was 1.6x slower: the lanes of a tap load are then 16 bytes apart and fetch four times the lines they use.)
// * warp_frames_kernel: a thread owns four consecutive pixels: float4 loads of the two flow planes where pointers and strides allow,
//   the twelve warped bytes as three 4-byte stores where w % 4 == 0, element accesses otherwise.  Its taps are bytes three apart;
//   the lane-consecutive mapping was 5-8 % slower here.
// The taps are a gather: element loads at data-dependent addresses that neighbouring pixels mostly share, served by L2.  The
// inside test is made on the float coordinates BEFORE any conversion to an integer: NaN, +-Inf and huge flows compare false and
// never form an address.
// No LDS beyond the block reduction, no atomics: per-block partial rows go to the caller's workspace and a second kernel (one block
// per field) sums them in a fixed order.  The grid depends on (n, h, w) alone, so repeated calls give bitwise equal rows.
//
// Arithmetic: fp32, every operation rounded on its own (FMA contraction is off for this file; hipcc's fp32 square root is correctly
// rounded), in the order the header states, so a numpy float32 restatement reproduces classes and bytes bit for bit.
#include "sf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kCallBlocks = 2048;                                        // blocks one call aims at (8 per CU), shared by its fields

// the block's totals in thread 0, in a fixed order: a shuffle tree inside every wave, then the waves in order
template <int kLen>
__device__ __forceinline__ void block_sum(double (&r)[kLen], double (*s)[kLen]) {
#pragma unroll
    for (int k = 0; k < kLen; ++k)
        for (int off = 32; off > 0; off >>= 1) r[k] += __shfl_xor(r[k], off, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < kLen; ++k) s[threadIdx.x >> 6][k] = r[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < kLen; ++k) {
            double a = s[0][k];
            for (int wv = 1; wv < kBlock / 64; ++wv) a += s[wv][k];
            r[k] = a;
        }
}

template <int kLen>
__global__ __launch_bounds__(kBlock) void fbc_finish_kernel(const double* __restrict__ partials, int nblocks, double* __restrict__ stats) {
    __shared__ double s[kBlock / 64][kLen];
    const int field = blockIdx.x;
    const double* p = partials + (int64_t)field * nblocks * kLen;
    double r[kLen];
#pragma unroll
    for (int k = 0; k < kLen; ++k) r[k] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kBlock)
#pragma unroll
        for (int k = 0; k < kLen; ++k) r[k] += p[(int64_t)b * kLen + k];
    block_sum<kLen>(r, s);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < kLen; ++k) stats[(int64_t)field * kLen + k] += r[k];
}

// where pixel (y, x) lands: the inside test on the float coordinates, then (only inside) the four tap positions and weights
struct Target {
    bool inside;
    int x0, x1, y0, y1;
    float fx, fy;
};

__device__ __forceinline__ Target target(int x, int y, float u, float v, int h, int w) {
    Target t;
    const float px = (float)x + u, py = (float)y + v;
    t.inside = px >= 0.0f && px <= (float)(w - 1) && py >= 0.0f && py <= (float)(h - 1);              // false for NaN
    t.x0 = t.x1 = t.y0 = t.y1 = 0;
    t.fx = t.fy = 0.0f;
    if (t.inside) {
        const float fx0 = floorf(px), fy0 = floorf(py);
        t.fx = px - fx0, t.fy = py - fy0;
        t.x0 = (int)fx0, t.y0 = (int)fy0;                                // 0 <= x0 <= w - 1, 0 <= y0 <= h - 1
        t.x1 = t.x0 + 1 < w - 1 ? t.x0 + 1 : w - 1;
        t.y1 = t.y0 + 1 < h - 1 ? t.y0 + 1 : h - 1;
    }
    return t;
}

__device__ __forceinline__ float blend(const Target& t, float a00, float a01, float a10, float a11) {
    const float gx = 1.0f - t.fx, gy = 1.0f - t.fy;
    const float top = gx * a00 + t.fx * a01;
    const float bot = gx * a10 + t.fx * a11;
    return gy * top + t.fy * bot;
}

__device__ __forceinline__ void load4(const float* p, bool vec, int left, float (&r)[4]) {
    if (vec && left == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        r[0] = q.x, r[1] = q.y, r[2] = q.z, r[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = j < left ? p[j] : 0.0f;
    }
}

struct FbcArgs {
    const float* fwd;
    const float* bwd;
    int64_t f_field, f_ch, f_row, b_field, b_ch, b_row;
    int h, w;
    float alpha, beta;
    unsigned code_vis, code_occ, code_out;
};

// units a row takes in flow_consistency_kernel: a unit is 256 consecutive pixels, the work of one wave at a time
__host__ __device__ inline int fbc_units_per_row(int w) { return (w + 255) >> 8; }

__global__ __launch_bounds__(kBlock) void flow_consistency_kernel(FbcArgs a, uint8_t* __restrict__ cls, double* __restrict__ partials) {
    __shared__ double s[kBlock / 64][SF_FBC_LEN];
    const int field = blockIdx.y;
    const int h = a.h, w = a.w;
    const float* __restrict__ fu = a.fwd + (int64_t)field * a.f_field;
    const float* __restrict__ bu = a.bwd + (int64_t)field * a.b_field;
    const float* __restrict__ bv = bu + a.b_ch;
    uint8_t* __restrict__ out = cls + (int64_t)field * h * w;
    unsigned n_px = 0, n_vis = 0, n_occ = 0, n_out = 0, n_fin = 0;       // (a thread sees fewer than 2^30 pixels)
    double sum_fb = 0.0, sum_mag = 0.0;
    const int nb = fbc_units_per_row(w);
    const int nunits = h * nb;                                           // < 2^30 / 256 + h: fits an int
    for (int unit = blockIdx.x * kWaves + (threadIdx.x >> 6); unit < nunits; unit += gridDim.x * kWaves) {
        // a wave owns a unit of 256 consecutive pixels of one row, lane l the pixels x0 + 64 j: every load, tap and store of a wave
        // instruction goes to consecutive (or, for the taps, nearly consecutive) addresses
        const int y = unit / nb, x0 = (unit - y * nb) * 256 + (threadIdx.x & 63);
        const float* pu = fu + (int64_t)y * a.f_row;
        float u[4], v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + 64 * j;
            u[j] = x < w ? pu[x] : 0.0f;
            v[j] = x < w ? pu[a.f_ch + x] : 0.0f;
        }
        uint8_t* o = out + (int64_t)y * w;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + 64 * j;
            if (x >= w) continue;
            const float uu = u[j], vv = v[j];
            const Target t = target(x, y, uu, vv, h, w);
            const float m2 = uu * uu + vv * vv;
            bool vis = false;
            if (t.inside) {
                const int64_t r0 = (int64_t)t.y0 * a.b_row, r1 = (int64_t)t.y1 * a.b_row;
                const float su = blend(t, bu[r0 + t.x0], bu[r0 + t.x1], bu[r1 + t.x0], bu[r1 + t.x1]);
                const float sv = blend(t, bv[r0 + t.x0], bv[r0 + t.x1], bv[r1 + t.x0], bv[r1 + t.x1]);
                const float dx = uu + su, dy = vv + sv;
                const float lhs = dx * dx + dy * dy;
                const float rhs = a.alpha * (m2 + (su * su + sv * sv)) + a.beta;
                vis = lhs <= rhs;                                        // false for NaN: occluded
                if (vis) sum_fb += (double)sqrtf(lhs);
            }
            const float mag = sqrtf(m2);
            if (mag < __builtin_inff()) {                                // false for NaN and for an overflowed square
                n_fin += 1u;
                sum_mag += (double)mag;
            }
            n_px += 1u;
            n_vis += vis ? 1u : 0u;
            n_occ += (t.inside && !vis) ? 1u : 0u;
            n_out += t.inside ? 0u : 1u;
            o[x] = (uint8_t)(t.inside ? (vis ? a.code_vis : a.code_occ) : a.code_out);
        }
    }
    double r[SF_FBC_LEN];
    r[SF_FBC_PIXELS] = (double)n_px, r[SF_FBC_VISIBLE] = (double)n_vis, r[SF_FBC_OCCLUDED] = (double)n_occ;
    r[SF_FBC_OUTSIDE] = (double)n_out, r[SF_FBC_SUM_FB] = sum_fb, r[SF_FBC_SUM_MAG] = sum_mag, r[SF_FBC_FINITE] = (double)n_fin;
    block_sum<SF_FBC_LEN>(r, s);
    if (threadIdx.x == 0) {
        double* p = partials + ((int64_t)field * gridDim.x + blockIdx.x) * SF_FBC_LEN;
#pragma unroll
        for (int k = 0; k < SF_FBC_LEN; ++k) p[k] = r[k];
    }
}

struct WarpArgs {
    const uint8_t* src;
    const uint8_t* ref;
    const uint8_t* cls;
    const float* flow;
    int64_t s_frame, s_row, s_px, s_ch, r_frame, r_row, r_px, r_ch, f_field, f_ch, f_row;
    int h, w;
    unsigned code_vis;
    int vec_load, vec_store;
};

template <bool kStats>
__global__ __launch_bounds__(kBlock) void warp_frames_kernel(WarpArgs a, uint8_t* __restrict__ out, double* __restrict__ partials) {
    __shared__ double s[kBlock / 64][SF_WARP_LEN];
    const int field = blockIdx.y;
    const int h = a.h, w = a.w;
    const float* __restrict__ fu = a.flow + (int64_t)field * a.f_field;
    const uint8_t* __restrict__ src = a.src + (int64_t)field * a.s_frame;
    const uint8_t* __restrict__ ref = kStats ? a.ref + (int64_t)field * a.r_frame : nullptr;
    const uint8_t* __restrict__ cls = kStats ? a.cls + (int64_t)field * h * w : nullptr;
    uint8_t* __restrict__ dst = out + (int64_t)field * h * w * 3;
    double sum_abs = 0.0;
    unsigned terms = 0;                                                  // (at most 3 * 2^22 per thread)
    const int gw = (w + 3) >> 2;
    const int ngroups = h * gw;
    for (int q = blockIdx.x * kBlock + threadIdx.x; q < ngroups; q += gridDim.x * kBlock) {
        const int y = q / gw, x0 = (q - y * gw) << 2;
        const int left = w - x0 < 4 ? w - x0 : 4;
        const float* pu = fu + (int64_t)y * a.f_row + x0;
        float u[4], v[4];
        load4(pu, a.vec_load, left, u);
        load4(pu + a.f_ch, a.vec_load, left, v);
        unsigned byte[12];                                               // [pixel][channel], as they lie in the output
#pragma unroll
        for (int k = 0; k < 12; ++k) byte[k] = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= left) continue;
            const Target t = target(x0 + j, y, u[j], v[j], h, w);
            if (!t.inside) continue;
            const uint8_t* p00 = src + (int64_t)t.y0 * a.s_row + (int64_t)t.x0 * a.s_px;
            const uint8_t* p01 = src + (int64_t)t.y0 * a.s_row + (int64_t)t.x1 * a.s_px;
            const uint8_t* p10 = src + (int64_t)t.y1 * a.s_row + (int64_t)t.x0 * a.s_px;
            const uint8_t* p11 = src + (int64_t)t.y1 * a.s_row + (int64_t)t.x1 * a.s_px;
            bool vis = false;
            const uint8_t* pr = nullptr;
            if (kStats) {
                vis = cls[(int64_t)y * w + x0 + j] == a.code_vis;
                pr = ref + (int64_t)y * a.r_row + (int64_t)(x0 + j) * a.r_px;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int64_t co = (int64_t)c * a.s_ch;
                const float val = blend(t, (float)p00[co], (float)p01[co], (float)p10[co], (float)p11[co]);
                byte[3 * j + c] = (unsigned)floorf(val + 0.5f);          // 0 <= val <= 255
                if (kStats && vis) {
                    sum_abs += (double)fabsf(val - (float)pr[(int64_t)c * a.r_ch]);
                    terms += 1u;
                }
            }
        }
        uint8_t* o = dst + ((int64_t)y * w + x0) * 3;
        if (a.vec_store && left == 4) {
            unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                o4[k] = byte[4 * k] | (byte[4 * k + 1] << 8) | (byte[4 * k + 2] << 16) | (byte[4 * k + 3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k)
                if (k < 3 * left) o[k] = (uint8_t)byte[k];
        }
    }
    if (kStats) {
        double r[SF_WARP_LEN];
        r[SF_WARP_SUM_ABS] = sum_abs, r[SF_WARP_TERMS] = (double)terms;
        block_sum<SF_WARP_LEN>(r, s);
        if (threadIdx.x == 0) {
            double* p = partials + ((int64_t)field * gridDim.x + blockIdx.x) * SF_WARP_LEN;
#pragma unroll
            for (int k = 0; k < SF_WARP_LEN; ++k) p[k] = r[k];
        }
    }
}

bool shape_ok(int n, int h, int w) { return n >= 1 && n <= 65535 && h > 0 && w > 0 && (int64_t)h * w < (1 << 30); }

// blocks per field: `want` (enough for four pixels per thread), at most the field's share of kCallBlocks (at least one)
int blocks_per_field(int n, int want) {
    const int cap = kCallBlocks / n > 1 ? kCallBlocks / n : 1;
    return want < cap ? want : cap;
}
int fbc_blocks(int n, int h, int w) { return blocks_per_field(n, sf::ceil_div(h * fbc_units_per_row(w), kWaves)); }
int warp_blocks(int n, int h, int w) { return blocks_per_field(n, sf::ceil_div(h * ((w + 3) / 4), kBlock)); }

bool flow_vec(const float* p, int64_t field, int64_t ch, int64_t row) {
    return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && field % 4 == 0 && ch % 4 == 0 && row % 4 == 0;
}

}  // namespace

extern "C" int64_t sf_flow_consistency_ws_bytes(int n, int h, int w) {
    if (!shape_ok(n, h, w)) return sf::fail(SF_ERR_BAD_ARG, "sf_flow_consistency_ws_bytes: bad shape (%d fields of %d x %d)", n, h, w);
    return (int64_t)n * fbc_blocks(n, h, w) * SF_FBC_LEN * (int64_t)sizeof(double);
}

extern "C" int64_t sf_warp_frames_ws_bytes(int n, int h, int w) {
    if (!shape_ok(n, h, w)) return sf::fail(SF_ERR_BAD_ARG, "sf_warp_frames_ws_bytes: bad shape (%d frames of %d x %d)", n, h, w);
    return (int64_t)n * warp_blocks(n, h, w) * SF_WARP_LEN * (int64_t)sizeof(double);
}

extern "C" int sf_flow_consistency(const float* fwd, int64_t fwd_field_stride, int64_t fwd_ch_stride, int64_t fwd_row_stride,
                                   const float* bwd, int64_t bwd_field_stride, int64_t bwd_ch_stride, int64_t bwd_row_stride, int n,
                                   int h, int w, float alpha, float beta, uint8_t code_visible, uint8_t code_occluded,
                                   uint8_t code_outside, uint8_t* cls, double* stats, void* ws, int64_t ws_bytes, void* stream) {
    SF_REQUIRE(fwd && bwd && cls && stats && ws, "sf_flow_consistency: null argument");
    SF_REQUIRE(h > 0 && w > 0, "sf_flow_consistency: bad shape %d x %d", h, w);
    SF_REQUIRE((int64_t)h * w < (1 << 30), "sf_flow_consistency: field %d x %d too large", h, w);
    SF_REQUIRE(n >= 1 && n <= 65535, "sf_flow_consistency: %d fields in one call (1 .. 65535)", n);
    SF_REQUIRE(fwd_row_stride >= w && bwd_row_stride >= w, "sf_flow_consistency: a row stride (%lld, %lld) below w = %d",
               (long long)fwd_row_stride, (long long)bwd_row_stride, w);
    SF_REQUIRE(fwd_ch_stride != 0 && bwd_ch_stride != 0 && fwd_field_stride >= 0 && bwd_field_stride >= 0,
               "sf_flow_consistency: bad channel / field strides (%lld, %lld, %lld, %lld)", (long long)fwd_ch_stride,
               (long long)bwd_ch_stride, (long long)fwd_field_stride, (long long)bwd_field_stride);
    SF_REQUIRE(!(alpha != alpha) && !(beta != beta), "sf_flow_consistency: alpha / beta is NaN");
    const int64_t need = sf_flow_consistency_ws_bytes(n, h, w);
    SF_REQUIRE(ws_bytes >= need, "sf_flow_consistency: workspace of %lld bytes (needs %lld)", (long long)ws_bytes, (long long)need);
    SF_REQUIRE((reinterpret_cast<uintptr_t>(fwd) & 3u) == 0 && (reinterpret_cast<uintptr_t>(bwd) & 3u) == 0,
               "sf_flow_consistency: fwd / bwd not 4-byte aligned");
    SF_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7u) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0,
               "sf_flow_consistency: stats / ws not 8-byte aligned");
    FbcArgs a;
    a.fwd = fwd, a.bwd = bwd;
    a.f_field = fwd_field_stride, a.f_ch = fwd_ch_stride, a.f_row = fwd_row_stride;
    a.b_field = bwd_field_stride, a.b_ch = bwd_ch_stride, a.b_row = bwd_row_stride;
    a.h = h, a.w = w, a.alpha = alpha, a.beta = beta;
    a.code_vis = code_visible, a.code_occ = code_occluded, a.code_out = code_outside;
    const int nblocks = fbc_blocks(n, h, w);
    hipStream_t s = (hipStream_t)stream;
    double* partials = static_cast<double*>(ws);
    hipLaunchKernelGGL(flow_consistency_kernel, dim3(nblocks, n), dim3(kBlock), 0, s, a, cls, partials);
    const int st = sf::check_launch("sf_flow_consistency");
    if (st != SF_OK) return st;
    hipLaunchKernelGGL(fbc_finish_kernel<SF_FBC_LEN>, dim3(n), dim3(kBlock), 0, s, partials, nblocks, stats);
    return sf::check_launch("sf_flow_consistency (finish)");
}

extern "C" int sf_warp_frames(const uint8_t* src, int64_t src_frame_stride, int64_t src_row_stride, int64_t src_px_stride,
                              int64_t src_ch_stride, const float* flows, int64_t flow_field_stride, int64_t flow_ch_stride,
                              int64_t flow_row_stride, int n, int h, int w, uint8_t* out, const uint8_t* cls, uint8_t code_visible,
                              const uint8_t* ref, int64_t ref_frame_stride, int64_t ref_row_stride, int64_t ref_px_stride,
                              int64_t ref_ch_stride, double* stats, void* ws, int64_t ws_bytes, void* stream) {
    SF_REQUIRE(src && flows && out, "sf_warp_frames: null argument");
    SF_REQUIRE(h > 0 && w > 0, "sf_warp_frames: bad shape %d x %d", h, w);
    SF_REQUIRE((int64_t)h * w < (1 << 30), "sf_warp_frames: frame %d x %d too large", h, w);
    SF_REQUIRE(n >= 1 && n <= 65535, "sf_warp_frames: %d frames in one call (1 .. 65535)", n);
    SF_REQUIRE(flow_row_stride >= w && flow_ch_stride != 0 && flow_field_stride >= 0, "sf_warp_frames: bad flow strides (%lld, %lld, %lld)",
               (long long)flow_field_stride, (long long)flow_ch_stride, (long long)flow_row_stride);
    SF_REQUIRE(src_frame_stride >= 0 && src_row_stride >= 0 && src_px_stride >= 0 && src_ch_stride >= 0,
               "sf_warp_frames: negative source stride (%lld, %lld, %lld, %lld)", (long long)src_frame_stride, (long long)src_row_stride,
               (long long)src_px_stride, (long long)src_ch_stride);
    SF_REQUIRE((reinterpret_cast<uintptr_t>(flows) & 3u) == 0, "sf_warp_frames: flows not 4-byte aligned");
    const bool want_stats = cls != nullptr || ref != nullptr;
    if (want_stats) {
        SF_REQUIRE(cls && ref, "sf_warp_frames: the class map and the reference frames come together (one of them is null)");
        SF_REQUIRE(stats && ws, "sf_warp_frames: stats / ws is null with a class map and reference frames");
        SF_REQUIRE(ref_frame_stride >= 0 && ref_row_stride >= 0 && ref_px_stride >= 0 && ref_ch_stride >= 0,
                   "sf_warp_frames: negative reference stride (%lld, %lld, %lld, %lld)", (long long)ref_frame_stride,
                   (long long)ref_row_stride, (long long)ref_px_stride, (long long)ref_ch_stride);
        const int64_t need = sf_warp_frames_ws_bytes(n, h, w);
        SF_REQUIRE(ws_bytes >= need, "sf_warp_frames: workspace of %lld bytes (needs %lld)", (long long)ws_bytes, (long long)need);
        SF_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7u) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0,
                   "sf_warp_frames: stats / ws not 8-byte aligned");
    }
    WarpArgs a;
    a.src = src, a.ref = ref, a.cls = cls, a.flow = flows;
    a.s_frame = src_frame_stride, a.s_row = src_row_stride, a.s_px = src_px_stride, a.s_ch = src_ch_stride;
    a.r_frame = ref_frame_stride, a.r_row = ref_row_stride, a.r_px = ref_px_stride, a.r_ch = ref_ch_stride;
    a.f_field = flow_field_stride, a.f_ch = flow_ch_stride, a.f_row = flow_row_stride;
    a.h = h, a.w = w, a.code_vis = code_visible;
    a.vec_load = flow_vec(flows, flow_field_stride, flow_ch_stride, flow_row_stride);
    // a group's twelve bytes start at 3 (y w + x0): whole words when w is a multiple of four and the dense output is word-aligned
    a.vec_store = w % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
    const int nblocks = warp_blocks(n, h, w);
    hipStream_t s = (hipStream_t)stream;
    double* partials = static_cast<double*>(ws);
    if (want_stats) hipLaunchKernelGGL(warp_frames_kernel<true>, dim3(nblocks, n), dim3(kBlock), 0, s, a, out, partials);
    else hipLaunchKernelGGL(warp_frames_kernel<false>, dim3(nblocks, n), dim3(kBlock), 0, s, a, out, partials);
    const int st = sf::check_launch("sf_warp_frames");
    if (st != SF_OK || !want_stats) return st;
    hipLaunchKernelGGL(fbc_finish_kernel<SF_WARP_LEN>, dim3(n), dim3(kBlock), 0, s, partials, nblocks, stats);
    return sf::check_launch("sf_warp_frames (finish)");
}
