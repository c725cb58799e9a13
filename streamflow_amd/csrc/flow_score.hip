// Spring scoring on the device (reference evaluate_mf.py:50-102 validate_spring_mf): one predicted field against one ground-truth
// field, ADDED into a fixed-length fp64 accumulator (layout: include/streamflow_hip.h, SF_SCORE_*).  The reference copies every flow
// to the host and keeps every per-pixel EPE array until the end of the split; here the flows stay where the model wrote them and the
// state of a whole report is SF_SCORE_LEN doubles.
//
// Two kernels, no atomics.  flow_score_kernel: every thread walks groups of four pixels of one row (grid-stride), float4 loads of
// the prediction where its planes, rows and pointer allow it (scalar loads otherwise, as flow_viz.hip does), float2 loads of the
// interleaved ground truth; per thread two fp64 sums and twelve counts, reduced inside the block in a fixed order (shuffle tree,
// then the four waves in order) and written as one row of per-block partials.  flow_score_finish_kernel: ONE block sums the
// partial rows in a fixed order and adds the totals to the accumulator.  The grid depends on (h, w) alone, so repeated calls give
// bitwise equal accumulators.
//
// Arithmetic: fp32, every operation rounded on its own (FMA contraction is off for this file, as in tile_blend.hip and
// flow_viz.hip; hipcc's fp32 square root is correctly rounded), the same expressions as the reference's torch code.
#include "sf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = SF_SCORE_WS_BYTES / (SF_SCORE_LEN * (int)sizeof(double));

struct Tally {
    double v[SF_SCORE_LEN];
};

__device__ __forceinline__ void score_px(float pu, float pv, float gu, float gv, Tally& t) {
    const float du = pu - gu, dv = pv - gv;
    const float e = sqrtf(du * du + dv * dv);
    const float gs = gu + gv;
    const bool valid = !(gs != gs);
    const float mag = sqrtf(gu * gu + gv * gv);
    const bool gt1 = e > 1.0f;
    t.v[SF_SCORE_PIXELS] += 1.0;
    t.v[SF_SCORE_SUM_EPE] += (double)e;
    t.v[SF_SCORE_LT1] += e < 1.0f ? 1.0 : 0.0;
    t.v[SF_SCORE_LT3] += e < 3.0f ? 1.0 : 0.0;
    t.v[SF_SCORE_LT5] += e < 5.0f ? 1.0 : 0.0;
    t.v[SF_SCORE_GT1] += gt1 ? 1.0 : 0.0;
    if (valid) {                                                         // (constant indices only: the tally stays in registers)
        const bool b0 = mag < 10.0f, b2 = mag >= 40.0f, b1 = !b0 && !b2;
        t.v[SF_SCORE_VALID] += 1.0;
        t.v[SF_SCORE_SUM_EPE_VALID] += (double)e;
        t.v[SF_SCORE_S0_10] += b0 ? 1.0 : 0.0;
        t.v[SF_SCORE_S0_10_GT1] += (b0 && gt1) ? 1.0 : 0.0;
        t.v[SF_SCORE_S10_40] += b1 ? 1.0 : 0.0;
        t.v[SF_SCORE_S10_40_GT1] += (b1 && gt1) ? 1.0 : 0.0;
        t.v[SF_SCORE_S40] += b2 ? 1.0 : 0.0;
        t.v[SF_SCORE_S40_GT1] += (b2 && gt1) ? 1.0 : 0.0;
    }
}

// the block's totals in thread 0, in a fixed order: a shuffle tree inside every wave, then the waves in order
__device__ __forceinline__ void block_sum(Tally& t, double (*s)[SF_SCORE_LEN]) {
#pragma unroll
    for (int k = 0; k < SF_SCORE_LEN; ++k)
        for (int off = 32; off > 0; off >>= 1) t.v[k] += __shfl_xor(t.v[k], off, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < SF_SCORE_LEN; ++k) s[threadIdx.x >> 6][k] = t.v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < SF_SCORE_LEN; ++k) {
            double a = s[0][k];
            for (int wv = 1; wv < kBlock / 64; ++wv) a += s[wv][k];
            t.v[k] = a;
        }
}

template <bool kVec>
__global__ __launch_bounds__(kBlock) void flow_score_kernel(const float* __restrict__ pred, int64_t ch_stride, int64_t row_stride,
                                                            const float* __restrict__ gt, int64_t gt_row_floats, int step, int h,
                                                            int w, bool gt_f2, double* __restrict__ partials) {
    __shared__ double s[kBlock / 64][SF_SCORE_LEN];
    Tally t;
#pragma unroll
    for (int k = 0; k < SF_SCORE_LEN; ++k) t.v[k] = 0.0;
    const int gw = (w + 3) >> 2;
    const int ngroups = h * gw;                                          // < 2^30 / 4 + h: fits an int
    for (int q = blockIdx.x * kBlock + threadIdx.x; q < ngroups; q += gridDim.x * kBlock) {
        const int y = q / gw, x0 = (q - y * gw) << 2;
        const float* pu = pred + (int64_t)y * row_stride + x0;
        const float* pv = pu + ch_stride;
        const float* g = gt + (int64_t)step * y * gt_row_floats + (int64_t)2 * step * x0;
        const int left = w - x0 < 4 ? w - x0 : 4;                        // pixels of this group that exist (>= 1)
        float u[4], v[4];
        if (kVec && left == 4) {
            const float4 u4 = *reinterpret_cast<const float4*>(pu), v4 = *reinterpret_cast<const float4*>(pv);
            u[0] = u4.x, u[1] = u4.y, u[2] = u4.z, u[3] = u4.w;
            v[0] = v4.x, v[1] = v4.y, v[2] = v4.z, v[3] = v4.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                u[j] = j < left ? pu[j] : 0.0f;
                v[j] = j < left ? pv[j] : 0.0f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= left) break;
            const float* gj = g + 2 * step * j;
            float gu, gv;
            if (gt_f2) {
                const float2 g2 = *reinterpret_cast<const float2*>(gj);
                gu = g2.x, gv = g2.y;
            } else {
                gu = gj[0], gv = gj[1];
            }
            score_px(u[j], v[j], gu, gv, t);
        }
    }
    block_sum(t, s);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < SF_SCORE_LEN; ++k) partials[(int64_t)blockIdx.x * SF_SCORE_LEN + k] = t.v[k];
}

__global__ __launch_bounds__(kBlock) void flow_score_finish_kernel(const double* __restrict__ partials, int nblocks,
                                                                   double* __restrict__ acc) {
    __shared__ double s[kBlock / 64][SF_SCORE_LEN];
    Tally t;
#pragma unroll
    for (int k = 0; k < SF_SCORE_LEN; ++k) t.v[k] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kBlock)
#pragma unroll
        for (int k = 0; k < SF_SCORE_LEN; ++k) t.v[k] += partials[(int64_t)b * SF_SCORE_LEN + k];
    block_sum(t, s);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < SF_SCORE_LEN; ++k) acc[k] += t.v[k];
}

}  // namespace

extern "C" int sf_flow_score(const float* pred, int64_t pred_ch_stride, int64_t pred_row_stride, const float* gt, int gt_h, int gt_w,
                             int step, int h, int w, double* acc, void* ws, int64_t ws_bytes, void* stream) {
    SF_REQUIRE(pred && gt && acc && ws, "sf_flow_score: null argument");
    SF_REQUIRE(h > 0 && w > 0, "sf_flow_score: bad shape %d x %d", h, w);
    SF_REQUIRE((int64_t)h * w < (1 << 30), "sf_flow_score: field %d x %d too large", h, w);
    SF_REQUIRE(step == 1 || step == 2, "sf_flow_score: step %d (1 or 2)", step);
    SF_REQUIRE(gt_h > (int64_t)step * (h - 1) && gt_w > (int64_t)step * (w - 1),
               "sf_flow_score: ground truth %d x %d does not cover %d x %d at step %d", gt_h, gt_w, h, w, step);
    SF_REQUIRE(pred_row_stride >= w && pred_ch_stride != 0, "sf_flow_score: bad prediction strides (%lld, %lld)",
               (long long)pred_ch_stride, (long long)pred_row_stride);
    SF_REQUIRE(ws_bytes >= SF_SCORE_WS_BYTES, "sf_flow_score: workspace of %lld bytes (needs %d)", (long long)ws_bytes,
               SF_SCORE_WS_BYTES);
    SF_REQUIRE((reinterpret_cast<uintptr_t>(acc) & 7u) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0,
               "sf_flow_score: acc / ws not 8-byte aligned");
    const int gw = (w + 3) / 4, ngroups = h * gw;
    const int nblocks = sf::ceil_div(ngroups, kBlock) < kMaxBlocks ? sf::ceil_div(ngroups, kBlock) : kMaxBlocks;
    // float4 loads need 16-byte aligned rows in both planes; float2 loads of the ground truth an 8-byte aligned base (its rows and
    // pixels are whole float pairs)
    const bool vec = (reinterpret_cast<uintptr_t>(pred) & 15u) == 0 && pred_ch_stride % 4 == 0 && pred_row_stride % 4 == 0;
    const bool gt_f2 = (reinterpret_cast<uintptr_t>(gt) & 7u) == 0;
    hipStream_t s = (hipStream_t)stream;
    double* partials = static_cast<double*>(ws);
    const int64_t gt_row_floats = (int64_t)2 * gt_w;
    if (vec) hipLaunchKernelGGL(flow_score_kernel<true>, dim3(nblocks), dim3(kBlock), 0, s, pred, pred_ch_stride, pred_row_stride, gt,
                                gt_row_floats, step, h, w, gt_f2, partials);
    else hipLaunchKernelGGL(flow_score_kernel<false>, dim3(nblocks), dim3(kBlock), 0, s, pred, pred_ch_stride, pred_row_stride, gt,
                            gt_row_floats, step, h, w, gt_f2, partials);
    const int st = sf::check_launch("sf_flow_score");
    if (st != SF_OK) return st;
    hipLaunchKernelGGL(flow_score_finish_kernel, dim3(1), dim3(kBlock), 0, s, partials, nblocks, acc);
    return sf::check_launch("sf_flow_score (finish)");
}
