// Sintel / KITTI scoring on the device, a batch of fields per call (reference evaluate_mf.py:106-142 validate_kitti_mf, :468-503
// validate_sintel_mf, :549-592 validate_sintel_occ_mf): n_fields predicted fields of one size, each against its own ground truth,
// each ADDED into its own row of an fp64 accumulator acc[n_fields][SF_EVAL_LEN] (layout: include/streamflow_hip.h, SF_EVAL_*).
// The field pointers travel in the kernel arguments (SfScoreFields by value, as SfPairPtrs does): nothing is uploaded.
//
// The ground truth is read as its decoder left it: float32 (u, v) pairs of a .flo file, or the 16-bit (u, v, valid) samples of a
// KITTI flow_occ PNG, decoded here ((s - 32768) / 64: exact in fp32); the optional occlusion map is the bytes of a Sintel
// occlusions PNG.
//
// Two kernels, no atomics.  flow_score_batch_kernel: grid (blocks per field, n_fields); every thread walks groups of four pixels
// of one row of its field (grid-stride) -- float4 loads of the two prediction planes, 2 x 16 / 4 x 8 bytes of float ground truth or
// 3 x 8 / 6 x 4 bytes of 16-bit ground truth, 4 mask bytes in one load, each where pointers, strides and w allow it, element loads
// otherwise and in the last group of a row that is no multiple of four; per thread four fp64 sums and eight 32-bit counts (a
// thread sees at most 2^16 pixels), reduced inside the block in a fixed order and written as one row of per-block partials.
// flow_score_batch_finish_kernel: one block per field sums that field's partial rows in a fixed order and adds them to its
// accumulator row.  The grid depends on (n_fields, h, w) alone, so repeated calls give bitwise equal accumulators.
//
// Arithmetic: fp32, every operation rounded on its own (FMA contraction is off for this file; hipcc's fp32 square root and
// division are correctly rounded), the reference's torch expressions.  |gt| and e / |gt| are formed only where the outlier rule
// can hold (valid, e > 3): a pixel that skips them would have failed the rule whatever they are.
#include "sf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kCallBlocks = 2048;                                        // blocks one call aims at (8 per CU), shared by its fields

struct Tally {
    double sum, sum_valid, sum_occ, sum_noc;
    unsigned pixels, lt1, lt3, lt5, valid, outlier, occ, noc;
};

template <bool kMask>
__device__ __forceinline__ void score_px(float pu, float pv, float gu, float gv, bool valid, bool occ, Tally& t) {
    const float du = pu - gu, dv = pv - gv;
    const float e = sqrtf(du * du + dv * dv);
    t.pixels += 1u;
    t.sum += (double)e;
    t.lt1 += e < 1.0f ? 1u : 0u;
    t.lt3 += e < 3.0f ? 1u : 0u;
    t.lt5 += e < 5.0f ? 1u : 0u;
    if (valid) {
        t.valid += 1u;
        t.sum_valid += (double)e;
        if (e > 3.0f) {                                                  // e / 0 = inf counts, 0 / 0 = NaN cannot get here
            const float mag = sqrtf(gu * gu + gv * gv);
            t.outlier += (e / mag) > 0.05f ? 1u : 0u;
        }
    }
    if (kMask) {
        if (occ) {
            t.occ += 1u;
            t.sum_occ += (double)e;
        } else {
            t.noc += 1u;
            t.sum_noc += (double)e;
        }
    }
}

__device__ __forceinline__ void to_row(const Tally& t, double (&r)[SF_EVAL_LEN]) {
    r[SF_EVAL_PIXELS] = (double)t.pixels, r[SF_EVAL_SUM_EPE] = t.sum;
    r[SF_EVAL_LT1] = (double)t.lt1, r[SF_EVAL_LT3] = (double)t.lt3, r[SF_EVAL_LT5] = (double)t.lt5;
    r[SF_EVAL_VALID] = (double)t.valid, r[SF_EVAL_SUM_EPE_VALID] = t.sum_valid, r[SF_EVAL_OUTLIER] = (double)t.outlier;
    r[SF_EVAL_OCC] = (double)t.occ, r[SF_EVAL_SUM_EPE_OCC] = t.sum_occ;
    r[SF_EVAL_NOC] = (double)t.noc, r[SF_EVAL_SUM_EPE_NOC] = t.sum_noc;
}

// the block's totals in thread 0, in a fixed order: a shuffle tree inside every wave, then the waves in order
__device__ __forceinline__ void block_sum(double (&r)[SF_EVAL_LEN], double (*s)[SF_EVAL_LEN]) {
#pragma unroll
    for (int k = 0; k < SF_EVAL_LEN; ++k)
        for (int off = 32; off > 0; off >>= 1) r[k] += __shfl_xor(r[k], off, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < SF_EVAL_LEN; ++k) s[threadIdx.x >> 6][k] = r[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < SF_EVAL_LEN; ++k) {
            double a = s[0][k];
            for (int wv = 1; wv < kBlock / 64; ++wv) a += s[wv][k];
            r[k] = a;
        }
}

__device__ __forceinline__ float kitti_px(unsigned s) { return ((float)s - 32768.0f) / 64.0f; }

struct BatchArgs {
    SfScoreFields f;
    int64_t ch_stride, row_stride;
    int h, w;
    int pred_vec;                                                        // float4 loads of the prediction planes
    int gt_align;                                                        // bytes every group of four ground-truth pixels is aligned to
    int mask_vec;                                                        // one 4-byte load of a group's mask bytes
};

template <int kKind, bool kMask>
__global__ __launch_bounds__(kBlock) void flow_score_batch_kernel(BatchArgs a, double* __restrict__ partials) {
    __shared__ double s[kBlock / 64][SF_EVAL_LEN];
    const int field = blockIdx.y;
    const float* __restrict__ pred = a.f.pred[field];
    const void* __restrict__ gt = a.f.gt[field];
    const uint8_t* __restrict__ mask = kMask ? a.f.mask[field] : nullptr;
    const int h = a.h, w = a.w;
    Tally t = {};
    const int gw = (w + 3) >> 2;
    const int ngroups = h * gw;                                          // < 2^30 / 4 + h: fits an int
    for (int q = blockIdx.x * kBlock + threadIdx.x; q < ngroups; q += gridDim.x * kBlock) {
        const int y = q / gw, x0 = (q - y * gw) << 2;
        const int left = w - x0 < 4 ? w - x0 : 4;                        // pixels of this group that exist (>= 1)
        const bool full = left == 4;
        const int64_t px = (int64_t)y * w + x0;                          // first pixel of the group in the dense ground truth
        const float* pu = pred + (int64_t)y * a.row_stride + x0;
        const float* pv = pu + a.ch_stride;
        float u[4], v[4], gu[4], gv[4];
        bool valid[4], occ[4];
        if (a.pred_vec && full) {
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
        if constexpr (kKind == SF_GT_FLO32) {
            const float* g = static_cast<const float*>(gt) + 2 * px;
            if (a.gt_align >= 16 && full) {
                const float4 g0 = reinterpret_cast<const float4*>(g)[0], g1 = reinterpret_cast<const float4*>(g)[1];
                gu[0] = g0.x, gv[0] = g0.y, gu[1] = g0.z, gv[1] = g0.w;
                gu[2] = g1.x, gv[2] = g1.y, gu[3] = g1.z, gv[3] = g1.w;
            } else if (a.gt_align >= 8 && full) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float2 g2 = reinterpret_cast<const float2*>(g)[j];
                    gu[j] = g2.x, gv[j] = g2.y;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    gu[j] = j < left ? g[2 * j] : 0.0f;
                    gv[j] = j < left ? g[2 * j + 1] : 0.0f;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float gs = gu[j] + gv[j];
                valid[j] = !(gs != gs);
            }
        } else {
            const uint16_t* g = static_cast<const uint16_t*>(gt) + 3 * px;
            unsigned sm[12];                                             // (u, v, valid) samples of the four pixels
            if (a.gt_align >= 8 && full) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const uint2 d = reinterpret_cast<const uint2*>(g)[k];
                    sm[4 * k] = d.x & 0xffffu, sm[4 * k + 1] = d.x >> 16, sm[4 * k + 2] = d.y & 0xffffu, sm[4 * k + 3] = d.y >> 16;
                }
            } else if (a.gt_align >= 4 && full) {
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const unsigned d = reinterpret_cast<const unsigned*>(g)[k];
                    sm[2 * k] = d & 0xffffu, sm[2 * k + 1] = d >> 16;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k) sm[k] = k < 3 * left ? (unsigned)g[k] : 0u;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                gu[j] = kitti_px(sm[3 * j]);
                gv[j] = kitti_px(sm[3 * j + 1]);
                valid[j] = sm[3 * j + 2] != 0u;
            }
        }
        if constexpr (kMask) {
            const uint8_t* m = mask + px;
            if (a.mask_vec && full) {
                const unsigned d = *reinterpret_cast<const unsigned*>(m);
#pragma unroll
                for (int j = 0; j < 4; ++j) occ[j] = ((d >> (8 * j)) & 0xffu) == 255u;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) occ[j] = j < left && m[j] == 255;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) occ[j] = false;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= left) break;
            score_px<kMask>(u[j], v[j], gu[j], gv[j], valid[j], occ[j], t);
        }
    }
    double r[SF_EVAL_LEN];
    to_row(t, r);
    block_sum(r, s);
    if (threadIdx.x == 0) {
        double* out = partials + ((int64_t)field * gridDim.x + blockIdx.x) * SF_EVAL_LEN;
#pragma unroll
        for (int k = 0; k < SF_EVAL_LEN; ++k) out[k] = r[k];
    }
}

__global__ __launch_bounds__(kBlock) void flow_score_batch_finish_kernel(const double* __restrict__ partials, int nblocks,
                                                                         double* __restrict__ acc) {
    __shared__ double s[kBlock / 64][SF_EVAL_LEN];
    const int field = blockIdx.x;
    const double* p = partials + (int64_t)field * nblocks * SF_EVAL_LEN;
    double r[SF_EVAL_LEN];
#pragma unroll
    for (int k = 0; k < SF_EVAL_LEN; ++k) r[k] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kBlock)
#pragma unroll
        for (int k = 0; k < SF_EVAL_LEN; ++k) r[k] += p[(int64_t)b * SF_EVAL_LEN + k];
    block_sum(r, s);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < SF_EVAL_LEN; ++k) acc[(int64_t)field * SF_EVAL_LEN + k] += r[k];
}

// blocks per field: enough for one group of four pixels per thread, at most the field's share of kCallBlocks
int blocks_per_field(int n_fields, int h, int w) {
    const int ngroups = h * ((w + 3) / 4);
    const int cap = kCallBlocks / n_fields;                              // >= 64 for n_fields <= SF_SCORE_BATCH_MAX
    const int want = sf::ceil_div(ngroups, kBlock);
    return want < cap ? want : cap;
}

bool shape_ok(int n_fields, int h, int w) {
    return n_fields >= 1 && n_fields <= SF_SCORE_BATCH_MAX && h > 0 && w > 0 && (int64_t)h * w < (1 << 30);
}

template <int kKind>
void launch(const BatchArgs& a, bool masks, dim3 grid, hipStream_t s, double* partials) {
    if (masks) hipLaunchKernelGGL((flow_score_batch_kernel<kKind, true>), grid, dim3(kBlock), 0, s, a, partials);
    else hipLaunchKernelGGL((flow_score_batch_kernel<kKind, false>), grid, dim3(kBlock), 0, s, a, partials);
}

}  // namespace

extern "C" int64_t sf_flow_score_batch_ws_bytes(int n_fields, int h, int w) {
    if (!shape_ok(n_fields, h, w)) return sf::fail(SF_ERR_BAD_ARG, "sf_flow_score_batch_ws_bytes: bad shape (%d fields of %d x %d)", n_fields, h, w);
    return (int64_t)n_fields * blocks_per_field(n_fields, h, w) * SF_EVAL_LEN * (int64_t)sizeof(double);
}

extern "C" int sf_flow_score_batch(const SfScoreFields* f, int n_fields, int64_t pred_ch_stride, int64_t pred_row_stride,
                                   int gt_kind, int h, int w, double* acc, void* ws, int64_t ws_bytes, void* stream) {
    SF_REQUIRE(f && acc && ws, "sf_flow_score_batch: null argument");
    SF_REQUIRE(n_fields >= 1 && n_fields <= SF_SCORE_BATCH_MAX, "sf_flow_score_batch: %d fields (1 .. %d)", n_fields,
               SF_SCORE_BATCH_MAX);
    SF_REQUIRE(gt_kind == SF_GT_FLO32 || gt_kind == SF_GT_KITTI16, "sf_flow_score_batch: unknown ground-truth kind %d", gt_kind);
    SF_REQUIRE(h > 0 && w > 0, "sf_flow_score_batch: bad shape %d x %d", h, w);
    SF_REQUIRE((int64_t)h * w < (1 << 30), "sf_flow_score_batch: field %d x %d too large", h, w);
    SF_REQUIRE(pred_row_stride >= w && pred_ch_stride != 0, "sf_flow_score_batch: bad prediction strides (%lld, %lld)",
               (long long)pred_ch_stride, (long long)pred_row_stride);
    const int64_t need = sf_flow_score_batch_ws_bytes(n_fields, h, w);
    SF_REQUIRE(ws_bytes >= need, "sf_flow_score_batch: workspace of %lld bytes (needs %lld)", (long long)ws_bytes, (long long)need);
    SF_REQUIRE((reinterpret_cast<uintptr_t>(acc) & 7u) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0,
               "sf_flow_score_batch: acc / ws not 8-byte aligned");
    const uintptr_t gt_elem = gt_kind == SF_GT_FLO32 ? 4u : 2u;
    uintptr_t pred_bits = 0, gt_bits = 0, mask_bits = 0;                 // the low bits any of the pointers has set
    int n_masks = 0;
    for (int i = 0; i < n_fields; ++i) {
        SF_REQUIRE(f->pred[i] && f->gt[i], "sf_flow_score_batch: null prediction or ground truth of field %d", i);
        SF_REQUIRE((reinterpret_cast<uintptr_t>(f->pred[i]) & 3u) == 0, "sf_flow_score_batch: prediction %d not 4-byte aligned", i);
        SF_REQUIRE((reinterpret_cast<uintptr_t>(f->gt[i]) & (gt_elem - 1)) == 0,
                   "sf_flow_score_batch: ground truth %d not aligned to its %d-byte elements", i, (int)gt_elem);
        pred_bits |= reinterpret_cast<uintptr_t>(f->pred[i]);
        gt_bits |= reinterpret_cast<uintptr_t>(f->gt[i]);
        mask_bits |= reinterpret_cast<uintptr_t>(f->mask[i]);
        n_masks += f->mask[i] != nullptr;
    }
    SF_REQUIRE(n_masks == 0 || n_masks == n_fields, "sf_flow_score_batch: %d of %d fields have a mask (all or none)", n_masks,
               n_fields);
    BatchArgs a = {};
    for (int i = 0; i < n_fields; ++i) a.f.pred[i] = f->pred[i], a.f.gt[i] = f->gt[i], a.f.mask[i] = f->mask[i];
    a.ch_stride = pred_ch_stride, a.row_stride = pred_row_stride, a.h = h, a.w = w;
    // a group starts at pixel y w + x0 with x0 a multiple of four: float4 loads need 16-byte aligned rows in both planes; the
    // ground truth has 8 (float) or 6 (16-bit) bytes per pixel, so a group is aligned to 16 / 8 bytes when w is even / a multiple
    // of four and to 8 / 4 bytes when the base allows nothing more; the mask's four bytes need w to be a multiple of four
    a.pred_vec = (pred_bits & 15u) == 0 && pred_ch_stride % 4 == 0 && pred_row_stride % 4 == 0;
    if (gt_kind == SF_GT_FLO32) a.gt_align = ((gt_bits & 15u) == 0 && w % 2 == 0) ? 16 : (gt_bits & 7u) == 0 ? 8 : 4;
    else a.gt_align = ((gt_bits & 7u) == 0 && w % 4 == 0) ? 8 : ((gt_bits & 3u) == 0 && w % 2 == 0) ? 4 : 2;
    a.mask_vec = (mask_bits & 3u) == 0 && w % 4 == 0;
    const int nblocks = blocks_per_field(n_fields, h, w);
    hipStream_t s = (hipStream_t)stream;
    double* partials = static_cast<double*>(ws);
    const dim3 grid(nblocks, n_fields);
    if (gt_kind == SF_GT_FLO32) launch<SF_GT_FLO32>(a, n_masks != 0, grid, s, partials);
    else launch<SF_GT_KITTI16>(a, n_masks != 0, grid, s, partials);
    const int st = sf::check_launch("sf_flow_score_batch");
    if (st != SF_OK) return st;
    hipLaunchKernelGGL(flow_score_batch_finish_kernel, dim3(n_fields), dim3(kBlock), 0, s, partials, nblocks, acc);
    return sf::check_launch("sf_flow_score_batch (finish)");
}
