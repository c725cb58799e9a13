// Frame interpolation by forward splatting, a batch of frame pairs per call (softmax-splatting's "summation splatting" of Niklaus &
// Liu 2020 with fixed integer importances in place of a learned metric; include/streamflow_hip.h, "frame interpolation", has the
// contract).
//
// sf_frame_interp: the frame at time t = num / den between frame A (time 0) and frame B (time 1) of each of n pairs.  Every pixel of
// A is pushed along t * (forward flow), every pixel of B along (1 - t) * (backward flow); where it lands, its colour is ADDED with
// bilinear weights to four target pixels.  A target that received something from a side takes that side's weighted mean; both sides
// are cross-faded by t; a target nothing reached (a hole) takes the cross-fade of the co-located pixels of A and B.  Every output
// byte is rounded ONCE, half up, from the exact rational value: where both sides are present the two means are blended as fractions
// (one quotient of products of the sums), not rounded to bytes first, so the byte is within half a level of the real-valued result.
//
// This is the project's scatter kernel, and it is deterministic by construction: the weights are INTEGERS (the bilinear fractions
// in 1/64ths, so the four taps of a source pixel sum to exactly 4096), the importances are integers 1 .. 16, the accumulators are
// unsigned 64-bit.  Integer sums do not depend on the order in which the adds arrive, so the result is bitwise the same from run to
// run and for any grid.  (A target that receives EVERY pixel of a 2^30-pixel field at the largest weight, importance and byte sums to
// 2^30 * 4096 * 16 * 255 < 2^54; 32-bit fields would overflow after 255 such contributions.)
//
// Launches: a clear of the accumulators (sf::fill_async: a kernel); splat_kernel, grid (blocks per field, n, 2 sides); resolve_kernel, grid
// (blocks per field, n); the stats finish (a block per pair).  Accumulators are planar, uint64 [n][side][W, C0, C1, C2][h][w], and
// both kernels use the lane mapping of flow_consistency_kernel: a wave owns 256 consecutive pixels of a row, lane l the pixels
// l + 64 j.  For smooth flows the 64 lanes of an atomic wave-instruction then go to 64 consecutive accumulators: 512 contiguous bytes.
// The adds are plain atomicAdd on unsigned long long whose result is discarded (no-return global atomics); 4 taps x 4 planes x 8
// bytes = at most 128 added bytes per source pixel and side.  The inside test is made on the float coordinates BEFORE any conversion
// to an integer: NaN, +-Inf and huge flows compare false and never form an address; every tap position is checked against the frame.
// Stats: per-block partial rows in the caller's workspace and a fixed-order finish kernel, as in flow_consistency.hip; the grid
// depends on (n, h, w) alone.
//
// Arithmetic: the coordinates are fp32 with every operation rounded on its own (FMA contraction is off for this file), everything
// after the weights is integer, in the order the header states, so a numpy restatement reproduces every byte.
#include "sf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kCallBlocks = 2048;                                        // blocks one call aims at (8 per CU), shared by its pairs
constexpr int kPlanes = 4;                                               // W, C0, C1, C2
constexpr int kPhaseClear = 1, kPhaseSplat = 2, kPhaseResolve = 4;

typedef unsigned long long u64;

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
            for (int wv = 1; wv < kWaves; ++wv) a += s[wv][k];
            r[k] = a;
        }
}

__global__ __launch_bounds__(kBlock) void interp_finish_kernel(const double* __restrict__ partials, int nblocks, double* __restrict__ stats) {
    __shared__ double s[kWaves][SF_INTERP_LEN];
    const int pair = blockIdx.x;
    const double* p = partials + (int64_t)pair * nblocks * SF_INTERP_LEN;
    double r[SF_INTERP_LEN];
#pragma unroll
    for (int k = 0; k < SF_INTERP_LEN; ++k) r[k] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kBlock)
#pragma unroll
        for (int k = 0; k < SF_INTERP_LEN; ++k) r[k] += p[(int64_t)b * SF_INTERP_LEN + k];
    block_sum<SF_INTERP_LEN>(r, s);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < SF_INTERP_LEN; ++k) stats[(int64_t)pair * SF_INTERP_LEN + k] += r[k];
}

struct Side {
    const uint8_t* img;                                                  // the frames that are splatted
    const float* flow;                                                   // along these fields ...
    const uint8_t* cls;                                                  // (optional) with importances chosen by these classes
    int64_t i_frame, i_row, i_px, i_ch, f_field, f_ch, f_row;
    float ts;                                                            // ... scaled by this
};

struct InterpArgs {
    Side side[2];                                                        // A with the forward flows, B with the backward flows
    int h, w, num, den;
    unsigned code_vis, code_occ, imp_vis, imp_occ, imp_other;
};

// units a row takes: a unit is 256 consecutive pixels, the work of one wave at a time
__host__ __device__ inline int units_per_row(int w) { return (w + 255) >> 8; }

// one axis of the splat: the first tap's position and the two integer weights (in 1/64ths)
__device__ __forceinline__ void taps(float p, int& i0, unsigned& w0, unsigned& w1) {
    const float f0 = floorf(p);
    const float fr = p - f0;                                             // in [0, 1]
    i0 = (int)f0;                                                        // -1 <= i0 <= size - 1: the caller has tested p
    w1 = (unsigned)(int)floorf(fr * 64.0f + 0.5f);                       // 0 .. 64
    w0 = 64u - w1;
}

__global__ __launch_bounds__(kBlock) void splat_kernel(InterpArgs a, u64* __restrict__ acc) {
    const int pair = blockIdx.y, sd = blockIdx.z;
    const int h = a.h, w = a.w;
    const Side& s = a.side[sd];
    const float* __restrict__ fu = s.flow + (int64_t)pair * s.f_field;
    const uint8_t* __restrict__ img = s.img + (int64_t)pair * s.i_frame;
    const uint8_t* __restrict__ cls = s.cls ? s.cls + (int64_t)pair * h * w : nullptr;
    const int64_t plane = (int64_t)h * w;
    u64* __restrict__ base = acc + ((int64_t)pair * 2 + sd) * kPlanes * plane;
    const float ts = s.ts;
    const int nb = units_per_row(w);
    const int nunits = h * nb;                                           // < 2^30 / 256 + h: fits an int
    for (int unit = blockIdx.x * kWaves + (threadIdx.x >> 6); unit < nunits; unit += gridDim.x * kWaves) {
        const int y = unit / nb, xl = (unit - y * nb) * 256 + (threadIdx.x & 63);
        const float* pu = fu + (int64_t)y * s.f_row;
        const uint8_t* prow = img + (int64_t)y * s.i_row;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = xl + 64 * j;
            if (x >= w) continue;
            const float u = pu[x], v = pu[s.f_ch + x];
            const float px = (float)x + ts * u, py = (float)y + ts * v;
            if (!(px > -1.0f && px < (float)w && py > -1.0f && py < (float)h)) continue;              // false for NaN
            unsigned imp = a.imp_vis;
            if (cls) {
                const unsigned c = cls[(int64_t)y * w + x];
                imp = c == a.code_vis ? a.imp_vis : (c == a.code_occ ? a.imp_occ : a.imp_other);
            }
            const uint8_t* pp = prow + (int64_t)x * s.i_px;
            const unsigned c0 = pp[0], c1 = pp[s.i_ch], c2 = pp[2 * s.i_ch];
            int x0, y0;
            unsigned wx[2], wy[2];
            taps(px, x0, wx[0], wx[1]);
            taps(py, y0, wy[0], wy[1]);
#pragma unroll
            for (int ty = 0; ty < 2; ++ty)
#pragma unroll
                for (int tx = 0; tx < 2; ++tx) {
                    const int xi = x0 + tx, yi = y0 + ty;
                    const unsigned wt = wx[tx] * wy[ty];
                    if (wt == 0u || xi < 0 || xi >= w || yi < 0 || yi >= h) continue;
                    const u64 wi = (u64)(wt * imp);                      // <= 4096 * 16
                    u64* t = base + (int64_t)yi * w + xi;
                    atomicAdd(t, wi);
                    atomicAdd(t + plane, wi * c0);
                    atomicAdd(t + 2 * plane, wi * c1);
                    atomicAdd(t + 3 * plane, wi * c2);
                }
        }
    }
}

// (2 c + wsum) / (2 wsum) = c / wsum rounded half up, at most 255; 32-bit division wherever numerator AND denominator fit
// (everywhere but under extreme contention: dark pixels keep the numerator small while 2 wsum passes 2^32)
__device__ __forceinline__ unsigned mean_byte(u64 c, u64 wsum) {
    const u64 nu = 2 * c + wsum, de = 2 * wsum;
    if (((nu | de) >> 32) == 0) return (unsigned)nu / (unsigned)de;
    return (unsigned)(nu / de);
}

typedef unsigned __int128 u128;

// ((den - num) ca / wa + num cb / wb) / den rounded half up, exactly: with N = (den - num) ca wb + num cb wa and D = den wa wb it
// is (2 N + D) / (2 D), at most 255.  64-bit where the sums are small enough for 2 N + D to fit (wa, wb < 2^24 and ca, cb < 2^32:
// everywhere but under heavy contention); otherwise 128-bit products, and the byte found by bisection (no 128-bit division): the
// largest r with (2 r - 1) D <= 2 N.
__device__ __forceinline__ unsigned blend_byte(u64 ca, u64 wa, u64 cb, u64 wb, unsigned num, unsigned den) {
    if (((wa | wb) >> 24) == 0 && ((ca | cb) >> 32) == 0) {
        const u64 n2 = 2 * ((u64)(den - num) * ca * wb + (u64)num * cb * wa), d = (u64)den * wa * wb;   // n2 <= 2^63, d <= 2^54
        return (unsigned)((n2 + d) / (2 * d));
    }
    const u128 n2 = 2 * ((u128)ca * wb * (den - num) + (u128)cb * wa * num), d = (u128)wa * wb * den;   // n2 < 2^109, 511 d < 2^108
    unsigned lo = 0u, hi = 255u;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const unsigned mid = (lo + hi + 1u) >> 1;
        if (d * (2u * mid - 1u) <= n2) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void resolve_kernel(InterpArgs a, const u64* __restrict__ acc, uint8_t* __restrict__ out,
                                                         uint8_t* __restrict__ cover, double* __restrict__ partials) {
    __shared__ double s[kWaves][SF_INTERP_LEN];
    const int pair = blockIdx.y;
    const int h = a.h, w = a.w;
    const int64_t plane = (int64_t)h * w;
    const u64* __restrict__ accA = acc + (int64_t)pair * 2 * kPlanes * plane;
    const u64* __restrict__ accB = accA + kPlanes * plane;
    const uint8_t* __restrict__ imA = a.side[0].img + (int64_t)pair * a.side[0].i_frame;
    const uint8_t* __restrict__ imB = a.side[1].img + (int64_t)pair * a.side[1].i_frame;
    uint8_t* __restrict__ dst = out + (int64_t)pair * plane * 3;
    uint8_t* __restrict__ cov = cover ? cover + (int64_t)pair * plane : nullptr;
    const unsigned num = (unsigned)a.num, den = (unsigned)a.den;
    unsigned n_px = 0, n_code[4] = {0u, 0u, 0u, 0u};                     // (a thread sees fewer than 2^30 pixels)
    const int nb = units_per_row(w);
    const int nunits = h * nb;
    for (int unit = blockIdx.x * kWaves + (threadIdx.x >> 6); unit < nunits; unit += gridDim.x * kWaves) {
        const int y = unit / nb, xl = (unit - y * nb) * 256 + (threadIdx.x & 63);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = xl + 64 * j;
            if (x >= w) continue;
            const int64_t q = (int64_t)y * w + x;
            const u64 wa = accA[q], wb = accB[q];
            const unsigned code = wa ? (wb ? 0u : 1u) : (wb ? 2u : 3u);
            unsigned byte[3];
            if (code == 3u) {                                            // a hole: the blend of the co-located bytes
                const uint8_t* pa = imA + (int64_t)y * a.side[0].i_row + (int64_t)x * a.side[0].i_px;
                const uint8_t* pb = imB + (int64_t)y * a.side[1].i_row + (int64_t)x * a.side[1].i_px;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    byte[c] = ((unsigned)pa[c * a.side[0].i_ch] * (den - num) + (unsigned)pb[c * a.side[1].i_ch] * num + den / 2u) / den;
            } else if (code == 0u) {
#pragma unroll
                for (int c = 0; c < 3; ++c) byte[c] = blend_byte(accA[q + (c + 1) * plane], wa, accB[q + (c + 1) * plane], wb, num, den);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) byte[c] = code == 1u ? mean_byte(accA[q + (c + 1) * plane], wa) : mean_byte(accB[q + (c + 1) * plane], wb);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[q * 3 + c] = (uint8_t)byte[c];
            if (cov) cov[q] = (uint8_t)code;
            n_px += 1u;
#pragma unroll
            for (int k = 0; k < 4; ++k) n_code[k] += code == (unsigned)k ? 1u : 0u;
        }
    }
    double r[SF_INTERP_LEN];
    r[SF_INTERP_PIXELS] = (double)n_px, r[SF_INTERP_BOTH] = (double)n_code[0], r[SF_INTERP_A_ONLY] = (double)n_code[1];
    r[SF_INTERP_B_ONLY] = (double)n_code[2], r[SF_INTERP_HOLES] = (double)n_code[3];
    block_sum<SF_INTERP_LEN>(r, s);
    if (threadIdx.x == 0) {
        double* p = partials + ((int64_t)pair * gridDim.x + blockIdx.x) * SF_INTERP_LEN;
#pragma unroll
        for (int k = 0; k < SF_INTERP_LEN; ++k) p[k] = r[k];
    }
}

bool shape_ok(int n, int h, int w) { return n >= 1 && n <= 65535 && h > 0 && w > 0 && (int64_t)h * w < (1 << 30); }

// blocks per pair: enough for four pixels per thread, at most the pair's share of kCallBlocks (at least one)
int interp_blocks(int n, int h, int w) {
    const int want = sf::ceil_div(h * units_per_row(w), kWaves);
    const int cap = kCallBlocks / n > 1 ? kCallBlocks / n : 1;
    return want < cap ? want : cap;
}

int64_t acc_bytes(int n, int h, int w) { return (int64_t)2 * kPlanes * (int64_t)sizeof(u64) * n * h * w; }

bool strides_ok(int64_t a, int64_t b, int64_t c, int64_t d) { return a >= 0 && b >= 0 && c >= 0 && d >= 0; }

}  // namespace

extern "C" int64_t sf_frame_interp_ws_bytes(int n, int h, int w) {
    if (!shape_ok(n, h, w)) return sf::fail(SF_ERR_BAD_ARG, "sf_frame_interp_ws_bytes: bad shape (%d pairs of %d x %d)", n, h, w);
    return acc_bytes(n, h, w) + (int64_t)n * interp_blocks(n, h, w) * SF_INTERP_LEN * (int64_t)sizeof(double);
}

extern "C" int sf_frame_interp_phases(const uint8_t* a, int64_t a_frame_stride, int64_t a_row_stride, int64_t a_px_stride,
                                      int64_t a_ch_stride, const uint8_t* b, int64_t b_frame_stride, int64_t b_row_stride,
                                      int64_t b_px_stride, int64_t b_ch_stride, const float* fwd, int64_t fwd_field_stride,
                                      int64_t fwd_ch_stride, int64_t fwd_row_stride, const float* bwd, int64_t bwd_field_stride,
                                      int64_t bwd_ch_stride, int64_t bwd_row_stride, int n, int h, int w, int num, int den,
                                      const uint8_t* cls_f, const uint8_t* cls_b, uint8_t code_visible, uint8_t code_occluded,
                                      int imp_vis, int imp_occ, int imp_other, uint8_t* out, uint8_t* cover, double* stats, void* ws,
                                      int64_t ws_bytes, int phases, void* stream) {
    SF_REQUIRE(a && b && fwd && bwd && out && stats && ws, "sf_frame_interp: null argument");
    SF_REQUIRE(h > 0 && w > 0, "sf_frame_interp: bad shape %d x %d", h, w);
    SF_REQUIRE((int64_t)h * w < (1 << 30), "sf_frame_interp: frame %d x %d too large", h, w);
    SF_REQUIRE(n >= 1 && n <= 65535, "sf_frame_interp: %d pairs in one call (1 .. 65535)", n);
    SF_REQUIRE(den >= 2 && den <= 64 && num > 0 && num < den, "sf_frame_interp: t = %d / %d (0 < num < den <= 64)", num, den);
    SF_REQUIRE(fwd_row_stride >= w && bwd_row_stride >= w, "sf_frame_interp: a row stride (%lld, %lld) below w = %d",
               (long long)fwd_row_stride, (long long)bwd_row_stride, w);
    SF_REQUIRE(fwd_ch_stride != 0 && bwd_ch_stride != 0 && fwd_field_stride >= 0 && bwd_field_stride >= 0,
               "sf_frame_interp: bad channel / field strides (%lld, %lld, %lld, %lld)", (long long)fwd_ch_stride,
               (long long)bwd_ch_stride, (long long)fwd_field_stride, (long long)bwd_field_stride);
    SF_REQUIRE(strides_ok(a_frame_stride, a_row_stride, a_px_stride, a_ch_stride), "sf_frame_interp: negative stride of A (%lld, %lld, %lld, %lld)",
               (long long)a_frame_stride, (long long)a_row_stride, (long long)a_px_stride, (long long)a_ch_stride);
    SF_REQUIRE(strides_ok(b_frame_stride, b_row_stride, b_px_stride, b_ch_stride), "sf_frame_interp: negative stride of B (%lld, %lld, %lld, %lld)",
               (long long)b_frame_stride, (long long)b_row_stride, (long long)b_px_stride, (long long)b_ch_stride);
    SF_REQUIRE((cls_f != nullptr) == (cls_b != nullptr), "sf_frame_interp: the two class maps come together (one of them is null)");
    SF_REQUIRE(imp_vis >= 1 && imp_vis <= 16 && imp_occ >= 1 && imp_occ <= 16 && imp_other >= 1 && imp_other <= 16,
               "sf_frame_interp: importances (%d, %d, %d) outside 1 .. 16", imp_vis, imp_occ, imp_other);
    const int64_t need = sf_frame_interp_ws_bytes(n, h, w);
    SF_REQUIRE(ws_bytes >= need, "sf_frame_interp: workspace of %lld bytes (needs %lld)", (long long)ws_bytes, (long long)need);
    SF_REQUIRE((reinterpret_cast<uintptr_t>(fwd) & 3u) == 0 && (reinterpret_cast<uintptr_t>(bwd) & 3u) == 0,
               "sf_frame_interp: fwd / bwd not 4-byte aligned");
    SF_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7u) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0,
               "sf_frame_interp: stats / ws not 8-byte aligned");
    SF_REQUIRE(phases >= 1 && phases <= 7, "sf_frame_interp: phases = %d (a mask of 1 clear, 2 splat, 4 resolve)", phases);
    InterpArgs p;
    Side& sa = p.side[0];
    Side& sb = p.side[1];
    sa.img = a, sa.flow = fwd, sa.cls = cls_f;
    sa.i_frame = a_frame_stride, sa.i_row = a_row_stride, sa.i_px = a_px_stride, sa.i_ch = a_ch_stride;
    sa.f_field = fwd_field_stride, sa.f_ch = fwd_ch_stride, sa.f_row = fwd_row_stride;
    sa.ts = (float)num / (float)den;
    sb.img = b, sb.flow = bwd, sb.cls = cls_b;
    sb.i_frame = b_frame_stride, sb.i_row = b_row_stride, sb.i_px = b_px_stride, sb.i_ch = b_ch_stride;
    sb.f_field = bwd_field_stride, sb.f_ch = bwd_ch_stride, sb.f_row = bwd_row_stride;
    sb.ts = (float)(den - num) / (float)den;
    p.h = h, p.w = w, p.num = num, p.den = den;
    p.code_vis = code_visible, p.code_occ = code_occluded;
    p.imp_vis = (unsigned)imp_vis, p.imp_occ = (unsigned)imp_occ, p.imp_other = (unsigned)imp_other;
    const int nblocks = interp_blocks(n, h, w);
    hipStream_t s = (hipStream_t)stream;
    u64* acc = static_cast<u64*>(ws);
    double* partials = reinterpret_cast<double*>(static_cast<char*>(ws) + acc_bytes(n, h, w));
    if (phases & kPhaseClear) {
        const int st = sf::fill_async("sf_frame_interp (clear)", acc, 0, acc_bytes(n, h, w), s);
        if (st != SF_OK) return st;
    }
    if (phases & kPhaseSplat) {
        hipLaunchKernelGGL(splat_kernel, dim3(nblocks, n, 2), dim3(kBlock), 0, s, p, acc);
        const int st = sf::check_launch("sf_frame_interp (splat)");
        if (st != SF_OK) return st;
    }
    if (phases & kPhaseResolve) {
        hipLaunchKernelGGL(resolve_kernel, dim3(nblocks, n), dim3(kBlock), 0, s, p, acc, out, cover, partials);
        const int st = sf::check_launch("sf_frame_interp (resolve)");
        if (st != SF_OK) return st;
        hipLaunchKernelGGL(interp_finish_kernel, dim3(n), dim3(kBlock), 0, s, partials, nblocks, stats);
        return sf::check_launch("sf_frame_interp (finish)");
    }
    return SF_OK;
}

extern "C" int sf_frame_interp(const uint8_t* a, int64_t a_frame_stride, int64_t a_row_stride, int64_t a_px_stride, int64_t a_ch_stride,
                               const uint8_t* b, int64_t b_frame_stride, int64_t b_row_stride, int64_t b_px_stride, int64_t b_ch_stride,
                               const float* fwd, int64_t fwd_field_stride, int64_t fwd_ch_stride, int64_t fwd_row_stride,
                               const float* bwd, int64_t bwd_field_stride, int64_t bwd_ch_stride, int64_t bwd_row_stride, int n, int h,
                               int w, int num, int den, const uint8_t* cls_f, const uint8_t* cls_b, uint8_t code_visible,
                               uint8_t code_occluded, int imp_vis, int imp_occ, int imp_other, uint8_t* out, uint8_t* cover,
                               double* stats, void* ws, int64_t ws_bytes, void* stream) {
    return sf_frame_interp_phases(a, a_frame_stride, a_row_stride, a_px_stride, a_ch_stride, b, b_frame_stride, b_row_stride, b_px_stride,
                                  b_ch_stride, fwd, fwd_field_stride, fwd_ch_stride, fwd_row_stride, bwd, bwd_field_stride, bwd_ch_stride,
                                  bwd_row_stride, n, h, w, num, den, cls_f, cls_b, code_visible, code_occluded, imp_vis, imp_occ,
                                  imp_other, out, cover, stats, ws, ws_bytes, 7, stream);
}
