// Video stabilisation: a global (camera) motion fitted to every flow field by iteratively reweighted least squares, and frames
// re-rendered through an affine map (include/streamflow_hip.h, "video stabilisation", has the contract).
//
// sf_motion_moments: one weighting pass.  Every taking-part pixel gets a weight (class weight x Tukey's biweight of its residual
// against an input model) and adds thirteen fp64 products of (weight, normalised position, flow) to its field's moment row.
// sf_motion_solve: a thread per field solves the normal equations in fp64 (closed forms for translation and similarity, one
// Cholesky factor for the two 3 x 3 systems of the affine model) and derives the scale of the next pass.  sf_motion_fit: the chain
// of R rounds on the stream, two launches a round -- the finish kernel that sums a round's partials also solves it.
// sf_warp_affine_u8: a gather like sf_warp_frames whose source coordinate comes from six numbers per frame, not from a flow field.
//
// Moments kernel: grid (blocks per field, n); a wave owns 256 consecutive SAMPLES of a sampled row (sample = pixel when step is 1),
// lane l the samples l, l + 64, l + 128, l + 192, as flow_consistency_kernel lays its pixels out: coalesced element loads for any
// strides and alignment.  Warp kernel: a thread owns four consecutive pixels, twelve bytes as three 4-byte stores where w % 4 == 0,
// as warp_frames_kernel.  The inside test is made on float coordinates before any conversion to an integer, and replicate clamps
// with fminf / fmaxf after a NaN test: NaN, +-Inf and huge maps or flows never form an address.
// No atomics: per-block partials go to the caller's workspace and a second kernel (a block per field) sums them in a fixed order.
// The grids depend on (n, h, w, step) alone, so repeated calls give bitwise equal results.
//
// Arithmetic: weights and coordinates in fp32, every operation rounded on its own (FMA contraction is off for this file), sums in
// fp64 of fp64 products in the header's order, so a numpy restatement has the same terms and differs by summation order alone.
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
            for (int wv = 1; wv < kWaves; ++wv) a += s[wv][k];
            r[k] = a;
        }
}

struct MomArgs {
    const float* flow;
    const uint8_t* cls;
    const float* model;                                                  // [n][6] or null
    const float* inv_c2;                                                 // [n], with model
    int64_t f_field, f_ch, f_row;
    int h, w, step, hs, wsm;                                             // hs x wsm samples: rows y = ys step, columns x = xs step
    float max_mag, cx, cy, s;
    float wt_vis, wt_occ, wt_out;
    unsigned code_vis, code_occ, code_out;
};

__host__ __device__ inline int mom_units_per_row(int wsm) { return (wsm + 255) >> 8; }

__global__ __launch_bounds__(kBlock) void motion_moments_kernel(MomArgs a, double* __restrict__ partials) {
    __shared__ double s[kWaves][SF_MOT_LEN];
    const int field = blockIdx.y;
    const float* __restrict__ fu = a.flow + (int64_t)field * a.f_field;
    const uint8_t* __restrict__ cls = a.cls ? a.cls + (int64_t)field * a.h * a.w : nullptr;
    const bool robust = a.model != nullptr;
    float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f, m4 = 0.0f, m5 = 0.0f, inv_c2 = 0.0f;
    if (robust) {
        const float* m = a.model + (int64_t)field * 6;
        m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
        inv_c2 = a.inv_c2[field];
    }
    double s1 = 0.0, sx = 0.0, sy = 0.0, sxx = 0.0, sxy = 0.0, syy = 0.0, su = 0.0, sxu = 0.0, syu = 0.0, sv = 0.0, sxv = 0.0, syv = 0.0,
           sqq = 0.0;
    unsigned count = 0;                                                  // (a thread sees fewer than 2^30 samples)
    const int nb = mom_units_per_row(a.wsm);
    const int nunits = a.hs * nb;                                        // < 2^30 / 256 + hs: fits an int
    for (int unit = blockIdx.x * kWaves + (threadIdx.x >> 6); unit < nunits; unit += gridDim.x * kWaves) {
        const int ys = unit / nb, xs0 = (unit - ys * nb) * 256 + (threadIdx.x & 63);
        const int y = ys * a.step;                                       // <= h - 1
        const float* pu = fu + (int64_t)y * a.f_row;
        const float yn = ((float)y - a.cy) * a.s;
        float u[4], v[4];
        unsigned code[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xs = xs0 + 64 * j;
            const int64_t x = (int64_t)xs * a.step;                      // <= w - 1 where xs < wsm
            const bool in = xs < a.wsm;
            u[j] = in ? pu[x] : 0.0f;
            v[j] = in ? pu[a.f_ch + x] : 0.0f;
            code[j] = in && cls ? cls[(int64_t)y * a.w + x] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xs = xs0 + 64 * j;
            if (xs >= a.wsm) continue;
            const int x = xs * a.step;
            const float xn = ((float)x - a.cx) * a.s;
            const float uu = u[j], vv = v[j];
            const bool valid = fabsf(uu) <= a.max_mag && fabsf(vv) <= a.max_mag;         // false for NaN
            float wt = 1.0f;
            if (cls) wt = code[j] == a.code_vis ? a.wt_vis : code[j] == a.code_occ ? a.wt_occ : code[j] == a.code_out ? a.wt_out : 0.0f;
            if (robust) {
                const float pu_ = m0 + (m1 * xn + m2 * yn);
                const float pv_ = m3 + (m4 * xn + m5 * yn);
                const float ru = uu - pu_, rv = vv - pv_;
                const float r2 = ru * ru + rv * rv;
                const float t = r2 * inv_c2;
                const float g = 1.0f - t;
                const float wr = t < 1.0f ? g * g : 0.0f;                // Tukey's biweight; 0 for NaN
                wt = wt * wr;
            }
            if (!valid) wt = 0.0f;
            if (wt > 0.0f) {                                             // (valid: u, v are finite)
                const double W = (double)wt, X = (double)xn, Y = (double)yn, U = (double)uu, V = (double)vv;
                const double WX = W * X, WY = W * Y;
                s1 += W, sx += WX, sy += WY;
                sxx += WX * X, sxy += WX * Y, syy += WY * Y;
                su += W * U, sxu += WX * U, syu += WY * U;
                sv += W * V, sxv += WX * V, syv += WY * V;
                sqq += W * (U * U + V * V);
                count += 1u;
            }
        }
    }
    double r[SF_MOT_LEN];
    r[SF_MOT_S1] = s1, r[SF_MOT_SX] = sx, r[SF_MOT_SY] = sy, r[SF_MOT_SXX] = sxx, r[SF_MOT_SXY] = sxy, r[SF_MOT_SYY] = syy;
    r[SF_MOT_SU] = su, r[SF_MOT_SXU] = sxu, r[SF_MOT_SYU] = syu, r[SF_MOT_SV] = sv, r[SF_MOT_SXV] = sxv, r[SF_MOT_SYV] = syv;
    r[SF_MOT_SQQ] = sqq, r[SF_MOT_N] = (double)count;
    block_sum<SF_MOT_LEN>(r, s);
    if (threadIdx.x == 0) {
        double* p = partials + ((int64_t)field * gridDim.x + blockIdx.x) * SF_MOT_LEN;
#pragma unroll
        for (int k = 0; k < SF_MOT_LEN; ++k) p[k] = r[k];
    }
}

struct Solved {
    double a[6];
    double c;
    float inv_c2;
    int status;
};

// u ~ a0 + a1 x + a2 y, v ~ a3 + a4 x + a5 y from the moments, fp64, in the header's order
__device__ __forceinline__ Solved solve_field(const double (&m)[SF_MOT_LEN], int kind, double kappa, double c_floor) {
    const double S1 = m[SF_MOT_S1], Sx = m[SF_MOT_SX], Sy = m[SF_MOT_SY], Sxx = m[SF_MOT_SXX], Sxy = m[SF_MOT_SXY], Syy = m[SF_MOT_SYY];
    const double Su = m[SF_MOT_SU], Sxu = m[SF_MOT_SXU], Syu = m[SF_MOT_SYU], Sv = m[SF_MOT_SV], Sxv = m[SF_MOT_SXV], Syv = m[SF_MOT_SYV];
    Solved o;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0;
    o.status = SF_MOT_OK;
    double rss = 0.0;
    if (!(S1 > 0.0)) {                                                   // (a NaN included)
        o.status = SF_MOT_EMPTY;
    } else {
        const double thr = 0x1p-40 * S1;
        bool done = kind == SF_MOTION_TRANSLATION;
        if (kind == SF_MOTION_AFFINE) {
            const double l00 = sqrt(S1), l10 = Sx / l00, l20 = Sy / l00;
            const double d1 = Sxx - l10 * l10;
            if (d1 > thr) {
                const double l11 = sqrt(d1), l21 = (Sxy - l20 * l10) / l11;
                const double d2 = (Syy - l20 * l20) - l21 * l21;
                if (d2 > thr) {
                    const double l22 = sqrt(d2);
                    double z0 = Su / l00, z1 = (Sxu - l10 * z0) / l11, z2 = ((Syu - l20 * z0) - l21 * z1) / l22;
                    a2 = z2 / l22, a1 = (z1 - l21 * a2) / l11, a0 = ((z0 - l10 * a1) - l20 * a2) / l00;
                    z0 = Sv / l00, z1 = (Sxv - l10 * z0) / l11, z2 = ((Syv - l20 * z0) - l21 * z1) / l22;
                    a5 = z2 / l22, a4 = (z1 - l21 * a5) / l11, a3 = ((z0 - l10 * a4) - l20 * a5) / l00;
                    done = true;
                }
            }
        } else if (kind == SF_MOTION_SIMILARITY) {
            const double D = (Sxx + Syy) - (Sx * Sx + Sy * Sy) / S1;
            if (D > thr) {
                const double a = ((Sxu + Syv) - (Sx * Su + Sy * Sv) / S1) / D;
                const double b = ((Syu - Sxv) - (Sy * Su - Sx * Sv) / S1) / D;
                a0 = ((Su - a * Sx) - b * Sy) / S1;
                a3 = ((Sv + b * Sx) - a * Sy) / S1;
                a1 = a, a5 = a, a2 = b, a4 = -b;
                done = true;
            }
        }
        if (!done) o.status = SF_MOT_DEGENERATE;
        if (!done || kind == SF_MOTION_TRANSLATION) a0 = Su / S1, a3 = Sv / S1;
        const double pb = ((a0 * Su + a1 * Sxu) + a2 * Syu) + ((a3 * Sv + a4 * Sxv) + a5 * Syv);
        const double qu = (a0 * ((S1 * a0 + Sx * a1) + Sy * a2) + a1 * ((Sx * a0 + Sxx * a1) + Sxy * a2)) + a2 * ((Sy * a0 + Sxy * a1) + Syy * a2);
        const double qv = (a3 * ((S1 * a3 + Sx * a4) + Sy * a5) + a4 * ((Sx * a3 + Sxx * a4) + Sxy * a5)) + a5 * ((Sy * a3 + Sxy * a4) + Syy * a5);
        rss = fmax(0.0, (m[SF_MOT_SQQ] - 2.0 * pb) + (qu + qv));
        rss = rss / S1;
    }
    o.a[0] = a0, o.a[1] = a1, o.a[2] = a2, o.a[3] = a3, o.a[4] = a4, o.a[5] = a5;
    o.c = fmax(c_floor, kappa * sqrt(rss));                              // (fmax drops a NaN: c_floor)
    o.inv_c2 = (float)(1.0 / (o.c * o.c));
    return o;
}

struct SolveOut {
    double* model64;                                                     // [n][6]
    float* model32;                                                      // [n][6]
    double* c;                                                           // [n]
    float* inv_c2;                                                       // [n]
    int32_t* status;                                                     // [n]
    double* trace;                                                       // round r of field 0, or null; fields trace_stride doubles apart
    int64_t trace_stride;
};

__device__ __forceinline__ void store_solved(const Solved& o, const SolveOut& out, int field) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (out.model64) out.model64[(int64_t)field * 6 + k] = o.a[k];
        if (out.model32) out.model32[(int64_t)field * 6 + k] = (float)o.a[k];
    }
    if (out.c) out.c[field] = o.c;
    if (out.inv_c2) out.inv_c2[field] = o.inv_c2;
    if (out.status) out.status[field] = o.status;
    if (out.trace) {
        double* t = out.trace + (int64_t)field * out.trace_stride;
#pragma unroll
        for (int k = 0; k < 6; ++k) t[SF_MOT_TRACE_MODEL + k] = o.a[k];
        t[SF_MOT_TRACE_C] = o.c, t[SF_MOT_TRACE_INV_C2] = (double)o.inv_c2, t[SF_MOT_TRACE_STATUS] = (double)o.status;
    }
}

// a block per field: the partial rows in a fixed order -> the field's moment row (WRITTEN); kSolve: thread 0 goes on to solve it
template <bool kSolve>
__global__ __launch_bounds__(kBlock) void motion_finish_kernel(const double* __restrict__ partials, int nblocks, double* __restrict__ moments,
                                                               int64_t moments_stride, int kind, double kappa, double c_floor, SolveOut out) {
    __shared__ double s[kWaves][SF_MOT_LEN];
    const int field = blockIdx.x;
    const double* p = partials + (int64_t)field * nblocks * SF_MOT_LEN;
    double r[SF_MOT_LEN];
#pragma unroll
    for (int k = 0; k < SF_MOT_LEN; ++k) r[k] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kBlock)
#pragma unroll
        for (int k = 0; k < SF_MOT_LEN; ++k) r[k] += p[(int64_t)b * SF_MOT_LEN + k];
    block_sum<SF_MOT_LEN>(r, s);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < SF_MOT_LEN; ++k) moments[(int64_t)field * moments_stride + k] = r[k];
        if (kSolve) store_solved(solve_field(r, kind, kappa, c_floor), out, field);
    }
}

__global__ __launch_bounds__(64) void motion_solve_kernel(const double* __restrict__ moments, int n, int kind, double kappa, double c_floor,
                                                          SolveOut out) {
    const int field = blockIdx.x * 64 + threadIdx.x;
    if (field >= n) return;
    double m[SF_MOT_LEN];
#pragma unroll
    for (int k = 0; k < SF_MOT_LEN; ++k) m[k] = moments[(int64_t)field * SF_MOT_LEN + k];
    store_solved(solve_field(m, kind, kappa, c_floor), out, field);
}

struct AffArgs {
    const uint8_t* src;
    const float* maps;
    int64_t s_frame, s_row, s_px, s_ch;
    int h, w, border;
    unsigned fill0, fill1, fill2;
    int vec_store;
};

__global__ __launch_bounds__(kBlock) void warp_affine_kernel(AffArgs a, uint8_t* __restrict__ out, unsigned* __restrict__ partials) {
    __shared__ unsigned s[kWaves];
    const int frame = blockIdx.y;
    const int h = a.h, w = a.w;
    const uint8_t* __restrict__ src = a.src + (int64_t)frame * a.s_frame;
    uint8_t* __restrict__ dst = out + (int64_t)frame * h * w * 3;
    const float* m = a.maps + (int64_t)frame * 6;
    const float m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    const float xmax = (float)(w - 1), ymax = (float)(h - 1);
    unsigned outside = 0;                                                // (a thread sees fewer than 2^30 pixels)
    const int gw = (w + 3) >> 2;
    const int ngroups = h * gw;
    for (int q = blockIdx.x * kBlock + threadIdx.x; q < ngroups; q += gridDim.x * kBlock) {
        const int y = q / gw, x0 = (q - y * gw) << 2;
        const int left = w - x0 < 4 ? w - x0 : 4;
        const float fy_ = (float)y;
        const float bx = m1 * fy_ + m2, by = m4 * fy_ + m5;
        unsigned byte[12];                                               // [pixel][channel], as they lie in the output
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            byte[3 * j] = a.fill0, byte[3 * j + 1] = a.fill1, byte[3 * j + 2] = a.fill2;
            if (j >= left) continue;
            const float fx_ = (float)(x0 + j);
            float px = m0 * fx_ + bx, py = m3 * fx_ + by;
            bool take = px >= 0.0f && px <= xmax && py >= 0.0f && py <= ymax;              // false for NaN
            if (!take) {
                outside += 1u;
                if (a.border == SF_BORDER_REPLICATE && px == px && py == py) {
                    px = fminf(fmaxf(px, 0.0f), xmax), py = fminf(fmaxf(py, 0.0f), ymax);    // +-Inf and huge values included
                    take = true;
                }
            }
            if (!take) continue;
            const float fx0 = floorf(px), fy0 = floorf(py);
            const float tx = px - fx0, ty = py - fy0;
            const int ix0 = (int)fx0, iy0 = (int)fy0;                    // 0 <= ix0 <= w - 1, 0 <= iy0 <= h - 1
            const int ix1 = ix0 + 1 < w - 1 ? ix0 + 1 : w - 1, iy1 = iy0 + 1 < h - 1 ? iy0 + 1 : h - 1;
            const uint8_t* p00 = src + (int64_t)iy0 * a.s_row + (int64_t)ix0 * a.s_px;
            const uint8_t* p01 = src + (int64_t)iy0 * a.s_row + (int64_t)ix1 * a.s_px;
            const uint8_t* p10 = src + (int64_t)iy1 * a.s_row + (int64_t)ix0 * a.s_px;
            const uint8_t* p11 = src + (int64_t)iy1 * a.s_row + (int64_t)ix1 * a.s_px;
            const float gx = 1.0f - tx, gy = 1.0f - ty;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int64_t co = (int64_t)c * a.s_ch;
                const float top = gx * (float)p00[co] + tx * (float)p01[co];
                const float bot = gx * (float)p10[co] + tx * (float)p11[co];
                const float val = gy * top + ty * bot;
                byte[3 * j + c] = (unsigned)floorf(val + 0.5f);          // 0 <= val <= 255
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
    for (int off = 32; off > 0; off >>= 1) outside += (unsigned)__shfl_xor((int)outside, off, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = outside;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = s[0];
        for (int wv = 1; wv < kWaves; ++wv) t += s[wv];
        partials[(int64_t)frame * gridDim.x + blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kBlock) void warp_affine_finish_kernel(const unsigned* __restrict__ partials, int nblocks,
                                                                    unsigned* __restrict__ counts) {
    __shared__ unsigned s[kWaves];
    const int frame = blockIdx.x;
    unsigned t = 0;
    for (int b = threadIdx.x; b < nblocks; b += kBlock) t += partials[(int64_t)frame * nblocks + b];
    for (int off = 32; off > 0; off >>= 1) t += (unsigned)__shfl_xor((int)t, off, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned r = s[0];
        for (int wv = 1; wv < kWaves; ++wv) r += s[wv];
        counts[frame] = r;
    }
}

bool shape_ok(int n, int h, int w) { return n >= 1 && n <= 65535 && h > 0 && w > 0 && (int64_t)h * w < (1 << 30); }

// blocks per field: `want` (enough for four samples per thread), at most the field's share of kCallBlocks (at least one)
int blocks_per_field(int n, int want) {
    const int cap = kCallBlocks / n > 1 ? kCallBlocks / n : 1;
    return want < cap ? want : cap;
}
int samples(int len, int step) { return (len - 1) / step + 1; }          // 0, step, 2 step, ... below len
int mom_blocks(int n, int h, int w, int step) {
    return blocks_per_field(n, sf::ceil_div(samples(h, step) * mom_units_per_row(samples(w, step)), kWaves));
}
int aff_blocks(int n, int h, int w) { return blocks_per_field(n, sf::ceil_div(h * ((w + 3) / 4), kBlock)); }
int64_t mom_partial_bytes(int n, int h, int w, int step) { return (int64_t)n * mom_blocks(n, h, w, step) * SF_MOT_LEN * (int64_t)sizeof(double); }

// the checks the moments pass and the chain share; fills the kernel's arguments
int moments_args(const char* who, const float* flows, int64_t field_stride, int64_t ch_stride, int64_t row_stride, int n, int h, int w,
                 const uint8_t* cls, uint8_t code_visible, uint8_t code_occluded, uint8_t code_outside, float w_visible, float w_occluded,
                 float w_outside, int step, float max_mag, MomArgs* a) {
    SF_REQUIRE(flows, "%s: null flows", who);
    SF_REQUIRE(h > 0 && w > 0, "%s: bad shape %d x %d", who, h, w);
    SF_REQUIRE((int64_t)h * w < (1 << 30), "%s: field %d x %d too large", who, h, w);
    SF_REQUIRE(n >= 1 && n <= 65535, "%s: %d fields in one call (1 .. 65535)", who, n);
    SF_REQUIRE(row_stride >= w && ch_stride != 0 && field_stride >= 0, "%s: bad flow strides (%lld, %lld, %lld)", who,
               (long long)field_stride, (long long)ch_stride, (long long)row_stride);
    SF_REQUIRE((reinterpret_cast<uintptr_t>(flows) & 3u) == 0, "%s: flows not 4-byte aligned", who);
    SF_REQUIRE(step >= 1, "%s: step = %d (>= 1)", who, step);
    SF_REQUIRE(max_mag >= 0.0f, "%s: max_mag is negative or NaN", who);
    SF_REQUIRE(w_visible >= 0.0f && w_occluded >= 0.0f && w_outside >= 0.0f && w_visible < __builtin_inff() &&
                   w_occluded < __builtin_inff() && w_outside < __builtin_inff(),
               "%s: a class weight is negative, infinite or NaN", who);
    a->flow = flows, a->cls = cls, a->model = nullptr, a->inv_c2 = nullptr;
    a->f_field = field_stride, a->f_ch = ch_stride, a->f_row = row_stride;
    a->h = h, a->w = w, a->step = step, a->hs = samples(h, step), a->wsm = samples(w, step);
    const int longest = w - 1 > h - 1 ? w - 1 : h - 1;
    a->max_mag = max_mag, a->cx = (float)(w - 1) * 0.5f, a->cy = (float)(h - 1) * 0.5f, a->s = 2.0f / (float)(longest > 1 ? longest : 1);
    a->wt_vis = w_visible, a->wt_occ = w_occluded, a->wt_out = w_outside;
    a->code_vis = code_visible, a->code_occ = code_occluded, a->code_out = code_outside;
    return SF_OK;
}

bool kind_ok(int kind) { return kind == SF_MOTION_TRANSLATION || kind == SF_MOTION_SIMILARITY || kind == SF_MOTION_AFFINE; }

}  // namespace

extern "C" int64_t sf_motion_moments_ws_bytes(int n, int h, int w, int step) {
    if (!shape_ok(n, h, w) || step < 1)
        return sf::fail(SF_ERR_BAD_ARG, "sf_motion_moments_ws_bytes: bad shape (%d fields of %d x %d, step %d)", n, h, w, step);
    return mom_partial_bytes(n, h, w, step);
}

extern "C" int64_t sf_motion_fit_ws_bytes(int n, int h, int w, int step) {
    if (!shape_ok(n, h, w) || step < 1)
        return sf::fail(SF_ERR_BAD_ARG, "sf_motion_fit_ws_bytes: bad shape (%d fields of %d x %d, step %d)", n, h, w, step);
    return mom_partial_bytes(n, h, w, step) + (int64_t)n * 8 * (int64_t)sizeof(float);       // + fp32 model [n][6], inv_c2 [n], padding
}

extern "C" int64_t sf_warp_affine_ws_bytes(int n, int h, int w) {
    if (!shape_ok(n, h, w)) return sf::fail(SF_ERR_BAD_ARG, "sf_warp_affine_ws_bytes: bad shape (%d frames of %d x %d)", n, h, w);
    return (int64_t)n * aff_blocks(n, h, w) * (int64_t)sizeof(unsigned);
}

extern "C" int sf_motion_moments(const float* flows, int64_t field_stride, int64_t ch_stride, int64_t row_stride, int n, int h, int w,
                                 const uint8_t* cls, uint8_t code_visible, uint8_t code_occluded, uint8_t code_outside, float w_visible,
                                 float w_occluded, float w_outside, int step, float max_mag, const float* model, const float* inv_c2,
                                 double* moments, void* ws, int64_t ws_bytes, void* stream) {
    MomArgs a;
    const int ok = moments_args("sf_motion_moments", flows, field_stride, ch_stride, row_stride, n, h, w, cls, code_visible, code_occluded,
                                code_outside, w_visible, w_occluded, w_outside, step, max_mag, &a);
    if (ok != SF_OK) return ok;
    SF_REQUIRE(moments && ws, "sf_motion_moments: null moments / ws");
    SF_REQUIRE((model == nullptr) == (inv_c2 == nullptr), "sf_motion_moments: model and inv_c2 come together (one of them is null)");
    SF_REQUIRE((reinterpret_cast<uintptr_t>(model) & 3u) == 0 && (reinterpret_cast<uintptr_t>(inv_c2) & 3u) == 0,
               "sf_motion_moments: model / inv_c2 not 4-byte aligned");
    SF_REQUIRE((reinterpret_cast<uintptr_t>(moments) & 7u) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0,
               "sf_motion_moments: moments / ws not 8-byte aligned");
    const int64_t need = mom_partial_bytes(n, h, w, step);
    SF_REQUIRE(ws_bytes >= need, "sf_motion_moments: workspace of %lld bytes (needs %lld)", (long long)ws_bytes, (long long)need);
    a.model = model, a.inv_c2 = inv_c2;
    const int nblocks = mom_blocks(n, h, w, step);
    hipStream_t s = (hipStream_t)stream;
    double* partials = static_cast<double*>(ws);
    hipLaunchKernelGGL(motion_moments_kernel, dim3(nblocks, n), dim3(kBlock), 0, s, a, partials);
    const int st = sf::check_launch("sf_motion_moments");
    if (st != SF_OK) return st;
    hipLaunchKernelGGL(motion_finish_kernel<false>, dim3(n), dim3(kBlock), 0, s, partials, nblocks, moments, (int64_t)SF_MOT_LEN, 0, 0.0, 0.0,
                       SolveOut{});
    return sf::check_launch("sf_motion_moments (finish)");
}

extern "C" int sf_motion_solve(const double* moments, int n, int kind, double kappa, double c_floor, double* model64, float* model32,
                               double* c, float* inv_c2, int32_t* status, void* stream) {
    SF_REQUIRE(moments && model64 && model32 && c && inv_c2 && status, "sf_motion_solve: null argument");
    SF_REQUIRE(n >= 1 && n <= 65535, "sf_motion_solve: %d fields in one call (1 .. 65535)", n);
    SF_REQUIRE(kind_ok(kind), "sf_motion_solve: unknown kind %d", kind);
    SF_REQUIRE(kappa >= 0.0 && c_floor > 0.0 && kappa < __builtin_inf() && c_floor < __builtin_inf(),
               "sf_motion_solve: kappa must be finite and >= 0, c_floor finite and > 0 (NaN included)");
    SF_REQUIRE((reinterpret_cast<uintptr_t>(moments) & 7u) == 0 && (reinterpret_cast<uintptr_t>(model64) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(c) & 7u) == 0,
               "sf_motion_solve: moments / model64 / c not 8-byte aligned");
    SF_REQUIRE((reinterpret_cast<uintptr_t>(model32) & 3u) == 0 && (reinterpret_cast<uintptr_t>(inv_c2) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(status) & 3u) == 0,
               "sf_motion_solve: model32 / inv_c2 / status not 4-byte aligned");
    SolveOut out{model64, model32, c, inv_c2, status, nullptr, 0};
    hipLaunchKernelGGL(motion_solve_kernel, dim3(sf::ceil_div(n, 64)), dim3(64), 0, (hipStream_t)stream, moments, n, kind, kappa, c_floor, out);
    return sf::check_launch("sf_motion_solve");
}

extern "C" int sf_motion_fit(const float* flows, int64_t field_stride, int64_t ch_stride, int64_t row_stride, int n, int h, int w,
                             const uint8_t* cls, uint8_t code_visible, uint8_t code_occluded, uint8_t code_outside, float w_visible,
                             float w_occluded, float w_outside, int step, float max_mag, int kind, int rounds, double kappa, double c_floor,
                             double* trace, void* ws, int64_t ws_bytes, void* stream) {
    MomArgs a;
    const int ok = moments_args("sf_motion_fit", flows, field_stride, ch_stride, row_stride, n, h, w, cls, code_visible, code_occluded,
                                code_outside, w_visible, w_occluded, w_outside, step, max_mag, &a);
    if (ok != SF_OK) return ok;
    SF_REQUIRE(trace && ws, "sf_motion_fit: null trace / ws");
    SF_REQUIRE(kind_ok(kind), "sf_motion_fit: unknown kind %d", kind);
    SF_REQUIRE(rounds >= 1 && rounds <= SF_MOT_MAX_ROUNDS, "sf_motion_fit: %d rounds (1 .. %d)", rounds, SF_MOT_MAX_ROUNDS);
    SF_REQUIRE(kappa >= 0.0 && c_floor > 0.0 && kappa < __builtin_inf() && c_floor < __builtin_inf(),
               "sf_motion_fit: kappa must be finite and >= 0, c_floor finite and > 0 (NaN included)");
    SF_REQUIRE((reinterpret_cast<uintptr_t>(trace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0,
               "sf_motion_fit: trace / ws not 8-byte aligned");
    const int64_t need = sf_motion_fit_ws_bytes(n, h, w, step);
    SF_REQUIRE(ws_bytes >= need, "sf_motion_fit: workspace of %lld bytes (needs %lld)", (long long)ws_bytes, (long long)need);
    const int nblocks = mom_blocks(n, h, w, step);
    hipStream_t s = (hipStream_t)stream;
    double* partials = static_cast<double*>(ws);
    float* model32 = reinterpret_cast<float*>(static_cast<char*>(ws) + mom_partial_bytes(n, h, w, step));
    float* inv_c2 = model32 + (int64_t)n * 6;
    const int64_t field_doubles = (int64_t)rounds * SF_MOT_TRACE_LEN;
    for (int r = 0; r < rounds; ++r) {
        a.model = r ? model32 : nullptr, a.inv_c2 = r ? inv_c2 : nullptr;
        hipLaunchKernelGGL(motion_moments_kernel, dim3(nblocks, n), dim3(kBlock), 0, s, a, partials);
        int st = sf::check_launch("sf_motion_fit (moments)");
        if (st != SF_OK) return st;
        double* row = trace + (int64_t)r * SF_MOT_TRACE_LEN;             // round r of field 0
        SolveOut out{nullptr, model32, nullptr, inv_c2, nullptr, row, field_doubles};
        hipLaunchKernelGGL(motion_finish_kernel<true>, dim3(n), dim3(kBlock), 0, s, partials, nblocks, row + SF_MOT_TRACE_MOMENTS,
                           field_doubles, kind, kappa, c_floor, out);
        st = sf::check_launch("sf_motion_fit (finish + solve)");
        if (st != SF_OK) return st;
    }
    return SF_OK;
}

extern "C" int sf_warp_affine_u8(const uint8_t* src, int64_t src_frame_stride, int64_t src_row_stride, int64_t src_px_stride,
                                 int64_t src_ch_stride, const float* inv_maps, int n, int h, int w, int border, uint8_t fill0,
                                 uint8_t fill1, uint8_t fill2, uint8_t* out, uint32_t* outside, void* ws, int64_t ws_bytes, void* stream) {
    SF_REQUIRE(src && inv_maps && out && outside && ws, "sf_warp_affine_u8: null argument");
    SF_REQUIRE(h > 0 && w > 0, "sf_warp_affine_u8: bad shape %d x %d", h, w);
    SF_REQUIRE((int64_t)h * w < (1 << 30), "sf_warp_affine_u8: frame %d x %d too large", h, w);
    SF_REQUIRE(n >= 1 && n <= 65535, "sf_warp_affine_u8: %d frames in one call (1 .. 65535)", n);
    SF_REQUIRE(src_frame_stride >= 0 && src_row_stride >= 0 && src_px_stride >= 0 && src_ch_stride >= 0,
               "sf_warp_affine_u8: negative source stride (%lld, %lld, %lld, %lld)", (long long)src_frame_stride, (long long)src_row_stride,
               (long long)src_px_stride, (long long)src_ch_stride);
    SF_REQUIRE(border == SF_BORDER_CONSTANT || border == SF_BORDER_REPLICATE, "sf_warp_affine_u8: unknown border mode %d", border);
    SF_REQUIRE((reinterpret_cast<uintptr_t>(inv_maps) & 3u) == 0 && (reinterpret_cast<uintptr_t>(outside) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(ws) & 3u) == 0,
               "sf_warp_affine_u8: inv_maps / outside / ws not 4-byte aligned");
    const int64_t need = sf_warp_affine_ws_bytes(n, h, w);
    SF_REQUIRE(ws_bytes >= need, "sf_warp_affine_u8: workspace of %lld bytes (needs %lld)", (long long)ws_bytes, (long long)need);
    AffArgs a;
    a.src = src, a.maps = inv_maps;
    a.s_frame = src_frame_stride, a.s_row = src_row_stride, a.s_px = src_px_stride, a.s_ch = src_ch_stride;
    a.h = h, a.w = w, a.border = border, a.fill0 = fill0, a.fill1 = fill1, a.fill2 = fill2;
    // a group's twelve bytes start at 3 (y w + x0): whole words when w is a multiple of four and the dense output is word-aligned
    a.vec_store = w % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
    const int nblocks = aff_blocks(n, h, w);
    hipStream_t s = (hipStream_t)stream;
    unsigned* partials = static_cast<unsigned*>(ws);
    hipLaunchKernelGGL(warp_affine_kernel, dim3(nblocks, n), dim3(kBlock), 0, s, a, out, partials);
    const int st = sf::check_launch("sf_warp_affine_u8");
    if (st != SF_OK) return st;
    hipLaunchKernelGGL(warp_affine_finish_kernel, dim3(n), dim3(kBlock), 0, s, partials, nblocks, outside);
    return sf::check_launch("sf_warp_affine_u8 (finish)");
}
