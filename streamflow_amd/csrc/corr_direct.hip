// Correlation lookup WITHOUT the all-pairs volume: pack (once per clip) and on-demand radius-4 lookup (every iteration).
//
// Reference: core/corr.py:7-21,46-54 (volume + avg-pool pyramid), :23-44 (lookup).  Pooling is linear, so level l of the volume
// at target cell J is <f1_i, pool_l(f2)_J> / sqrt(D) with pool_l the floor 2 x 2 mean applied l times to the FEATURES of frame 2:
// nothing that grows with N^2 has to be stored.  The pack keeps f1 and the four-level feature pyramid of f2 in the operand
// format of the matrix cores; the lookup computes the cells a pixel's 10 x 10 windows touch and blends them at once.
//
// WORKSPACE (per image img = b * pairs + t, images back to back, each img_bytes = parts * (Dp / 8) * 16 * (2 N + N1 + N2 + N3)):
//     region 0: f1            region 1 + l: level l of pool(f2), Nl = (h >> l) * (w >> l) cells, row-major (y * (w >> l) + x)
//     region   = [part][k-octet][cell][8] fp16: part 0 = the rounded value (F16) or hi of split8() (F16X3), part 1 = lo (F16X3 only);
//                Dp = D rounded up to 32, the rows D .. Dp - 1 are zero.
// A lane's MFMA fragment (8 consecutive k of one pixel / cell) is one 16-byte piece: both operands go from L2 straight into
// registers, no LDS staging.
//
// LOOKUP.  A workgroup of four waves takes 16 consecutive source pixels (the M side of v_mfma_f32_16x16x32_f16; their f1
// fragments stay in registers for the whole kernel).  Per level it takes the bounding box of the pixels' windows clipped to the
// level and walks it in chunks of 16 cells (the N side), a wave per chunk; a chunk no pixel of the tile needs is skipped before
// its k-loop.  Of a chunk's 16 x 16 products a lane keeps those that fall into its pixels' own windows: W[pixel][level][10 x 10]
// in LDS, zero wherever the level ends.  Then 16 x 324 bilinear blends read W.
// THE SUMMATION ORDER of a cell is fixed: k-steps of 32 in ascending order (hi * hi, hi * lo, lo * hi per step in the split
// class), one accumulator, the scale 1 / sqrt(D) once at the end.  Row i of an MFMA result depends on row i of A and column j
// of B only, so a pixel's 324 values depend on its own features and coordinates alone -- not on the box, the chunking, its
// neighbours or the batch (tests/test_gpu_corr_direct.py asserts this bitwise).
#include "sf_common.h"
#include "split_operand.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int TP = 16;                 // source pixels per workgroup
constexpr int kThreads = 256;
constexpr int NCH = 324, NOCT = 41, TROW = NOCT * 8;
constexpr int WIN = 10, WCELLS = WIN * WIN;

struct Geom {
    int h, w, N, D, Dp;
    int nl[4];                         // cells per level
    int64_t reg_off[5];                // byte offset of region r inside an image
    int64_t img_bytes;
    int parts;
};

Geom make_geom(int D, int h, int w, int precision) {
    Geom g;
    g.h = h; g.w = w; g.N = h * w; g.D = D; g.Dp = (D + 31) / 32 * 32;
    g.parts = precision == SF_PRECISION_F16X3 ? 2 : 1;
    const int64_t cell = (int64_t)g.parts * (g.Dp / 8) * 16;         // bytes per cell over all parts and k-octets
    int64_t o = 0;
    g.reg_off[0] = 0;
    o += cell * g.N;
    for (int l = 0; l < 4; ++l) {
        g.nl[l] = (h >> l) * (w >> l);
        g.reg_off[1 + l] = o;
        o += cell * g.nl[l];
    }
    g.img_bytes = o;
    return g;
}

// ------------------------------------------------------------------------------------------------
// pack
// ------------------------------------------------------------------------------------------------
// level L of one feature plane (width w at level 0): fp32 from the fp32 level below, vertical pair, horizontal pair, times 0.25
template <int L>
__device__ __forceinline__ float pooled(const float* f, int w, int y, int x) {
    if constexpr (L == 0) {
        return f[(int64_t)y * w + x];
    } else {
        const float v0 = pooled<L - 1>(f, w, 2 * y, 2 * x) + pooled<L - 1>(f, w, 2 * y + 1, 2 * x);
        const float v1 = pooled<L - 1>(f, w, 2 * y, 2 * x + 1) + pooled<L - 1>(f, w, 2 * y + 1, 2 * x + 1);
        return 0.25f * (v0 + v1);
    }
}

struct PackArgs {
    const float* f1;
    const float* f2;
    int64_t f_clip_stride, f_pair_stride;
    char* ws;
    int pairs;
    Geom g;
};

// grid: x = cells of the five regions (2 N + N1 + N2 + N3) in blocks of 256, y = k-octet, z = image
template <bool kSplit>
__global__ __launch_bounds__(256) void corr_direct_pack_kernel(const PackArgs a) {
    const Geom& g = a.g;
    int c = blockIdx.x * 256 + threadIdx.x;
    const int kq = blockIdx.y, img = blockIdx.z;
    int region = 0, n = g.N;
    if (c >= n) {
        c -= n;
        for (region = 1; region < 5; ++region) {
            n = g.nl[region - 1];
            if (c < n) break;
            c -= n;
        }
        if (region == 5) return;
    }
    const int64_t fo = (int64_t)(img / a.pairs) * a.f_clip_stride + (int64_t)(img % a.pairs) * a.f_pair_stride;
    const float* f = (region == 0 ? a.f1 : a.f2) + fo;
    float v[8];
    const int l = region == 0 ? 0 : region - 1, wl = g.w >> l;
    const int y = c / wl, x = c % wl;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = kq * 8 + i;
        float r = 0.f;
        if (k < g.D) {
            const float* p = f + (int64_t)k * g.N;
            r = l == 0 ? pooled<0>(p, g.w, y, x) : l == 1 ? pooled<1>(p, g.w, y, x) : l == 2 ? pooled<2>(p, g.w, y, x) : pooled<3>(p, g.w, y, x);
        }
        v[i] = r;
    }
    char* o = a.ws + (int64_t)img * g.img_bytes + g.reg_off[region];
    const int64_t part = (int64_t)(g.Dp / 8) * n * 16, at = ((int64_t)kq * n + c) * 16;
    if constexpr (kSplit) {
        const sf_split::Split8 s = sf_split::split8(v);
        *reinterpret_cast<f16x8*>(o + at) = s.hi;
        *reinterpret_cast<f16x8*>(o + part + at) = s.lo;
    } else {
        f16x8 hv;
#pragma unroll
        for (int i = 0; i < 8; ++i) hv[i] = (_Float16)v[i];
        *reinterpret_cast<f16x8*>(o + at) = hv;
    }
}

// ------------------------------------------------------------------------------------------------
// lookup
// ------------------------------------------------------------------------------------------------
struct LookArgs {
    const char* ws;
    const float* coords;
    float* out;                   // optional fp32 planes [324][N] per image
    int64_t out_img_stride;
    _Float16* out16;              // optional k-octet planes [41][N][8] per image
    int64_t out16_img_stride;     // halves
    float scale;
    Geom g;
};

// KS = Dp / 32 k-steps; kSplit: three products per step
template <int KS, bool kSplit>
__global__ __launch_bounds__(kThreads) void corr_direct_lookup_kernel(const LookArgs a) {
    __shared__ float W[TP * 4 * WCELLS];                              // [pixel][level][dy][dx]
    __shared__ __attribute__((aligned(16))) _Float16 T[TP * TROW];    // fp16 results, [pixel][328]
    __shared__ int X0[4][TP], Y0[4][TP];                              // first window column / row (floor - 4)
    __shared__ float FX[4][TP], FY[4][TP];
    const Geom& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int img = blockIdx.y, p0 = blockIdx.x * TP;
    const char* const wsi = a.ws + (int64_t)img * g.img_bytes;

    if (tid < TP) {
        const int p = p0 + tid;
        const bool live = p < g.N;
        const int pc = live ? p : g.N - 1;
        const float cx0 = a.coords[((int64_t)img * 2 + 0) * g.N + pc], cy0 = a.coords[((int64_t)img * 2 + 1) * g.N + pc];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const float inv = 1.0f / (float)(1 << l);
            float cx = cx0 * inv, cy = cy0 * inv;
            // anything this far out samples only zero padding; also swallows NaN / inf
            if (!(cx > -1.0e6f && cx < 1.0e6f) || !live) cx = -1.0e6f;
            if (!(cy > -1.0e6f && cy < 1.0e6f) || !live) cy = -1.0e6f;
            const float fx0 = floorf(cx), fy0 = floorf(cy);
            X0[l][tid] = (int)fx0 - 4; Y0[l][tid] = (int)fy0 - 4;
            FX[l][tid] = cx - fx0; FY[l][tid] = cy - fy0;
        }
    }
    for (int i = tid; i < TP * 4 * WCELLS; i += kThreads) W[i] = 0.f;
    if (tid < TP) *reinterpret_cast<unsigned long long*>(T + tid * TROW + NCH) = 0ull;      // rows 324..327 of the last octet

    // the tile's f1 fragments: lane = (pixel lane & 15, k-octet lane >> 4 of every step)
    const int q = lane >> 4, j16 = lane & 15;
    f16x8 ah[KS], al[KS];
    {
        const int px = min(p0 + j16, g.N - 1);
        const int64_t part = (int64_t)(g.Dp / 8) * g.N * 16;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const char* p = wsi + ((int64_t)(ks * 4 + q) * g.N + px) * 16;
            ah[ks] = *reinterpret_cast<const f16x8*>(p);
            if constexpr (kSplit) al[ks] = *reinterpret_cast<const f16x8*>(p + part);
        }
    }
    __syncthreads();

    for (int l = 0; l < 4; ++l) {
        const int hl = g.h >> l, wl = g.w >> l, nl = g.nl[l];
        // bounding box of the tile's windows, clipped to the level (every thread computes the same)
        int bx0 = wl, bx1 = -1, by0 = hl, by1 = -1;
        for (int i = 0; i < TP; ++i) {
            const int lx = max(X0[l][i], 0), hx = min(X0[l][i] + WIN - 1, wl - 1);
            const int ly = max(Y0[l][i], 0), hy = min(Y0[l][i] + WIN - 1, hl - 1);
            if (lx <= hx && ly <= hy) {
                bx0 = min(bx0, lx); bx1 = max(bx1, hx);
                by0 = min(by0, ly); by1 = max(by1, hy);
            }
        }
        if (bx1 < bx0) continue;                                      // workgroup-uniform: no window reaches this level
        const int bw = bx1 - bx0 + 1, ncell = bw * (by1 - by0 + 1), nchunk = (ncell + 15) / 16;
        // the lane's four pixels of the C/D layout: rows 4 q + r, column = cell j16 of the chunk
        int wx[4], wy[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { wx[r] = X0[l][4 * q + r]; wy[r] = Y0[l][4 * q + r]; }
        const char* const lvl = wsi + g.reg_off[1 + l];
        const int64_t part = (int64_t)(g.Dp / 8) * nl * 16;
        for (int ch = wave; ch < nchunk; ch += kThreads / 64) {
            const int j = ch * 16 + j16;
            const bool inbox = j < ncell;
            const int cy = by0 + (inbox ? j / bw : 0), cx = bx0 + (inbox ? j % bw : 0);
            int wi[4];
            bool any = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int dx = cx - wx[r], dy = cy - wy[r];
                const bool need = inbox & ((unsigned)dx < (unsigned)WIN) & ((unsigned)dy < (unsigned)WIN);
                wi[r] = need ? ((4 * q + r) * 4 + l) * WCELLS + dy * WIN + dx : -1;
                any |= need;
            }
            if (__builtin_amdgcn_ballot_w64(any) == 0) continue;      // wave-uniform
            const char* const cp = lvl + ((int64_t)q * nl + (int64_t)cy * wl + cx) * 16;     // inside the level by construction
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const char* p = cp + (int64_t)ks * 4 * nl * 16;
                const f16x8 bh = *reinterpret_cast<const f16x8*>(p);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[ks], bh, acc, 0, 0, 0);
                if constexpr (kSplit) {
                    const f16x8 bl = *reinterpret_cast<const f16x8*>(p + part);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[ks], bl, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[ks], bh, acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (wi[r] >= 0) W[wi[r]] = acc[r] * a.scale;
        }
    }
    __syncthreads();

    // ---- blend: item = (channel, pixel), the pixel fastest (64-byte runs of the fp32 planes) ----
    for (int it = tid; it < NCH * TP; it += kThreads) {
        const int i = it & (TP - 1), chn = it >> 4;
        const int l = chn / 81, ab = chn - l * 81, wa = ab / 9, wb = ab - wa * 9;       // channel = l * 81 + a * 9 + b: a moves x
        const float* c = W + (i * 4 + l) * WCELLS + wb * WIN + wa;
        const float wy1 = FY[l][i], wy0 = 1.f - wy1, wx1 = FX[l][i], wx0 = 1.f - wx1;
        const float v0 = c[0] * wy0 + c[WIN] * wy1, v1 = c[1] * wy0 + c[WIN + 1] * wy1;
        const float R = v0 * wx0 + v1 * wx1;
        if (p0 + i < g.N) {
            if (a.out != nullptr) a.out[(int64_t)img * a.out_img_stride + (int64_t)chn * g.N + p0 + i] = R;
            T[i * TROW + chn] = (_Float16)R;
        }
    }
    if (a.out16 == nullptr) return;                                   // workgroup-uniform
    __syncthreads();
    _Float16* o16 = a.out16 + (int64_t)img * a.out16_img_stride;
    for (int it = tid; it < NOCT * TP; it += kThreads) {
        const int i = it & (TP - 1), oc = it >> 4;
        if (p0 + i >= g.N) continue;
        const u32x4 v = *reinterpret_cast<const u32x4*>(T + i * TROW + oc * 8);
        *reinterpret_cast<u32x4*>(o16 + ((int64_t)oc * g.N + p0 + i) * 8) = v;
    }
}

template <bool kSplit>
void launch_lookup(int ks, dim3 grid, hipStream_t st, const LookArgs& a) {
    switch (ks) {
        case 1: hipLaunchKernelGGL((corr_direct_lookup_kernel<1, kSplit>), grid, dim3(kThreads), 0, st, a); break;
        case 2: hipLaunchKernelGGL((corr_direct_lookup_kernel<2, kSplit>), grid, dim3(kThreads), 0, st, a); break;
        case 3: hipLaunchKernelGGL((corr_direct_lookup_kernel<3, kSplit>), grid, dim3(kThreads), 0, st, a); break;
        case 4: hipLaunchKernelGGL((corr_direct_lookup_kernel<4, kSplit>), grid, dim3(kThreads), 0, st, a); break;
        case 5: hipLaunchKernelGGL((corr_direct_lookup_kernel<5, kSplit>), grid, dim3(kThreads), 0, st, a); break;
        case 6: hipLaunchKernelGGL((corr_direct_lookup_kernel<6, kSplit>), grid, dim3(kThreads), 0, st, a); break;
        case 7: hipLaunchKernelGGL((corr_direct_lookup_kernel<7, kSplit>), grid, dim3(kThreads), 0, st, a); break;
        default: hipLaunchKernelGGL((corr_direct_lookup_kernel<8, kSplit>), grid, dim3(kThreads), 0, st, a); break;
    }
}

int check_common(const char* who, int B, int pairs, int D, int h, int w, int precision) {
    if (precision != SF_PRECISION_F16 && precision != SF_PRECISION_F16X3)
        return sf::fail(SF_ERR_UNSUPPORTED, "%s: precision %d (SF_PRECISION_F16 or SF_PRECISION_F16X3 only)", who, precision);
    SF_REQUIRE(B > 0 && pairs > 0 && D > 0 && h > 0 && w > 0, "%s: bad dims", who);
    SF_REQUIRE((h >> 3) >= 1 && (w >> 3) >= 1, "%s: feature grid %dx%d too small for 4 levels", who, h, w);
    if (D > 256) return sf::fail(SF_ERR_UNSUPPORTED, "%s: feature depth %d > 256 (the tile's f1 fragments stay in registers)", who, D);
    SF_REQUIRE((int64_t)h * w < ((int64_t)1 << 26), "%s: feature grid %dx%d too large", who, h, w);
    SF_REQUIRE((int64_t)B * pairs <= 65535, "%s: B*pairs too large", who);
    return SF_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" int64_t sf_corr_direct_ws_bytes(int B, int pairs, int D, int h, int w, int precision) {
    if (B <= 0 || pairs <= 0 || D <= 0 || h < 8 || w < 8) return 0;
    if (precision != SF_PRECISION_F16 && precision != SF_PRECISION_F16X3) return 0;
    return (int64_t)B * pairs * make_geom(D, h, w, precision).img_bytes;
}

extern "C" int sf_corr_direct_pack(const float* f1, const float* f2, int64_t f_clip_stride, int64_t f_pair_stride,
                                   void* ws, int64_t ws_bytes, int B, int pairs, int D, int h, int w, int precision,
                                   void* stream) {
    if (int e = check_common("sf_corr_direct_pack", B, pairs, D, h, w, precision)) return e;
    SF_REQUIRE(f1 && f2 && ws, "sf_corr_direct_pack: null pointer");
    SF_REQUIRE(ws_bytes >= sf_corr_direct_ws_bytes(B, pairs, D, h, w, precision) && (reinterpret_cast<uintptr_t>(ws) & 15) == 0,
               "sf_corr_direct_pack: needs a 16-byte aligned workspace of sf_corr_direct_ws_bytes() bytes");
    PackArgs a;
    a.f1 = f1; a.f2 = f2; a.f_clip_stride = f_clip_stride; a.f_pair_stride = f_pair_stride;
    a.ws = static_cast<char*>(ws);
    a.pairs = pairs;
    a.g = make_geom(D, h, w, precision);
    const int cells = 2 * a.g.N + a.g.nl[1] + a.g.nl[2] + a.g.nl[3];
    const dim3 grid(sf::ceil_div(cells, 256), a.g.Dp / 8, B * pairs);
    if (precision == SF_PRECISION_F16X3) hipLaunchKernelGGL(corr_direct_pack_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(corr_direct_pack_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return sf::check_launch("sf_corr_direct_pack");
}

extern "C" int sf_corr_direct_lookup(const void* ws, const float* coords, float* out, int64_t out_img_stride,
                                     void* out_koct, int64_t out_koct_img_stride, int B, int pairs, int D, int h, int w,
                                     int precision, void* stream) {
    if (int e = check_common("sf_corr_direct_lookup", B, pairs, D, h, w, precision)) return e;
    SF_REQUIRE(ws && coords && (out || out_koct), "sf_corr_direct_lookup: null pointer");
    SF_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "sf_corr_direct_lookup: ws must be 16-byte aligned");
    SF_REQUIRE(!out_koct || ((reinterpret_cast<uintptr_t>(out_koct) & 15) == 0 && (out_koct_img_stride & 7) == 0),
               "sf_corr_direct_lookup: out_koct must be 16-byte aligned, its stride a multiple of 8 halves");
    LookArgs a;
    a.ws = static_cast<const char*>(ws);
    a.coords = coords;
    a.out = out; a.out_img_stride = out_img_stride;
    a.out16 = static_cast<_Float16*>(out_koct); a.out16_img_stride = out_koct_img_stride;
    a.scale = 1.0f / sqrtf((float)D);
    a.g = make_geom(D, h, w, precision);
    const dim3 grid(sf::ceil_div(a.g.N, TP), B * pairs);
    if (precision == SF_PRECISION_F16X3) launch_lookup<true>(a.g.Dp / 32, grid, (hipStream_t)stream, a);
    else launch_lookup<false>(a.g.Dp / 32, grid, (hipStream_t)stream, a);
    return sf::check_launch("sf_corr_direct_lookup");
}
