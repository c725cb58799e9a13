// Separable resampling of uint8 frames and fp32 flow planes with caller-built coefficient tables (include/streamflow_hip.h,
// "resize", has the contract).
//
// sf_resize_u8 is Pillow's ImagingResample for 8-bit images restated: per axis a table of (first tap, tap count) and of
// coefficients scaled by 2^22; a horizontal pass (only if w != W) into a uint8 intermediate, then a vertical pass (only if h != H);
// each pass computes ss = 2^21 + sum(pixel * k) in 32-bit integers and stores clamp(ss >> 22, 0, 255).  Everything is integer, so a
// numpy restatement reproduces every byte (tests/resize_cases.py), and that restatement is bitwise PIL.Image.resize.
// sf_resize_f32 is the same two passes on fp32 planes with fp32 tables: products and sums rounded one by one in tap order (FMA
// contraction is off for this file), an fp32 intermediate, and one multiply by sx (channel 0) / sy (channel 1) on the final store.
//
// Launches: one per pass (the work is memory-bound), or one copy launch when neither axis changes.
//   horizontal: a block owns 64 output columns for kRowsPerBlock rows.  It stages its 64 rows of the coefficient table in LDS (they
//     are contiguous in the table: one coalesced copy); a thread owns one output pixel (u8: its three channels) and reads its
//     coefficients at a stride of ksize dwords, which is odd (2 ceil(support) + 1): no bank conflicts.
//   vertical: a block owns one output row, so first tap, tap count and coefficients are wave-uniform (scalar loads).  u8: a thread
//     owns four consecutive bytes of the packed 3 w-byte row; the taps are dword loads from consecutive source rows where the source
//     is packed, 3 w % 4 == 0 and every base is 4-byte aligned, byte accesses otherwise (also for a strided source, which the
//     vertical pass reads directly when there is no horizontal pass).  f32: a thread owns one element.
//
// Addressing: no address depends on pixel data.  The only data-dependent indices come from the tables: first tap + i, clamped into
// [0, size - 1] here, and the tap count, clamped into [0, ksize].  A wrong table gives wrong pixels and nothing else.  The integer
// sums are formed in unsigned arithmetic (wrap-around, no undefined overflow for a wrong table) and read back as signed.
#include "sf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kCols = 64;                                                // output columns of a horizontal block: one per lane
constexpr int kRowsPerBlock = 16;                                        // rows a horizontal block walks (4 at a time)
constexpr int kPrecision = 22;                                           // Pillow's PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ unsigned clip8(unsigned acc) {
    const int ss = (int)acc >> kPrecision;
    return (unsigned)clampi(ss, 0, 255);
}

// the block's rows x0 .. x0 + ncol - 1 of a [out][ksize] table and of the [out][2] bounds, as raw dwords
__device__ __forceinline__ void stage_tables(const uint32_t* __restrict__ k, const int* __restrict__ bounds, int x0, int ncol, int ksize,
                                             uint32_t* s_k, int* s_b) {
    const uint32_t* src = k + (int64_t)x0 * ksize;
    for (int i = threadIdx.x; i < ncol * ksize; i += kBlock) s_k[i] = src[i];
    for (int i = threadIdx.x; i < ncol * 2; i += kBlock) s_b[i] = bounds[(int64_t)x0 * 2 + i];
    __syncthreads();
}

struct SrcU8 {
    const uint8_t* p;
    int64_t fs, rs, ps, cs;                                              // bytes: frame, row, pixel, channel
};

// dst: packed [n][rows][w][3]
__global__ __launch_bounds__(kBlock) void resize_h_u8_kernel(SrcU8 s, int rows, int W, int w, const int* __restrict__ bounds,
                                                             const int* __restrict__ k, int ksize, uint8_t* __restrict__ dst, int cblocks) {
    extern __shared__ uint32_t smem[];
    uint32_t* s_k = smem;
    int* s_b = reinterpret_cast<int*>(smem + kCols * ksize);
    const int cb = blockIdx.x % cblocks, rb = blockIdx.x / cblocks, f = blockIdx.y;
    const int x0 = cb * kCols;
    const int ncol = w - x0 < kCols ? w - x0 : kCols;
    stage_tables(reinterpret_cast<const uint32_t*>(k), bounds, x0, ncol, ksize, s_k, s_b);
    const int col = threadIdx.x & 63;
    if (col >= ncol) return;
    const int first = s_b[2 * col], cnt = clampi(s_b[2 * col + 1], 0, ksize);
    const uint32_t* kc = s_k + col * ksize;
    const int y_end = (rb + 1) * kRowsPerBlock < rows ? (rb + 1) * kRowsPerBlock : rows;
    for (int y = rb * kRowsPerBlock + (threadIdx.x >> 6); y < y_end; y += kBlock / 64) {
        const uint8_t* __restrict__ row = s.p + (int64_t)f * s.fs + (int64_t)y * s.rs;
        unsigned a0 = 1u << (kPrecision - 1), a1 = a0, a2 = a0;
        for (int i = 0; i < cnt; ++i) {
            const int xi = clampi(first + i, 0, W - 1);
            const unsigned c = kc[i];
            const uint8_t* px = row + (int64_t)xi * s.ps;
            a0 += (unsigned)px[0] * c;
            a1 += (unsigned)px[s.cs] * c;
            a2 += (unsigned)px[2 * s.cs] * c;
        }
        uint8_t* d = dst + (((int64_t)f * rows + y) * w + x0 + col) * 3;
        d[0] = (uint8_t)clip8(a0), d[1] = (uint8_t)clip8(a1), d[2] = (uint8_t)clip8(a2);
    }
}

// out: packed [n][h][R = 3 w]; a thread owns the bytes b0 .. b0 + 3 of a row.  fast: dword loads and stores (wave-uniform flag)
__global__ __launch_bounds__(kBlock) void resize_v_u8_kernel(SrcU8 s, int H, int R, int h, const int* __restrict__ bounds,
                                                             const int* __restrict__ k, int ksize, uint8_t* __restrict__ out, int cblocks,
                                                             int fast) {
    const int cb = blockIdx.x % cblocks, y = blockIdx.x / cblocks, f = blockIdx.y;
    const int first = bounds[2 * y], cnt = clampi(bounds[2 * y + 1], 0, ksize);
    const int* __restrict__ ky = k + (int64_t)y * ksize;
    const int b0 = (cb * kBlock + (int)threadIdx.x) * 4;
    if (b0 >= R) return;
    const uint8_t* __restrict__ base = s.p + (int64_t)f * s.fs;
    uint8_t* d = out + ((int64_t)f * h + y) * R + b0;
    unsigned a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = 1u << (kPrecision - 1);
    if (fast) {                                                          // packed source, R % 4 == 0, every base 4-byte aligned
        for (int i = 0; i < cnt; ++i) {
            const int yi = clampi(first + i, 0, H - 1);
            const unsigned c = (unsigned)ky[i];
            const unsigned v = *reinterpret_cast<const uint32_t*>(base + (int64_t)yi * s.rs + b0);
            a[0] += (v & 255u) * c;
            a[1] += ((v >> 8) & 255u) * c;
            a[2] += ((v >> 16) & 255u) * c;
            a[3] += (v >> 24) * c;
        }
        *reinterpret_cast<uint32_t*>(d) = clip8(a[0]) | (clip8(a[1]) << 8) | (clip8(a[2]) << 16) | (clip8(a[3]) << 24);
        return;
    }
    const int nb = R - b0 < 4 ? R - b0 : 4;
    int64_t off[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int b = b0 + (j < nb ? j : 0);                             // (bytes past the row repeat the first: computed, not stored)
        const int x = b / 3;
        off[j] = (int64_t)x * s.ps + (int64_t)(b - 3 * x) * s.cs;
    }
    for (int i = 0; i < cnt; ++i) {
        const int yi = clampi(first + i, 0, H - 1);
        const unsigned c = (unsigned)ky[i];
        const uint8_t* __restrict__ row = base + (int64_t)yi * s.rs;
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] += (unsigned)row[off[j]] * c;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < nb) d[j] = (uint8_t)clip8(a[j]);
}

// neither axis changes: the frames into the packed layout, a thread per pixel
__global__ __launch_bounds__(kBlock) void resize_copy_u8_kernel(SrcU8 s, int h, int w, uint8_t* __restrict__ out, int cblocks) {
    const int cb = blockIdx.x % cblocks, y = blockIdx.x / cblocks, f = blockIdx.y;
    const int x = cb * kBlock + (int)threadIdx.x;
    if (x >= w) return;
    const uint8_t* px = s.p + (int64_t)f * s.fs + (int64_t)y * s.rs + (int64_t)x * s.ps;
    uint8_t* d = out + (((int64_t)f * h + y) * w + x) * 3;
    d[0] = px[0], d[1] = px[s.cs], d[2] = px[2 * s.cs];
}

struct SrcF32 {
    const float* p;
    int64_t fs, cs, rs;                                                  // floats: field, channel, row
};

__device__ __forceinline__ const float* plane_of(const SrcF32& s, int pl) { return s.p + (int64_t)(pl >> 1) * s.fs + (int64_t)(pl & 1) * s.cs; }

// dst: dense [planes][rows][w]; scale: applied when this pass is the last one (1 otherwise is NOT applied: `last` says which)
__global__ __launch_bounds__(kBlock) void resize_h_f32_kernel(SrcF32 s, int rows, int W, int w, const int* __restrict__ bounds,
                                                              const float* __restrict__ k, int ksize, float* __restrict__ dst, int cblocks,
                                                              int last, float sx, float sy) {
    extern __shared__ uint32_t smem[];
    uint32_t* s_k = smem;
    int* s_b = reinterpret_cast<int*>(smem + kCols * ksize);
    const int cb = blockIdx.x % cblocks, rb = blockIdx.x / cblocks, pl = blockIdx.y;
    const int x0 = cb * kCols;
    const int ncol = w - x0 < kCols ? w - x0 : kCols;
    stage_tables(reinterpret_cast<const uint32_t*>(k), bounds, x0, ncol, ksize, s_k, s_b);
    const int col = threadIdx.x & 63;
    if (col >= ncol) return;
    const int first = s_b[2 * col], cnt = clampi(s_b[2 * col + 1], 0, ksize);
    const float* kc = reinterpret_cast<const float*>(s_k) + col * ksize;
    const float* __restrict__ src = plane_of(s, pl);
    const float sc = (pl & 1) ? sy : sx;
    const int y_end = (rb + 1) * kRowsPerBlock < rows ? (rb + 1) * kRowsPerBlock : rows;
    for (int y = rb * kRowsPerBlock + (threadIdx.x >> 6); y < y_end; y += kBlock / 64) {
        const float* __restrict__ row = src + (int64_t)y * s.rs;
        float acc = 0.0f;
        for (int i = 0; i < cnt; ++i) acc += row[clampi(first + i, 0, W - 1)] * kc[i];
        dst[((int64_t)pl * rows + y) * w + x0 + col] = last ? acc * sc : acc;
    }
}

// out: dense [planes][h][w]; always the last pass
__global__ __launch_bounds__(kBlock) void resize_v_f32_kernel(SrcF32 s, int H, int w, int h, const int* __restrict__ bounds,
                                                              const float* __restrict__ k, int ksize, float* __restrict__ out, int cblocks,
                                                              float sx, float sy) {
    const int cb = blockIdx.x % cblocks, y = blockIdx.x / cblocks, pl = blockIdx.y;
    const int x = cb * kBlock + (int)threadIdx.x;
    if (x >= w) return;
    const int first = bounds[2 * y], cnt = clampi(bounds[2 * y + 1], 0, ksize);
    const float* __restrict__ ky = k + (int64_t)y * ksize;
    const float* __restrict__ src = plane_of(s, pl);
    float acc = 0.0f;
    for (int i = 0; i < cnt; ++i) acc += src[(int64_t)clampi(first + i, 0, H - 1) * s.rs + x] * ky[i];
    out[((int64_t)pl * h + y) * w + x] = acc * ((pl & 1) ? sy : sx);
}

// neither axis changes: the planes into the dense layout, scaled
__global__ __launch_bounds__(kBlock) void resize_copy_f32_kernel(SrcF32 s, int h, int w, float* __restrict__ out, int cblocks, float sx,
                                                                 float sy) {
    const int cb = blockIdx.x % cblocks, y = blockIdx.x / cblocks, pl = blockIdx.y;
    const int x = cb * kBlock + (int)threadIdx.x;
    if (x >= w) return;
    out[((int64_t)pl * h + y) * w + x] = plane_of(s, pl)[(int64_t)y * s.rs + x] * ((pl & 1) ? sy : sx);
}

bool sizes_ok(int H, int W, int h, int w) {
    return H > 0 && W > 0 && h > 0 && w > 0 && (int64_t)H * W < (1 << 30) && (int64_t)h * w < (1 << 30) && (int64_t)H * w < (1 << 30);
}

size_t h_lds_bytes(int ksize) { return (size_t)(kCols * ksize + kCols * 2) * sizeof(uint32_t); }

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" int64_t sf_resize_u8_ws_bytes(int n, int H, int W, int h, int w) {
    if (n < 1 || n > 65535 || !sizes_ok(H, W, h, w))
        return sf::fail(SF_ERR_BAD_ARG, "sf_resize_u8_ws_bytes: bad shape (%d frames %d x %d -> %d x %d)", n, H, W, h, w);
    return (w != W && h != H) ? (int64_t)n * H * w * 3 : 0;
}

extern "C" int sf_resize_u8(const uint8_t* src, int64_t frame_stride, int64_t row_stride, int64_t px_stride, int64_t ch_stride, int n,
                            int H, int W, int h, int w, const int32_t* bounds_x, const int32_t* kx, int ksize_x,
                            const int32_t* bounds_y, const int32_t* ky, int ksize_y, uint8_t* out, void* ws, int64_t ws_bytes,
                            void* stream) {
    SF_REQUIRE(src && out, "sf_resize_u8: null argument");
    SF_REQUIRE(H > 0 && W > 0 && h > 0 && w > 0, "sf_resize_u8: bad shape %d x %d -> %d x %d", H, W, h, w);
    SF_REQUIRE(sizes_ok(H, W, h, w), "sf_resize_u8: %d x %d -> %d x %d too large (every stage below 2^30 pixels)", H, W, h, w);
    SF_REQUIRE(n >= 1 && n <= 65535, "sf_resize_u8: %d frames in one call (1 .. 65535)", n);
    SF_REQUIRE(frame_stride >= 0 && row_stride >= 0 && px_stride >= 0 && ch_stride >= 0, "sf_resize_u8: negative stride (%lld, %lld, %lld, %lld)",
               (long long)frame_stride, (long long)row_stride, (long long)px_stride, (long long)ch_stride);
    SF_REQUIRE(aligned4(out), "sf_resize_u8: out not 4-byte aligned");
    const bool horiz = w != W, vert = h != H;
    if (horiz) {
        SF_REQUIRE(bounds_x && kx, "sf_resize_u8: null horizontal table (w = %d != W = %d)", w, W);
        SF_REQUIRE(ksize_x >= 1 && ksize_x <= SF_RESIZE_MAX_KSIZE, "sf_resize_u8: ksize_x = %d (1 .. %d)", ksize_x, SF_RESIZE_MAX_KSIZE);
        SF_REQUIRE(aligned4(bounds_x) && aligned4(kx), "sf_resize_u8: horizontal tables not 4-byte aligned");
    }
    if (vert) {
        SF_REQUIRE(bounds_y && ky, "sf_resize_u8: null vertical table (h = %d != H = %d)", h, H);
        SF_REQUIRE(ksize_y >= 1 && ksize_y <= SF_RESIZE_MAX_KSIZE, "sf_resize_u8: ksize_y = %d (1 .. %d)", ksize_y, SF_RESIZE_MAX_KSIZE);
        SF_REQUIRE(aligned4(bounds_y) && aligned4(ky), "sf_resize_u8: vertical tables not 4-byte aligned");
    }
    const int64_t need = (horiz && vert) ? (int64_t)n * H * w * 3 : 0;
    if (need) {
        SF_REQUIRE(ws, "sf_resize_u8: null workspace (two passes need %lld bytes)", (long long)need);
        SF_REQUIRE(aligned4(ws), "sf_resize_u8: ws not 4-byte aligned");
        SF_REQUIRE(ws_bytes >= need, "sf_resize_u8: workspace of %lld bytes (needs %lld)", (long long)ws_bytes, (long long)need);
    }
    hipStream_t st = (hipStream_t)stream;
    SrcU8 s{src, frame_stride, row_stride, px_stride, ch_stride};
    if (!horiz && !vert) {
        const int cblocks = sf::ceil_div(w, kBlock);
        hipLaunchKernelGGL(resize_copy_u8_kernel, dim3(cblocks * h, n), dim3(kBlock), 0, st, s, h, w, out, cblocks);
        return sf::check_launch("sf_resize_u8 (copy)");
    }
    if (horiz) {
        uint8_t* dst = vert ? static_cast<uint8_t*>(ws) : out;
        const int cblocks = sf::ceil_div(w, kCols), rblocks = sf::ceil_div(H, kRowsPerBlock);
        hipLaunchKernelGGL(resize_h_u8_kernel, dim3(cblocks * rblocks, n), dim3(kBlock), h_lds_bytes(ksize_x), st, s, H, W, w, bounds_x, kx,
                           ksize_x, dst, cblocks);
        const int rc = sf::check_launch("sf_resize_u8 (horizontal)");
        if (rc != SF_OK || !vert) return rc;
        s = SrcU8{dst, (int64_t)H * w * 3, (int64_t)w * 3, 3, 1};
    }
    const int R = 3 * w;
    const int cblocks = sf::ceil_div(sf::ceil_div(R, 4), kBlock);
    const int fast = s.ps == 3 && s.cs == 1 && R % 4 == 0 && s.rs % 4 == 0 && s.fs % 4 == 0 && aligned4(s.p);
    hipLaunchKernelGGL(resize_v_u8_kernel, dim3(cblocks * h, n), dim3(kBlock), 0, st, s, H, R, h, bounds_y, ky, ksize_y, out, cblocks, fast);
    return sf::check_launch("sf_resize_u8 (vertical)");
}

extern "C" int64_t sf_resize_f32_ws_bytes(int n, int H, int W, int h, int w) {
    if (n < 1 || n > 32767 || !sizes_ok(H, W, h, w))
        return sf::fail(SF_ERR_BAD_ARG, "sf_resize_f32_ws_bytes: bad shape (%d fields %d x %d -> %d x %d)", n, H, W, h, w);
    return (w != W && h != H) ? (int64_t)n * 2 * H * w * (int64_t)sizeof(float) : 0;
}

extern "C" int sf_resize_f32(const float* src, int64_t field_stride, int64_t ch_stride, int64_t row_stride, int n, int H, int W, int h,
                             int w, const int32_t* bounds_x, const float* kx, int ksize_x, const int32_t* bounds_y, const float* ky,
                             int ksize_y, float sx, float sy, float* out, void* ws, int64_t ws_bytes, void* stream) {
    SF_REQUIRE(src && out, "sf_resize_f32: null argument");
    SF_REQUIRE(H > 0 && W > 0 && h > 0 && w > 0, "sf_resize_f32: bad shape %d x %d -> %d x %d", H, W, h, w);
    SF_REQUIRE(sizes_ok(H, W, h, w), "sf_resize_f32: %d x %d -> %d x %d too large (every stage below 2^30 pixels)", H, W, h, w);
    SF_REQUIRE(n >= 1 && n <= 32767, "sf_resize_f32: %d fields in one call (1 .. 32767)", n);
    SF_REQUIRE(row_stride >= W, "sf_resize_f32: row stride %lld below W = %d", (long long)row_stride, W);
    SF_REQUIRE(ch_stride != 0 && field_stride >= 0, "sf_resize_f32: bad channel / field strides (%lld, %lld)", (long long)ch_stride,
               (long long)field_stride);
    SF_REQUIRE(aligned4(src) && aligned4(out), "sf_resize_f32: src / out not 4-byte aligned");
    const bool horiz = w != W, vert = h != H;
    if (horiz) {
        SF_REQUIRE(bounds_x && kx, "sf_resize_f32: null horizontal table (w = %d != W = %d)", w, W);
        SF_REQUIRE(ksize_x >= 1 && ksize_x <= SF_RESIZE_MAX_KSIZE, "sf_resize_f32: ksize_x = %d (1 .. %d)", ksize_x, SF_RESIZE_MAX_KSIZE);
        SF_REQUIRE(aligned4(bounds_x) && aligned4(kx), "sf_resize_f32: horizontal tables not 4-byte aligned");
    }
    if (vert) {
        SF_REQUIRE(bounds_y && ky, "sf_resize_f32: null vertical table (h = %d != H = %d)", h, H);
        SF_REQUIRE(ksize_y >= 1 && ksize_y <= SF_RESIZE_MAX_KSIZE, "sf_resize_f32: ksize_y = %d (1 .. %d)", ksize_y, SF_RESIZE_MAX_KSIZE);
        SF_REQUIRE(aligned4(bounds_y) && aligned4(ky), "sf_resize_f32: vertical tables not 4-byte aligned");
    }
    const int64_t need = (horiz && vert) ? (int64_t)n * 2 * H * w * (int64_t)sizeof(float) : 0;
    if (need) {
        SF_REQUIRE(ws, "sf_resize_f32: null workspace (two passes need %lld bytes)", (long long)need);
        SF_REQUIRE(aligned4(ws), "sf_resize_f32: ws not 4-byte aligned");
        SF_REQUIRE(ws_bytes >= need, "sf_resize_f32: workspace of %lld bytes (needs %lld)", (long long)ws_bytes, (long long)need);
    }
    hipStream_t st = (hipStream_t)stream;
    SrcF32 s{src, field_stride, ch_stride, row_stride};
    const int planes = 2 * n;
    if (!horiz && !vert) {
        const int cblocks = sf::ceil_div(w, kBlock);
        hipLaunchKernelGGL(resize_copy_f32_kernel, dim3(cblocks * h, planes), dim3(kBlock), 0, st, s, h, w, out, cblocks, sx, sy);
        return sf::check_launch("sf_resize_f32 (copy)");
    }
    if (horiz) {
        float* dst = vert ? static_cast<float*>(ws) : out;
        const int cblocks = sf::ceil_div(w, kCols), rblocks = sf::ceil_div(H, kRowsPerBlock);
        hipLaunchKernelGGL(resize_h_f32_kernel, dim3(cblocks * rblocks, planes), dim3(kBlock), h_lds_bytes(ksize_x), st, s, H, W, w, bounds_x,
                           kx, ksize_x, dst, cblocks, vert ? 0 : 1, sx, sy);
        const int rc = sf::check_launch("sf_resize_f32 (horizontal)");
        if (rc != SF_OK || !vert) return rc;
        s = SrcF32{dst, (int64_t)2 * H * w, (int64_t)H * w, (int64_t)w};
    }
    const int cblocks = sf::ceil_div(w, kBlock);
    hipLaunchKernelGGL(resize_v_f32_kernel, dim3(cblocks * h, planes), dim3(kBlock), 0, st, s, H, w, h, bounds_y, ky, ksize_y, out, cblocks,
                       sx, sy);
    return sf::check_launch("sf_resize_f32 (vertical)");
}
