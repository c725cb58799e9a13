// PNG row unfiltering (PNG specification, section 9 "Filtering": the inverse of the five adaptive filter types) on the inflated
// IDAT stream of a batch of images: the byte arithmetic flow_io.read_png does on the host, as one launch.  The inflate stays on the
// host (zlib); the reconstructed bytes are wanted on the device anyway (sf_frames_to_clips and sf_flow_score_batch read them).
//
// Dependencies: the byte at (y, x) needs the reconstructed bytes at (y, x - bpp) = a, (y - 1, x) = b and (y - 1, x - bpp) = c, so
// the pixels of one anti-diagonal are independent.  png_unfilter_kernel: one workgroup owns one image from top to bottom, in bands
// of SF_PNG_BAND_ROWS rows.  Thread r owns row band * SF_PNG_BAND_ROWS + r; at step t it reconstructs pixel t - r of that row (all
// bpp bytes, packed in one 64-bit word), stores it and publishes it to LDS slot [t & 1][r]; one barrier per step; at step t + 1
// thread r + 1 reads it as b.  a and c never leave the thread's registers.  The last row of a band stays in an LDS row buffer of
// w * bpp bytes: thread 0 of the next band reads position x at step x, SF_PNG_BAND_ROWS - 1 steps before that band's last thread
// overwrites it -- the row never goes through global memory.  Nothing is exchanged between workgroups (no flags, no atomics, no
// spinning) and every trip count is a function of (h, w), so no scanline content can make the kernel wait.
//
// Rows of the scanline block start at arbitrary byte addresses (1 + w * bpp is odd for most formats) and `out` has arbitrary
// strides: the source is read with alignment-1 loads and the result written byte by byte.  The next pixel's source bytes are
// requested one step ahead, and the step barrier orders LDS only (global loads and stores stay in flight across it).
#include "sf_common.h"

namespace {

constexpr int kRows = SF_PNG_BAND_ROWS;

struct PngArgs {
    const uint8_t* scan;
    int64_t scan_image_stride;
    int h, w;
    uint8_t* out;
    int64_t out_image_stride, out_row_stride;
    int swap16;
};

// The source bytes of one pixel, requested one step before they are looked at.  They stay in the registers the loads fill (dword,
// halfword and byte pieces, assembled on use): arithmetic on them at the point of the request would make the wave wait there.
// The pieces are loaded through memcpy, i.e. with alignment 1.
template <int BPP>
struct RawPixel {
    static constexpr int kW = BPP / 4, kH = (BPP % 4) / 2, kB = BPP % 2;
    uint32_t w[kW ? kW : 1];
    uint16_t h;
    uint8_t b;
    __device__ __forceinline__ void load(const uint8_t* p) {
#pragma unroll
        for (int i = 0; i < kW; ++i) {
            uint32_t v;
            __builtin_memcpy(&v, p + 4 * i, 4);
            w[i] = v;
        }
        if constexpr (kH) {
            uint16_t v;
            __builtin_memcpy(&v, p + 4 * kW, 2);
            h = v;
        }
        if constexpr (kB) b = p[4 * kW + 2 * kH];
    }
    __device__ __forceinline__ uint64_t value() const {                  // byte k of the pixel in bits 8 k .. 8 k + 7
        uint64_t v = 0;
#pragma unroll
        for (int i = 0; i < kW; ++i) v |= (uint64_t)w[i] << (32 * i);
        if constexpr (kH) v |= (uint64_t)h << (32 * kW);
        if constexpr (kB) v |= (uint64_t)b << (32 * kW + 16 * kH);
        return v;
    }
};

// PNG specification 9.4: p = a + b - c; the nearest of a, b, c to p, ties in that order.  |p - a| = |b - c|, |p - b| = |a - c|.
__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// LDS-only barrier: the exchanged pixels live in LDS, so the release / acquire pair covers the local address space alone and the
// byte loads and stores to global memory are not drained at every step.
__device__ __forceinline__ void step_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// One step of one row: pixel x = t - r from the bytes requested a step ago (`cur`); the request for pixel x + 1 goes into `nxt`.
template <int BPP>
struct Row {
    const uint8_t* src;                                                  // the row's filter byte
    uint8_t* dst;
    int ft, w, swap16;
    bool have, carried;                                                  // the row exists; a band above left its last row in LDS
    uint64_t a, c;

    __device__ __forceinline__ void step(int t, int r, const RawPixel<BPP>& cur, RawPixel<BPP>& nxt, uint64_t (*s_px)[kRows],
                                         uint8_t* s_carry) {
        const int x = t - r;
        const int xn = x + 1 < 0 ? 0 : (x + 1 > w - 1 ? w - 1 : x + 1);   // every thread requests at every step, from a clamped (always
        nxt.load(src + 1 + (int64_t)xn * BPP);                           // valid) address: the wait below can then count requests
        if (have && x >= 0 && x < w) {
            uint64_t b = 0;                                              // zero in row 0
            if (r > 0) {
                b = s_px[(t + 1) & 1][r - 1];                            // made by the row above at step t - 1
            } else if (carried) {
#pragma unroll
                for (int k = 0; k < BPP; ++k) b |= (uint64_t)s_carry[x * BPP + k] << (8 * k);
            }
            const uint64_t raw = cur.value();
            uint64_t res = 0;
#pragma unroll
            for (int k = 0; k < BPP; ++k) {
                const int fa = (int)((a >> (8 * k)) & 255), fb = (int)((b >> (8 * k)) & 255), fc = (int)((c >> (8 * k)) & 255);
                int pred = ft == 1 ? fa : 0;
                pred = ft == 2 ? fb : pred;
                pred = ft == 3 ? (fa + fb) >> 1 : pred;                  // on 9 bits
                pred = ft == 4 ? paeth(fa, fb, fc) : pred;
                res |= (uint64_t)(((int)((raw >> (8 * k)) & 255) + pred) & 255) << (8 * k);
            }
            a = res, c = b;
            s_px[t & 1][r] = res;
            if (r == kRows - 1) {                                        // a full band: the next band's row above
#pragma unroll
                for (int k = 0; k < BPP; ++k) s_carry[x * BPP + k] = (uint8_t)(res >> (8 * k));
            }
            const uint64_t o = swap16 ? ((res & 0x00ff00ff00ff00ffull) << 8) | ((res >> 8) & 0x00ff00ff00ff00ffull) : res;
#pragma unroll
            for (int k = 0; k < BPP; ++k) dst[(int64_t)x * BPP + k] = (uint8_t)(o >> (8 * k));
        }
    }
};

template <int BPP>
__global__ __launch_bounds__(kRows) void png_unfilter_kernel(PngArgs g) {
    __shared__ uint64_t s_px[2][kRows];                                  // [step parity][row of the band]: the pixel just made
    __shared__ uint8_t s_carry[SF_PNG_MAX_ROW_BYTES];                    // the last row of the previous band
    const int r = threadIdx.x;
    const int64_t line = 1 + (int64_t)g.w * BPP;
    const uint8_t* scan = g.scan + (int64_t)blockIdx.x * g.scan_image_stride;
    uint8_t* out = g.out + (int64_t)blockIdx.x * g.out_image_stride;
    for (int band0 = 0; band0 < g.h; band0 += kRows) {
        const int y = band0 + r;
        const int nrows = g.h - band0 < kRows ? g.h - band0 : kRows;
        const int steps = g.w + nrows - 1;
        Row<BPP> row;
        row.have = y < g.h;
        row.src = scan + (int64_t)(row.have ? y : g.h - 1) * line;       // threads past the image read its last row, and drop it
        row.dst = out + (row.have ? (int64_t)y * g.out_row_stride : 0);
        row.ft = row.src[0];
        row.ft = row.ft > 4 ? 0 : row.ft;                                // (the Python layer rejects such files before any upload)
        row.w = g.w, row.swap16 = g.swap16, row.carried = band0 > 0;
        row.a = row.c = 0;                                               // zero in the first pixel of a row
        RawPixel<BPP> even = {}, odd = {};                               // two sets of registers in turn: no copy that would wait for a load
        even.load(row.src + 1);                                          // thread 0 starts at step 0: nobody requested its pixel 0
        for (int t = 0; t < steps; t += 2) {
            row.step(t, r, even, odd, s_px, s_carry);
            step_barrier();
            if (t + 1 < steps) {                                         // uniform: the whole workgroup takes it or not
                row.step(t + 1, r, odd, even, s_px, s_carry);
                step_barrier();
            }
        }
    }
}

template <int BPP>
void launch(const PngArgs& a, int n_images, hipStream_t stream) {
    hipLaunchKernelGGL(png_unfilter_kernel<BPP>, dim3(n_images), dim3(kRows), 0, stream, a);
}

}  // namespace

extern "C" int sf_png_unfilter(const uint8_t* scan, int64_t scan_image_stride, int n_images, int h, int w, int bpp, uint8_t* out,
                               int64_t out_image_stride, int64_t out_row_stride, int swap16, void* stream) {
    SF_REQUIRE(scan && out, "sf_png_unfilter: null argument (scan / out)");
    SF_REQUIRE(n_images >= 1 && n_images <= 65535, "sf_png_unfilter: n_images = %d (1 .. 65535)", n_images);
    SF_REQUIRE(h >= 1 && w >= 1, "sf_png_unfilter: bad size h = %d, w = %d", h, w);
    SF_REQUIRE(bpp == 1 || bpp == 2 || bpp == 3 || bpp == 4 || bpp == 6 || bpp == 8, "sf_png_unfilter: bpp = %d (1, 2, 3, 4, 6 or 8)", bpp);
    SF_REQUIRE(!swap16 || bpp % 2 == 0, "sf_png_unfilter: swap16 needs an even bpp (got %d)", bpp);
    const int64_t row = (int64_t)w * bpp, image = (int64_t)h * (1 + row);
    SF_REQUIRE(image < ((int64_t)1 << 31), "sf_png_unfilter: h * (1 + w * bpp) = %lld is 2^31 or more", (long long)image);
    SF_REQUIRE(scan_image_stride >= image, "sf_png_unfilter: scan_image_stride = %lld is smaller than h * (1 + w * bpp) = %lld",
               (long long)scan_image_stride, (long long)image);
    SF_REQUIRE(out_row_stride >= row, "sf_png_unfilter: out_row_stride = %lld is smaller than w * bpp = %lld", (long long)out_row_stride,
               (long long)row);
    SF_REQUIRE(out_image_stride >= (int64_t)(h - 1) * out_row_stride + row,
               "sf_png_unfilter: out_image_stride = %lld is smaller than (h - 1) * out_row_stride + w * bpp = %lld",
               (long long)out_image_stride, (long long)((int64_t)(h - 1) * out_row_stride + row));
    if (row > SF_PNG_MAX_ROW_BYTES)
        return sf::fail(SF_ERR_UNSUPPORTED, "sf_png_unfilter: w * bpp = %lld (at most SF_PNG_MAX_ROW_BYTES = %d)", (long long)row,
                        SF_PNG_MAX_ROW_BYTES);
    PngArgs a;
    a.scan = scan, a.scan_image_stride = scan_image_stride, a.h = h, a.w = w;
    a.out = out, a.out_image_stride = out_image_stride, a.out_row_stride = out_row_stride, a.swap16 = swap16 ? 1 : 0;
    const hipStream_t s = (hipStream_t)stream;
    switch (bpp) {
        case 1: launch<1>(a, n_images, s); break;
        case 2: launch<2>(a, n_images, s); break;
        case 3: launch<3>(a, n_images, s); break;
        case 4: launch<4>(a, n_images, s); break;
        case 6: launch<6>(a, n_images, s); break;
        default: launch<8>(a, n_images, s); break;
    }
    return sf::check_launch("sf_png_unfilter");
}
