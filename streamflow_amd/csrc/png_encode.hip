// PNG encoding of a batch of device images into zlib streams (RFC 1950 / 1951, PNG specification sections 9 and 12.8): the adaptive
// row filter and a Huffman-only deflate, so that the colour-wheel and KITTI images sf_flow_to_image / sf_flow_to_kitti16 leave on the
// device cross to the host compressed.  The host keeps the chunk framing and the CRC-32 (flow_io.png_file).  The format -- filter
// choice, bands, table construction, header bits -- is restated in tests/png_encode_cases.py, and the output equals it byte for byte.
//
// Four launches behind one clear launch (sf::fill_async), every dependency between workgroups a launch boundary:
//   png_filter_kernel   one wave per row: the five filtered versions' sums of min(v, 256 - v), the cheapest type (ties: the lowest),
//                       the filtered scanline into the workspace.
//   png_table_kernel    one workgroup per band of SF_PNG_ENC_BAND_ROWS scanlines: the band's Huffman tables, its block's exact bit
//                       length and its Adler-32 sums (table_block of csrc/huff_deflate.h, shared with csrc/flo5_encode.hip).
//   png_offsets_kernel  one thread per image: prefix sum of the blocks' bit lengths, the Adler-32 of the whole image, `78 01`, the
//                       checksum bytes and out_bytes.
//   png_pack_kernel     one workgroup per band: the block's bits ORed into the output with vector atomics (pack_block of the same
//                       header; a 32-bit word is shared by neighbouring threads, passes and bands: the entry point clears
//                       sf_png_encode_bound bytes of every slot first).
// No workgroup waits for another, and every trip count is a function of (n, h, w, bpp): LDS holds tables and histograms only, a band
// is streamed from the workspace.
#include "huff_deflate.h"

namespace {

using namespace sf_huff;

constexpr int kBand = SF_PNG_ENC_BAND_ROWS;

struct EncArgs {
    const uint8_t* img;
    int64_t img_image_stride, img_row_stride;
    int h, w, bpp, swap16, nbands;
    int64_t line;                                                       // 1 + w * bpp
    uint8_t* scan;                                                      // [n][scan_stride]: the filtered scanlines, dense
    int64_t scan_stride;
    uint32_t* rec;                                                      // [n][nbands][kRecWords]
    uint8_t* out;
    int64_t out_image_stride;
    int64_t* out_bytes;
    int n_images;
};

__device__ __forceinline__ int paeth(int a, int b, int c) {             // PNG specification 9.4; ties a, b, c
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int cost(int v) { return v < 128 ? v : 256 - v; }

// ---- 1. filter ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void png_filter_kernel(EncArgs g) {
    const int lane = threadIdx.x & 63;
    const int64_t y = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (y >= g.h) return;                                               // whole waves leave; there is no barrier in this kernel
    const int row = g.w * g.bpp, bpp = g.bpp, sw = g.swap16;
    const uint8_t* cur = g.img + (int64_t)blockIdx.y * g.img_image_stride + y * g.img_row_stride;
    const uint8_t* up = cur - g.img_row_stride;                         // read only where y > 0
    const bool top = y == 0;
    int s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    for (int x = lane; x < row; x += 64) {
        const bool left = x >= bpp;
        const int v = cur[x ^ sw], a = left ? cur[(x - bpp) ^ sw] : 0, b = top ? 0 : up[x ^ sw], c = (left && !top) ? up[(x - bpp) ^ sw] : 0;
        s0 += cost(v), s1 += cost((v - a) & 255), s2 += cost((v - b) & 255), s3 += cost((v - ((a + b) >> 1)) & 255);
        s4 += cost((v - paeth(a, b, c)) & 255);
    }
    s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2), s3 = wave_sum(s3), s4 = wave_sum(s4);
    int ft = 0, best = s0;
    if (s1 < best) ft = 1, best = s1;
    if (s2 < best) ft = 2, best = s2;
    if (s3 < best) ft = 3, best = s3;
    if (s4 < best) ft = 4, best = s4;
    uint8_t* dst = g.scan + (int64_t)blockIdx.y * g.scan_stride + y * g.line;
    if (lane == 0) dst[0] = (uint8_t)ft;
    for (int x = lane; x < row; x += 64) {
        const bool left = x >= bpp;
        const int v = cur[x ^ sw], a = left ? cur[(x - bpp) ^ sw] : 0, b = top ? 0 : up[x ^ sw], c = (left && !top) ? up[(x - bpp) ^ sw] : 0;
        int pred = ft == 1 ? a : 0;
        pred = ft == 2 ? b : pred;
        pred = ft == 3 ? (a + b) >> 1 : pred;
        pred = ft == 4 ? paeth(a, b, c) : pred;
        dst[1 + x] = (uint8_t)(v - pred);
    }
}

// ---- 2. tables ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void png_table_kernel(EncArgs g) {
    const int rows = g.h - (int)blockIdx.x * kBand < kBand ? g.h - (int)blockIdx.x * kBand : kBand;
    const int64_t nbytes = rows * g.line;                               // < 2^31 / 1: the image's scanlines are
    const uint8_t* p = g.scan + (int64_t)blockIdx.y * g.scan_stride + (int64_t)blockIdx.x * kBand * g.line;     // 16-byte aligned
    table_block(p, nbytes, g.rec + ((int64_t)blockIdx.y * g.nbands + blockIdx.x) * kRecWords);
}

// ---- 3. offsets --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void png_offsets_kernel(EncArgs g) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= g.n_images) return;
    uint32_t* rec = g.rec + (int64_t)i * g.nbands * kRecWords;
    uint64_t bit = 16, A = 0, B = 0;                                    // behind `78 01`
    for (int b = 0; b < g.nbands; ++b, rec += kRecWords) {
        rec[kRecStartLo] = (uint32_t)bit, rec[kRecStartHi] = (uint32_t)(bit >> 32);
        bit += rec[kRecBits];
        const int rows = g.h - b * kBand < kBand ? g.h - b * kBand : kBand;
        adler_append(A, B, rec, (uint64_t)rows * g.line);
    }
    g.out_bytes[i] = stream_ends(g.out + (int64_t)i * g.out_image_stride, bit, A, B, (uint64_t)g.h * g.line);
}

// ---- 4. pack -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void png_pack_kernel(EncArgs g) {
    const int rows = g.h - (int)blockIdx.x * kBand < kBand ? g.h - (int)blockIdx.x * kBand : kBand;
    const int64_t nbytes = rows * g.line;
    const uint8_t* p = g.scan + (int64_t)blockIdx.y * g.scan_stride + (int64_t)blockIdx.x * kBand * g.line;     // 16-byte aligned
    pack_block(p, nbytes, g.rec + ((int64_t)blockIdx.y * g.nbands + blockIdx.x) * kRecWords,
               reinterpret_cast<uint32_t*>(g.out + (int64_t)blockIdx.y * g.out_image_stride),                  // 4-byte aligned
               (int)blockIdx.x == g.nbands - 1);
}

// ---- flow -> KITTI codes -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void flow_to_kitti16_kernel(const float* flow, uint16_t* out, int64_t plane) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= plane) return;
    const float* f = flow + (int64_t)blockIdx.y * 2 * plane;
    uint16_t* o = out + ((int64_t)blockIdx.y * plane + i) * 3;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float v = __fadd_rn(__fmul_rn(64.0f, f[k * plane + i]), 32768.0f);      // two roundings, never fused
        o[k] = v >= 65535.0f ? (uint16_t)65535 : (v > 0.0f ? (uint16_t)(int)v : (uint16_t)0);     // NaN fails both tests: 0
    }
    o[2] = 1;
}

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
int64_t scan_stride_of(int h, int w, int bpp) { return align_up((int64_t)h * (1 + (int64_t)w * bpp), 16) + 16; }
int bands_of(int h) { return (h + kBand - 1) / kBand; }
bool shape_ok(int h, int w, int bpp) {
    return h >= 1 && w >= 1 && (bpp == 1 || bpp == 2 || bpp == 3 || bpp == 4 || bpp == 6 || bpp == 8) &&
           (int64_t)h * (1 + (int64_t)w * bpp) < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int64_t sf_png_encode_bound(int h, int w, int bpp) {
    if (!shape_ok(h, w, bpp)) return -1;
    const int64_t bits = (int64_t)bands_of(h) * (kHeaderBitsMax + 9) + 9 * (int64_t)h * (1 + (int64_t)w * bpp);
    return align_up(2 + (bits + 7) / 8 + 4, 4);
}

extern "C" int64_t sf_png_encode_ws_bytes(int n_images, int h, int w, int bpp) {
    if (!shape_ok(h, w, bpp) || n_images < 1 || n_images > 65535) return -1;
    return 16 + (int64_t)n_images * (scan_stride_of(h, w, bpp) + (int64_t)bands_of(h) * kRecWords * 4);
}

extern "C" int sf_png_encode(const uint8_t* img, int64_t img_image_stride, int64_t img_row_stride, int n_images, int h, int w, int bpp,
                             int swap16, uint8_t* out, int64_t out_image_stride, int64_t* out_bytes, void* ws, int64_t ws_bytes,
                             void* stream) {
    SF_REQUIRE(img && out && out_bytes && ws, "sf_png_encode: null argument (img / out / out_bytes / ws)");
    SF_REQUIRE(n_images >= 1 && n_images <= 65535, "sf_png_encode: n_images = %d (1 .. 65535)", n_images);
    SF_REQUIRE(h >= 1 && w >= 1, "sf_png_encode: bad size h = %d, w = %d", h, w);
    SF_REQUIRE(bpp == 1 || bpp == 2 || bpp == 3 || bpp == 4 || bpp == 6 || bpp == 8, "sf_png_encode: bpp = %d (1, 2, 3, 4, 6 or 8)", bpp);
    SF_REQUIRE(!swap16 || bpp % 2 == 0, "sf_png_encode: swap16 needs an even bpp (got %d)", bpp);
    const int64_t row = (int64_t)w * bpp, image = (int64_t)h * (1 + row);
    SF_REQUIRE(image < ((int64_t)1 << 31), "sf_png_encode: h * (1 + w * bpp) = %lld is 2^31 or more", (long long)image);
    SF_REQUIRE(img_row_stride >= row, "sf_png_encode: img_row_stride = %lld is smaller than w * bpp = %lld", (long long)img_row_stride,
               (long long)row);
    SF_REQUIRE(img_image_stride >= (int64_t)(h - 1) * img_row_stride + row,
               "sf_png_encode: img_image_stride = %lld is smaller than (h - 1) * img_row_stride + w * bpp = %lld",
               (long long)img_image_stride, (long long)((int64_t)(h - 1) * img_row_stride + row));
    const int64_t bound = sf_png_encode_bound(h, w, bpp);
    SF_REQUIRE(out_image_stride >= bound, "sf_png_encode: out_image_stride = %lld is smaller than sf_png_encode_bound = %lld",
               (long long)out_image_stride, (long long)bound);
    SF_REQUIRE(((uintptr_t)out & 3) == 0 && out_image_stride % 4 == 0,
               "sf_png_encode: out and out_image_stride = %lld must be multiples of 4 (the bits are ORed into 32-bit words)",
               (long long)out_image_stride);
    SF_REQUIRE(((uintptr_t)out_bytes & 7) == 0, "sf_png_encode: out_bytes is not 8-byte aligned");
    const int64_t need = sf_png_encode_ws_bytes(n_images, h, w, bpp);
    SF_REQUIRE(ws_bytes >= need, "sf_png_encode: ws_bytes = %lld is smaller than sf_png_encode_ws_bytes = %lld", (long long)ws_bytes,
               (long long)need);
    if (row > SF_PNG_MAX_ROW_BYTES)
        return sf::fail(SF_ERR_UNSUPPORTED, "sf_png_encode: w * bpp = %lld (at most SF_PNG_MAX_ROW_BYTES = %d)", (long long)row,
                        SF_PNG_MAX_ROW_BYTES);
    EncArgs a;
    a.img = img, a.img_image_stride = img_image_stride, a.img_row_stride = img_row_stride;
    a.h = h, a.w = w, a.bpp = bpp, a.swap16 = swap16 ? 1 : 0, a.nbands = bands_of(h), a.line = 1 + row;
    a.scan = reinterpret_cast<uint8_t*>(((uintptr_t)ws + 15) & ~(uintptr_t)15);
    a.scan_stride = scan_stride_of(h, w, bpp);
    a.rec = reinterpret_cast<uint32_t*>(a.scan + (int64_t)n_images * a.scan_stride);
    a.out = out, a.out_image_stride = out_image_stride, a.out_bytes = out_bytes, a.n_images = n_images;
    const hipStream_t s = (hipStream_t)stream;
    // the pack kernel ORs into zeroed words; nothing past sf_png_encode_bound bytes of a slot is touched
    const int cleared = sf::fill_async("sf_png_encode (clearing the slots)", out, 0, bound, s, n_images, out_image_stride);
    if (cleared != SF_OK) return cleared;
    const dim3 per_band(a.nbands, n_images);
    hipLaunchKernelGGL(png_filter_kernel, dim3((h + kThreads / 64 - 1) / (kThreads / 64), n_images), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(png_table_kernel, per_band, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(png_offsets_kernel, dim3((n_images + 63) / 64), dim3(64), 0, s, a);
    hipLaunchKernelGGL(png_pack_kernel, per_band, dim3(kThreads), 0, s, a);
    return sf::check_launch("sf_png_encode");
}

extern "C" int sf_flow_to_kitti16(const float* flow, uint16_t* out, int n, int h, int w, void* stream) {
    SF_REQUIRE(flow && out, "sf_flow_to_kitti16: null argument (flow / out)");
    SF_REQUIRE(n >= 1 && n <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 30),
               "sf_flow_to_kitti16: bad size n = %d, h = %d, w = %d (n <= 65535, h * w < 2^30)", n, h, w);
    SF_REQUIRE(((uintptr_t)out & 1) == 0 && ((uintptr_t)flow & 3) == 0, "sf_flow_to_kitti16: misaligned flow / out");
    const int64_t plane = (int64_t)h * w;
    hipLaunchKernelGGL(flow_to_kitti16_kernel, dim3((unsigned)((plane + kThreads - 1) / kThreads), n), dim3(kThreads), 0,
                       (hipStream_t)stream, flow, out, plane);
    return sf::check_launch("sf_flow_to_kitti16");
}
