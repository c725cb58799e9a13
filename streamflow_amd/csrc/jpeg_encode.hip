// Baseline JPEG encoding (ITU-T T.81, sequential, 8 bit, Huffman) of a batch of device images into entropy-coded segments, so that
// the colour-wheel images sf_flow_to_image leaves on the device cross to the host compressed and become the frames of a Motion-JPEG
// video.  The host keeps the marker segments (jpeg_gpu.jpeg_file) and the AVI container (avi.MjpegWriter).  The format -- colour
// conversion, the integer DCT, quantisation, the Annex K.3 tables, one restart interval per MCU row -- is stated in
// include/streamflow_hip.h and restated in tests/jpeg_cases.py; the output equals that restatement byte for byte.
//
// Five launches, every dependency between workgroups a launch boundary:
//   jpeg_dct_kernel      one thread per 8 x 8 block: for each component the level-shifted samples (edges replicated), the two DCT
//                        passes in registers, the quantised levels as int16 in zigzag order into the workspace.
//   jpeg_pack_kernel     one workgroup per restart interval (MCU row), a thread per block of a component: the block's bit length, a
//                        workgroup scan, the words of the pass cleared, then its codes ORed MSB-first into the interval's staging
//                        area with vector atomics (a 32-bit word is shared by neighbouring threads and passes); the padding 1-bits.
//   jpeg_count_kernel    one workgroup per interval: the 0xFF bytes of the staged interval -> its length behind byte stuffing.
//   jpeg_offsets_kernel  one thread per image: prefix sum of the intervals' lengths, out_bytes.
//   jpeg_gather_kernel   one workgroup per interval: the staged bytes to their place in the segment, 0x00 behind every 0xFF, the RSTm
//                        marker behind every interval but the last; plain byte stores, every byte of the segment written once.
// No workgroup waits for another, and every trip count is a function of (n, h, w, channels) and the interval's own length.
#include "huff_deflate.h"

namespace {

using sf_huff::kThreads;
using sf_huff::scan_bits;
using sf_huff::wave_sum;

constexpr int kBlockBitsMax = 22 + 63 * 26;                            // DC: 11-bit code + 11 bits; AC: 16-bit code + 10 bits each

// The DCT table: kDct[u][x] = round(2^13 sqrt 2 c(u) / 2 cos((2 x + 1) u pi / 16)), x = 0 .. 3; column 7 - x is (-1)^u times column x.
// The factor sqrt 2 makes rows 0 and 4 exact (4096), so the DC coefficient of a block is exact; two passes give 2 F.
constexpr int kDct[8][4] = {{4096, 4096, 4096, 4096},   {5681, 4816, 3218, 1130},  {5352, 2217, -2217, -5352}, {4816, -1130, -5681, -3218},
                            {4096, -4096, -4096, 4096}, {3218, -5681, 1130, 4816}, {2217, -5352, 5352, -2217}, {1130, -3218, 4816, -5681}};

constexpr int kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};    // natural index of scan position k

// The typical Huffman tables of T.81 Annex K.3 (BITS, HUFFVAL) and their canonical codes (Annex C): entry = code | length << 16.
struct HuffSpec {
    uint8_t bits[16];
    uint8_t vals[162];
};
constexpr HuffSpec kDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr HuffSpec kAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

struct HuffTabs {
    uint32_t dc[2][16];                                                 // by category 0 .. 11
    uint32_t ac[2][256];                                                // by run << 4 | size
};

constexpr void fill_codes(const HuffSpec& spec, uint32_t* tab) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < spec.bits[len - 1]; ++i) tab[spec.vals[k++]] = code++ | (uint32_t)len << 16;
        code <<= 1;
    }
}

constexpr HuffTabs make_tabs() {
    HuffTabs t{};
    fill_codes(kDcLuma, t.dc[0]), fill_codes(kDcChroma, t.dc[1]), fill_codes(kAcLuma, t.ac[0]), fill_codes(kAcChroma, t.ac[1]);
    return t;
}

__constant__ HuffTabs kTabs = make_tabs();

struct JpegArgs {
    const uint8_t* img;
    int64_t img_image_stride, img_row_stride;
    int h, w, nc, bw, bh, n_images;                                     // bw x bh blocks; an interval is bw nc units
    int16_t* coef;                                                      // [n][bh][bw][nc][64]: quantised levels, zigzag order
    uint8_t* stage;                                                     // [n][bh][stage_stride]: an interval before byte stuffing
    int64_t stage_stride;
    int64_t* ioff;                                                      // [n][bh]: the interval's first byte in its segment
    uint32_t* ibits;                                                    // [n][bh]: its bits before padding
    uint32_t* ilen;                                                     // [n][bh]: its bytes, stuffed, with its RSTm marker
    uint8_t* out;
    int64_t out_image_stride;
    int64_t* out_bytes;
    uint16_t q[2][64];                                                  // zigzag order
};

// ---- 1. colour, DCT, quantisation ----------------------------------------------------------------------------------------------------
// One pass over 8 values STRIDE apart: r[u] = sum_x kDct[u][x] v[x], through the sums and differences of v[x] and v[7 - x] (exact in
// integers); SHIFT > 0 rounds to SHIFT fewer fraction bits, half up.
template <int STRIDE, int SHIFT>
__device__ __forceinline__ void dct8(int* v) {
    int a[4], d[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) a[x] = v[x * STRIDE] + v[(7 - x) * STRIDE], d[x] = v[x * STRIDE] - v[(7 - x) * STRIDE];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int* s = (u & 1) ? d : a;
        int r = kDct[u][0] * s[0] + kDct[u][1] * s[1] + kDct[u][2] * s[2] + kDct[u][3] * s[3];
        if (SHIFT > 0) r = (r + (1 << (SHIFT - 1))) >> SHIFT;
        v[u * STRIDE] = r;
    }
}

__global__ __launch_bounds__(kThreads) void jpeg_dct_kernel(JpegArgs g) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= g.bh * g.bw) return;                                       // no barrier in this kernel
    const int by = b / g.bw, bx = b - by * g.bw, nc = g.nc;
    const uint8_t* img = g.img + (int64_t)blockIdx.y * g.img_image_stride;
    int16_t* dst = g.coef + ((((int64_t)blockIdx.y * g.bh + by) * g.bw + bx) * nc) * 64;
    int xo[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) xo[x] = min(bx * 8 + x, g.w - 1) * nc;  // the last column replicated
#pragma unroll 1
    for (int c = 0; c < nc; ++c, dst += 64) {
        // JFIF YCbCr in 16-bit fixed point: (kr R + kg G + kb B + add) >> 16; grey passes through
        const int kr = c == 0 ? 19595 : (c == 1 ? -11059 : 32768), kg = c == 0 ? 38470 : (c == 1 ? -21709 : -27439);
        const int kb = c == 0 ? 7471 : (c == 1 ? 32768 : -5329), add = c == 0 ? 32768 : (128 << 16) + 32767;
        int v[64];
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const uint8_t* row = img + (int64_t)min(by * 8 + y, g.h - 1) * g.img_row_stride;       // the last row replicated
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const uint8_t* p = row + xo[x];
                v[y * 8 + x] = (nc == 3 ? (kr * p[0] + kg * p[1] + kb * p[2] + add) >> 16 : (int)p[0]) - 128;
            }
        }
#pragma unroll
        for (int y = 0; y < 8; ++y) dct8<1, 9>(v + y * 8);              // rows: 13 - 9 = 4 fraction bits
#pragma unroll
        for (int x = 0; x < 8; ++x) dct8<8, 0>(v + x);                  // columns: 2 F with 17 fraction bits
        const uint16_t* q = g.q[c ? 1 : 0];
        uint32_t packed[32];
#pragma unroll
        for (int k = 0; k < 64; ++k) {
            const int f = v[kZigzag[k]];
            const uint32_t qk = q[k];
            const int mag = (int)(((uint32_t)abs(f) + (qk << 17)) / (qk << 18));        // round half away from zero
            const uint32_t lvl = (uint32_t)(f < 0 ? -mag : mag) & 0xffffu;
            packed[k >> 1] = (k & 1) ? packed[k >> 1] | lvl << 16 : lvl;
        }
        uint4* d4 = reinterpret_cast<uint4*>(dst);                      // 128-byte aligned
#pragma unroll
        for (int i = 0; i < 8; ++i) d4[i] = make_uint4(packed[4 * i], packed[4 * i + 1], packed[4 * i + 2], packed[4 * i + 3]);
    }
}

// ---- 2. entropy coding ---------------------------------------------------------------------------------------------------------------
struct BitCount {
    int n = 0;
    __device__ __forceinline__ void put(uint32_t, int len) { n += len; }
};

// MSB-first bits into 32-bit words of a byte stream: a word leaves, byte-swapped, as soon as it is full.
struct BitSink {
    uint32_t* w;
    uint64_t acc = 0;
    int n;
    __device__ __forceinline__ BitSink(uint32_t* words, uint64_t pos) : w(words + (pos >> 5)), n((int)(pos & 31)) {}
    __device__ __forceinline__ void put(uint32_t code, int len) {      // len <= 26, so one word at most leaves
        acc = acc << len | code, n += len;
        if (n >= 32) {
            n -= 32;
            atomicOr(w++, __builtin_bswap32((uint32_t)(acc >> n)));
            acc &= ((uint64_t)1 << n) - 1;
        }
    }
    __device__ __forceinline__ void flush() {
        if (n > 0) atomicOr(w, __builtin_bswap32((uint32_t)(acc << (32 - n))));
    }
};

__device__ __forceinline__ int category(int v) { return 32 - __clz(abs(v)); }                     // 0 for 0
__device__ __forceinline__ uint32_t value_bits(int v, int cat) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1); }

// One block of 64 levels: the DC difference by category, the AC levels as run / size symbols with ZRL and EOB.
template <class Sink>
__device__ __forceinline__ void code_unit(const int16_t* lv, int prev_dc, const uint32_t* dc, const uint32_t* ac, Sink& s) {
    int run = 0;
#pragma unroll 1
    for (int q = 0; q < 8; ++q) {
        const uint4 v4 = reinterpret_cast<const uint4*>(lv)[q];
        const uint32_t wv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int val = (int)(int16_t)(wv[j >> 1] >> (16 * (j & 1)));
            if (j == 0 && q == 0) {
                const int diff = val - prev_dc, cat = category(diff);
                const uint32_t e = dc[cat];
                s.put((e & 0xffff) << cat | value_bits(diff, cat), (int)(e >> 16) + cat);
            } else if (val == 0) {
                ++run;
            } else {
                for (; run > 15; run -= 16) s.put(ac[0xf0] & 0xffff, (int)(ac[0xf0] >> 16));
                const int cat = category(val);
                const uint32_t e = ac[run << 4 | cat];
                s.put((e & 0xffff) << cat | value_bits(val, cat), (int)(e >> 16) + cat);
                run = 0;
            }
        }
    }
    if (run > 0) s.put(ac[0] & 0xffff, (int)(ac[0] >> 16));
}

__global__ __launch_bounds__(kThreads) void jpeg_pack_kernel(JpegArgs g) {
    __shared__ uint32_t s_dc[2][16], s_ac[2][256];
    __shared__ int s_wave[kThreads / 64];
    const int tid = threadIdx.x, nc = g.nc, units = g.bw * nc;
    for (int i = tid; i < 2 * 256; i += kThreads) (&s_ac[0][0])[i] = (&kTabs.ac[0][0])[i];
    if (tid < 32) (&s_dc[0][0])[tid] = (&kTabs.dc[0][0])[tid];
    const int64_t interval = (int64_t)blockIdx.y * g.bh + blockIdx.x;
    const int16_t* coef = g.coef + interval * units * 64;
    uint32_t* words = reinterpret_cast<uint32_t*>(g.stage + interval * g.stage_stride);           // 16-byte aligned
    uint64_t base = 0;                                                  // every thread keeps the same running offset
    __syncthreads();
    for (int u0 = 0; u0 < units; u0 += kThreads) {
        const int u = u0 + tid, cls = (u % nc) ? 1 : 0;
        const bool live = u < units;
        const int prev = live && u >= nc ? coef[(int64_t)(u - nc) * 64] : 0;                     // DC prediction starts at 0
        BitCount count;
        if (live) code_unit(coef + (int64_t)u * 64, prev, s_dc[cls], s_ac[cls], count);
        const uint64_t before = base;
        const uint64_t pos = scan_bits(count.n, &base, s_wave);
        // the words this pass reaches and no earlier pass has cleared
        for (uint64_t i = ((before + 31) >> 5) + tid; i < ((base + 31) >> 5); i += kThreads) words[i] = 0;
        __syncthreads();
        if (live) {
            BitSink sink(words, pos);
            code_unit(coef + (int64_t)u * 64, prev, s_dc[cls], s_ac[cls], sink);
            sink.flush();
        }
    }
    if (tid == 0) {
        if (base & 7) {                                                 // 1-bits up to the byte boundary
            const uint64_t byte = base >> 3;
            atomicOr(words + (byte >> 2), ((1u << (8 - (int)(base & 7))) - 1) << (8 * (int)(byte & 3)));
        }
        g.ibits[interval] = (uint32_t)base;
    }
}

// ---- 3. stuffed lengths -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int count_ff(uint32_t v) {
    return ((v & 0xff) == 0xff) + ((v & 0xff00) == 0xff00) + ((v & 0xff0000) == 0xff0000) + ((v >> 24) == 0xff);
}

__global__ __launch_bounds__(kThreads) void jpeg_count_kernel(JpegArgs g) {
    __shared__ int s_sum;
    const int tid = threadIdx.x;
    if (tid == 0) s_sum = 0;
    __syncthreads();
    const int64_t interval = (int64_t)blockIdx.y * g.bh + blockIdx.x;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(g.stage + interval * g.stage_stride);
    const uint32_t nbytes = (g.ibits[interval] + 7) >> 3, nwords = (nbytes + 3) >> 2;           // the last word's tail is zero
    int ff = 0;
    for (uint32_t i = tid; i < nwords; i += kThreads) ff += count_ff(words[i]);
    ff = wave_sum(ff);
    if ((tid & 63) == 0) atomicAdd(&s_sum, ff);
    __syncthreads();
    if (tid == 0) g.ilen[interval] = nbytes + (uint32_t)s_sum + ((int)blockIdx.x < g.bh - 1 ? 2u : 0u);
}

// ---- 4. offsets ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void jpeg_offsets_kernel(JpegArgs g) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= g.n_images) return;
    int64_t off = 0;
    for (int r = 0; r < g.bh; ++r) {
        g.ioff[(int64_t)i * g.bh + r] = off;
        off += g.ilen[(int64_t)i * g.bh + r];
    }
    g.out_bytes[i] = off;
}

// ---- 5. gather ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void jpeg_gather_kernel(JpegArgs g) {
    __shared__ int s_wave[kThreads / 64];
    const int tid = threadIdx.x;
    const int64_t interval = (int64_t)blockIdx.y * g.bh + blockIdx.x;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(g.stage + interval * g.stage_stride);
    const uint32_t nbytes = (g.ibits[interval] + 7) >> 3, nwords = (nbytes + 3) >> 2;
    uint8_t* dst = g.out + (int64_t)blockIdx.y * g.out_image_stride + g.ioff[interval];
    uint64_t base = 0;
    for (uint32_t i0 = 0; i0 < nwords; i0 += kThreads) {
        const uint32_t i = i0 + tid;
        const uint32_t v = i < nwords ? words[i] : 0;
        const int valid = i < nwords ? (int)min(4u, nbytes - 4 * i) : 0;
        const uint64_t pos = scan_bits(valid + count_ff(v), &base, s_wave);                       // bytes here, not bits
        uint8_t* p = dst + pos;
        for (int k = 0; k < valid; ++k) {
            const uint8_t byte = (uint8_t)(v >> (8 * k));
            *p++ = byte;
            if (byte == 0xff) *p++ = 0;
        }
    }
    if (tid == 0 && (int)blockIdx.x < g.bh - 1) dst[base] = 0xff, dst[base + 1] = (uint8_t)(0xd0 + (blockIdx.x & 7));
}

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
bool shape_ok(int h, int w, int channels) {
    return h >= 1 && w >= 1 && h <= SF_JPEG_MAX_DIM && w <= SF_JPEG_MAX_DIM && (channels == 1 || channels == 3);
}
int64_t interval_bytes(int w, int channels) { return ((int64_t)((w + 7) / 8) * channels * kBlockBitsMax + 7) / 8; }
int64_t stage_stride_of(int w, int channels) { return align_up(interval_bytes(w, channels), 16); }

}  // namespace

extern "C" int64_t sf_jpeg_encode_bound(int h, int w, int channels) {
    if (!shape_ok(h, w, channels)) return -1;
    return align_up((int64_t)((h + 7) / 8) * (2 * interval_bytes(w, channels) + 2), 4);
}

extern "C" int64_t sf_jpeg_encode_ws_bytes(int n_images, int h, int w, int channels) {
    if (!shape_ok(h, w, channels) || n_images < 1 || n_images > 65535) return -1;
    const int64_t intervals = (int64_t)n_images * ((h + 7) / 8);
    return 16 + intervals * ((int64_t)((w + 7) / 8) * channels * 128 + stage_stride_of(w, channels) + 16);
}

extern "C" int sf_jpeg_encode(const uint8_t* img, int64_t img_image_stride, int64_t img_row_stride, int n_images, int h, int w,
                              int channels, const uint16_t* qtables, uint8_t* out, int64_t out_image_stride, int64_t* out_bytes,
                              void* ws, int64_t ws_bytes, void* stream) {
    SF_REQUIRE(img && qtables && out && out_bytes && ws, "sf_jpeg_encode: null argument (img / qtables / out / out_bytes / ws)");
    SF_REQUIRE(n_images >= 1 && n_images <= 65535, "sf_jpeg_encode: n_images = %d (1 .. 65535)", n_images);
    SF_REQUIRE(h >= 1 && w >= 1, "sf_jpeg_encode: bad size h = %d, w = %d", h, w);
    SF_REQUIRE(channels == 1 || channels == 3, "sf_jpeg_encode: channels = %d (1 or 3)", channels);
    for (int i = 0; i < 128; ++i)
        SF_REQUIRE(qtables[i] >= 1 && qtables[i] <= 255, "sf_jpeg_encode: qtables[%d][%d] = %d (1 .. 255)", i / 64, i % 64, (int)qtables[i]);
    if (h > SF_JPEG_MAX_DIM || w > SF_JPEG_MAX_DIM)
        return sf::fail(SF_ERR_UNSUPPORTED, "sf_jpeg_encode: h = %d, w = %d (at most SF_JPEG_MAX_DIM = %d)", h, w, SF_JPEG_MAX_DIM);
    const int64_t row = (int64_t)w * channels;
    SF_REQUIRE(img_row_stride >= row, "sf_jpeg_encode: img_row_stride = %lld is smaller than w * channels = %lld",
               (long long)img_row_stride, (long long)row);
    SF_REQUIRE(img_image_stride >= (int64_t)(h - 1) * img_row_stride + row,
               "sf_jpeg_encode: img_image_stride = %lld is smaller than (h - 1) * img_row_stride + w * channels = %lld",
               (long long)img_image_stride, (long long)((int64_t)(h - 1) * img_row_stride + row));
    const int64_t bound = sf_jpeg_encode_bound(h, w, channels);
    SF_REQUIRE(out_image_stride >= bound, "sf_jpeg_encode: out_image_stride = %lld is smaller than sf_jpeg_encode_bound = %lld",
               (long long)out_image_stride, (long long)bound);
    SF_REQUIRE(((uintptr_t)out & 3) == 0 && out_image_stride % 4 == 0,
               "sf_jpeg_encode: out and out_image_stride = %lld must be multiples of 4", (long long)out_image_stride);
    SF_REQUIRE(((uintptr_t)out_bytes & 7) == 0, "sf_jpeg_encode: out_bytes is not 8-byte aligned");
    const int64_t need = sf_jpeg_encode_ws_bytes(n_images, h, w, channels);
    SF_REQUIRE(ws_bytes >= need, "sf_jpeg_encode: ws_bytes = %lld is smaller than sf_jpeg_encode_ws_bytes = %lld", (long long)ws_bytes,
               (long long)need);
    JpegArgs a;
    a.img = img, a.img_image_stride = img_image_stride, a.img_row_stride = img_row_stride;
    a.h = h, a.w = w, a.nc = channels, a.bw = (w + 7) / 8, a.bh = (h + 7) / 8, a.n_images = n_images;
    const int64_t intervals = (int64_t)n_images * a.bh;
    a.coef = reinterpret_cast<int16_t*>(((uintptr_t)ws + 15) & ~(uintptr_t)15);
    a.stage = reinterpret_cast<uint8_t*>(a.coef + intervals * a.bw * channels * 64);
    a.stage_stride = stage_stride_of(w, channels);
    a.ioff = reinterpret_cast<int64_t*>(a.stage + intervals * a.stage_stride);
    a.ibits = reinterpret_cast<uint32_t*>(a.ioff + intervals);
    a.ilen = a.ibits + intervals;
    a.out = out, a.out_image_stride = out_image_stride, a.out_bytes = out_bytes;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) a.q[t][k] = qtables[t * 64 + kZigzag[k]];
    const hipStream_t s = (hipStream_t)stream;
    const dim3 per_interval(a.bh, n_images);
    hipLaunchKernelGGL(jpeg_dct_kernel, dim3((a.bh * a.bw + kThreads - 1) / kThreads, n_images), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(jpeg_pack_kernel, per_interval, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(jpeg_count_kernel, per_interval, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3((n_images + 63) / 64), dim3(64), 0, s, a);
    hipLaunchKernelGGL(jpeg_gather_kernel, per_interval, dim3(kThreads), 0, s, a);
    return sf::check_launch("sf_jpeg_encode");
}
