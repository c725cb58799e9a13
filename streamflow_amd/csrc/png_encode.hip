// PNG encoding of a batch of device images into zlib streams (RFC 1950 / 1951, PNG specification sections 9 and 12.8): the adaptive
// row filter and a Huffman-only deflate, so that the colour-wheel and KITTI images sf_flow_to_image / sf_flow_to_kitti16 leave on the
// device cross to the host compressed.  The host keeps the chunk framing and the CRC-32 (flow_io.png_file).  The format -- filter
// choice, bands, table construction, header bits -- is restated in tests/png_encode_cases.py, and the output equals it byte for byte.
//
// Four launches behind one memset, every dependency between workgroups a launch boundary:
//   png_filter_kernel   one wave per row: the five filtered versions' sums of min(v, 256 - v), the cheapest type (ties: the lowest),
//                       the filtered scanline into the workspace.
//   png_table_kernel    one workgroup per band of SF_PNG_ENC_BAND_ROWS scanlines: byte histogram in LDS, the used symbols ranked by
//                       (frequency, symbol), Huffman's algorithm on two queues and the length limit by one thread, canonical codes;
//                       the same for the code-length alphabet; the block's exact bit length and the band's Adler-32 sums.
//   png_offsets_kernel  one thread per image: prefix sum of the blocks' bit lengths, the Adler-32 of the whole image, `78 01`, the
//                       checksum bytes and out_bytes.
//   png_pack_kernel     one workgroup per band: header items and literals, 4 items per thread and pass, their bit offsets by a
//                       workgroup scan, the bits ORed into the output with vector atomics (a 32-bit word is shared by neighbouring
//                       threads, passes and bands; the entry point clears sf_png_encode_bound bytes of every slot first).
// No workgroup waits for another, and every trip count is a function of (n, h, w, bpp): LDS holds tables and histograms only, a band
// is streamed from the workspace.
#include "sf_common.h"

namespace {

constexpr int kBand = SF_PNG_ENC_BAND_ROWS;
constexpr int kThreads = 256;
constexpr int kLit = 257;                                               // literals and end-of-block
constexpr int kHeaderItems = 1 + 19 + kLit + 2;                         // fixed fields, code-length code lengths, literal and distance lengths
constexpr int kHeaderBitsMax = 17 + 19 * 3 + (kLit + 2) * 7;
constexpr uint32_t kAdler = 65521;

// One band's record in the workspace (uint32 words): 257 literal and 16 code-length entries (bit-reversed code | length << 16),
// the code-length code lengths of symbols 0 .. 15 are the entries' lengths.
constexpr int kRecLit = 0, kRecCl = kLit, kRecBits = kLit + 16, kRecAdlerA = kRecBits + 1, kRecAdlerB = kRecBits + 2,
              kRecStartLo = kRecBits + 3, kRecStartHi = kRecBits + 4, kRecWords = 280;

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

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

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
// Rank of every used symbol by (frequency, symbol), by all threads: s_sym[r], s_w[r] for r < *s_n.  Barriers inside.
__device__ void rank_symbols(const int* freq, int nsym, uint16_t* s_sym, int* s_w, int* s_n) {
    if (threadIdx.x == 0) *s_n = 0;
    __syncthreads();
    for (int s = threadIdx.x; s < nsym; s += kThreads) {
        const int f = freq[s];
        if (f > 0) {
            int r = 0;
            for (int t = 0; t < nsym; ++t) {
                const int ft = freq[t];
                r += (ft > 0 && (ft < f || (ft == f && t < s))) ? 1 : 0;
            }
            s_sym[r] = (uint16_t)s, s_w[r] = f;
            atomicAdd(s_n, 1);
        }
    }
    __syncthreads();
}

// Code lengths of the n >= 2 ranked symbols, by ONE thread: Huffman's algorithm on two queues (the ranked leaves w[0 .. n), the
// created nodes w[n .. 2 n - 1) in creation order; a leaf is taken when its weight is <= the front node's), leaves per depth with
// depths above `limit` counted at the limit, then, while the Kraft sum is above 1, one code off the limit and one code of the deepest
// shorter length turned into two codes one bit longer (each step lowers the sum by 2^-limit and keeps the number of codes), and the
// lengths handed out along the rank, longest first: len[s_sym[r]].  w has room for 2 n - 1 weights, par for as many.
__device__ void huffman_lengths(int n, int limit, int* w, uint16_t* par, uint8_t* depth, const uint16_t* s_sym, uint8_t* len) {
    int i = 0, j = n;
    for (int k = n; k < 2 * n - 1; ++k) {
        int sum = 0;
        for (int two = 0; two < 2; ++two) {
            if (i < n && (j >= k || w[i] <= w[j])) par[i] = (uint16_t)k, sum += w[i], ++i;
            else par[j] = (uint16_t)k, sum += w[j], ++j;
        }
        w[k] = sum;
    }
    int count[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) count[l] = 0;
    depth[2 * n - 2] = 0;
    for (int m = 2 * n - 3; m >= 0; --m) {
        const int d = depth[par[m]] + 1;
        depth[m] = (uint8_t)(d > 255 ? 255 : d);                        // (a depth above the limit is all that is asked of it)
        if (m < n) {
            const int l = d < limit ? d : limit;
#pragma unroll
            for (int q = 1; q < 16; ++q) count[q] += q == l ? 1 : 0;    // static indices: `count` stays in registers
        }
    }
    int total = 0;
#pragma unroll
    for (int l = 1; l < 16; ++l) total += l <= limit ? count[l] << (limit - l) : 0;
    while (total > (1 << limit)) {
        int deepest = 0;
#pragma unroll
        for (int l = 1; l < 16; ++l) deepest = (l < limit && count[l] > 0) ? l : deepest;
#pragma unroll
        for (int l = 1; l < 16; ++l) count[l] += (l == limit ? -1 : 0) + (l == deepest ? -1 : 0) + (l == deepest + 1 ? 2 : 0);
        --total;
    }
    int r = 0;
#pragma unroll
    for (int l = 15; l >= 1; --l)
        for (int q = 0; q < count[l]; ++q) len[s_sym[r++]] = (uint8_t)l;
}

__device__ __forceinline__ uint32_t reversed(uint32_t code, int len) { return len ? __brev(code) >> (32 - len) : 0; }

// Canonical codes (RFC 1951 3.2.2) of len[0 .. nsym), by all threads: entry[s] = bit-reversed code | len << 16.  cnt[l] = the number
// of symbols of length l >= 1.  No barrier inside.
__device__ void canonical(const uint8_t* len, int nsym, const int* cnt, uint32_t* entry) {
    for (int s = threadIdx.x; s < nsym; s += kThreads) {
        const int l = len[s];
        uint32_t code = 0;
        for (int q = 1; q <= l; ++q) code = (code + (q > 1 ? cnt[q - 1] : 0)) << 1;
        for (int t = 0; t < s; ++t) code += len[t] == l ? 1 : 0;
        entry[s] = reversed(code, l) | ((uint32_t)l << 16);
    }
}

__global__ __launch_bounds__(kThreads) void png_table_kernel(EncArgs g) {
    __shared__ int s_hist[4][256];                                      // one histogram per wave
    __shared__ int s_freq[kLit + 3];
    __shared__ int s_w[2 * kLit];
    __shared__ uint16_t s_par[2 * kLit], s_sym[kLit + 3];
    __shared__ uint8_t s_depth[2 * kLit], s_len[kLit + 3], s_cllen[16];
    __shared__ int s_clfreq[16], s_n, s_bits;
    __shared__ uint32_t s_adler[2][4];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int rows = g.h - (int)blockIdx.x * kBand < kBand ? g.h - (int)blockIdx.x * kBand : kBand;
    const int64_t nbytes = rows * g.line;                               // < 2^31 / 1: the image's scanlines are
    const uint8_t* p = g.scan + (int64_t)blockIdx.y * g.scan_stride + (int64_t)blockIdx.x * kBand * g.line;     // 16-byte aligned
    uint32_t* rec = g.rec + ((int64_t)blockIdx.y * g.nbands + blockIdx.x) * kRecWords;

    for (int i = tid; i < 4 * 256; i += kThreads) (&s_hist[0][0])[i] = 0;
    __syncthreads();
    // Adler-32 of the band alone, without the leading 1: A = sum d, B = sum (nbytes - position) d, both mod 65521 at the end
    uint64_t A = 0, B = 0;
    const int64_t nwords = nbytes >> 2;
    for (int64_t i = tid; i < nwords; i += kThreads) {
        const uint32_t v = reinterpret_cast<const uint32_t*>(p)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t d = (v >> (8 * k)) & 255;
            atomicAdd(&s_hist[wave][d], 1);
            A += d, B += (uint64_t)(nbytes - (4 * i + k)) * d;
        }
    }
    if (tid < (int)(nbytes & 3)) {
        const int64_t pos = 4 * nwords + tid;
        const uint32_t d = p[pos];
        atomicAdd(&s_hist[wave][d], 1);
        A += d, B += (uint64_t)(nbytes - pos) * d;
    }
    int a32 = wave_sum((int)(A % kAdler)), b32 = wave_sum((int)(B % kAdler));          // 64 x 65520 fits
    if ((tid & 63) == 0) s_adler[0][wave] = (uint32_t)a32, s_adler[1][wave] = (uint32_t)b32;
    __syncthreads();
    s_freq[tid] = s_hist[0][tid] + s_hist[1][tid] + s_hist[2][tid] + s_hist[3][tid];
    s_len[tid] = 0;
    if (tid == 0) s_freq[256] = 1, s_len[256] = 0;                      // one end-of-block
    if (tid < 16) s_clfreq[tid] = 0;
    __syncthreads();

    // literal / end-of-block lengths, at most 15 bits
    rank_symbols(s_freq, kLit, s_sym, s_w, &s_n);
    if (tid == 0) {
        huffman_lengths(s_n, 15, s_w, s_par, s_depth, s_sym, s_len);
        // the fixed table 8 x 255, 9, 9 where it is cheaper: a band of N bytes then takes at most 9 N + 9 bits whatever it holds
        int64_t dyn = 0, fixed = 0;
        for (int s = 0; s < kLit; ++s) dyn += (int64_t)s_freq[s] * s_len[s], fixed += (int64_t)s_freq[s] * (s < 255 ? 8 : 9);
        if (dyn > fixed)
            for (int s = 0; s < kLit; ++s) s_len[s] = s < 255 ? 8 : 9;
        s_bits = (int)(dyn > fixed ? fixed : dyn);
    }
    __syncthreads();
    for (int s = tid; s < kLit; s += kThreads) atomicAdd(&s_clfreq[s_len[s]], 1);
    __syncthreads();
    canonical(s_len, kLit, s_clfreq, rec + kRecLit);                    // s_clfreq[l >= 1] counts the literal lengths so far
    __syncthreads();
    if (tid == 0) s_clfreq[1] += 2;                                     // the two distance codes of one bit
    if (tid < 16) s_cllen[tid] = 0;
    __syncthreads();

    // code-length alphabet (symbols 0 .. 15 only: no repeat codes), at most 7 bits; lengths 0 and 1 are always in use
    rank_symbols(s_clfreq, 16, s_sym, s_w, &s_n);
    if (tid == 0) {
        huffman_lengths(s_n, 7, s_w, s_par, s_depth, s_sym, s_cllen);
        int bits = 17 + 19 * 3 + s_bits;
        for (int l = 0; l < 16; ++l) bits += s_clfreq[l] * s_cllen[l];
        rec[kRecBits] = (uint32_t)bits;
        rec[kRecAdlerA] = (s_adler[0][0] + s_adler[0][1] + s_adler[0][2] + s_adler[0][3]) % kAdler;
        rec[kRecAdlerB] = (s_adler[1][0] + s_adler[1][1] + s_adler[1][2] + s_adler[1][3]) % kAdler;
    }
    __syncthreads();
    if (tid < 16) s_freq[tid] = 0;                                      // s_freq is free now: the counts per code-length code length
    __syncthreads();
    if (tid < 16 && s_cllen[tid]) atomicAdd(&s_freq[s_cllen[tid]], 1);
    __syncthreads();
    canonical(s_cllen, 16, s_freq, rec + kRecCl);
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
        const uint64_t nbytes = (uint64_t)rows * g.line;
        B = (B + (nbytes % kAdler) * A + rec[kRecAdlerB]) % kAdler;     // the bytes before this band are summed nbytes times more
        A = (A + rec[kRecAdlerA]) % kAdler;
    }
    const uint64_t total = (uint64_t)g.h * g.line;
    A = (A + 1) % kAdler, B = (B + total % kAdler) % kAdler;            // the leading 1, summed once per byte
    const int64_t end = (int64_t)((bit + 7) >> 3);
    uint8_t* out = g.out + (int64_t)i * g.out_image_stride;
    out[0] = 0x78, out[1] = 0x01;                                       // deflate, 32 KiB window, fastest level: (0x7801 % 31 == 0)
    out[end] = (uint8_t)(B >> 8), out[end + 1] = (uint8_t)B, out[end + 2] = (uint8_t)(A >> 8), out[end + 3] = (uint8_t)A;
    g.out_bytes[i] = end + 4;
}

// ---- 4. pack -----------------------------------------------------------------------------------------------------------------------
// `nbits` bits of `acc` at bit `pos` of the image's stream: at most 60 + 31 bits, three words.
__device__ __forceinline__ void put_bits(uint32_t* out32, uint64_t pos, uint64_t acc, int nbits) {
    if (nbits == 0) return;
    const int sh = (int)(pos & 31);
    const uint64_t lo = acc << sh;
    const uint32_t hi = sh ? (uint32_t)(acc >> (64 - sh)) : 0;
    uint32_t* q = out32 + (pos >> 5);
    if ((uint32_t)lo) atomicOr(q, (uint32_t)lo);
    if ((uint32_t)(lo >> 32)) atomicOr(q + 1, (uint32_t)(lo >> 32));
    if (hi) atomicOr(q + 2, hi);
}

// Exclusive prefix of `nbits` over the workgroup, added to *base; *base moves on by the workgroup's total.  Two barriers.
__device__ __forceinline__ uint64_t scan_bits(int nbits, uint64_t* base, int* s_wave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = nbits;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d, 64);
        incl += lane >= d ? t : 0;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < kThreads / 64; ++q) before += q < wave ? s_wave[q] : 0, all += s_wave[q];
    const uint64_t pos = *base + (uint64_t)(before + incl - nbits);
    *base += (uint64_t)all;
    __syncthreads();
    return pos;
}

__global__ __launch_bounds__(kThreads) void png_pack_kernel(EncArgs g) {
    __shared__ uint32_t s_lit[kLit], s_cl[16];
    __shared__ int s_wave[kThreads / 64];
    const int tid = threadIdx.x;
    const int rows = g.h - (int)blockIdx.x * kBand < kBand ? g.h - (int)blockIdx.x * kBand : kBand;
    const int64_t nbytes = rows * g.line;
    const uint8_t* p = g.scan + (int64_t)blockIdx.y * g.scan_stride + (int64_t)blockIdx.x * kBand * g.line;     // 16-byte aligned
    const uint32_t* rec = g.rec + ((int64_t)blockIdx.y * g.nbands + blockIdx.x) * kRecWords;
    uint32_t* out32 = reinterpret_cast<uint32_t*>(g.out + (int64_t)blockIdx.y * g.out_image_stride);           // 4-byte aligned
    for (int s = tid; s < kLit; s += kThreads) s_lit[s] = rec[kRecLit + s];
    if (tid < 16) s_cl[tid] = rec[kRecCl + tid];
    uint64_t base = rec[kRecStartLo] | ((uint64_t)rec[kRecStartHi] << 32);            // every thread keeps the same running offset
    __syncthreads();

    // the block header: BFINAL, BTYPE = 2, HLIT = 0 (257 codes), HDIST = 1 (two codes), HCLEN = 15 (19 lengths) as one item of 17 bits,
    // the 19 code-length code lengths in RFC 1951's order, the 257 + 2 lengths; two items per thread
    {
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        uint64_t acc = 0;
        int nbits = 0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int item = 2 * tid + k;
            uint32_t code = 0;
            int len = 0;
            if (item == 0) {
                code = ((int)blockIdx.x == g.nbands - 1 ? 1u : 0u) | (2u << 1) | (1u << 8) | (15u << 13), len = 17;
            } else if (item < 20) {
                int sym = 0;
#pragma unroll
                for (int q = 0; q < 19; ++q) sym = q == item - 1 ? order[q] : sym;
                code = sym < 16 ? s_cl[sym] >> 16 : 0, len = 3;
            } else if (item < kHeaderItems) {
                const int s = item - 20;
                const uint32_t e = s_cl[s < kLit ? s_lit[s] >> 16 : 1];
                code = e & 0xffff, len = (int)(e >> 16);
            }
            acc |= (uint64_t)code << nbits, nbits += len;
        }
        const uint64_t pos = scan_bits(nbits, &base, s_wave);
        put_bits(out32, pos, acc, nbits);
    }
    // the literals and the end-of-block: items 0 .. nbytes, four per thread and pass
    const int64_t passes = (nbytes + 1 + 4 * kThreads - 1) / (4 * kThreads);
    for (int64_t pass = 0; pass < passes; ++pass) {
        const int64_t d0 = (pass * kThreads + tid) * 4;
        uint32_t v = 0;
        if (d0 + 4 <= nbytes) {
            v = *reinterpret_cast<const uint32_t*>(p + d0);
        } else {
            for (int k = 0; k < 4; ++k) v |= d0 + k < nbytes ? (uint32_t)p[d0 + k] << (8 * k) : 0;
        }
        uint64_t acc = 0;
        int nbits = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t d = d0 + k;
            const uint32_t e = d < nbytes ? s_lit[(v >> (8 * k)) & 255] : (d == nbytes ? s_lit[256] : 0);
            acc |= (uint64_t)(e & 0xffff) << nbits, nbits += (int)(e >> 16);
        }
        const uint64_t pos = scan_bits(nbits, &base, s_wave);
        put_bits(out32, pos, acc, nbits);
    }
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
    hipError_t e = hipMemset2DAsync(out, (size_t)out_image_stride, 0, (size_t)bound, (size_t)n_images, s);
    if (e != hipSuccess) return sf::fail(SF_ERR_HIP, "sf_png_encode: clearing the slots: %s", hipGetErrorString(e));
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
