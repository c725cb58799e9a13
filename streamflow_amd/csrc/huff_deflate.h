// Huffman-only deflate blocks (RFC 1951) on the device, shared by csrc/png_encode.hip (a block per band of scanlines) and
// csrc/flo5_encode.hip (a block per segment of a byte plane).  A block is `nbytes` bytes at a 4-byte aligned pointer `p`, its record
// of kRecWords uint32 in the workspace, and its place in a stream: the 32-bit words `out32` of the stream's slot, the block's first
// bit, and whether it is the stream's last block.  Three steps, each behind a launch boundary of its caller:
//   table_block    by one workgroup: byte histogram in LDS, the used symbols ranked by (frequency, symbol), Huffman's algorithm on two
//                  queues and the length limit by one thread, canonical codes; the same for the code-length alphabet; the block's
//                  exact bit length and its Adler-32 sums -> the record.
//   (the caller)   prefix sum of the blocks' bit lengths -> kRecStartLo / kRecStartHi of every record; adler_append joins the sums.
//   pack_block     by one workgroup: header items and literals, 4 items per thread and pass, their bit offsets by a workgroup scan,
//                  the bits ORed into the stream with vector atomics (a 32-bit word is shared by neighbouring threads, passes and
//                  blocks: the slot is cleared beforehand).
// The block format -- header fields, table construction, the fixed-table replacement -- is the one include/streamflow_hip.h states
// for sf_png_encode and tests/png_encode_cases.py restates.  Every trip count is a function of nbytes alone; LDS holds tables and
// histograms only, the block is streamed from memory.
#pragma once
#include "sf_common.h"

namespace sf_huff {

constexpr int kThreads = 256;
constexpr int kLit = 257;                                               // literals and end-of-block
constexpr int kHeaderItems = 1 + 19 + kLit + 2;                         // fixed fields, code-length code lengths, literal and distance lengths
constexpr int kHeaderBitsMax = 17 + 19 * 3 + (kLit + 2) * 7;
constexpr uint32_t kAdler = 65521;

// One block's record in the workspace (uint32 words): 257 literal and 16 code-length entries (bit-reversed code | length << 16),
// the code-length code lengths of symbols 0 .. 15 are the entries' lengths.
constexpr int kRecLit = 0, kRecCl = kLit, kRecBits = kLit + 16, kRecAdlerA = kRecBits + 1, kRecAdlerB = kRecBits + 2,
              kRecStartLo = kRecBits + 3, kRecStartHi = kRecBits + 4, kRecWords = 280;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Rank of every used symbol by (frequency, symbol), by all threads: s_sym[r], s_w[r] for r < *s_n.  Barriers inside.
__device__ inline void rank_symbols(const int* freq, int nsym, uint16_t* s_sym, int* s_w, int* s_n) {
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
__device__ inline void huffman_lengths(int n, int limit, int* w, uint16_t* par, uint8_t* depth, const uint16_t* s_sym, uint8_t* len) {
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
__device__ inline void canonical(const uint8_t* len, int nsym, const int* cnt, uint32_t* entry) {
    for (int s = threadIdx.x; s < nsym; s += kThreads) {
        const int l = len[s];
        uint32_t code = 0;
        for (int q = 1; q <= l; ++q) code = (code + (q > 1 ? cnt[q - 1] : 0)) << 1;
        for (int t = 0; t < s; ++t) code += len[t] == l ? 1 : 0;
        entry[s] = reversed(code, l) | ((uint32_t)l << 16);
    }
}

// The tables, the bit length and the Adler-32 sums of one block, by a workgroup of kThreads: rec[kRecLit .. kRecAdlerB].
__device__ __forceinline__ void table_block(const uint8_t* p, int64_t nbytes, uint32_t* rec) {
    __shared__ int s_hist[4][256];                                      // one histogram per wave
    __shared__ int s_freq[kLit + 3];
    __shared__ int s_w[2 * kLit];
    __shared__ uint16_t s_par[2 * kLit], s_sym[kLit + 3];
    __shared__ uint8_t s_depth[2 * kLit], s_len[kLit + 3], s_cllen[16];
    __shared__ int s_clfreq[16], s_n, s_bits;
    __shared__ uint32_t s_adler[2][4];
    const int tid = threadIdx.x, wave = tid >> 6;

    for (int i = tid; i < 4 * 256; i += kThreads) (&s_hist[0][0])[i] = 0;
    __syncthreads();
    // Adler-32 of the block alone, without the leading 1: A = sum d, B = sum (nbytes - position) d, both mod 65521 at the end
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
        // the fixed table 8 x 255, 9, 9 where it is cheaper: a block of N bytes then takes at most 9 N + 9 bits whatever it holds
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

// The running Adler-32 sums (A, B; without the leading 1) of a stream after one more block of `nbytes` bytes with the record `rec`:
// the bytes before the block are summed nbytes times more.
__device__ __forceinline__ void adler_append(uint64_t& A, uint64_t& B, const uint32_t* rec, uint64_t nbytes) {
    B = (B + (nbytes % kAdler) * A + rec[kRecAdlerB]) % kAdler;
    A = (A + rec[kRecAdlerA]) % kAdler;
}

// `78 01` in front of a stream of `total` bytes whose blocks end at bit `bit`, the big-endian Adler-32 behind them; the stream's length.
__device__ __forceinline__ int64_t stream_ends(uint8_t* out, uint64_t bit, uint64_t A, uint64_t B, uint64_t total) {
    A = (A + 1) % kAdler, B = (B + total % kAdler) % kAdler;            // the leading 1, summed once per byte
    const int64_t end = (int64_t)((bit + 7) >> 3);
    out[0] = 0x78, out[1] = 0x01;                                       // deflate, 32 KiB window, fastest level: (0x7801 % 31 == 0)
    out[end] = (uint8_t)(B >> 8), out[end + 1] = (uint8_t)B, out[end + 2] = (uint8_t)(A >> 8), out[end + 3] = (uint8_t)A;
    return end + 4;
}

// `nbits` bits of `acc` at bit `pos` of the stream: at most 60 + 31 bits, three words.
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

// One block's bits into its stream, by a workgroup of kThreads: the record's tables and start bit, the bytes of the block once more.
__device__ __forceinline__ void pack_block(const uint8_t* p, int64_t nbytes, const uint32_t* rec, uint32_t* out32, bool final) {
    __shared__ uint32_t s_lit[kLit], s_cl[16];
    __shared__ int s_wave[kThreads / 64];
    const int tid = threadIdx.x;
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
                code = (final ? 1u : 0u) | (2u << 1) | (1u << 8) | (15u << 13), len = 17;
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

}  // namespace sf_huff
