// Baseline JPEG decoding (ITU-T T.81, sequential DCT, 8 bit, Huffman) of a batch of files of one geometry into device images: the
// frames of a Motion-JPEG AVI file or of a directory of .jpg files become uint8 [n][h][w][3] where predict_video reads them.  The
// host walks the marker segments (jpeg_gpu.parse) and uploads the entropy-coded bytes as they are, one descriptor per restart
// interval and the de-duplicated table sets; everything from the first Huffman code to the RGB byte happens here.  The format
// subset, the arithmetic and the status words are stated in include/streamflow_hip.h and restated in tests/jpeg_decode_cases.py;
// the output equals that restatement, and libjpeg's, bit for bit.
//
// One clear launch (sf::fill_async) and four more, every dependency between workgroups a launch boundary:
//   jpeg_entropy_kernel  one wave per restart interval.  The decoder is csrc/jpeg_decode_core.h, the same code the sanitized host
//                        program runs; this file adds the wave's policy.  The decode state (bit buffer, positions, symbol, DC
//                        predictions) is the same in all 64 lanes; the lanes differ where they share work: the input window, the
//                        table build, and the block store -- lane k holds coefficient k, so a finished block leaves as one
//                        coalesced 128-byte store and the coefficient workspace needs no clearing.
//   jpeg_status_kernel   one thread per image: the first failed interval's status, or whether the clean ones cover its MCUs.
//   jpeg_idct_kernel     one thread per 8 x 8 block: libjpeg's jidctint "islow" in 32-bit integers, uint8 samples into the
//                        component's plane (padded to whole blocks).
//   jpeg_colour_kernel   one thread per output pixel: libjpeg's "fancy" chroma upsampling and the JFIF YCbCr -> RGB conversion.
// No workgroup waits for another; there is no flag, no spinning and no host synchronisation.
//
// The two invariants of the entropy stage, for ANY input (the core's header comment has the argument; here is where this policy
// keeps them):
//   (a) window() reads in[q] only for q < in_len, and `in` already points at the interval's own range, which desc_ok() has checked
//       against the buffer; store() writes the 128 bytes of block_index(), which the core bounds to the interval's own MCUs.
//   (b) the policy's only loop is window()'s lane-strided fill of kWinBytes + 8 bytes; the only barrier is the one of this
//       single-wave workgroup.
//
// The split route (sf_jpeg_decode_split; the functions are csrc/jpeg_sync_core.h, the same ones csrc/host/jpeg_sync_host_main.cpp
// runs under the host sanitizers).  One wave per interval leaves a file without DRI -- one interval -- to one wave, so an interval
// of at least split_min_bytes is decoded a THREAD per segment of segment_bytes unstuffed bytes instead, by the self-synchronising
// method the core's header describes.  Two more clear launches (the coefficient area: a block may be written by two segments, each its
// own coefficients; the workgroup map; the error keys) and seven more launches in front of jpeg_entropy_kernel, which skips the
// intervals that split; again every dependency between workgroups is a launch boundary, there is no flag, no spinning, no host
// synchronisation, and the only atomics are vector atomics (min on an interval's key, add / max on an image's words, an LDS min):
//   jpeg_plan_kernel     one workgroup scans desc: an acceptable interval of in_len >= split_min_bytes gets ceil(max(1, ceil(in_len /
//                        segment_bytes)) / kSegThreads) workgroups of segment slots and align16(in_len) bytes of the unstuffed area,
//                        both by exclusive scans.  The host never reads desc: it sizes the grids and the areas from the bounds
//                        data_bytes / (segment_bytes kSegThreads) + n_intervals and data_bytes + 16 n_intervals, which intervals
//                        that do not overlap always fit; one that does not fit stays on the wave route.
//   jpeg_unstuff_kernel  a workgroup per split interval, windows of kSegThreads chunks of segment_bytes: count, scan, copy; the
//                        first FF without its 00 ends the stream there (its length and SF_JPEG_BAD_MARKER go to u_len / u_err).
//   jpeg_spec_kernel     a thread per segment: the lenient walk from (first bit of the segment, slot 0, k 0).
//   jpeg_sync_kernel     a workgroup per split interval, windows of kSegThreads segments in stream order: the window's first segment
//                        enters with the previous window's final exit (the interval's first with (0, 0, 0)); each round hands
//                        segment k the exit of segment k - 1, and the segments whose entry changed walk again; until a round changes
//                        nothing -- at most the window's segment count, by induction from its first segment.  A scan of the block
//                        counts then gives every segment the ordinal of its first block.
//   jpeg_write_kernel    a thread per segment: the strict walk from the true entry; AC coefficients dequantised and the raw DC
//                        difference into the block, errors into the interval's key by atomicMin.
//   jpeg_dc_kernel       a workgroup per split interval and component: 64-bit prefix sums of the DC differences in scan order, the
//                        DC range checks, the dequantised DC into coefficient 0, the block's sum check.
//   jpeg_finish_kernel   a thread per interval: the smallest key's status into the image's first_error / covered words, as
//                        jpeg_entropy_kernel does for its intervals.
// The two invariants of the split route, for ANY input:
//   (a) desc is checked once, by jpeg_plan_kernel (desc_ok), and only intervals that passed are in first_wg / wg_interval, which
//       nothing but that kernel writes.  `data` is read through in = data + in_off at indices < in_len only (unstuff_count / _copy);
//       every later stage reads the interval's own unstuffed bytes u[0 .. u_len), u_len <= in_len <= its share of the area.  Segment
//       words are read and written at slots first_wg kSegThreads + seg with seg < nseg <= the slots jpeg_plan_kernel gave the
//       interval.  Coefficients: SegSink::begin is called by strict_segment with ordinal < n_mcus x blocks per MCU only, so
//       block_index() is a block of the interval's own MCUs, and put() writes one of its 64 coefficients; jpeg_dc_kernel visits the
//       same blocks.  States read back from the workspace are clamped to their ranges before use.
//   (b) both walks consume a bit per iteration and stop within 8 segment_bytes + 27 bits; jpeg_sync_kernel's round loop has a hard
//       cap of kSegThreads + 1 rounds on top of the inductive bound; the scans are log2 steps of barriers that every thread of the
//       workgroup reaches (the early exits in front of them are uniform per workgroup); jpeg_plan_kernel's loop over its
//       workgroups is bounded by the capacity it checked.  Nothing waits for anything.
#include "sf_common.h"
#include "jpeg_sync_core.h"

namespace {

using namespace sf_jpegdec;

constexpr int kWave = 64;
constexpr int kWinBytes = 512;                                          // input window in LDS, plus two words so that a read may straddle
constexpr int kThreads = 256;

struct DecodeArgs {
    const uint8_t* data;
    int64_t data_bytes;
    const int64_t* desc;                                                // [n_intervals][kDescWords]
    const uint8_t* tables;                                              // [n_sets][kSetBytes]
    int n_intervals, n_sets, n_images, h, w;
    Geom g;
    int16_t* coef;                                                      // [n][component][block row][block column][64], dequantised, natural order
    uint8_t* planes;                                                    // [n][component][8 bh][8 bw]
    uint32_t* first_error;                                              // [n]: ~(interval << 5 | status) of the first failed interval, 0: none
    uint32_t* covered;                                                  // [n]: MCUs of the clean intervals
    int32_t* status;
    uint8_t* out;
    int64_t out_image_stride, out_row_stride;
    int out_channels;
    const int32_t* split_first;                                         // the split route's first_wg, or null: intervals >= 0 are not the wave's
};

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

struct WavePolicy {
    const uint8_t* in;                                                  // the interval's input, in_len bytes
    int64_t in_len;
    uint32_t* win;                                                      // LDS: input bytes [win_base, win_base + kWinBytes + 8), zeros past in_len
    int64_t win_base;
    int lane_;
    int16_t* coef_out;
    Geom g;
    int64_t image;
    int c_;                                                             // this lane's coefficient of the current block

    __device__ __forceinline__ void window(int64_t pos) {
        win_base = pos & ~(int64_t)3;
        uint8_t* wb = reinterpret_cast<uint8_t*>(win);
        __syncthreads();                                                // the reads of the old window are done
        for (int i = lane_; i < kWinBytes + 8; i += kWave) {
            const int64_t q = win_base + i;
            wb[i] = q < in_len ? in[q] : (uint8_t)0;                    // (a)
        }
        __syncthreads();
    }
    __device__ __forceinline__ uint32_t bytes(int64_t pos, int k) {
        if (pos < win_base || pos + 4 > win_base + kWinBytes) window(pos);
        const int off = (int)(pos - win_base), r = 8 * (off & 3);
        const uint64_t two = (uint64_t)win[(off >> 2) + 1] << 32 | win[off >> 2];
        const uint32_t be = __builtin_bswap32((uint32_t)(two >> r));    // byte pos on top
        return rfl(be >> (8 * (4 - k)));
    }
    __device__ __forceinline__ uint32_t uni(uint32_t v) { return rfl(v); }
    __device__ __forceinline__ int lane() { return lane_; }
    __device__ __forceinline__ int lanes() { return kWave; }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ void coef(int k, int v) {
        if (lane_ == k) c_ = v;
    }
    __device__ __forceinline__ void store(int c, int64_t mi, int j) {
        coef_out[block_index(g, image, c, mi, j) * 64 + lane_] = (int16_t)c_;      // (a); |c_| <= kCoefMax
        c_ = 0;
    }
};

// ---- 1. entropy decode --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void jpeg_entropy_kernel(DecodeArgs a) {
    __shared__ Tables tables;
    __shared__ uint32_t win[kWinBytes / 4 + 2];
    if (a.split_first && a.split_first[blockIdx.x] >= 0) return;        // decoded by the split route (uniform: one wave)
    const int64_t* d = a.desc + (int64_t)blockIdx.x * kDescWords;
    const int64_t mcus = mcu_count(a.g);
    int st;
    if (!desc_ok(d, a.data_bytes, a.n_images, mcus, a.n_sets)) {
        st = kBadDesc;
    } else {
        const int64_t in_off = d[0], in_len = d[1], image = d[2], first = d[3], n = d[4], set = d[5];
        WavePolicy p{a.data + in_off, in_len, win, -(int64_t)(2 * kWinBytes), (int)threadIdx.x, a.coef, a.g, image, 0};
        st = build_tables(p, tables, a.tables + set * kSetBytes, a.g.nc);
        if (st == kOk) st = decode_interval(p, tables, a.g, in_len, first, n);
    }
    if (threadIdx.x == 0) {
        const int64_t image = desc_image(d, a.n_images);
        if (st != kOk) atomicMax(a.first_error + image, ~((uint32_t)blockIdx.x << 5 | (uint32_t)st));
        else atomicAdd(a.covered + image, (uint32_t)d[4]);
    }
}

// ---- 2. status -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void jpeg_status_kernel(DecodeArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n_images) return;
    const uint32_t e = a.first_error[i];
    a.status[i] = image_status(e ? (int64_t)(~e) : -1, a.covered[i], mcu_count(a.g));
}

// ---- 3. inverse DCT ------------------------------------------------------------------------------------------------------------------
// libjpeg's jidctint.c "islow" (Loeffler, Ligtenberg and Moschytz), one pass over 8 values STRIDE apart: CONST_BITS = 13, the
// constants FIX(0.298631336) .. FIX(3.072711026).  The caller descales.
template <int STRIDE>
__device__ __forceinline__ void idct8(const int* in, int* out) {
    int z2 = in[2 * STRIDE], z3 = in[6 * STRIDE];
    int z1 = (z2 + z3) * 4433;
    const int e2 = z1 - z3 * 15137, e3 = z1 + z2 * 6270;
    const int e0 = (in[0] + in[4 * STRIDE]) << 13, e1 = (in[0] - in[4 * STRIDE]) << 13;
    const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    int o0 = in[7 * STRIDE], o1 = in[5 * STRIDE], o2 = in[3 * STRIDE], o3 = in[1 * STRIDE];
    z1 = o0 + o3, z2 = o1 + o2, z3 = o0 + o2;
    int z4 = o1 + o3;
    const int z5 = (z3 + z4) * 9633;
    o0 *= 2446, o1 *= 16819, o2 *= 25172, o3 *= 12299;
    z1 *= -7373, z2 *= -20995, z3 *= -16069, z4 *= -3196;
    z3 += z5, z4 += z5;
    o0 += z1 + z3, o1 += z2 + z4, o2 += z2 + z3, o3 += z1 + z4;
    out[0 * STRIDE] = t10 + o3, out[7 * STRIDE] = t10 - o3;
    out[1 * STRIDE] = t11 + o2, out[6 * STRIDE] = t11 - o2;
    out[2 * STRIDE] = t12 + o1, out[5 * STRIDE] = t12 - o1;
    out[3 * STRIDE] = t13 + o0, out[4 * STRIDE] = t13 - o0;
}

__global__ __launch_bounds__(kThreads) void jpeg_idct_kernel(DecodeArgs a) {
    const int c = blockIdx.z, bw = a.g.bw[c];
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= bw * a.g.bh[c]) return;                                    // no barrier in this kernel
    const int by = b / bw, bx = b - by * bw;
    const int64_t block = (int64_t)blockIdx.y * a.g.image_blocks + a.g.comp_off[c] + b;
    const uint4* src = reinterpret_cast<const uint4*>(a.coef + block * 64);      // 128-byte aligned
    int v[64], t[64];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 q = src[i];
        const uint32_t wv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) v[8 * i + j] = (int)(int16_t)(wv[j >> 1] >> (16 * (j & 1)));
    }
#pragma unroll
    for (int x = 0; x < 8; ++x) {                                       // columns: PASS1_BITS = 2 fraction bits stay
        idct8<8>(v + x, t + x);
#pragma unroll
        for (int y = 0; y < 8; ++y) t[8 * y + x] = (t[8 * y + x] + 1024) >> 11;
    }
    uint8_t* dst = a.planes + block * 64 - (int64_t)b * 64 + ((int64_t)by * 8 * bw + bx) * 8;
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        idct8<1>(t + 8 * y, v + 8 * y);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const uint32_t s = (uint32_t)min(max(((v[8 * y + x] + (1 << 17)) >> 18) + 128, 0), 255);
            if (x < 4) lo |= s << (8 * x);
            else hi |= s << (8 * (x - 4));
        }
        *reinterpret_cast<uint2*>(dst + (int64_t)y * 8 * bw) = make_uint2(lo, hi);
    }
}

// ---- 4. upsampling and colour --------------------------------------------------------------------------------------------------------
// libjpeg's jdsample.c "fancy" (triangle) filters on one chroma plane of cw x ch real samples, row stride ps.
__device__ __forceinline__ int chroma_h2v1(const uint8_t* row, int x, int cw) {
    const int i = x >> 1, c = row[i];
    if (x & 1) return i == cw - 1 ? c : (3 * c + row[i + 1] + 2) >> 2;
    return i == 0 ? c : (3 * c + row[i - 1] + 1) >> 2;
}

__device__ __forceinline__ int chroma_h2v2(const uint8_t* plane, int64_t ps, int x, int y, int cw, int ch) {
    const int cy = y >> 1, ny = min(max((y & 1) ? cy + 1 : cy - 1, 0), ch - 1);  // the nearer neighbour row, the edge rows replicated
    const uint8_t *r0 = plane + cy * ps, *r1 = plane + ny * ps;
    const int i = x >> 1, t = 3 * r0[i] + r1[i];
    if (x & 1) return i == cw - 1 ? (4 * t + 7) >> 4 : (3 * t + 3 * r0[i + 1] + r1[i + 1] + 7) >> 4;
    return i == 0 ? (4 * t + 8) >> 4 : (3 * t + 3 * r0[i - 1] + r1[i - 1] + 8) >> 4;
}

__global__ __launch_bounds__(kThreads) void jpeg_colour_kernel(DecodeArgs a) {
    const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y;
    if (x >= a.w) return;
    const Geom& g = a.g;
    const uint8_t* base = a.planes + (int64_t)blockIdx.z * g.image_blocks * 64;
    const int Y = base[(int64_t)y * 8 * g.bw[0] + x];
    uint8_t* o = a.out + (int64_t)blockIdx.z * a.out_image_stride + (int64_t)y * a.out_row_stride + (int64_t)x * a.out_channels;
    if (g.nc == 1) {
        o[0] = (uint8_t)Y;
        if (a.out_channels == 3) o[1] = (uint8_t)Y, o[2] = (uint8_t)Y;
        return;
    }
    const int64_t ps = 8 * (int64_t)g.bw[1];
    const uint8_t *pb = base + g.comp_off[1] * 64, *pr = base + g.comp_off[2] * 64;
    const int cw = (a.w + g.hs - 1) / g.hs, ch = (a.h + g.vs - 1) / g.vs;
    int cb, cr;
    if (g.hs == 1) cb = pb[y * ps + x], cr = pr[y * ps + x];
    else if (cw <= 2) cb = pb[(y / g.vs) * ps + (x >> 1)], cr = pr[(y / g.vs) * ps + (x >> 1)];       // libjpeg: too narrow for the filter
    else if (g.vs == 1) cb = chroma_h2v1(pb + y * ps, x, cw), cr = chroma_h2v1(pr + y * ps, x, cw);
    else cb = chroma_h2v2(pb, ps, x, y, cw, ch), cr = chroma_h2v2(pr, ps, x, y, cw, ch);
    cb -= 128, cr -= 128;
    o[0] = (uint8_t)min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
    o[1] = (uint8_t)min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
    o[2] = (uint8_t)min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
}

// ---- the split route -------------------------------------------------------------------------------------------------------------------
constexpr int kSegThreads = kSyncWindow;                                      // the per-segment workgroup, and jpeg_sync_kernel's window
constexpr int kDcThreads = 1024;

struct SplitArgs {
    int segment_bytes;
    int64_t split_min_bytes;
    int64_t wg_cap, u_cap;                                              // workgroups of kSegThreads segment slots; bytes of `ustream`
    int32_t* first_wg;                                                  // [n_intervals]: the interval's first workgroup, -1: the wave route
    int64_t* u_off;                                                     // [n_intervals]: its unstuffed bytes start at ustream + u_off ...
    int64_t* u_len;                                                     //                ... and are u_len bytes
    int32_t* u_err;                                                     // [n_intervals]: kBadMarker where they end at a marker
    unsigned long long* err_key;                                        // [n_intervals]: the smallest error key, kNoError: none
    int32_t* wg_interval;                                               // [wg_cap]: the interval a workgroup of segment slots belongs to, -1: none
    uint8_t* ustream;
    int64_t* ex_bit;                                                    // [wg_cap kSegThreads]: a segment's exit state ...
    int32_t* ex_sk;                                                     //                       ... slot << 8 | k
    int32_t* nblk;                                                      // the blocks its walk ended
    int64_t* first_blk;                                                 // the ordinal of the block its entry lies in
};

// every thread decodes its own segment: nothing is uniform across the lanes but the tables
struct LanePolicy {
    int lane_, lanes_;
    __device__ __forceinline__ uint32_t uni(uint32_t v) { return v; }
    __device__ __forceinline__ int lane() { return lane_; }
    __device__ __forceinline__ int lanes() { return lanes_; }
    __device__ __forceinline__ void sync() { __syncthreads(); }
};

// Inclusive scan over the N threads of the workgroup; sh[N - 1] is the total until the next call.  Every thread calls it.
template <int N>
__device__ __forceinline__ int64_t block_scan(int64_t v, int64_t* sh) {
    const int t = threadIdx.x;
    __syncthreads();                                                    // the reads of the previous call's total are done
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < N; d <<= 1) {
        const int64_t o = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += o;
        __syncthreads();
    }
    return sh[t];
}

__device__ __forceinline__ int64_t seg_count(int64_t bytes, int segment_bytes) {
    const int64_t n = (bytes + segment_bytes - 1) / segment_bytes;
    return n < 1 ? 1 : n;                                               // an empty stream still has a segment: someone reports kTruncated
}

__global__ __launch_bounds__(kSegThreads) void jpeg_plan_kernel(DecodeArgs a, SplitArgs s) {
    __shared__ int64_t sh_wg[kSegThreads], sh_u[kSegThreads];
    const int64_t mcus = mcu_count(a.g);
    int64_t carry_wg = 0, carry_u = 0;                                  // each saturates at its capacity + 1
    for (int base = 0; base < a.n_intervals; base += kSegThreads) {
        const int i = base + (int)threadIdx.x;
        int64_t nwg = 0, ub = 0;
        if (i < a.n_intervals) {
            const int64_t* d = a.desc + (int64_t)i * kDescWords;
            if (desc_ok(d, a.data_bytes, a.n_images, mcus, a.n_sets) && d[1] >= s.split_min_bytes) {
                nwg = (seg_count(d[1], s.segment_bytes) + kSegThreads - 1) / kSegThreads;
                ub = (d[1] + 15) & ~(int64_t)15;
                nwg = min(nwg, s.wg_cap + 1), ub = min(ub, s.u_cap + 16);
            }
        }
        const int64_t end_wg = carry_wg + block_scan<kSegThreads>(nwg, sh_wg), end_u = carry_u + block_scan<kSegThreads>(ub, sh_u);
        if (i < a.n_intervals) {
            const bool split = nwg > 0 && end_wg <= s.wg_cap && end_u <= s.u_cap;
            s.first_wg[i] = split ? (int32_t)(end_wg - nwg) : -1;       // wg_cap < 2^31
            s.u_off[i] = end_u - ub;
            if (split)
                for (int64_t j = end_wg - nwg; j < end_wg; ++j) s.wg_interval[j] = i;      // (a) j < wg_cap
        }
        carry_wg = min(carry_wg + sh_wg[kSegThreads - 1], s.wg_cap + 1);
        carry_u = min(carry_u + sh_u[kSegThreads - 1], s.u_cap + 1);
    }
}

__global__ __launch_bounds__(kSegThreads) void jpeg_unstuff_kernel(DecodeArgs a, SplitArgs s) {
    __shared__ int64_t sh[kSegThreads];
    __shared__ int first_marker;
    const int i = blockIdx.x, t = threadIdx.x;
    if (s.first_wg[i] < 0) return;
    const int64_t* d = a.desc + (int64_t)i * kDescWords;
    const uint8_t* in = a.data + d[0];
    const int64_t in_len = d[1];
    uint8_t* dst = s.ustream + s.u_off[i];
    int64_t done = 0;
    int err = 0;
    for (int64_t base = 0; base < in_len; base += (int64_t)kSegThreads * s.segment_bytes) {
        if (t == 0) first_marker = kSegThreads;
        __syncthreads();
        const int64_t lo = base + (int64_t)t * s.segment_bytes, hi = min(lo + s.segment_bytes, in_len);
        bool marker = false;
        int n = lo < in_len ? unstuff_count(in, in_len, lo, hi, marker) : 0;
        if (marker) atomicMin(&first_marker, t);
        __syncthreads();
        const int fm = first_marker;
        if (t > fm) n = 0;                                              // behind the marker nothing belongs to the stream
        const int64_t end = done + block_scan<kSegThreads>(n, sh);
        if (n > 0) unstuff_copy(in, in_len, lo, hi, dst + end - n);     // (a) end <= in_len
        done += sh[kSegThreads - 1];
        if (fm < kSegThreads) {
            err = kBadMarker;
            break;
        }
    }
    if (t == 0) s.u_len[i] = done, s.u_err[i] = err;
}

// What a thread knows of the split interval it works on (jpeg_plan_kernel has checked its descriptor, jpeg_unstuff_kernel has
// written u_len / u_err).
struct SegWork {
    int i;
    const int64_t* d;
    const uint8_t* u;
    int64_t ulen, nseg;
    int err;
};

__device__ __forceinline__ SegWork seg_work(const DecodeArgs& a, const SplitArgs& s, int i) {
    SegWork w;
    w.i = i, w.d = a.desc + (int64_t)i * kDescWords;
    w.u = s.ustream + s.u_off[i];
    w.ulen = s.u_len[i], w.err = s.u_err[i];
    w.nseg = seg_count(w.ulen, s.segment_bytes);
    return w;
}

__device__ __forceinline__ int64_t seg_end_bit(const SegWork& w, int64_t seg, int segment_bytes) {
    return 8 * min((seg + 1) * segment_bytes, w.ulen);
}

__global__ __launch_bounds__(kSegThreads) void jpeg_spec_kernel(DecodeArgs a, SplitArgs s) {
    __shared__ Tables tables;
    const int i = s.wg_interval[blockIdx.x];
    if (i < 0) return;
    const SegWork w = seg_work(a, s, i);
    LanePolicy p{(int)threadIdx.x, kSegThreads};
    if (build_tables(p, tables, a.tables + w.d[5] * kSetBytes, a.g.nc) != kOk) return;      // jpeg_sync_kernel reports it
    const int64_t seg = (int64_t)(blockIdx.x - s.first_wg[i]) * kSegThreads + threadIdx.x;
    if (seg >= w.nseg) return;
    const int64_t slot = (int64_t)blockIdx.x * kSegThreads + threadIdx.x;
    const SegExit e = lenient_segment(p, tables, a.g, w.u, w.ulen, w.err, 8 * seg * s.segment_bytes, 0, 0, seg_end_bit(w, seg, s.segment_bytes));
    s.ex_bit[slot] = e.bit, s.ex_sk[slot] = e.slot << 8 | e.k, s.nblk[slot] = e.blocks;
}

__global__ __launch_bounds__(kSegThreads) void jpeg_sync_kernel(DecodeArgs a, SplitArgs s) {
    __shared__ Tables tables;
    __shared__ int64_t sh_bit[kSegThreads], sh_scan[kSegThreads];
    __shared__ int sh_sk[kSegThreads];
    const int i = blockIdx.x, t = threadIdx.x;
    const int fw = s.first_wg[i];
    if (fw < 0) return;
    const SegWork w = seg_work(a, s, i);
    LanePolicy p{t, kSegThreads};
    const int ts = build_tables(p, tables, a.tables + w.d[5] * kSetBytes, a.g.nc);
    if (ts != kOk) {
        if (t == 0) atomicMin(s.err_key + i, (unsigned long long)error_key(0, 0, ts));
        return;
    }
    int64_t carry_bit = 0, carry_ord = 0;
    int carry_sk = 0;
    for (int64_t wbase = 0; wbase < w.nseg; wbase += kSegThreads) {
        const int64_t seg = wbase + t, slot = (int64_t)fw * kSegThreads + seg;
        const bool active = seg < w.nseg;
        const int last = (int)min((int64_t)kSegThreads, w.nseg - wbase) - 1;
        const int64_t end_bit = seg_end_bit(w, seg, s.segment_bytes);
        int64_t eb = 8 * seg * s.segment_bytes, xb = 0;                 // the entry jpeg_spec_kernel walked from
        int esk = 0, xsk = 0, nb = 0;
        if (active) xb = s.ex_bit[slot], xsk = s.ex_sk[slot], nb = s.nblk[slot];
        for (int round = 0; round <= kSegThreads; ++round) {            // (b) it ends by itself within last + 2 rounds
            sh_bit[t] = xb, sh_sk[t] = xsk;
            __syncthreads();
            const int64_t nbit = t == 0 ? carry_bit : sh_bit[t - 1];
            const int nsk = t == 0 ? carry_sk : sh_sk[t - 1];
            const bool changed = active && (nbit != eb || nsk != esk);
            if (changed) {
                eb = nbit, esk = nsk;
                const SegExit e = lenient_segment(p, tables, a.g, w.u, w.ulen, w.err, eb, esk >> 8, esk & 255, end_bit);
                xb = e.bit, xsk = e.slot << 8 | e.k, nb = e.blocks;
            }
            if (!__syncthreads_or(changed)) break;                      // also: everyone has read its neighbour's exit
        }
        const int64_t ord_end = carry_ord + block_scan<kSegThreads>(active ? nb : 0, sh_scan);
        sh_bit[t] = xb, sh_sk[t] = xsk;
        __syncthreads();
        if (active) s.ex_bit[slot] = xb, s.ex_sk[slot] = xsk, s.first_blk[slot] = ord_end - nb;
        carry_bit = sh_bit[last], carry_sk = sh_sk[last], carry_ord += sh_scan[kSegThreads - 1];
        __syncthreads();
    }
}

struct SegSink {
    int16_t* coef;
    const Geom& g;
    int64_t image, first_mcu;
    unsigned long long* key;
    int16_t* cur;
    __device__ __forceinline__ void begin(int64_t mcu, int slot) {
        cur = coef + block_index(g, image, slot_comp(g, slot), first_mcu + mcu, slot_block(g, slot)) * 64;      // (a)
    }
    __device__ __forceinline__ void put(int nat, int v) { cur[nat & 63] = (int16_t)v; }
    __device__ __forceinline__ void error(int64_t ordinal, int phase, int status) {
        atomicMin(key, (unsigned long long)error_key(ordinal, phase, status));
    }
};

__global__ __launch_bounds__(kSegThreads) void jpeg_write_kernel(DecodeArgs a, SplitArgs s) {
    __shared__ Tables tables;
    const int i = s.wg_interval[blockIdx.x];
    if (i < 0) return;
    const SegWork w = seg_work(a, s, i);
    LanePolicy p{(int)threadIdx.x, kSegThreads};
    if (build_tables(p, tables, a.tables + w.d[5] * kSetBytes, a.g.nc) != kOk) return;
    const int64_t seg = (int64_t)(blockIdx.x - s.first_wg[i]) * kSegThreads + threadIdx.x;
    if (seg >= w.nseg) return;
    const int64_t slot = (int64_t)blockIdx.x * kSegThreads + threadIdx.x;
    const int bpm = blocks_per_mcu(a.g);
    int64_t bit = 0, ord = s.first_blk[slot];
    int sk = 0;
    if (seg > 0) bit = s.ex_bit[slot - 1], sk = s.ex_sk[slot - 1];      // the predecessor is a segment of the same interval
    bit = min(max(bit, (int64_t)0), 8 * w.ulen);
    if (ord < 0) return;
    SegSink sink{a.coef, a.g, w.d[2], w.d[3], s.err_key + i, nullptr};
    strict_segment(p, sink, tables, a.g, w.u, w.ulen, w.err, bit, min(max(sk >> 8, 0), bpm - 1), sk & 63, seg_end_bit(w, seg, s.segment_bytes), ord,
                   w.d[4] * bpm, seg == w.nseg - 1);
}

__global__ __launch_bounds__(kDcThreads) void jpeg_dc_kernel(DecodeArgs a, SplitArgs s) {
    __shared__ int64_t sh[kDcThreads];
    const int i = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
    if (s.first_wg[i] < 0) return;
    const int64_t* d = a.desc + (int64_t)i * kDescWords;
    const int cb = comp_blocks(a.g, c), bpm = blocks_per_mcu(a.g), slot0 = c == 0 ? 0 : a.g.hs * a.g.vs + c - 1;
    const int64_t nblocks = d[4] * cb;
    const int q0 = a.tables[d[5] * kSetBytes + c * kCompBytes];
    int64_t carry = 0;
    for (int64_t base = 0; base < nblocks; base += kDcThreads) {
        const int64_t n = base + t, mcu = n / cb;
        const int j = (int)(n - mcu * cb);
        const bool active = n < nblocks;
        int16_t* blk = active ? a.coef + block_index(a.g, d[2], c, d[3] + mcu, j) * 64 : nullptr;      // (a) mcu < n_mcus, j < cb
        const int64_t pred = carry + block_scan<kDcThreads>(active ? blk[0] : 0, sh);
        if (active) {
            const int64_t ordinal = mcu * bpm + slot0 + j;
            int v;
            const int st = dc_value(pred, q0, v);
            if (st != kOk) atomicMin(s.err_key + i, (unsigned long long)error_key(ordinal, 0, st));
            blk[0] = (int16_t)v;
            const uint4* src = reinterpret_cast<const uint4*>(blk);      // 128-byte aligned
            int sum = v < 0 ? -v : v;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const uint4 q = src[r];
                const uint32_t wv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int e = (r == 0 ? 1 : 0); e < 8; ++e) {
                    const int x = (int)(int16_t)(wv[e >> 1] >> (16 * (e & 1)));
                    sum += x < 0 ? -x : x;
                }
            }
            if (sum > kBlockSumMax) atomicMin(s.err_key + i, (unsigned long long)error_key(ordinal, 2, kCoefRange));
        }
        carry += sh[kDcThreads - 1];
    }
}

__global__ __launch_bounds__(kSegThreads) void jpeg_finish_kernel(DecodeArgs a, SplitArgs s) {
    const int i = blockIdx.x * kSegThreads + threadIdx.x;
    if (i >= a.n_intervals || s.first_wg[i] < 0) return;
    const int64_t* d = a.desc + (int64_t)i * kDescWords;
    const unsigned long long key = s.err_key[i];
    if (key != kNoError) atomicMax(a.first_error + d[2], ~((uint32_t)i << 5 | (uint32_t)key_status(key)));
    else atomicAdd(a.covered + d[2], (uint32_t)d[4]);
}

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// The split route's part of the workspace, behind sf_jpeg_decode's.  false: sizes this route does not take.
struct SplitLayout {
    int64_t wg_cap, u_cap, slots;
    int64_t first_wg, u_off, u_len, u_err, err_key, wg_interval, ustream, ex_bit, ex_sk, nblk, first_blk, bytes;        // offsets
};

bool split_layout(int64_t data_bytes, int n_intervals, int segment_bytes, SplitLayout& L) {
    if (data_bytes < 0 || data_bytes > (int64_t)1 << 40 || n_intervals < 1 || n_intervals > kMaxIntervals) return false;
    if (segment_bytes < kSegmentBytesMin || segment_bytes > kSegmentBytesMax || (segment_bytes & (segment_bytes - 1))) return false;
    L.wg_cap = data_bytes / ((int64_t)segment_bytes * kSegThreads) + n_intervals;
    if (L.wg_cap >= (int64_t)1 << 31) return false;
    L.u_cap = data_bytes + 16 * (int64_t)n_intervals;
    L.slots = L.wg_cap * kSegThreads;
    int64_t at = 0;
    auto take = [&](int64_t bytes) {
        const int64_t off = at;
        at += align_up(bytes, 128);
        return off;
    };
    L.first_wg = take(4 * (int64_t)n_intervals), L.u_off = take(8 * (int64_t)n_intervals), L.u_len = take(8 * (int64_t)n_intervals);
    L.u_err = take(4 * (int64_t)n_intervals);
    L.err_key = take(8 * (int64_t)n_intervals), L.wg_interval = take(4 * L.wg_cap);      // adjacent: one clear to 0xFF
    L.ustream = take(L.u_cap);
    L.ex_bit = take(8 * L.slots), L.ex_sk = take(4 * L.slots), L.nblk = take(4 * L.slots), L.first_blk = take(8 * L.slots);
    L.bytes = at;
    return true;
}

bool shape_ok(int n_images, int h, int w, int components, int hs, int vs) {
    if (n_images < 1 || n_images > 65535 || h < 1 || w < 1 || h > SF_JPEG_MAX_DIM || w > SF_JPEG_MAX_DIM) return false;
    if (components == 1) return hs == 1 && vs == 1;
    return components == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2));
}

// The refusals both entry points share, in the header's order; `fn` names the entry point in the message.
int check_args(const char* fn, const uint8_t* data, int64_t data_bytes, const int64_t* desc, int n_intervals, const uint8_t* tables,
               int n_table_sets, int n_images, int h, int w, int components, int hs, int vs, uint8_t* out, int64_t out_image_stride,
               int64_t out_row_stride, int out_channels, int32_t* status, void* ws) {
    SF_REQUIRE(data && desc && tables && out && status && ws, "%s: null argument (data / desc / tables / out / status / ws)", fn);
    SF_REQUIRE(data_bytes >= 0, "%s: data_bytes = %lld", fn, (long long)data_bytes);
    SF_REQUIRE(n_intervals >= 1 && n_intervals <= kMaxIntervals, "%s: n_intervals = %d (1 .. %d)", fn, n_intervals, kMaxIntervals);
    SF_REQUIRE(n_table_sets >= 1 && n_table_sets <= 65535, "%s: n_table_sets = %d (1 .. 65535)", fn, n_table_sets);
    SF_REQUIRE(n_images >= 1 && n_images <= 65535, "%s: n_images = %d (1 .. 65535)", fn, n_images);
    SF_REQUIRE(h >= 1 && w >= 1, "%s: bad size h = %d, w = %d", fn, h, w);
    SF_REQUIRE(components == 1 || components == 3, "%s: components = %d (1 or 3)", fn, components);
    SF_REQUIRE(components == 1 ? (hs == 1 && vs == 1) : ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)),
               "%s: luma sampling %d x %d with %d components (1 x 1, 2 x 1 or 2 x 2; grey: 1 x 1)", fn, hs, vs, components);
    SF_REQUIRE(out_channels == 3 || (out_channels == 1 && components == 1), "%s: out_channels = %d with %d components", fn, out_channels,
               components);
    if (h > SF_JPEG_MAX_DIM || w > SF_JPEG_MAX_DIM)
        return sf::fail(SF_ERR_UNSUPPORTED, "%s: h = %d, w = %d (at most SF_JPEG_MAX_DIM = %d)", fn, h, w, SF_JPEG_MAX_DIM);
    const int64_t row = (int64_t)w * out_channels;
    SF_REQUIRE(out_row_stride >= row, "%s: out_row_stride = %lld is smaller than w * out_channels = %lld", fn, (long long)out_row_stride,
               (long long)row);
    SF_REQUIRE(out_image_stride >= (int64_t)(h - 1) * out_row_stride + row,
               "%s: out_image_stride = %lld is smaller than (h - 1) * out_row_stride + w * out_channels = %lld", fn,
               (long long)out_image_stride, (long long)((int64_t)(h - 1) * out_row_stride + row));
    SF_REQUIRE(((uintptr_t)desc & 7) == 0, "%s: desc is not 8-byte aligned", fn);
    SF_REQUIRE(((uintptr_t)status & 3) == 0, "%s: status is not 4-byte aligned", fn);
    SF_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: ws is not 16-byte aligned", fn);
    return SF_OK;
}

// sf_jpeg_decode's part of the workspace, from the first 128-byte boundary in ws; returns the first byte behind it.
uint8_t* carve(DecodeArgs& a, void* ws) {
    const int64_t blocks = (int64_t)a.n_images * a.g.image_blocks;
    a.coef = reinterpret_cast<int16_t*>(((uintptr_t)ws + 127) & ~(uintptr_t)127);
    a.planes = reinterpret_cast<uint8_t*>(a.coef + blocks * 64);
    a.first_error = reinterpret_cast<uint32_t*>(a.planes + blocks * 64);
    a.covered = a.first_error + a.n_images;
    return reinterpret_cast<uint8_t*>(a.first_error) + align_up((int64_t)a.n_images * 8, 128);
}

// the launches behind the entropy stage: status, inverse DCT, upsampling and colour
void launch_pixels(const DecodeArgs& a, hipStream_t s) {
    const int max_blocks = a.g.bw[0] * a.g.bh[0];
    hipLaunchKernelGGL(jpeg_status_kernel, dim3((a.n_images + 63) / 64), dim3(64), 0, s, a);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((max_blocks + kThreads - 1) / kThreads, a.n_images, a.g.nc), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((a.w + kThreads - 1) / kThreads, a.h, a.n_images), dim3(kThreads), 0, s, a);
}

}  // namespace

extern "C" int64_t sf_jpeg_decode_ws_bytes(int n_images, int h, int w, int components, int hs, int vs) {
    if (!shape_ok(n_images, h, w, components, hs, vs)) return -1;
    const Geom g = make_geom(h, w, components, hs, vs);
    return 128 + (int64_t)n_images * g.image_blocks * (128 + 64) + align_up((int64_t)n_images * 8, 128);
}

extern "C" int sf_jpeg_decode(const uint8_t* data, int64_t data_bytes, const int64_t* desc, int n_intervals, const uint8_t* tables,
                              int n_table_sets, int n_images, int h, int w, int components, int hs, int vs, uint8_t* out,
                              int64_t out_image_stride, int64_t out_row_stride, int out_channels, int32_t* status, void* ws,
                              int64_t ws_bytes, void* stream) {
    const int rc = check_args("sf_jpeg_decode", data, data_bytes, desc, n_intervals, tables, n_table_sets, n_images, h, w, components, hs, vs, out,
                              out_image_stride, out_row_stride, out_channels, status, ws);
    if (rc != SF_OK) return rc;
    const int64_t need = sf_jpeg_decode_ws_bytes(n_images, h, w, components, hs, vs);
    SF_REQUIRE(ws_bytes >= need, "sf_jpeg_decode: ws_bytes = %lld is smaller than sf_jpeg_decode_ws_bytes = %lld", (long long)ws_bytes,
               (long long)need);
    DecodeArgs a;
    a.data = data, a.data_bytes = data_bytes, a.desc = desc, a.tables = tables;
    a.n_intervals = n_intervals, a.n_sets = n_table_sets, a.n_images = n_images, a.h = h, a.w = w;
    a.g = make_geom(h, w, components, hs, vs);
    carve(a, ws);
    a.status = status, a.out = out, a.out_image_stride = out_image_stride, a.out_row_stride = out_row_stride, a.out_channels = out_channels;
    a.split_first = nullptr;
    const hipStream_t s = (hipStream_t)stream;
    const int cleared = sf::fill_async("sf_jpeg_decode (clear)", a.first_error, 0, (int64_t)n_images * 8, s);
    if (cleared != SF_OK) return cleared;
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)n_intervals), dim3(kWave), 0, s, a);
    launch_pixels(a, s);
    return sf::check_launch("sf_jpeg_decode");
}

extern "C" int64_t sf_jpeg_decode_split_ws_bytes(int n_images, int h, int w, int components, int hs, int vs, int64_t data_bytes, int n_intervals,
                                                 int segment_bytes) {
    const int64_t base = sf_jpeg_decode_ws_bytes(n_images, h, w, components, hs, vs);
    SplitLayout L;
    if (base < 0 || !split_layout(data_bytes, n_intervals, segment_bytes, L)) return -1;
    return align_up(base, 128) + L.bytes;
}

extern "C" int sf_jpeg_decode_split(const uint8_t* data, int64_t data_bytes, const int64_t* desc, int n_intervals, const uint8_t* tables,
                                    int n_table_sets, int n_images, int h, int w, int components, int hs, int vs, uint8_t* out,
                                    int64_t out_image_stride, int64_t out_row_stride, int out_channels, int32_t* status, int segment_bytes,
                                    int64_t split_min_bytes, void* ws, int64_t ws_bytes, void* stream) {
    const int rc = check_args("sf_jpeg_decode_split", data, data_bytes, desc, n_intervals, tables, n_table_sets, n_images, h, w, components, hs, vs,
                              out, out_image_stride, out_row_stride, out_channels, status, ws);
    if (rc != SF_OK) return rc;
    SF_REQUIRE(segment_bytes >= kSegmentBytesMin && segment_bytes <= kSegmentBytesMax && (segment_bytes & (segment_bytes - 1)) == 0,
               "sf_jpeg_decode_split: segment_bytes = %d (a power of two in %d .. %d)", segment_bytes, kSegmentBytesMin, kSegmentBytesMax);
    SF_REQUIRE(split_min_bytes >= 0, "sf_jpeg_decode_split: split_min_bytes = %lld", (long long)split_min_bytes);
    const int64_t need = sf_jpeg_decode_split_ws_bytes(n_images, h, w, components, hs, vs, data_bytes, n_intervals, segment_bytes);
    SF_REQUIRE(need >= 0 && ws_bytes >= need, "sf_jpeg_decode_split: ws_bytes = %lld is smaller than sf_jpeg_decode_split_ws_bytes = %lld",
               (long long)ws_bytes, (long long)need);
    DecodeArgs a;
    a.data = data, a.data_bytes = data_bytes, a.desc = desc, a.tables = tables;
    a.n_intervals = n_intervals, a.n_sets = n_table_sets, a.n_images = n_images, a.h = h, a.w = w;
    a.g = make_geom(h, w, components, hs, vs);
    uint8_t* x = carve(a, ws);
    a.status = status, a.out = out, a.out_image_stride = out_image_stride, a.out_row_stride = out_row_stride, a.out_channels = out_channels;
    a.split_first = nullptr;
    const hipStream_t s = (hipStream_t)stream;
    int cleared = sf::fill_async("sf_jpeg_decode_split (clear)", a.first_error, 0, (int64_t)n_images * 8, s);
    if (cleared != SF_OK) return cleared;
    if (split_min_bytes <= data_bytes) {                                // else no acceptable interval is that long: sf_jpeg_decode's launches
        SplitLayout L;
        split_layout(data_bytes, n_intervals, segment_bytes, L);
        SplitArgs p;
        p.segment_bytes = segment_bytes, p.split_min_bytes = split_min_bytes, p.wg_cap = L.wg_cap, p.u_cap = L.u_cap;
        p.first_wg = reinterpret_cast<int32_t*>(x + L.first_wg), p.u_off = reinterpret_cast<int64_t*>(x + L.u_off);
        p.u_len = reinterpret_cast<int64_t*>(x + L.u_len), p.u_err = reinterpret_cast<int32_t*>(x + L.u_err);
        p.err_key = reinterpret_cast<unsigned long long*>(x + L.err_key), p.wg_interval = reinterpret_cast<int32_t*>(x + L.wg_interval);
        p.ustream = x + L.ustream, p.ex_bit = reinterpret_cast<int64_t*>(x + L.ex_bit), p.ex_sk = reinterpret_cast<int32_t*>(x + L.ex_sk);
        p.nblk = reinterpret_cast<int32_t*>(x + L.nblk), p.first_blk = reinterpret_cast<int64_t*>(x + L.first_blk);
        a.split_first = p.first_wg;
        cleared = sf::fill_async("sf_jpeg_decode_split (clear)", a.coef, 0, (int64_t)n_images * a.g.image_blocks * 128, s);
        if (cleared == SF_OK) cleared = sf::fill_async("sf_jpeg_decode_split (clear)", p.err_key, 0xFF, L.ustream - L.err_key, s);
        if (cleared != SF_OK) return cleared;
        const dim3 seg_grid((unsigned)L.wg_cap), iv_grid((unsigned)n_intervals), tb(kSegThreads);
        hipLaunchKernelGGL(jpeg_plan_kernel, dim3(1), tb, 0, s, a, p);
        hipLaunchKernelGGL(jpeg_unstuff_kernel, iv_grid, tb, 0, s, a, p);
        hipLaunchKernelGGL(jpeg_spec_kernel, seg_grid, tb, 0, s, a, p);
        hipLaunchKernelGGL(jpeg_sync_kernel, iv_grid, tb, 0, s, a, p);
        hipLaunchKernelGGL(jpeg_write_kernel, seg_grid, tb, 0, s, a, p);
        hipLaunchKernelGGL(jpeg_dc_kernel, dim3((unsigned)n_intervals, components), dim3(kDcThreads), 0, s, a, p);
        hipLaunchKernelGGL(jpeg_finish_kernel, dim3((n_intervals + kSegThreads - 1) / kSegThreads), tb, 0, s, a, p);
    }
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)n_intervals), dim3(kWave), 0, s, a);
    launch_pixels(a, s);
    return sf::check_launch("sf_jpeg_decode_split");
}
