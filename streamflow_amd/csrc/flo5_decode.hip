// Spring's .flo5 ground truth decoded on the device: a batch of zlib streams inflated by sf_inflate (generic: it knows nothing of
// HDF5), and the inflated chunks of n files of one geometry put together as [n][H][W][2] by sf_flo5_assemble.  A file h5py wrote is
// about a thousand independent streams of 65 280 bytes (chunks (68, 240, 1) of a 2160 x 3840 x 2 field), which is what makes a
// serial format a GPU workload: inflate_kernel runs ONE WAVE PER STREAM and as many streams at a time as the chip holds waves.
//
// inflate_kernel.  The decoder is csrc/inflate_core.h, the same code the sanitized host program runs; this file adds the wave's
// policy.  The decode state (bit buffer, positions, symbol) is the same in all 64 lanes and held in scalar registers (every value
// that comes out of LDS or global memory goes through readfirstlane); the lanes differ only where they share work: filling the
// input window and the first-level tables, storing literals, copying matches, the Adler-32 pass.
//
// The two invariants, for ANY input bytes (the core's header comment has the argument; here is where this policy keeps them):
//   (a) every read of `in` is at an index checked against in_len and every access of `out` at an index checked against out_len on
//       the same line; `in` and `out` already point at the stream's own ranges, which the kernel checks against the buffers first.
//   (b) the policy has four loops: window() and the copy loops of match() / raw() / adler() -- each a lane-strided walk over a range
//       whose length the core has bounded (520, len <= 258, n <= out_len).  No loop waits for another wave; there is no flag, no
//       atomic, and the only barrier is the one of this single-wave workgroup.
//
// Ordering of a match's reads behind the stores they depend on: see match().
#include "sf_common.h"
#include "inflate_core.h"

namespace {

using namespace sf_zinflate;

constexpr int kWave = 64;
constexpr int kWinBytes = 512;                                          // input window in LDS, plus one word so that an 8-byte read may straddle

struct InflateArgs {
    const uint8_t* in;
    int64_t in_bytes;
    const int64_t* desc;                                                // [n][SF_INFLATE_DESC_WORDS]
    uint8_t* out;
    int64_t out_bytes;
    int32_t* status;
};

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t rfl64(uint64_t v) { return (uint64_t)rfl((uint32_t)(v >> 32)) << 32 | rfl((uint32_t)v); }

struct WavePolicy {
    const uint8_t* in;                                                  // the stream's input, in_len bytes
    int64_t in_len;
    uint8_t* out;                                                       // the stream's slot, out_len bytes
    int64_t out_len;
    uint64_t* win;                                                      // LDS: input bytes [win_base, win_base + kWinBytes + 8), zeros past in_len
    int64_t win_base;
    int lane_;
    uint32_t pend;                                                      // lane i: literal number i of the pending run
    int npend;
    int64_t pend_at;

    __device__ __forceinline__ void window(int64_t pos) {
        win_base = pos & ~(int64_t)7;
        uint8_t* wb = reinterpret_cast<uint8_t*>(win);
        __syncthreads();                                                // the reads of the old window are done
        for (int i = lane_; i < kWinBytes + 8; i += kWave) {
            const int64_t q = win_base + i;
            wb[i] = q < in_len ? in[q] : (uint8_t)0;                    // (a)
        }
        __syncthreads();
    }
    __device__ __forceinline__ uint64_t bytes(int64_t pos, int k) {
        if (pos < win_base || pos + k > win_base + kWinBytes) window(pos);
        const int off = (int)(pos - win_base), r = 8 * (off & 7);
        const uint64_t w0 = win[off >> 3], w1 = win[(off >> 3) + 1];
        const uint64_t v = r ? (w0 >> r | w1 << (64 - r)) : w0;
        return rfl64(v) & ((1ull << (8 * k)) - 1);
    }
    __device__ __forceinline__ uint32_t uni(uint32_t v) { return rfl(v); }
    __device__ __forceinline__ int lane() { return lane_; }
    __device__ __forceinline__ int lanes() { return kWave; }
    __device__ __forceinline__ void sync() { __syncthreads(); }

    // up to 64 literals wait in registers, one per lane, and leave as one coalesced store
    __device__ __forceinline__ void flush() {
        const int64_t at = pend_at + lane_;
        if (lane_ < npend && at < out_len) out[at] = (uint8_t)pend;     // (a)
        npend = 0;
    }
    __device__ __forceinline__ void lit(int64_t at, uint32_t b) {
        if (npend == 0) pend_at = at;
        if (lane_ == npend) pend = b;
        if (++npend == kWave) flush();
    }
    // out[at + j] = out[at - dist + j % dist] for j < len: every source byte lies BEFORE the match (for dist < len the match
    // repeats its first dist bytes, RFC 1951 3.2.3), so the steps of 64 do not depend on each other -- only on earlier stores of
    // this wave, some of them by other lanes.  Those are ordered by the pair of workgroup-scope fences: the release completes this
    // wave's stores (s_waitcnt vmcnt(0): the vector L1 is write-through and shared by the whole CU, so a store that has completed is
    // what any lane of this CU loads next), the acquire keeps the loads behind it.  One pair per match, none per literal.
    __device__ __forceinline__ void match(int64_t at, uint32_t dist, uint32_t len) {
        flush();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int64_t src = at - (int64_t)dist;
        for (uint32_t j = lane_; j < len; j += kWave) {
            const int64_t s = src + (j < dist ? j : j % dist), d = at + j;
            if (s >= 0 && s < at && d < out_len) out[d] = out[s];       // (a)
        }
    }
    __device__ __forceinline__ void raw(int64_t at, int64_t pos, int64_t n) {
        flush();
        for (int64_t j = lane_; j < n; j += kWave)
            if (pos + j < in_len && at + j < out_len) out[at + j] = in[pos + j];   // (a)
    }
    // second pass over the slot: A = 1 + sum d_i, B = n + sum (n - i) d_i (mod 65521), lane-strided and reduced over the wave
    __device__ __forceinline__ uint32_t adler(int64_t n) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        uint64_t a = 0, b = 0;
        uint32_t it = 0;
        for (int64_t i = lane_; i < n && i < out_len; i += kWave) {     // (a)
            const uint64_t d = out[i];
            a += d, b += (uint64_t)(n - i) * d;                         // n < 2^31: 2^16 terms stay below 2^55
            if ((++it & 0xFFFF) == 0) b %= 65521;
        }
        uint32_t ra = (uint32_t)(a % 65521), rb = (uint32_t)(b % 65521);
        for (int m = 1; m < kWave; m <<= 1) ra += __shfl_xor(ra, m, kWave), rb += __shfl_xor(rb, m, kWave);
        const uint32_t A = (1 + ra) % 65521, B = (uint32_t)((uint64_t)(n % 65521) + rb) % 65521;
        return rfl(B << 16 | A);
    }
};

__global__ __launch_bounds__(kWave) void inflate_kernel(InflateArgs g) {
    __shared__ Tables tables;
    __shared__ uint64_t win[kWinBytes / 8 + 1];
    const int64_t* d = g.desc + (int64_t)blockIdx.x * SF_INFLATE_DESC_WORDS;
    const int64_t in_off = d[0], in_len = d[1], out_off = d[2], out_len = d[3], flags = d[4];
    int st;
    // the stream's ranges lie inside the buffers (written so that no sum overflows)
    if (in_off < 0 || in_len < 0 || in_off > g.in_bytes || in_len > g.in_bytes - in_off || out_off < 0 || out_len < 0 ||
        out_off > g.out_bytes || out_len > g.out_bytes - out_off || out_len > 0x7FFFFFFF) {
        st = kBadSlot;
    } else {
        WavePolicy p{g.in + in_off, in_len, g.out + out_off, out_len, win, -(int64_t)(kWinBytes + 8), (int)threadIdx.x, 0, 0, 0};
        if (flags & SF_INFLATE_STORED) {                                // the filter mask skipped deflate: the chunk is there as it is
            st = in_len > out_len ? kOutputLong : in_len < out_len ? kOutputShort : kOk;
            if (st == kOk) p.raw(0, 0, in_len);
        } else {
            st = inflate_stream(p, tables, in_len, out_len);
        }
    }
    if (threadIdx.x == 0) g.status[blockIdx.x] = st;
}

// ---- assemble ----------------------------------------------------------------------------------------------------------------------
struct AssembleArgs {
    const uint8_t* chunks;
    int64_t chunk_stride;
    const int32_t* grid;                                                // [n][ngy][ngx][2 / cc]
    uint32_t* out;                                                      // [n][h][w][2]
    int n_slots, h, w, ch, cw, cc, shuffle, ngy, ngx;
    int64_t N;                                                          // elements of a chunk
};

constexpr int kAsmThreads = 256;

__global__ __launch_bounds__(kAsmThreads) void flo5_assemble_kernel(AssembleArgs g) {
    const int x = blockIdx.x * kAsmThreads + threadIdx.x, y = blockIdx.y;
    if (x >= g.w) return;
    const int gy = y / g.ch, ly = y - gy * g.ch, gx = x / g.cw, lx = x - gx * g.cw, ngc = 2 / g.cc;
    const int32_t* cell = g.grid + (((int64_t)blockIdx.z * g.ngy + gy) * g.ngx + gx) * ngc;
    uint32_t v[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int slot = cell[g.cc == 2 ? 0 : c];
        const int64_t e = ((int64_t)ly * g.cw + lx) * g.cc + (g.cc == 2 ? c : 0);
        v[c] = 0;                                                       // a chunk the file does not store: the fill value, 0.0
        if (slot >= 0 && slot < g.n_slots) {
            const uint8_t* base = g.chunks + (int64_t)slot * g.chunk_stride;
            if (g.shuffle) v[c] = base[e] | (uint32_t)base[g.N + e] << 8 | (uint32_t)base[2 * g.N + e] << 16 | (uint32_t)base[3 * g.N + e] << 24;
            else v[c] = reinterpret_cast<const uint32_t*>(base)[e];
        }
    }
    uint2 o;
    o.x = v[0], o.y = v[1];
    reinterpret_cast<uint2*>(g.out)[((int64_t)blockIdx.z * g.h + y) * g.w + x] = o;
}

}  // namespace

extern "C" int sf_inflate(const uint8_t* in, int64_t in_bytes, const int64_t* desc, int n, uint8_t* out, int64_t out_bytes,
                          int32_t* status, void* stream) {
    SF_REQUIRE(in && desc && out && status, "sf_inflate: null argument (in / desc / out / status)");
    SF_REQUIRE(n >= 1 && n <= SF_INFLATE_MAX_STREAMS, "sf_inflate: n = %d (1 .. %d)", n, SF_INFLATE_MAX_STREAMS);
    SF_REQUIRE(in_bytes >= 0 && out_bytes >= 0, "sf_inflate: negative size (in_bytes = %lld, out_bytes = %lld)", (long long)in_bytes,
               (long long)out_bytes);
    SF_REQUIRE(((uintptr_t)desc & 7) == 0, "sf_inflate: desc is not 8-byte aligned");
    SF_REQUIRE(((uintptr_t)status & 3) == 0, "sf_inflate: status is not 4-byte aligned");
    InflateArgs a{in, in_bytes, desc, out, out_bytes, status};
    hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)n), dim3(kWave), 0, (hipStream_t)stream, a);
    return sf::check_launch("sf_inflate");
}

extern "C" int sf_flo5_assemble(const uint8_t* chunks, int64_t chunk_stride, int n_slots, const int32_t* grid, int n, int h, int w, int ch,
                                int cw, int cc, int shuffle, float* out, void* stream) {
    SF_REQUIRE(chunks && grid && out, "sf_flo5_assemble: null argument (chunks / grid / out)");
    SF_REQUIRE(n >= 1 && n <= 65535, "sf_flo5_assemble: n = %d (1 .. 65535)", n);
    SF_REQUIRE(h >= 1 && h <= 65535 && w >= 1, "sf_flo5_assemble: bad size h = %d (1 .. 65535), w = %d", h, w);
    SF_REQUIRE(ch >= 1 && cw >= 1 && (cc == 1 || cc == 2), "sf_flo5_assemble: bad chunk shape (%d, %d, %d): cc must be 1 or 2", ch, cw, cc);
    const int64_t N = (int64_t)ch * cw * cc;
    SF_REQUIRE(4 * N < ((int64_t)1 << 31), "sf_flo5_assemble: a chunk of %lld floats is 2^31 bytes or more", (long long)N);
    SF_REQUIRE(n_slots >= 0, "sf_flo5_assemble: n_slots = %d", n_slots);
    SF_REQUIRE(chunk_stride >= 4 * N && chunk_stride % 4 == 0, "sf_flo5_assemble: chunk_stride = %lld must be a multiple of 4 and at least %lld",
               (long long)chunk_stride, (long long)(4 * N));
    SF_REQUIRE(((uintptr_t)chunks & 3) == 0 && ((uintptr_t)grid & 3) == 0, "sf_flo5_assemble: chunks / grid are not 4-byte aligned");
    SF_REQUIRE(((uintptr_t)out & 7) == 0, "sf_flo5_assemble: out is not 8-byte aligned");
    AssembleArgs a;
    a.chunks = chunks, a.chunk_stride = chunk_stride, a.grid = grid, a.out = reinterpret_cast<uint32_t*>(out);
    a.n_slots = n_slots, a.h = h, a.w = w, a.ch = ch, a.cw = cw, a.cc = cc, a.shuffle = shuffle ? 1 : 0;
    a.ngy = (int)(((int64_t)h + ch - 1) / ch), a.ngx = (int)(((int64_t)w + cw - 1) / cw), a.N = N;
    hipLaunchKernelGGL(flo5_assemble_kernel, dim3((unsigned)((w + kAsmThreads - 1) / kAsmThreads), h, n), dim3(kAsmThreads), 0,
                       (hipStream_t)stream, a);
    return sf::check_launch("sf_flo5_assemble");
}
