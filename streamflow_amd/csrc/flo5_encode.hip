// Spring's .flo5 chunks compressed on the device: the HDF5 filter pipeline shuffle -> deflate of every chunk (rows_per_chunk, w, 2)
// of a batch of flow fields, so that a 1080 x 1920 field crosses to the host as zlib streams and flo5.flo5_file only frames them.
// The deflate is the Huffman-only one of csrc/huff_deflate.h (shared with csrc/png_encode.hip): a byte-shuffled float plane is what
// such a coder can compress -- sign / exponent bytes have few values, low mantissa bytes are noise.  The format -- chunk order,
// shuffle, blocks, table construction, header bits -- is restated in tests/flo5_encode_cases.py, and the output equals it byte for byte.
//
// Four launches behind one clear launch (sf::fill_async), every dependency between workgroups a launch boundary:
//   flo5_shuffle_kernel  a thread per 4 consecutive elements of a chunk (2 pixels x 2 channels): their bit patterns from the two
//                        channel planes (rows past h: zero bits), one 32-bit word into each of the chunk's 4 byte planes in the
//                        workspace.  Two floats per load where w, the strides and the base allow 8-byte loads, else float by float.
//   flo5_table_kernel    one workgroup per block = a segment of at most SF_FLO5_BLOCK_BYTES bytes of one byte plane.
//   flo5_offsets_kernel  one thread per chunk: prefix sum of its blocks' bit lengths, the Adler-32 of the 4 N shuffled bytes from the
//                        blocks' sums, `78 01`, the checksum bytes and out_bytes.
//   flo5_pack_kernel     one workgroup per block, bits ORed into the slot with vector atomics.
// No workgroup waits for another, and every trip count is a function of (n, h, w, rows_per_chunk): nothing in the flow values changes
// control flow beyond the choice of table.  A byte plane starts at a multiple of 16 bytes in the workspace (N need not be one), so a
// block is read in aligned words whatever N is.
#include "huff_deflate.h"

namespace {

using namespace sf_huff;

constexpr int64_t kBlock = SF_FLO5_BLOCK_BYTES;
constexpr int kMaxChunks = 64;                                          // flo5.flo5_file writes the chunk index as one B-tree leaf

struct Flo5Args {
    const uint32_t* flow;                                               // the floats' bit patterns
    int64_t field_stride, ch_stride, row_stride;
    int h, w, rpc, nchunks, segs, nblk, vec, nslots;
    int64_t N, plane_stride;                                            // elements of a chunk; bytes between its byte planes
    uint8_t* planes;                                                    // [n][nchunks][4][plane_stride]
    uint32_t* rec;                                                      // [n][nchunks][nblk][kRecWords]
    uint8_t* out;
    int64_t out_chunk_stride;
    int64_t* out_bytes;
};

// ---- 1. shuffle --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void flo5_shuffle_kernel(Flo5Args g) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;     // elements 4 q .. 4 q + 3 = pixels 2 q, 2 q + 1
    if (4 * q >= g.plane_stride) return;
    const int64_t slot = (int64_t)blockIdx.z * g.nchunks + blockIdx.y;
    const uint32_t* f = g.flow + (int64_t)blockIdx.z * g.field_stride;
    const int row0 = (int)blockIdx.y * g.rpc;                           // < h
    uint32_t v[4] = {0, 0, 0, 0};                                       // elements past N (the planes' padding) and rows past h
    if (g.vec) {                                                        // w even: both pixels in one row, N % 4 == 0
        if (4 * q < g.N) {
            const int pix = (int)(2 * q), y = pix / g.w, x = pix - y * g.w;
            if (row0 + y < g.h) {
                const uint32_t* src = f + (int64_t)(row0 + y) * g.row_stride + x;
                const uint2 a = *reinterpret_cast<const uint2*>(src), b = *reinterpret_cast<const uint2*>(src + g.ch_stride);
                v[0] = a.x, v[1] = b.x, v[2] = a.y, v[3] = b.y;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int64_t pix = 2 * q + k;
            if (2 * pix < g.N) {
                const int y = (int)pix / g.w, x = (int)pix - y * g.w;
                if (row0 + y < g.h) {
                    const uint32_t* src = f + (int64_t)(row0 + y) * g.row_stride + x;
                    v[2 * k] = src[0], v[2 * k + 1] = src[g.ch_stride];
                }
            }
        }
    }
    uint8_t* dst = g.planes + slot * 4 * g.plane_stride;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t word = ((v[0] >> (8 * j)) & 255) | (((v[1] >> (8 * j)) & 255) << 8) | (((v[2] >> (8 * j)) & 255) << 16) |
                              (((v[3] >> (8 * j)) & 255) << 24);
        reinterpret_cast<uint32_t*>(dst + j * g.plane_stride)[q] = word;
    }
}

// block b of a chunk: segment b % segs of byte plane b / segs
__device__ __forceinline__ int64_t block_bytes(const Flo5Args& g, int b) {
    const int64_t left = g.N - (int64_t)(b % g.segs) * kBlock;
    return left < kBlock ? left : kBlock;
}
__device__ __forceinline__ const uint8_t* block_data(const Flo5Args& g, int64_t slot, int b) {
    return g.planes + (slot * 4 + b / g.segs) * g.plane_stride + (int64_t)(b % g.segs) * kBlock;
}

// ---- 2. tables ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void flo5_table_kernel(Flo5Args g) {
    const int64_t slot = (int64_t)blockIdx.z * g.nchunks + blockIdx.y;
    table_block(block_data(g, slot, blockIdx.x), block_bytes(g, blockIdx.x), g.rec + (slot * g.nblk + blockIdx.x) * kRecWords);
}

// ---- 3. offsets --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void flo5_offsets_kernel(Flo5Args g) {
    const int slot = blockIdx.x * 64 + threadIdx.x;
    if (slot >= g.nslots) return;
    uint32_t* rec = g.rec + (int64_t)slot * g.nblk * kRecWords;
    uint64_t bit = 16, A = 0, B = 0;                                    // behind `78 01`
    for (int b = 0; b < g.nblk; ++b, rec += kRecWords) {
        rec[kRecStartLo] = (uint32_t)bit, rec[kRecStartHi] = (uint32_t)(bit >> 32);
        bit += rec[kRecBits];
        adler_append(A, B, rec, (uint64_t)block_bytes(g, b));
    }
    g.out_bytes[slot] = stream_ends(g.out + (int64_t)slot * g.out_chunk_stride, bit, A, B, (uint64_t)(4 * g.N));
}

// ---- 4. pack -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void flo5_pack_kernel(Flo5Args g) {
    const int64_t slot = (int64_t)blockIdx.z * g.nchunks + blockIdx.y;
    pack_block(block_data(g, slot, blockIdx.x), block_bytes(g, blockIdx.x), g.rec + (slot * g.nblk + blockIdx.x) * kRecWords,
               reinterpret_cast<uint32_t*>(g.out + slot * g.out_chunk_stride), (int)blockIdx.x == g.nblk - 1);
}

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
// elements of a chunk, or -1 where 4 N does not stay below 2^31
int64_t chunk_elems(int rows_per_chunk, int w) {
    if (rows_per_chunk < 1 || w < 1) return -1;
    const int64_t N = 2 * (int64_t)rows_per_chunk * w;
    return 4 * N < ((int64_t)1 << 31) ? N : -1;
}
int64_t blocks_of(int64_t N) { return 4 * ((N + kBlock - 1) / kBlock); }
int chunks_of(int h, int rows_per_chunk) { return (int)(((int64_t)h + rows_per_chunk - 1) / rows_per_chunk); }

}  // namespace

extern "C" int64_t sf_flo5_chunk_bound(int rows_per_chunk, int w) {
    const int64_t N = chunk_elems(rows_per_chunk, w);
    if (N < 0) return -1;
    const int64_t bits = blocks_of(N) * (kHeaderBitsMax + 9) + 9 * 4 * N;
    return align_up(2 + (bits + 7) / 8 + 4, 4);
}

extern "C" int64_t sf_flo5_encode_ws_bytes(int n, int h, int w, int rows_per_chunk) {
    const int64_t N = chunk_elems(rows_per_chunk, w);
    if (N < 0 || h < 1 || n < 1 || n > 65535 || chunks_of(h, rows_per_chunk) > kMaxChunks) return -1;
    return 16 + (int64_t)n * chunks_of(h, rows_per_chunk) * (4 * align_up(N, 16) + blocks_of(N) * kRecWords * 4);
}

extern "C" int sf_flo5_encode(const float* flow, int64_t field_stride, int64_t ch_stride, int64_t row_stride, int n, int h, int w,
                              int rows_per_chunk, uint8_t* out, int64_t out_chunk_stride, int64_t* out_bytes, void* ws, int64_t ws_bytes,
                              void* stream) {
    SF_REQUIRE(flow && out && out_bytes && ws, "sf_flo5_encode: null argument (flow / out / out_bytes / ws)");
    SF_REQUIRE(n >= 1 && n <= 65535, "sf_flo5_encode: n = %d (1 .. 65535)", n);
    SF_REQUIRE(h >= 1 && w >= 1 && rows_per_chunk >= 1, "sf_flo5_encode: bad size h = %d, w = %d, rows_per_chunk = %d", h, w, rows_per_chunk);
    const int nchunks = chunks_of(h, rows_per_chunk);
    SF_REQUIRE(nchunks <= kMaxChunks, "sf_flo5_encode: ceil(h / rows_per_chunk) = %d chunks (at most %d: the container writes one B-tree leaf)",
               nchunks, kMaxChunks);
    const int64_t N = chunk_elems(rows_per_chunk, w);
    SF_REQUIRE(N > 0, "sf_flo5_encode: a chunk of rows_per_chunk * w * 2 = %lld floats is 2^31 bytes or more",
               (long long)(2 * (int64_t)rows_per_chunk * w));
    SF_REQUIRE(row_stride >= w, "sf_flo5_encode: row_stride = %lld is smaller than w = %d", (long long)row_stride, w);
    const int64_t plane = (int64_t)(h - 1) * row_stride + w;
    SF_REQUIRE(ch_stride >= plane, "sf_flo5_encode: ch_stride = %lld is smaller than (h - 1) * row_stride + w = %lld (the channels overlap)",
               (long long)ch_stride, (long long)plane);
    SF_REQUIRE(field_stride >= ch_stride + plane,
               "sf_flo5_encode: field_stride = %lld is smaller than ch_stride + (h - 1) * row_stride + w = %lld (the fields overlap)",
               (long long)field_stride, (long long)(ch_stride + plane));
    SF_REQUIRE(((uintptr_t)flow & 3) == 0, "sf_flo5_encode: flow is not 4-byte aligned");
    const int64_t bound = sf_flo5_chunk_bound(rows_per_chunk, w);
    SF_REQUIRE(out_chunk_stride >= bound, "sf_flo5_encode: out_chunk_stride = %lld is smaller than sf_flo5_chunk_bound = %lld",
               (long long)out_chunk_stride, (long long)bound);
    SF_REQUIRE(((uintptr_t)out & 3) == 0 && out_chunk_stride % 4 == 0,
               "sf_flo5_encode: out and out_chunk_stride = %lld must be multiples of 4 (the bits are ORed into 32-bit words)",
               (long long)out_chunk_stride);
    SF_REQUIRE(((uintptr_t)out_bytes & 7) == 0, "sf_flo5_encode: out_bytes is not 8-byte aligned");
    const int64_t need = sf_flo5_encode_ws_bytes(n, h, w, rows_per_chunk);
    SF_REQUIRE(ws_bytes >= need, "sf_flo5_encode: ws_bytes = %lld is smaller than sf_flo5_encode_ws_bytes = %lld", (long long)ws_bytes,
               (long long)need);
    Flo5Args a;
    a.flow = reinterpret_cast<const uint32_t*>(flow), a.field_stride = field_stride, a.ch_stride = ch_stride, a.row_stride = row_stride;
    a.h = h, a.w = w, a.rpc = rows_per_chunk, a.nchunks = nchunks, a.N = N, a.plane_stride = align_up(N, 16);
    a.segs = (int)((N + kBlock - 1) / kBlock), a.nblk = 4 * a.segs, a.nslots = n * nchunks;
    // two floats per load: both pixels of a thread in one row, every row of every plane 8-byte aligned
    a.vec = (w % 2 == 0 && row_stride % 2 == 0 && ch_stride % 2 == 0 && field_stride % 2 == 0 && ((uintptr_t)flow & 7) == 0) ? 1 : 0;
    a.planes = reinterpret_cast<uint8_t*>(((uintptr_t)ws + 15) & ~(uintptr_t)15);
    a.rec = reinterpret_cast<uint32_t*>(a.planes + (int64_t)a.nslots * 4 * a.plane_stride);
    a.out = out, a.out_chunk_stride = out_chunk_stride, a.out_bytes = out_bytes;
    const hipStream_t s = (hipStream_t)stream;
    // the pack kernel ORs into zeroed words; nothing past sf_flo5_chunk_bound bytes of a slot is touched
    const int cleared = sf::fill_async("sf_flo5_encode (clearing the slots)", out, 0, bound, s, a.nslots, out_chunk_stride);
    if (cleared != SF_OK) return cleared;
    const dim3 per_block(a.nblk, nchunks, n);
    hipLaunchKernelGGL(flo5_shuffle_kernel, dim3((unsigned)((a.plane_stride / 4 + kThreads - 1) / kThreads), nchunks, n), dim3(kThreads), 0,
                       s, a);
    hipLaunchKernelGGL(flo5_table_kernel, per_block, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(flo5_offsets_kernel, dim3((a.nslots + 63) / 64), dim3(64), 0, s, a);
    hipLaunchKernelGGL(flo5_pack_kernel, per_block, dim3(kThreads), 0, s, a);
    return sf::check_launch("sf_flo5_encode");
}
