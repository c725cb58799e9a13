// Baseline JPEG decoding (ITU-T T.81, sequential DCT, 8 bit, Huffman) of a batch of files of one geometry into device images: the
// frames of a Motion-JPEG AVI file or of a directory of .jpg files become uint8 [n][h][w][3] where predict_video reads them.  The
// host walks the marker segments (jpeg_gpu.parse) and uploads the entropy-coded bytes as they are, one descriptor per restart
// interval and the de-duplicated table sets; everything from the first Huffman code to the RGB byte happens here.  The format
// subset, the arithmetic and the status words are stated in include/streamflow_hip.h and restated in tests/jpeg_decode_cases.py;
// the output equals that restatement, and libjpeg's, bit for bit.
//
// One memset and four launches, every dependency between workgroups a launch boundary:
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
#include "sf_common.h"
#include "jpeg_decode_core.h"

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

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

bool shape_ok(int n_images, int h, int w, int components, int hs, int vs) {
    if (n_images < 1 || n_images > 65535 || h < 1 || w < 1 || h > SF_JPEG_MAX_DIM || w > SF_JPEG_MAX_DIM) return false;
    if (components == 1) return hs == 1 && vs == 1;
    return components == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2));
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
    SF_REQUIRE(data && desc && tables && out && status && ws, "sf_jpeg_decode: null argument (data / desc / tables / out / status / ws)");
    SF_REQUIRE(data_bytes >= 0, "sf_jpeg_decode: data_bytes = %lld", (long long)data_bytes);
    SF_REQUIRE(n_intervals >= 1 && n_intervals <= kMaxIntervals, "sf_jpeg_decode: n_intervals = %d (1 .. %d)", n_intervals, kMaxIntervals);
    SF_REQUIRE(n_table_sets >= 1 && n_table_sets <= 65535, "sf_jpeg_decode: n_table_sets = %d (1 .. 65535)", n_table_sets);
    SF_REQUIRE(n_images >= 1 && n_images <= 65535, "sf_jpeg_decode: n_images = %d (1 .. 65535)", n_images);
    SF_REQUIRE(h >= 1 && w >= 1, "sf_jpeg_decode: bad size h = %d, w = %d", h, w);
    SF_REQUIRE(components == 1 || components == 3, "sf_jpeg_decode: components = %d (1 or 3)", components);
    SF_REQUIRE(components == 1 ? (hs == 1 && vs == 1) : ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)),
               "sf_jpeg_decode: luma sampling %d x %d with %d components (1 x 1, 2 x 1 or 2 x 2; grey: 1 x 1)", hs, vs, components);
    SF_REQUIRE(out_channels == 3 || (out_channels == 1 && components == 1), "sf_jpeg_decode: out_channels = %d with %d components",
               out_channels, components);
    if (h > SF_JPEG_MAX_DIM || w > SF_JPEG_MAX_DIM)
        return sf::fail(SF_ERR_UNSUPPORTED, "sf_jpeg_decode: h = %d, w = %d (at most SF_JPEG_MAX_DIM = %d)", h, w, SF_JPEG_MAX_DIM);
    const int64_t row = (int64_t)w * out_channels;
    SF_REQUIRE(out_row_stride >= row, "sf_jpeg_decode: out_row_stride = %lld is smaller than w * out_channels = %lld",
               (long long)out_row_stride, (long long)row);
    SF_REQUIRE(out_image_stride >= (int64_t)(h - 1) * out_row_stride + row,
               "sf_jpeg_decode: out_image_stride = %lld is smaller than (h - 1) * out_row_stride + w * out_channels = %lld",
               (long long)out_image_stride, (long long)((int64_t)(h - 1) * out_row_stride + row));
    SF_REQUIRE(((uintptr_t)desc & 7) == 0, "sf_jpeg_decode: desc is not 8-byte aligned");
    SF_REQUIRE(((uintptr_t)status & 3) == 0, "sf_jpeg_decode: status is not 4-byte aligned");
    SF_REQUIRE(((uintptr_t)ws & 15) == 0, "sf_jpeg_decode: ws is not 16-byte aligned");
    const int64_t need = sf_jpeg_decode_ws_bytes(n_images, h, w, components, hs, vs);
    SF_REQUIRE(ws_bytes >= need, "sf_jpeg_decode: ws_bytes = %lld is smaller than sf_jpeg_decode_ws_bytes = %lld", (long long)ws_bytes,
               (long long)need);
    DecodeArgs a;
    a.data = data, a.data_bytes = data_bytes, a.desc = desc, a.tables = tables;
    a.n_intervals = n_intervals, a.n_sets = n_table_sets, a.n_images = n_images, a.h = h, a.w = w;
    a.g = make_geom(h, w, components, hs, vs);
    const int64_t blocks = (int64_t)n_images * a.g.image_blocks;
    a.coef = reinterpret_cast<int16_t*>(((uintptr_t)ws + 127) & ~(uintptr_t)127);
    a.planes = reinterpret_cast<uint8_t*>(a.coef + blocks * 64);
    a.first_error = reinterpret_cast<uint32_t*>(a.planes + blocks * 64);
    a.covered = a.first_error + n_images;
    a.status = status, a.out = out, a.out_image_stride = out_image_stride, a.out_row_stride = out_row_stride, a.out_channels = out_channels;
    const hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(a.first_error, 0, (size_t)n_images * 8, s);
    if (e != hipSuccess) return sf::fail(SF_ERR_HIP, "sf_jpeg_decode: hipMemsetAsync: %s", hipGetErrorString(e));
    const int max_blocks = a.g.bw[0] * a.g.bh[0];
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)n_intervals), dim3(kWave), 0, s, a);
    hipLaunchKernelGGL(jpeg_status_kernel, dim3((n_images + 63) / 64), dim3(64), 0, s, a);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((max_blocks + kThreads - 1) / kThreads, n_images, components), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((w + kThreads - 1) / kThreads, h, n_images), dim3(kThreads), 0, s, a);
    return sf::check_launch("sf_jpeg_decode");
}
