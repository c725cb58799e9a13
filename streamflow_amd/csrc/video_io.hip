// Video in and out of the model (the batched counterpart of the reference's demo.py:502-534 read_video_and_group_predict): uint8
// frames -> the fp32 clip batch [n_clips][T][3][Hp][Wp] the encoders take, and the model's per-pair outputs -> flow fields
// [n_pairs][2][H][W] in video order.  One launch each per batch of clips; both kernels compute the clip schedule themselves
// (include/streamflow_hip.h, "video clips"), so no table is uploaded.
//
// frames_to_clips_kernel: a thread owns four consecutive output pixels of one row of one frame copy, all three channels: twelve
// source bytes -> three 16-byte stores (one per colour plane).  The normalisation is a table of 256 floats the caller built with
// the model's own expression (no arithmetic here, so the clips are bitwise what SKFlow_MF8.forward computes); a block keeps it in
// LDS.  Packed HWC frames (pixel stride 3, channel stride 1) take three dword loads where the thread's twelve bytes are 4-byte
// aligned and all four pixels lie inside the frame; the pad columns, unaligned rows and every other layout (CHW, strided views)
// take byte loads with the replicate clamp per pixel.  Memory-bound: 3 B read and 12 B written per pixel of a frame copy.
//
// clips_to_flows_kernel: a thread owns four consecutive pixels of one row of one plane of one kept pair; float4 loads / stores
// where the strides, the pad offset and the pointers allow it, scalar otherwise.  The pad is cropped away, the tail clip's
// duplicate pairs are never read.
#include "sf_common.h"

namespace {

constexpr int kBlock = 256;

__host__ __device__ inline int clip_count(int n, int T) { return (n - 2) / (T - 1) + 1; }          // ceil((n - 1) / (T - 1))
__host__ __device__ inline int clip_start(int c, int n, int T) {
    const int s = c * (T - 1);
    return s < n - T ? s : n - T;
}
__host__ __device__ inline int pair_clip(int j, int n, int T) {
    const int c = j / (T - 1), last = clip_count(n, T) - 1;
    return c < last ? c : last;
}

struct FramesArgs {
    const uint8_t* frames;
    int64_t frame_stride, row_stride, px_stride, ch_stride;
    int frame0, n, T, first_clip;
    int H, W, pad_top, pad_left, Hp, Wp;
    int packed;                                                          // px_stride == 3 && ch_stride == 1
};

__global__ __launch_bounds__(kBlock) void frames_to_clips_kernel(FramesArgs a, const float* __restrict__ lut, float* __restrict__ out) {
    __shared__ float s_lut[256];
    s_lut[threadIdx.x] = lut[threadIdx.x];                               // kBlock == 256
    __syncthreads();
    const int gw = a.Wp >> 2;
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= a.Hp * gw) return;
    const int y = q / gw, x0 = (q - y * gw) << 2;
    const int copy = blockIdx.y;                                         // clip-major: copy = c' * T + t
    const int cl = copy / a.T, t = copy - cl * a.T;
    const int f = clip_start(a.first_clip + cl, a.n, a.T) + t - a.frame0;             // host-checked: 0 <= f < n_buf
    int sy = y - a.pad_top;
    sy = sy < 0 ? 0 : (sy > a.H - 1 ? a.H - 1 : sy);
    const uint8_t* row = a.frames + (int64_t)f * a.frame_stride + (int64_t)sy * a.row_stride;
    const int sx0 = x0 - a.pad_left;
    unsigned int b[3][4];                                                // [channel][pixel]
    const bool inside = sx0 >= 0 && sx0 + 3 < a.W;
    const uint8_t* p12 = row + (int64_t)3 * sx0;
    if (a.packed && inside && (reinterpret_cast<uintptr_t>(p12) & 3u) == 0) {
        const unsigned int* p = reinterpret_cast<const unsigned int*>(p12);
        const unsigned int w0 = p[0], w1 = p[1], w2 = p[2];              // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        b[0][0] = w0 & 0xffu, b[1][0] = (w0 >> 8) & 0xffu, b[2][0] = (w0 >> 16) & 0xffu;
        b[0][1] = w0 >> 24, b[1][1] = w1 & 0xffu, b[2][1] = (w1 >> 8) & 0xffu;
        b[0][2] = (w1 >> 16) & 0xffu, b[1][2] = w1 >> 24, b[2][2] = w2 & 0xffu;
        b[0][3] = (w2 >> 8) & 0xffu, b[1][3] = (w2 >> 16) & 0xffu, b[2][3] = w2 >> 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int sx = sx0 + j;
            sx = sx < 0 ? 0 : (sx > a.W - 1 ? a.W - 1 : sx);
            const uint8_t* px = row + (int64_t)sx * a.px_stride;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) b[ch][j] = px[(int64_t)ch * a.ch_stride];
        }
    }
    const int64_t plane = (int64_t)a.Hp * a.Wp;
    float* o = out + ((int64_t)copy * 3) * plane + (int64_t)y * a.Wp + x0;             // 16-byte aligned: Wp % 8 == 0, x0 % 4 == 0
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float4 v;
        v.x = s_lut[b[ch][0]], v.y = s_lut[b[ch][1]], v.z = s_lut[b[ch][2]], v.w = s_lut[b[ch][3]];
        *reinterpret_cast<float4*>(o + ch * plane) = v;
    }
}

struct FlowsArgs {
    SfPairPtrs pairs;
    int64_t clip_stride, ch_stride, row_stride;
    int n, T, first_clip, pair0;
    int H, W, pad_top, pad_left;
    int vec_load, vec_store;
};

__device__ __forceinline__ const float* pick_pair(const SfPairPtrs& p, int k) {
    // a chain of selects on constant indices: the pointers stay in scalar registers (a dynamic index could go through scratch)
    const float* r = p.p[0];
#pragma unroll
    for (int i = 1; i < SF_VIDEO_MAX_PAIRS; ++i) r = k == i ? p.p[i] : r;
    return r;
}

__global__ __launch_bounds__(kBlock) void clips_to_flows_kernel(FlowsArgs a, float* __restrict__ out) {
    const int gw = (a.W + 3) >> 2;
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= a.H * gw) return;
    const int y = q / gw, x0 = (q - y * gw) << 2;
    const int jl = blockIdx.y >> 1, ch = blockIdx.y & 1;                  // pair of this call, plane
    const int j = a.pair0 + jl;
    const int c = pair_clip(j, a.n, a.T);
    const int k = j - clip_start(c, a.n, a.T);                           // 0 <= k < T - 1
    const float* src = pick_pair(a.pairs, k) + (int64_t)(c - a.first_clip) * a.clip_stride + (int64_t)ch * a.ch_stride +
                       (int64_t)(y + a.pad_top) * a.row_stride + a.pad_left + x0;
    float* dst = out + (((int64_t)jl * 2 + ch) * a.H + y) * a.W + x0;
    const int left = a.W - x0;                                           // pixels of this thread that exist (>= 1)
    float v[4];
    if (a.vec_load && left >= 4) {
        const float4 v4 = *reinterpret_cast<const float4*>(src);
        v[0] = v4.x, v[1] = v4.y, v[2] = v4.z, v[3] = v4.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = i < left ? src[i] : 0.0f;
    }
    if (a.vec_store && left >= 4) {
        float4 v4;
        v4.x = v[0], v4.y = v[1], v4.z = v[2], v4.w = v[3];
        *reinterpret_cast<float4*>(dst) = v4;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < left) dst[i] = v[i];
    }
}

}  // namespace

extern "C" int sf_frames_to_clips(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, int64_t px_stride,
                                  int64_t ch_stride, int frame0, int n_buf, int n, int T, int first_clip, int n_clips, int H, int W,
                                  int pad_top, int pad_left, int Hp, int Wp, const float* lut, float* out, void* stream) {
    SF_REQUIRE(frames && lut && out, "sf_frames_to_clips: null argument");
    SF_REQUIRE(T >= 2, "sf_frames_to_clips: T = %d (at least 2)", T);
    SF_REQUIRE(n >= T, "sf_frames_to_clips: a video of %d frames is shorter than one clip of %d", n, T);
    SF_REQUIRE(H > 0 && W > 0 && pad_top >= 0 && pad_left >= 0, "sf_frames_to_clips: bad shape %d x %d, pad (%d, %d)", H, W, pad_top,
               pad_left);
    SF_REQUIRE(Hp > 0 && Wp > 0 && Hp % 8 == 0 && Wp % 8 == 0, "sf_frames_to_clips: padded size %d x %d is not a multiple of 8", Hp, Wp);
    SF_REQUIRE((int64_t)H + pad_top <= Hp && (int64_t)W + pad_left <= Wp,
               "sf_frames_to_clips: padded size %d x %d is smaller than the frame %d x %d plus pad (%d, %d)", Hp, Wp, H, W, pad_top, pad_left);
    SF_REQUIRE((int64_t)Hp * Wp < (1 << 30), "sf_frames_to_clips: frame %d x %d too large", Hp, Wp);
    const int nc = clip_count(n, T);
    SF_REQUIRE(n_clips > 0 && first_clip >= 0 && (int64_t)first_clip + n_clips <= nc,
               "sf_frames_to_clips: clips %d .. %lld of a video with %d", first_clip, (long long)first_clip + n_clips - 1, nc);
    SF_REQUIRE((int64_t)n_clips * T <= 65535, "sf_frames_to_clips: %d clips of %d frames in one call (at most 65535 frame copies)",
               n_clips, T);
    // clip starts grow with the clip index: the first and the last clip bound the frames that are read
    const int lo = clip_start(first_clip, n, T), hi = clip_start(first_clip + n_clips - 1, n, T) + T;
    SF_REQUIRE(n_buf > 0 && frame0 >= 0 && lo >= frame0 && hi <= (int64_t)frame0 + n_buf,
               "sf_frames_to_clips: clips %d .. %d need frames %d .. %d, the buffer holds %d .. %lld", first_clip,
               first_clip + n_clips - 1, lo, hi - 1, frame0, (long long)frame0 + n_buf - 1);
    SF_REQUIRE(frame_stride >= 0 && row_stride >= 0 && px_stride >= 0 && ch_stride >= 0,
               "sf_frames_to_clips: negative stride (%lld, %lld, %lld, %lld)", (long long)frame_stride, (long long)row_stride,
               (long long)px_stride, (long long)ch_stride);
    SF_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15u) == 0 && (reinterpret_cast<uintptr_t>(lut) & 3u) == 0,
               "sf_frames_to_clips: out not 16-byte aligned / lut not 4-byte aligned");
    FramesArgs a;
    a.frames = frames, a.frame_stride = frame_stride, a.row_stride = row_stride, a.px_stride = px_stride, a.ch_stride = ch_stride;
    a.frame0 = frame0, a.n = n, a.T = T, a.first_clip = first_clip;
    a.H = H, a.W = W, a.pad_top = pad_top, a.pad_left = pad_left, a.Hp = Hp, a.Wp = Wp;
    a.packed = px_stride == 3 && ch_stride == 1;
    const dim3 grid(sf::ceil_div(Hp * (Wp / 4), kBlock), n_clips * T);
    hipLaunchKernelGGL(frames_to_clips_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a, lut, out);
    return sf::check_launch("sf_frames_to_clips");
}

extern "C" int sf_clips_to_flows(const SfPairPtrs* pairs, int64_t clip_stride, int64_t ch_stride, int64_t row_stride, int n, int T,
                                 int first_clip, int n_clips, int pair0, int n_pairs, int H, int W, int pad_top, int pad_left,
                                 float* out, void* stream) {
    SF_REQUIRE(pairs && out, "sf_clips_to_flows: null argument");
    SF_REQUIRE(T >= 2, "sf_clips_to_flows: T = %d (at least 2)", T);
    if (T - 1 > SF_VIDEO_MAX_PAIRS)
        return sf::fail(SF_ERR_UNSUPPORTED, "sf_clips_to_flows: %d pairs per clip (at most %d)", T - 1, SF_VIDEO_MAX_PAIRS);
    SF_REQUIRE(n >= T, "sf_clips_to_flows: a video of %d frames is shorter than one clip of %d", n, T);
    for (int k = 0; k < T - 1; ++k) SF_REQUIRE(pairs->p[k], "sf_clips_to_flows: null pointer for pair %d", k);
    SF_REQUIRE(H > 0 && W > 0 && pad_top >= 0 && pad_left >= 0, "sf_clips_to_flows: bad shape %d x %d, pad (%d, %d)", H, W, pad_top,
               pad_left);
    SF_REQUIRE((int64_t)H * W < (1 << 30), "sf_clips_to_flows: field %d x %d too large", H, W);
    SF_REQUIRE(row_stride >= (int64_t)W + pad_left && ch_stride > 0 && clip_stride >= 0,
               "sf_clips_to_flows: bad strides (%lld, %lld, %lld)", (long long)clip_stride, (long long)ch_stride, (long long)row_stride);
    const int nc = clip_count(n, T);
    SF_REQUIRE(n_clips > 0 && first_clip >= 0 && (int64_t)first_clip + n_clips <= nc,
               "sf_clips_to_flows: clips %d .. %lld of a video with %d", first_clip, (long long)first_clip + n_clips - 1, nc);
    SF_REQUIRE(n_pairs > 0 && pair0 >= 0 && (int64_t)pair0 + n_pairs <= n - 1,
               "sf_clips_to_flows: pairs %d .. %lld of a video with %d", pair0, (long long)pair0 + n_pairs - 1, n - 1);
    SF_REQUIRE(n_pairs <= 32767, "sf_clips_to_flows: %d pairs in one call (at most 32767)", n_pairs);
    // a pair's clip grows with the pair index: the first and the last pair bound the clips that are read
    const int c_lo = pair_clip(pair0, n, T), c_hi = pair_clip(pair0 + n_pairs - 1, n, T);
    SF_REQUIRE(c_lo >= first_clip && c_hi < first_clip + n_clips,
               "sf_clips_to_flows: pairs %d .. %d belong to clips %d .. %d, the batch holds %d .. %d", pair0, pair0 + n_pairs - 1, c_lo,
               c_hi, first_clip, first_clip + n_clips - 1);
    FlowsArgs a;
    a.pairs = *pairs;
    for (int k = T - 1; k < SF_VIDEO_MAX_PAIRS; ++k) a.pairs.p[k] = nullptr;
    a.clip_stride = clip_stride, a.ch_stride = ch_stride, a.row_stride = row_stride;
    a.n = n, a.T = T, a.first_clip = first_clip, a.pair0 = pair0;
    a.H = H, a.W = W, a.pad_top = pad_top, a.pad_left = pad_left;
    // float4 loads: every source address is base + multiples of the three strides + pad_left + 4 i
    bool vl = pad_left % 4 == 0 && clip_stride % 4 == 0 && ch_stride % 4 == 0 && row_stride % 4 == 0;
    for (int k = 0; k < T - 1; ++k) vl = vl && (reinterpret_cast<uintptr_t>(pairs->p[k]) & 15u) == 0;
    a.vec_load = vl;
    a.vec_store = W % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
    const dim3 grid(sf::ceil_div(H * ((W + 3) / 4), kBlock), 2 * n_pairs);
    hipLaunchKernelGGL(clips_to_flows_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a, out);
    return sf::check_launch("sf_clips_to_flows");
}
