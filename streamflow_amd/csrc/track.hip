// libstreamflow_track: points carried through a video's flow fields (sft_track_advance) and tracks drawn on its frames
// (sft_draw_tracks).  include/streamflow_track.h has the contract; csrc/track_core.h the per-point rules, shared with the host
// program that runs them under the sanitizers.  This file is a library of its own: it links none of libstreamflow_hip's objects and
// brings its own error buffer and launch helpers; everything but the sft_* entry points has hidden visibility.
//
// sft_track_advance: a thread owns a point and consecutive lanes own consecutive points, so in dense mode the state loads, the row
// stores and (for smooth flows) the taps of a wave cover consecutive addresses.  The thread walks all K fields itself -- one launch,
// K dependent gathers per point, position and status in registers between steps.  The taps are element loads at data-dependent
// addresses that neighbouring points mostly share, served by L2.  counts: per step and status a wave ballot, one integer atomic add
// per wave and status into words a kernel of the same call cleared (not hipMemsetAsync: csrc/sf_common.h has the note on memset
// nodes under graph replay).  Integer sums do not depend on the order of the adds.  No LDS.
//
// sft_draw_tracks: clear the key image, stamp (a thread per frame, point and age; atomic maxima of keys whose order is the drawing
// order), resolve (a thread per pixel).  Three launches.
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/streamflow_track.h"
#include "track_core.h"

#pragma clang fp contract(off)

#define SFT_API extern "C" __attribute__((visibility("default")))

namespace {

char* err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SFT_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return SFT_OK;
}

#define SFT_REQUIRE(cond, ...)                                     \
    do {                                                           \
        if (!(cond)) return fail(SFT_ERR_BAD_ARG, __VA_ARGS__);    \
    } while (0)

constexpr int kBlock = 256;
constexpr int64_t kMaxInt = 2147483647;
constexpr int kMaxSide = 1 << 24;                                        // (float)(w - 1) is exact up to here

__global__ __launch_bounds__(kBlock) void track_clear_kernel(uint32_t* __restrict__ p, int64_t words) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < words; i += (int64_t)gridDim.x * kBlock) p[i] = 0u;
}

int clear_words(const char* what, uint32_t* p, int64_t words, hipStream_t s) {
    const int64_t blocks = (words + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(track_clear_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(kBlock), 0, s, p, words);
    return check_launch(what);
}

struct AdvanceArgs {
    const float* fwd;
    const float* bwd;
    int64_t f_field, f_ch, f_row, b_field, b_ch, b_row;
    int n_steps, h, w, frame0;
    const float* state_xy;
    const uint8_t* state_status;
    const int32_t* start;
    int n_points;
    float alpha, beta;
    int sticky;
    float* out_xy;
    uint8_t* out_status;
    float* state_xy_out;
    uint8_t* state_status_out;
    uint32_t* counts;
};

__global__ __launch_bounds__(kBlock) void track_advance_kernel(AdvanceArgs a) {
    const int64_t i64 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i64 < a.n_points;
    const int i = live ? (int)i64 : 0;
    const int64_t P = a.n_points;
    const int h = a.h, w = a.w;
    sft_core::Point p;
    int start = -2147483647 - 1;
    if (a.state_xy != nullptr) {
        p.x = a.state_xy[i];
        p.y = a.state_xy[P + i];
        p.status = sft_core::read_status(a.state_status[i]);
        if (a.start != nullptr) start = a.start[i];
        if (p.status == sft_core::kPending && start <= a.frame0) sft_core::activate(p, h, w);
    } else {
        const int y = i / w;
        p.x = (float)(i - y * w), p.y = (float)y, p.status = sft_core::kVisible;
    }
    for (int k = 0; k < a.n_steps; ++k) {
        sft_core::Field fwd, bwd;
        fwd.u = a.fwd + (int64_t)k * a.f_field, fwd.v = fwd.u + a.f_ch, fwd.row = a.f_row;
        bwd.u = a.bwd != nullptr ? a.bwd + (int64_t)k * a.b_field : nullptr;
        bwd.v = a.bwd != nullptr ? bwd.u + a.b_ch : nullptr;
        bwd.row = a.b_row;
        if (live) {
            sft_core::advance_row(p, start, a.frame0 + k + 1, fwd, bwd, h, w, a.alpha, a.beta, a.sticky != 0);
            float* row = a.out_xy + (int64_t)k * 2 * P;
            row[i] = p.x;
            row[P + i] = p.y;
            a.out_status[(int64_t)k * P + i] = p.status;
        }
        if (a.counts != nullptr) {                                       // (uniform over the grid: every lane of a wave arrives)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const unsigned long long m = __ballot(live && p.status == s);
                if ((threadIdx.x & 63) == 0 && m != 0ull) atomicAdd(a.counts + (int64_t)k * 4 + s, (unsigned)__popcll(m));
            }
        }
    }
    if (live && a.state_xy_out != nullptr) {
        a.state_xy_out[i] = p.x;
        a.state_xy_out[P + i] = p.y;
        a.state_status_out[i] = p.status;
    }
}

struct DrawArgs {
    const uint8_t* src;
    int64_t s_frame, s_row, s_px, s_ch;
    int n_frames, h, w, first_frame;
    const float* xy;
    const uint8_t* status;
    int n_rows, n_points, first_row;
    int trail, radius, trail_radius, draw_occluded;
    const uint8_t* palette;
    int n_colours;
    const uint8_t* alpha_table;
    uint8_t* out;
    uint32_t* keys;
};

__global__ __launch_bounds__(kBlock) void track_stamp_kernel(DrawArgs a) {
    const int64_t P = a.n_points;
    const int64_t total = (int64_t)a.n_frames * P * a.trail;
    const int h = a.h, w = a.w;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        // consecutive lanes: consecutive points of one (frame, age)
        const int64_t point = t % P, fa = t / P;
        const int age = (int)(fa % a.trail), j = (int)(fa / a.trail);
        const int64_t r = (int64_t)a.first_frame + j - age - a.first_row;       // the sample's row of the window
        if (r < 0 || r >= a.n_rows) continue;
        const float x = a.xy[(r * 2) * P + point], y = a.xy[(r * 2 + 1) * P + point];
        if (!sft_core::drawable(x, y, a.status[r * P + point], a.draw_occluded != 0, h, w)) continue;
        bool newer_ok = false;
        float nx = 0.0f, ny = 0.0f;
        if (age >= 1 && r + 1 < a.n_rows) {
            nx = a.xy[((r + 1) * 2) * P + point], ny = a.xy[((r + 1) * 2 + 1) * P + point];
            newer_ok = sft_core::drawable(nx, ny, a.status[(r + 1) * P + point], a.draw_occluded != 0, h, w);
        }
        uint32_t* img = a.keys + (int64_t)j * h * w;
        const uint32_t key = sft_core::draw_key(a.trail, age, point);
        sft_core::stamp(x, y, newer_ok, nx, ny, age, a.radius, a.trail_radius, SFT_DRAW_MAX_SEG, h, w,
                        [=](int px, int py) { atomicMax(img + (int64_t)py * w + px, key); });
    }
}

__global__ __launch_bounds__(kBlock) void track_resolve_kernel(DrawArgs a) {
    const int64_t hw = (int64_t)a.h * a.w, total = hw * a.n_frames;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        const int64_t j = t / hw, q = t - j * hw;
        const int y = (int)(q / a.w), x = (int)(q - (int64_t)y * a.w);
        const uint8_t* s = a.src + j * a.s_frame + (int64_t)y * a.s_row + (int64_t)x * a.s_px;
        const unsigned c0 = s[0], c1 = s[a.s_ch], c2 = s[2 * a.s_ch];
        uint8_t* o = a.out + t * 3;
        const uint32_t key = a.keys[t];
        if (key == 0u) {
            o[0] = (uint8_t)c0, o[1] = (uint8_t)c1, o[2] = (uint8_t)c2;
            continue;
        }
        const int age = a.trail - (int)(key >> 20);
        const int point = (int)(key & 0xFFFFFu) - 1;
        const uint8_t* col = a.palette + (int64_t)(point % a.n_colours) * 3;
        const unsigned alpha = a.alpha_table[age];
        o[0] = sft_core::blend_channel(col[0], c0, alpha);
        o[1] = sft_core::blend_channel(col[1], c1, alpha);
        o[2] = sft_core::blend_channel(col[2], c2, alpha);
    }
}

unsigned grid_for(int64_t threads) {
    const int64_t blocks = (threads + kBlock - 1) / kBlock;
    return (unsigned)(blocks > (1 << 20) ? (1 << 20) : (blocks < 1 ? 1 : blocks));
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

SFT_API int sft_version(void) { return SFT_VERSION; }
SFT_API const char* sft_last_error(void) { return err_buf(); }

SFT_API int64_t sft_track_advance_ws_bytes(int n_steps, int64_t n_points) {
    if (n_steps < 1 || n_steps > SFT_MAX_STEPS || n_points < 1 || n_points > kMaxInt)
        return fail(SFT_ERR_BAD_ARG, "sft_track_advance_ws_bytes: %d steps of %lld points (1 .. %d steps, 1 .. 2^31 - 1 points)", n_steps,
                    (long long)n_points, SFT_MAX_STEPS);
    return 0;
}

SFT_API int sft_track_advance(const float* fwd, int64_t field_stride, int64_t ch_stride, int64_t row_stride, const float* bwd,
                              int64_t b_field_stride, int64_t b_ch_stride, int64_t b_row_stride, int n_steps, int h, int w, int frame0,
                              const float* state_xy, const uint8_t* state_status, const int32_t* start, int64_t n_points, float alpha,
                              float beta, int sticky, float* out_xy, uint8_t* out_status, float* state_xy_out,
                              uint8_t* state_status_out, uint32_t* counts, void* ws, int64_t ws_bytes, void* stream) {
    (void)ws;
    SFT_REQUIRE(fwd && out_xy && out_status, "sft_track_advance: null argument (fwd, out_xy or out_status)");
    SFT_REQUIRE(h >= 1 && w >= 1, "sft_track_advance: bad shape %d x %d", h, w);
    SFT_REQUIRE((int64_t)h * w <= kMaxInt && h <= kMaxSide && w <= kMaxSide,
                "sft_track_advance: field %d x %d too large (h * w < 2^31, a side at most 2^24: w - 1 is exact in fp32)", h, w);
    SFT_REQUIRE(n_steps >= 1 && n_steps <= SFT_MAX_STEPS, "sft_track_advance: n_steps = %d (1 .. %d)", n_steps, SFT_MAX_STEPS);
    SFT_REQUIRE(n_points >= 1 && n_points <= kMaxInt, "sft_track_advance: n_points = %lld (1 .. 2^31 - 1)", (long long)n_points);
    SFT_REQUIRE(frame0 >= 0 && frame0 <= (1 << 30), "sft_track_advance: frame0 = %d (0 .. 2^30)", frame0);
    SFT_REQUIRE(row_stride >= w && ch_stride >= 1 && field_stride >= 1, "sft_track_advance: bad fwd strides (field %lld, channel %lld, row %lld; w = %d)",
                (long long)field_stride, (long long)ch_stride, (long long)row_stride, w);
    if (bwd != nullptr)
        SFT_REQUIRE(b_row_stride >= w && b_ch_stride >= 1 && b_field_stride >= 1,
                    "sft_track_advance: bad bwd strides (field %lld, channel %lld, row %lld; w = %d)", (long long)b_field_stride,
                    (long long)b_ch_stride, (long long)b_row_stride, w);
    SFT_REQUIRE((state_xy == nullptr) == (state_status == nullptr), "sft_track_advance: state_xy and state_status come together (one of them is null)");
    SFT_REQUIRE((state_xy_out == nullptr) == (state_status_out == nullptr),
                "sft_track_advance: state_xy_out and state_status_out come together (one of them is null)");
    if (state_xy == nullptr)
        SFT_REQUIRE(n_points == (int64_t)h * w, "sft_track_advance: dense mode (null state) needs n_points = h * w = %lld, got %lld",
                    (long long)h * w, (long long)n_points);
    SFT_REQUIRE(!(alpha != alpha) && !(beta != beta), "sft_track_advance: alpha / beta is NaN");
    SFT_REQUIRE(aligned4(fwd) && aligned4(bwd) && aligned4(state_xy) && aligned4(out_xy) && aligned4(state_xy_out) && aligned4(start) &&
                    aligned4(counts),
                "sft_track_advance: a float / int32 pointer is not 4-byte aligned");
    const int64_t need = sft_track_advance_ws_bytes(n_steps, n_points);
    SFT_REQUIRE(ws_bytes >= need, "sft_track_advance: workspace of %lld bytes (needs %lld)", (long long)ws_bytes, (long long)need);
    AdvanceArgs a;
    a.fwd = fwd, a.bwd = bwd;
    a.f_field = field_stride, a.f_ch = ch_stride, a.f_row = row_stride;
    a.b_field = b_field_stride, a.b_ch = b_ch_stride, a.b_row = b_row_stride;
    a.n_steps = n_steps, a.h = h, a.w = w, a.frame0 = frame0;
    a.state_xy = state_xy, a.state_status = state_status, a.start = start, a.n_points = (int)n_points;
    a.alpha = alpha, a.beta = beta, a.sticky = sticky;
    a.out_xy = out_xy, a.out_status = out_status, a.state_xy_out = state_xy_out, a.state_status_out = state_status_out;
    a.counts = counts;
    hipStream_t s = (hipStream_t)stream;
    if (counts != nullptr) {
        const int st = clear_words("sft_track_advance (clear)", counts, (int64_t)n_steps * 4, s);
        if (st != SFT_OK) return st;
    }
    const unsigned blocks = (unsigned)((n_points + kBlock - 1) / kBlock);                    // <= 2^23
    hipLaunchKernelGGL(track_advance_kernel, dim3(blocks), dim3(kBlock), 0, s, a);
    return check_launch("sft_track_advance");
}

SFT_API int64_t sft_draw_tracks_ws_bytes(int n_frames, int h, int w) {
    if (n_frames < 1 || n_frames > 65535 || h < 1 || w < 1 || (int64_t)h * w > kMaxInt || (int64_t)h * w * n_frames >= ((int64_t)1 << 40))
        return fail(SFT_ERR_BAD_ARG, "sft_draw_tracks_ws_bytes: bad shape (%d frames of %d x %d)", n_frames, h, w);
    return (int64_t)n_frames * h * w * 4;
}

SFT_API int sft_draw_tracks(const uint8_t* src, int64_t src_frame_stride, int64_t src_row_stride, int64_t src_px_stride,
                            int64_t src_ch_stride, int n_frames, int h, int w, int first_frame, const float* xy, const uint8_t* status,
                            int n_rows, int64_t n_points, int first_row, int trail, int radius, int trail_radius, int draw_occluded,
                            const uint8_t* palette, int n_colours, const uint8_t* alpha_table, uint8_t* out, void* ws, int64_t ws_bytes,
                            void* stream) {
    SFT_REQUIRE(src && xy && status && palette && alpha_table && out && ws, "sft_draw_tracks: null argument");
    SFT_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= kMaxInt && h <= kMaxSide && w <= kMaxSide, "sft_draw_tracks: bad shape %d x %d", h, w);
    SFT_REQUIRE(n_frames >= 1 && n_frames <= 65535 && (int64_t)h * w * n_frames < ((int64_t)1 << 40),
                "sft_draw_tracks: %d frames of %d x %d in one call (1 .. 65535, fewer than 2^40 pixels)", n_frames, h, w);
    SFT_REQUIRE(n_rows >= 1, "sft_draw_tracks: n_rows = %d", n_rows);
    SFT_REQUIRE(n_points >= 1 && n_points <= SFT_DRAW_MAX_POINTS, "sft_draw_tracks: n_points = %lld (1 .. 2^20 - 1: the key holds 20 bits of it)",
                (long long)n_points);
    SFT_REQUIRE(trail >= 1 && trail <= SFT_DRAW_MAX_TRAIL, "sft_draw_tracks: trail = %d (1 .. %d)", trail, SFT_DRAW_MAX_TRAIL);
    SFT_REQUIRE(radius >= 0 && radius <= SFT_DRAW_MAX_RADIUS && trail_radius >= 0 && trail_radius <= SFT_DRAW_MAX_RADIUS,
                "sft_draw_tracks: radius = %d, trail_radius = %d (0 .. %d)", radius, trail_radius, SFT_DRAW_MAX_RADIUS);
    SFT_REQUIRE(n_colours >= 1, "sft_draw_tracks: n_colours = %d", n_colours);
    SFT_REQUIRE(src_frame_stride >= 0 && src_row_stride >= 0 && src_px_stride >= 0 && src_ch_stride >= 0,
                "sft_draw_tracks: negative source stride (%lld, %lld, %lld, %lld)", (long long)src_frame_stride, (long long)src_row_stride,
                (long long)src_px_stride, (long long)src_ch_stride);
    SFT_REQUIRE(first_frame >= 0 && first_frame <= (1 << 30) && first_row >= 0 && first_row <= (1 << 30),
                "sft_draw_tracks: first_frame = %d, first_row = %d (0 .. 2^30)", first_frame, first_row);
    SFT_REQUIRE(aligned4(xy) && aligned4(ws), "sft_draw_tracks: xy / ws not 4-byte aligned");
    const int64_t need = sft_draw_tracks_ws_bytes(n_frames, h, w);
    SFT_REQUIRE(ws_bytes >= need, "sft_draw_tracks: workspace of %lld bytes (needs %lld)", (long long)ws_bytes, (long long)need);
    DrawArgs a;
    a.src = src, a.s_frame = src_frame_stride, a.s_row = src_row_stride, a.s_px = src_px_stride, a.s_ch = src_ch_stride;
    a.n_frames = n_frames, a.h = h, a.w = w, a.first_frame = first_frame;
    a.xy = xy, a.status = status, a.n_rows = n_rows, a.n_points = (int)n_points, a.first_row = first_row;
    a.trail = trail, a.radius = radius, a.trail_radius = trail_radius, a.draw_occluded = draw_occluded;
    a.palette = palette, a.n_colours = n_colours, a.alpha_table = alpha_table;
    a.out = out, a.keys = static_cast<uint32_t*>(ws);
    hipStream_t s = (hipStream_t)stream;
    const int64_t pixels = (int64_t)n_frames * h * w;
    int st = clear_words("sft_draw_tracks (clear)", a.keys, pixels, s);
    if (st != SFT_OK) return st;
    hipLaunchKernelGGL(track_stamp_kernel, dim3(grid_for((int64_t)n_frames * n_points * trail)), dim3(kBlock), 0, s, a);
    st = check_launch("sft_draw_tracks (stamp)");
    if (st != SFT_OK) return st;
    hipLaunchKernelGGL(track_resolve_kernel, dim3(grid_for(pixels)), dim3(kBlock), 0, s, a);
    return check_launch("sft_draw_tracks (resolve)");
}
