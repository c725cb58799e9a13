// The per-point step of sft_track_advance and the drawing rules of sft_draw_tracks, as plain functions that compile for the GPU
// (csrc/track.hip) and for the host (csrc/host/track_host_main.cpp, run under the sanitizers): one copy of the rules.
// include/streamflow_track.h has the contract.  fp32 throughout, every operation rounded on its own: the pragma below (and
// -ffp-contract=off for the host program) keeps the compiler from fusing a multiply with an add.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SFT_HD __host__ __device__ __forceinline__
#else
#define SFT_HD inline
#endif

#pragma clang fp contract(off)

namespace sft_core {

constexpr uint8_t kVisible = 0, kOccluded = 1, kLost = 2, kPending = 3;

// one field of a direction: the u plane, the v plane, the row stride in floats (null u: the direction is absent)
struct Field {
    const float* u;
    const float* v;
    int64_t row;
};

struct Point {
    float x, y;
    uint8_t status;
};

// made on the floats, before any conversion to an integer: false for NaN, +-Inf and anything huge
SFT_HD bool inside(float x, float y, int h, int w) { return x >= 0.0f && x <= (float)(w - 1) && y >= 0.0f && y <= (float)(h - 1); }

// both planes of a field at an INSIDE position: the taps, weights and operation order of csrc/flow_consistency.hip's target() / blend()
SFT_HD void sample(const Field& f, float px, float py, int h, int w, float& su, float& sv) {
    const float fx0 = floorf(px), fy0 = floorf(py);
    const float fx = px - fx0, fy = py - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;                              // 0 <= x0 <= w - 1, 0 <= y0 <= h - 1
    const int x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1;
    const int y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
    const int64_t r0 = (int64_t)y0 * f.row, r1 = (int64_t)y1 * f.row;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    {
        const float top = gx * f.u[r0 + x0] + fx * f.u[r0 + x1];
        const float bot = gx * f.u[r1 + x0] + fx * f.u[r1 + x1];
        su = gy * top + fy * bot;
    }
    {
        const float top = gx * f.v[r0 + x0] + fx * f.v[r0 + x1];
        const float bot = gx * f.v[r1 + x0] + fx * f.v[r1 + x1];
        sv = gy * top + fy * bot;
    }
}

// a state byte as the walk reads it: anything above PENDING is LOST
SFT_HD uint8_t read_status(uint8_t s) { return s > kPending ? kLost : s; }

// a PENDING point whose start frame has come: VISIBLE at its query, or LOST at once
SFT_HD void activate(Point& p, int h, int w) { p.status = inside(p.x, p.y, h, w) ? kVisible : kLost; }

// an ACTIVE point through one field (bwd.u null: no visibility test, bwd is not read)
SFT_HD void step(Point& p, const Field& fwd, const Field& bwd, int h, int w, float alpha, float beta, bool sticky) {
    if (!inside(p.x, p.y, h, w)) {
        p.status = kLost;
        return;
    }
    float u, v;
    sample(fwd, p.x, p.y, h, w, u, v);
    const float qx = p.x + u, qy = p.y + v;
    if (!inside(qx, qy, h, w)) {
        p.status = kLost;                                                // terminal; the position stays
        return;
    }
    p.x = qx, p.y = qy;
    if (bwd.u == nullptr) {
        p.status = kVisible;
        return;
    }
    float su, sv;
    sample(bwd, qx, qy, h, w, su, sv);
    const float m2 = u * u + v * v;
    const float dx = u + su, dy = v + sv;
    const float lhs = dx * dx + dy * dy;
    const float rhs = alpha * (m2 + (su * su + sv * sv)) + beta;
    const bool vis = lhs <= rhs;                                         // false for NaN
    p.status = (vis && !(sticky && p.status == kOccluded)) ? kVisible : kOccluded;
}

// the row of frame f: what the point is after it
SFT_HD void advance_row(Point& p, int start, int f, const Field& fwd, const Field& bwd, int h, int w, float alpha, float beta,
                        bool sticky) {
    if (p.status == kPending) {
        if (start <= f) activate(p, h, w);
    } else if (p.status <= kOccluded) {
        step(p, fwd, bwd, h, w, alpha, beta, sticky);
    }
}

// ---- drawing ----------------------------------------------------------------------------------------------------------------------

SFT_HD bool drawable(float x, float y, uint8_t status, bool draw_occluded, int h, int w) {
    return (status == kVisible || (draw_occluded && status == kOccluded)) && inside(x, y, h, w);
}

SFT_HD uint32_t draw_key(int trail, int age, int64_t point) { return ((uint32_t)(trail - age) << 20) | (uint32_t)(point + 1); }

// point s of 0 .. n on the integer line from a along d (n = max(|dx|, |dy|) >= 1), one axis
SFT_HD int line_point(int a, int d, int s, int n) {
    const int m = d < 0 ? -d : d;
    const int t = (m * 2 * s + n) / (2 * n);
    return d < 0 ? a - t : a + t;
}

// the disc of radius r about (cx, cy), clipped to the frame: put(x, y) per pixel
template <class Put>
SFT_HD void disc(int cx, int cy, int r, int h, int w, Put put) {
    for (int dy = -r; dy <= r; ++dy) {
        const int y = cy + dy;
        if (y < 0 || y >= h) continue;
        for (int dx = -r; dx <= r; ++dx) {
            const int x = cx + dx;
            if (x < 0 || x >= w || dx * dx + dy * dy > r * r) continue;
            put(x, y);
        }
    }
}

// everything the sample of age `age` stamps: (x, y) its position, (nx, ny) the sample one frame newer (newer_ok: it is drawable)
template <class Put>
SFT_HD void stamp(float x, float y, bool newer_ok, float nx, float ny, int age, int radius, int trail_radius, int max_seg, int h, int w,
                  Put put) {
    const int cx = (int)rintf(x), cy = (int)rintf(y);
    if (age == 0) {
        disc(cx, cy, radius, h, w, put);
        return;
    }
    disc(cx, cy, trail_radius, h, w, put);
    if (!newer_ok) return;
    const int ddx = (int)rintf(nx) - cx, ddy = (int)rintf(ny) - cy;
    const int ax = ddx < 0 ? -ddx : ddx, ay = ddy < 0 ? -ddy : ddy;
    const int n = ax > ay ? ax : ay;
    if (n < 1 || n > max_seg) return;
    for (int s = 1; s <= n; ++s) disc(line_point(cx, ddx, s, n), line_point(cy, ddy, s, n), trail_radius, h, w, put);
}

SFT_HD uint8_t blend_channel(unsigned colour, unsigned src, unsigned alpha) {
    return (uint8_t)((colour * alpha + src * (255u - alpha) + 127u) / 255u);
}

}  // namespace sft_core
