/* libstreamflow_track: point tracking through a video's flow fields and track drawing, HIP kernels for gfx950 behind a C ABI.
 *
 * A second, small library next to libstreamflow_hip (include/streamflow_hip.h) with the same conventions:
 *   - return value: 0 on success, negative SFT_ERR_* otherwise; sft_last_error() gives the message (thread-local).
 *   - every pointer is a device pointer unless it says otherwise; the stream argument comes last (NULL: the default stream).
 *   - every argument is validated BEFORE any launch; a refused call has written nothing and enqueued nothing.
 *   - nothing synchronises with the host, allocates, or uses another stream: every entry point can be captured into a graph.
 *     Words an entry point must reset per call are cleared by a kernel, never by hipMemsetAsync (csrc/sf_common.h has the reason).
 * The two libraries share no symbol: nothing in one resolves into the other, and either loads alone.
 *
 * Conventions
 *   A flow field is two fp32 planes (u = x displacement, v = y displacement) of h rows of w floats with contiguous rows; strides are
 *   in floats, as sf_flow_consistency's.  Field k of a call is the pair (frame0 + k, frame0 + k + 1): it leads from frame
 *   frame0 + k to the next.  Positions are pixel coordinates (x, y), pixel centres at integers.  The INSIDE TEST of a position is
 *       x >= 0 && x <= (float)(w - 1) && y >= 0 && y <= (float)(h - 1)
 *   on the floats, before any conversion to an integer: NaN, +-Inf and 1e30 compare false and never form an address.
 *   Arithmetic is fp32 with every operation rounded on its own (no FMA contraction), in the order stated below, so a float32
 *   restatement reproduces positions, status bytes and drawn bytes bit for bit (tests/track_cases.py).
 *
 * Bilinear sampling of a plane a at an inside position (px, py), as csrc/flow_consistency.hip's target() / blend():
 *       x0 = floor(px), y0 = floor(py), fx = px - x0, fy = py - y0, x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1)
 *       gx = 1 - fx, gy = 1 - fy, top = gx a[y0][x0] + fx a[y0][x1], bot = gx a[y1][x0] + fx a[y1][x1], value = gy top + fy bot
 */
#ifndef STREAMFLOW_TRACK_H
#define STREAMFLOW_TRACK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFT_VERSION 1

enum {
    SFT_OK = 0,
    SFT_ERR_BAD_ARG = -1,     /* null pointer, size or stride outside the limits, inconsistent combination */
    SFT_ERR_UNSUPPORTED = -2, /* a shape the kernels are not built for                                     */
    SFT_ERR_HIP = -3          /* a HIP runtime call failed (message holds hipGetErrorString)               */
};

/* status byte of a point in a row */
enum {
    SFT_VISIBLE = 0,  /* active, and the forward-backward test of the step that led here passed (or there was no test) */
    SFT_OCCLUDED = 1, /* active, the test failed (positions keep advancing)                                          */
    SFT_LOST = 2,     /* left the frame or met a non-finite value: terminal, the position is frozen                  */
    SFT_PENDING = 3   /* the point's start frame has not come yet: the position is the query                         */
};

#define SFT_MAX_STEPS 4096    /* fields per sft_track_advance call */
#define SFT_DRAW_MAX_SEG 64   /* longest trail segment (in steps of its longer axis) that is drawn */
#define SFT_DRAW_MAX_TRAIL 255
#define SFT_DRAW_MAX_RADIUS 16
#define SFT_DRAW_MAX_POINTS ((1 << 20) - 1)

int sft_version(void);
const char* sft_last_error(void);

/* sft_track_advance: n_steps fields, n_points points, ONE launch; a thread owns a point and walks all fields, its position and
 * status in registers between steps.
 *
 * State: state_xy fp32 [2][P] (x plane, y plane) and state_status uint8 [P], both or neither.  start int32 [P] or NULL (every point
 * started).  A point whose state is PENDING holds its query position; it BECOMES ACTIVE at frame start[p]: on entry when start[p] <=
 * frame0, else in the row of that frame.  Becoming active it is VISIBLE at the query position, or LOST at once when the query fails the
 * inside test.  Any other state byte is carried as it is (a byte above 3 reads as LOST).
 * Dense mode: state_xy == NULL (and state_status == NULL): n_points must be h * w, point i is pixel (i % w, i / w), VISIBLE on entry;
 * `start` is not read.
 *
 * Row k (k = 0 .. n_steps - 1) describes frame f = frame0 + k + 1.  Per point:
 *   PENDING with start[p] > f: the row holds the query and PENDING.
 *   PENDING with start[p] <= f: becomes active as above; the row holds the query and VISIBLE or LOST.  Field k is not applied.
 *   LOST: the row holds the frozen position and LOST.
 *   active at p: p itself is held to the inside test first (a caller's state may hold anything): failing it the point is LOST and the
 *     row keeps p.  Else (u, v) = field k sampled bilinearly at p, q = p + (u, v).  q failing the inside test: LOST, the row keeps p.
 *     Else the row holds q.  With bwd: (su, sv) = bwd field k sampled at q, dx = u + su, dy = v + sv,
 *         visible = dx dx + dy dy <= alpha ((u u + v v) + (su su + sv sv)) + beta          (false for NaN)
 *     the expression and order of sf_flow_consistency; status VISIBLE or OCCLUDED; with `sticky` a point that was OCCLUDED stays
 *     OCCLUDED.  Without bwd (NULL) the status is VISIBLE and bwd is never read.
 *
 * out_xy fp32 [n_steps][2][P], out_status uint8 [n_steps][P]; state_xy_out / state_status_out (both or neither; may alias the
 * inputs) receive the last row.  counts (optional) uint32 [n_steps][4]: points of each status per row, WRITTEN, not added; exact and
 * independent of the launch order (wave reductions, integer atomics on words a kernel of the same call cleared).
 * ws / ws_bytes: sft_track_advance_ws_bytes (0 in this version: ws may be NULL).
 *
 * SFT_ERR_BAD_ARG before any launch for: a null fwd, out_xy or out_status; h or w < 1 or above 2^24, or h * w >= 2^31; n_steps outside
 * 1 .. SFT_MAX_STEPS; n_points outside 1 .. 2^31 - 1; frame0 outside 0 .. 2^30; a row stride below w, a channel or field stride < 1
 * (bwd's too when it is given); dense mode with n_points != h * w; one of state_xy / state_status (or of the two state outputs)
 * without the other; alpha or beta NaN; a float pointer not 4-byte aligned; ws_bytes below the need. */
int64_t sft_track_advance_ws_bytes(int n_steps, int64_t n_points);
int sft_track_advance(const float* fwd, int64_t field_stride, int64_t ch_stride, int64_t row_stride,
                      const float* bwd, int64_t b_field_stride, int64_t b_ch_stride, int64_t b_row_stride,
                      int n_steps, int h, int w, int frame0,
                      const float* state_xy, const uint8_t* state_status, const int32_t* start, int64_t n_points,
                      float alpha, float beta, int sticky,
                      float* out_xy, uint8_t* out_status, float* state_xy_out, uint8_t* state_status_out,
                      uint32_t* counts, void* ws, int64_t ws_bytes, void* stream);

/* sft_draw_tracks: tracks drawn on n_frames uint8 RGB frames, bitwise reproducible.
 *
 * src: frames with BYTE strides (frame, row, pixel, channel), as sf_warp_frames' src; frame j is frame first_frame + j of the video.
 * xy fp32 [n_rows][2][P], status uint8 [n_rows][P]: row r describes frame first_row + r (the rows of sft_track_advance, stacked).
 * out: uint8 [n_frames][h][w][3], dense.  palette uint8 [n_colours][3]; alpha_table uint8 [trail].
 *
 * Stamp (a thread per frame, point and age a = 0 .. trail - 1): the sample of age a of frame g is the point's row of frame g - a.
 * A sample is DRAWABLE when its row is in the window, its status is VISIBLE (or OCCLUDED with draw_occluded) and its position passes
 * the inside test; its centre is (rintf(x), rintf(y)).  Age 0 stamps the integer disc dx^2 + dy^2 <= radius^2 about its centre;
 * age a >= 1 stamps the disc of trail_radius and, when the sample of age a - 1 is drawable too and n = max(|dx|, |dy|) between the two
 * centres is 1 .. SFT_DRAW_MAX_SEG, the same disc about every point s = 0 .. n of the integer line from its own centre c to the newer
 * one, c + sgn(d) ((|d| 2 s + n) / (2 n)) per axis in non-negative integer division.  Longer segments are skipped.  Everything is
 * clipped to the frame.  A pixel is written by an atomic maximum of the key ((trail - a) << 20) | (point + 1): the newest age
 * wins, then the higher point index, whatever the launch order.  The key image (uint32 per pixel) lives in ws and is cleared by
 * a kernel of the call.
 * Resolve (a thread per pixel): key 0 passes the source bytes through; else colour = palette[point % n_colours], alpha =
 * alpha_table[age] and every channel is (c alpha + src (255 - alpha) + 127) / 255 in integers.
 *
 * SFT_ERR_BAD_ARG before any launch for: null pointers; h or w < 1 or above 2^24, or h * w >= 2^31; n_frames outside 1 .. 65535 or n_frames * h * w
 * >= 2^40; n_rows < 1; n_points outside 1 .. SFT_DRAW_MAX_POINTS; trail outside 1 .. SFT_DRAW_MAX_TRAIL; a radius outside
 * 0 .. SFT_DRAW_MAX_RADIUS; n_colours < 1; a negative source stride; first_frame or first_row outside 0 .. 2^30; xy not 4-byte or ws
 * not 4-byte aligned; ws_bytes below sft_draw_tracks_ws_bytes (4 n_frames h w). */
int64_t sft_draw_tracks_ws_bytes(int n_frames, int h, int w);
int sft_draw_tracks(const uint8_t* src, int64_t src_frame_stride, int64_t src_row_stride, int64_t src_px_stride, int64_t src_ch_stride,
                    int n_frames, int h, int w, int first_frame,
                    const float* xy, const uint8_t* status, int n_rows, int64_t n_points, int first_row,
                    int trail, int radius, int trail_radius, int draw_occluded,
                    const uint8_t* palette, int n_colours, const uint8_t* alpha_table,
                    uint8_t* out, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
