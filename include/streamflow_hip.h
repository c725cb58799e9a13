/* streamflow_hip.h -- C ABI of libstreamflow_hip.so (MI355X / gfx950 only).
 *
 * The reference (littlespray/StreamFlow) is pure Python/PyTorch and has no FFI or plugin registry
 * (SURVEY.md section 8b): its "interface" for the hot path is the Python call surface of
 * core/corr.py, core/utils/utils.py, core/gma.py, core/update.py and core/models/streamflow.py.
 * Each entry point below replaces the library kernels one of those call sites dispatches to; the
 * reference file:line it stands in for is cited per function.  The Python classes in
 * streamflow_amd/ keep the reference signatures and state-dict keys and call these through ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 data unless stated; the caller owns all memory
 *     (inputs, outputs, workspaces); the library never allocates or frees device memory and keeps
 *     no global state besides a thread-local error string.
 *   - `stream` is a hipStream_t passed as void*; every call only ENQUEUES work on it (no host sync,
 *     no default-stream use), so calls may be captured into a HIP graph.
 *   - return value: 0 on success, negative SF_ERR_* otherwise; sf_last_error() gives the message.
 *   - feature planes are "channel-major": tensor [n_img][C][P] with P = h*w contiguous (NCHW).
 */
#ifndef STREAMFLOW_HIP_H
#define STREAMFLOW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SF_VERSION 141

enum {
    SF_OK = 0,
    SF_ERR_BAD_ARG = -1,     /* null pointer, non-positive dim, unsupported combination */
    SF_ERR_UNSUPPORTED = -2, /* shape outside what the kernels are built for            */
    SF_ERR_HIP = -3          /* a HIP runtime call failed (message holds hipGetErrorString) */
};

int sf_version(void);
const char* sf_last_error(void);

/* ---- a5: coords_grid  (core/utils/utils.py:82-85) --------------------------------------------
 * out [batch][2][ht][wd]; out[b][0][y][x] = x, out[b][1][y][x] = y (exact small integers). */
int sf_coords_grid(float* out, int batch, int ht, int wd, void* stream);

/* ---- a4: bilinear_sampler  (core/utils/utils.py:65-79; F.grid_sample bilinear/zeros/align_corners)
 * img [M][C][Hi][Wi], coords [M][Ho][Wo][2] pixel (x,y)  ->  out [M][C][Ho][Wo].
 * mask_out (optional, may be NULL): [M][Ho][Wo][1] in-bounds indicator as the reference's mask=True.
 * A tap outside the image is zero.  A non-finite coordinate (and one beyond +-1e6 pixels) samples zero, and the output is
 * finite: the rule the lookup kernels follow for the same input. */
int sf_bilinear_sampler(const float* img, const float* coords, float* out, float* mask_out,
                        int M, int C, int Hi, int Wi, int Ho, int Wo, void* stream);

/* ---- a1+a2: CorrBlock.__init__  (core/corr.py:7-21,46-54) -------------------------------------
 * One launch builds the 4-level pyramids of `pairs` frame pairs of `B` clips.
 * Features: clip b, pair t reads f1 + b*f_clip_stride + t*f_pair_stride and the same offset from f2,
 * each a [D][h*w] plane set (for a single reference-style call: pairs=1, f_clip_stride=D*h*w).
 * Volumes: level l of (pair t, clip b, source pixel i) is the [h>>l][w>>l] map at
 * lvl{l} + t*lvl_pair_stride[l] + (b*h*w + i)*(h>>l)*(w>>l)   (floor pooling over the TARGET dims),
 * i.e. per pair exactly the reference's corr_pyramid[l] of shape [B*h*w, 1, h>>l, w>>l].
 * Level 0 = f1^T f2 / sqrt(D); levels 1..3 are pooled in the GEMM epilogue while the tile is still in
 * registers, so every pyramid cell is written once and level 0 is never re-read.
 * lvl_pair_stride: HOST array of 4 strides in floats (ignored when pairs == 1; may be NULL then).
 * num_levels must be 4 (streamflow.py:38).  precision: SF_PRECISION_FP32 (exact fp32 MFMA, k-ordered fmaf
 * chain), SF_PRECISION_F16X3 (split fp16, fp32 accumulate; see sf_gemm) -- both write fp32 volumes -- or
 * SF_PRECISION_F16: lvl0..lvl3 then point to IEEE fp16 cells (same indexing, lvl_pair_stride in cells; half the
 * bytes), products are single f16 MFMAs with fp32 accumulation. */
int sf_corr_build_pyramid(const float* f1, const float* f2, int64_t f_clip_stride, int64_t f_pair_stride,
                          float* lvl0, float* lvl1, float* lvl2, float* lvl3,
                          const int64_t* lvl_pair_stride, int B, int pairs, int D, int h, int w,
                          int num_levels, int precision, void* split_ws, int64_t split_ws_bytes, void* stream);
/* Workspace of the SF_PRECISION_F16X3 build: the (hi, lo) fp16 split of every f1 / f2 image, packed in k-octets
 * per pixel so that the build kernel can DMA operand tiles straight into LDS.  Not needed (may be NULL / 0) for
 * SF_PRECISION_FP32.  Contents are scratch: dead once the call's kernels have run. */
int64_t sf_corr_build_ws_bytes(int B, int pairs, int D, int h, int w);
/* The same build into PITCHED maps (fp32 and fp16 cells): level l of (pair t, clip b, source pixel i) is (h>>l) rows of
 * lvl_pitch[l] cells at lvl{l} + t*lvl_pair_stride[l] + (b*h*w + i)*(h>>l)*lvl_pitch[l]; cell (y, x), x < w>>l, at y*lvl_pitch[l] + x.
 * lvl_pitch: HOST array of 4 row pitches in cells, w>>l <= lvl_pitch[l] <= w rounded up to 32; NULL = the reference's dense layout
 * (== sf_corr_build_pyramid).  Why: core/corr.py:13-21 keeps [N, h_l, w_l] maps; at KITTI's 156-cell rows (624 bytes) every
 * 128-byte store run of the build straddles two cache lines.  A pitch of a multiple of 32 cells puts every row on a line
 * boundary; the pad cells x >= w>>l of a row are WRITTEN (unspecified values) so that whole lines are written; the reference's
 * [N, 1, h_l, w_l] tensor is the strided view [..., :w_l] of the pitched one (streamflow_amd.corr.CorrBlock.corr_pyramid). */
int sf_corr_build_pyramid_pitched(const float* f1, const float* f2, int64_t f_clip_stride, int64_t f_pair_stride,
                                  float* lvl0, float* lvl1, float* lvl2, float* lvl3,
                                  const int64_t* lvl_pair_stride, const int32_t* lvl_pitch, int B, int pairs, int D, int h, int w,
                                  int num_levels, int precision, void* split_ws, int64_t split_ws_bytes, void* stream);

/* ---- a3: CorrBlock.__call__  (core/corr.py:23-44) ----------------------------------------------
 * Image index img = b*pairs + t.  coords [B*pairs][2][h][w] (ch0 = x, ch1 = y)  ->
 * out[img][l*(2r+1)^2 + a*(2r+1) + b'][p] samples level l of (pair t, clip b) at
 * (x/2^l + a - r, y/2^l + b' - r), bilinear, zeros outside (first window axis moves x, corr.py:31-37).
 * out image img starts at out + img*out_img_stride (floats), channel stride h*w, so the caller can
 * write straight into a wider concatenation buffer.  Volumes are addressed as in
 * sf_corr_build_pyramid.  radius must be 4, num_levels 4.  vol_precision: the precision the volumes were built
 * with -- SF_PRECISION_F16 means lvl0..lvl3 hold fp16 cells (taps are blended in fp32), anything else fp32 cells.
 * out_koct (optional, fp16 volumes only): the same 324 channels a second time, rounded to fp16, as k-octet planes
 * [41][h*w][8] per image (SF_LAYOUT_F16_KOCT, image stride out_koct_img_stride halves, rows 324..327 zero): the
 * B operand of the first sf_gemm of the correlation encoder.
 * Established by tests/test_gpu_corr_kernels.py (grids 8 x 8 .. 24 x 40, D = 1 .. 256, B x pairs up to 2 x 2 and 1 x 3, every base,
 * stride and pitch below with gaps and off 16 bytes):
 *   sf_corr_build_ws_bytes = 2 * B * pairs * (D rounded up to 32) * h * w * 4; exactly that many bytes suffice, 16-byte aligned; the
 *       SF_PRECISION_F16 build needs the same workspace as F16X3, SF_PRECISION_FP32 none.
 *   builds write the data cells of the four levels -- with a pitch, the (h>>l) * lvl_pitch[l] cells of every map, pad cells included --
 *       and nothing else: no cell between two pairs' spans, before the first or behind the last; f1, f2 are read only.
 *   alignment: f1, f2, the level bases and `out` need their element's alignment only (4 bytes; 4 bytes for fp16 cells too, as the
 *       parameters are float*); f_clip_stride, f_pair_stride, lvl_pair_stride (odd numbers of fp16 cells included), out_img_stride are
 *       free.  An odd lvl_pair_stride in fp16 cells puts the packed 4-byte level-0 stores of the odd pairs on 2-byte aligned
 *       addresses: the kernel has NO branch for that, the rule rests on gfx950 executing unaligned dword buffer stores (measured,
 *       bitwise equal); code that assumes 4-byte alignment there must refuse odd strides first.
 *       Aligned / vector and unaligned / scalar forms are bitwise the same: a placed run equals the contiguous one, pitched
 *       data cells equal the dense ones, f2 in a buffer of its own equals f2 = f1 + f_pair_stride.
 *   image (b, t) of a batch is bitwise the call on that pair alone (B = pairs = 1), builds and lookups.
 *   F16X3 splits with streamflow_amd/csrc/split_operand.h split8(): towards zero twice, |x - (hi + lo)| < max(2^-20 |x|, 2^-24), 2^-23 for
 *       |x| < 2^-14 -- not the round-to-nearest split of sf_gemm's ~2^-22; cells stay within the per-cell bound of tests/corr_cases.py.
 *   lookups: a coordinate that is NaN, +-inf or, after the division by 2^l, not strictly inside (-1e6, 1e6) samples zero at that
 *       level; the output is finite everywhere and exactly zero where all four taps lie outside the level (a 1 x 1 level included);
 *       -0.0 is 0.  Beside fp32 planes out_koct is bitwise fp16(out) of the same launch, rows 324..327 zero; nothing else is written. */
int sf_corr_lookup(const float* lvl0, const float* lvl1, const float* lvl2, const float* lvl3,
                   const int64_t* lvl_pair_stride, const float* coords, float* out, int64_t out_img_stride,
                   void* out_koct, int64_t out_koct_img_stride, int B, int pairs, int h, int w, int num_levels,
                   int radius, int vol_precision, void* stream);
/* Lookup in the pitched maps of sf_corr_build_pyramid_pitched (fp32 cells only; lvl_pitch as there, NULL = dense). */
int sf_corr_lookup_pitched(const float* lvl0, const float* lvl1, const float* lvl2, const float* lvl3,
                           const int64_t* lvl_pair_stride, const int32_t* lvl_pitch, const float* coords, float* out,
                           int64_t out_img_stride, void* out_koct, int64_t out_koct_img_stride, int B, int pairs, int h, int w,
                           int num_levels, int radius, int vol_precision, void* stream);

/* ---- a1 + a2 + a3 in the BLOCKED fp16 volume layout (core/corr.py:7-54; csrc/corr_blocked.hip) --------------------------
 * Same mathematics as sf_corr_build_pyramid(SF_PRECISION_F16) / sf_corr_lookup, different memory layout: ONE buffer per
 * launch; image img = b*pairs + t starts at vol + img * vol_img_stride_bytes and holds one RECORD of rec_bytes per source
 * pixel (src_rows = h*w rounded up to 128 records; the padding records are written by the build and never read):
 *     record = [level 0 | level 1 | level 2 | level 3], level l = nby[l] x nbx[l] blocks of 8 x 8 cells (nb = ceil(size/8)),
 *     block (by, bx) at lvl_off[l] + (by*nbx[l] + bx)*128, cell (ty, tx) at byte ((tx%8)*8 + ty%8)*2 of block (ty/8, tx/8).
 * A 128-byte block is one cache line: a 10 x 10 lookup footprint touches ~4.5 lines per level instead of ~11 in the
 * row-major volume, and the build stores a level-0 block column (16 bytes) per lane and accumulator register.
 * Cells of a block outside the level (hl, wl not multiples of 8) have UNSPECIFIED contents; the lookup ignores them.
 *   sf_corr_blocked_geometry: the numbers above for an h x w feature grid (any output pointer may be NULL).
 *   sf_corr_blocked_bytes: n_img * src_rows * rec_bytes.
 *   sf_corr_build_blocked: features as in sf_corr_build_pyramid; ws = scratch of sf_corr_build_blocked_ws_bytes() bytes
 *       (fp16 k-octet repack of the features, 16-byte aligned); vol 128-byte aligned, vol_img_stride_bytes % 128 == 0.
 *   sf_corr_lookup_blocked: coords / channel order / sampling rule exactly as sf_corr_lookup.  out_koct: the 324 channels
 *       rounded to fp16 as k-octet planes [41][h*w][8] per image (SF_LAYOUT_F16_KOCT, rows 324..327 zero) -- the operand
 *       (and, through SfGemm.r_f16, the residual) of the correlation encoder's first block: no fp32 copy is written.
 *       out: optional fp32 planes [324][h*w] per image (un-rounded taps; API parity and tests).  At least one of the two.
 * Established by tests/test_gpu_corr_kernels.py (the same grids, depths and batches):
 *   sf_corr_blocked_bytes = n_img * src_rows * rec_bytes and sf_corr_build_blocked_ws_bytes = 2 * n_img * 32 * Np * 16 with
 *       Np = h*w + 1 rounded up to 8 (whatever D): exactly that many bytes suffice.  The build writes the src_rows * rec_bytes of every
 *       image (padding cells and records included) and nothing between or behind the images; features are read only.
 *   alignment: the build needs vol % 128 == 0 and a stride % 128 == 0 of at least sf_corr_blocked_bytes(1, h, w); the LOOKUP needs 16
 *       bytes for vol and its stride only (a built volume may be moved); f1, f2, coords, out need 4 bytes, out_koct 16 and a stride % 8.
 *   every frame is packed ONCE for both sides iff pairs > 1, f2 == f1 + f_pair_stride and 1 / sqrt(D) is not a power of two unless its
 *       root is one too (D = 16, 256: sqrt(scale) folded into every frame; D = 64: packed per side, scale folded into f1).  With the
 *       same folded factors the volume is bitwise the same whichever way f2 is handed over, and image (b, t) of a batch is bitwise the
 *       call on that pair alone; with different ones (D = 16, 256) the two agree within the rounding of fp16 subnormal features.
 *   placed runs (vol_img_stride_bytes, feature strides and bases, out / out_koct strides and bases) are bitwise the contiguous one.
 *   lookup: non-finite and far coordinates as sf_corr_lookup; out alone, out_koct alone and both give bitwise the same values
 *       (out_koct = fp16(out), rows 324..327 zero). */
int sf_corr_blocked_geometry(int h, int w, int64_t* rec_bytes, int64_t* lvl_off, int32_t* nby, int32_t* nbx,
                             int64_t* src_rows);
int64_t sf_corr_blocked_bytes(int n_img, int h, int w);
int64_t sf_corr_build_blocked_ws_bytes(int n_img, int D, int h, int w);
int sf_corr_build_blocked(const float* f1, const float* f2, int64_t f_clip_stride, int64_t f_pair_stride,
                          void* vol, int64_t vol_img_stride_bytes, int B, int pairs, int D, int h, int w,
                          void* ws, int64_t ws_bytes, void* stream);
int sf_corr_lookup_blocked(const void* vol, int64_t vol_img_stride_bytes, const float* coords, float* out,
                           int64_t out_img_stride, void* out_koct, int64_t out_koct_img_stride, int B, int pairs,
                           int h, int w, void* stream);

/* ---- a1 + a2 + a3 with fp32 cells in a BLOCKED layout (core/corr.py:7-54 in the reference's own fp32: streamflow.py:107,110;
 * csrc/corr_blocked32.hip) -- the volumes of the fp32-class presets and of BASELINE.json configuration 3 as worded ---------
 * Same mathematics as sf_corr_build_pyramid(SF_PRECISION_F16X3) / sf_corr_lookup(SF_PRECISION_FP32); the memory layout is the
 * one of sf_corr_build_blocked with fp32 cells: level l = nby[l] x nbx[l] blocks of 4 ROWS x 8 COLUMNS (nby = ceil(hl/4),
 * nbx = ceil(wl/8)), block (by, bx) at lvl_off[l] + (by*nbx[l] + bx)*128, cell (ty, tx) at byte ((tx%8)*4 + ty%4)*4 of block
 * (ty/4, tx/8).  A footprint touches ~6.9 cache lines per level instead of ~11.6 in the pitched row-major maps.
 * Padding cells / records: unspecified contents, never read.
 *   sf_corr_lookup_blocked32: out = fp32 planes [324][h*w] per image (channel order / sampling rule of sf_corr_lookup).
 * Established by tests/test_gpu_corr_kernels.py (the same grids, depths and batches):
 *   sf_corr_blocked32_bytes = n_img * src_rows * rec_bytes; sf_corr_build_blocked32_ws_bytes = 2 * n_img * 2 * (D rounded up to 32) / 8
 *       * h * w * 16 (= sf_corr_build_ws_bytes): exactly that many bytes suffice; the build writes the images' src_rows * rec_bytes only.
 *   alignment as for the blocked fp16 volume (128 bytes for the build, 16 for the lookup, 4 for features, coords and out); frames
 *       shared or f2 in a buffer of its own, placed or contiguous, batch or single pair: bitwise the same cells and features.
 *   for unit-normal features (cells of O(1), D up to 256) cells agree with the pitched F16X3 build within 2e-6 and looked-up features
 *       within 2e-5 (the same split8() operands, another summation order); the limits scale with the square of the feature scale;
 *       non-finite and far coordinates as sf_corr_lookup. */
int sf_corr_blocked32_geometry(int h, int w, int64_t* rec_bytes, int64_t* lvl_off, int32_t* nby, int32_t* nbx,
                               int64_t* src_rows);
int64_t sf_corr_blocked32_bytes(int n_img, int h, int w);
int64_t sf_corr_build_blocked32_ws_bytes(int n_img, int D, int h, int w);
int sf_corr_build_blocked32(const float* f1, const float* f2, int64_t f_clip_stride, int64_t f_pair_stride,
                            void* vol, int64_t vol_img_stride_bytes, int B, int pairs, int D, int h, int w,
                            void* ws, int64_t ws_bytes, void* stream);
int sf_corr_lookup_blocked32(const void* vol, int64_t vol_img_stride_bytes, const float* coords, float* out,
                             int64_t out_img_stride, int B, int pairs, int h, int w, void* stream);

/* ---- a1 + a2 + a3 WITHOUT a volume: on-demand lookup from packed features (core/corr.py:7-54; csrc/corr_direct.hip) -------
 * Pooling is linear: level l of the volume at target cell J is <f1_i, pool_l(f2)_J> / sqrt(D), pool_l = the floor 2 x 2 mean
 * applied l times to the features of frame 2.  Nothing of size N^2 is stored; every lookup computes the cells its windows touch.
 *   sf_corr_direct_pack: once per clip; features addressed exactly as in sf_corr_build_blocked.  Writes, per image img = b*pairs + t
 *       at ws + img * img_bytes, five REGIONS back to back: f1 (N = h*w cells), then level l = 0..3 of the pyramid of f2
 *       (Nl = (h>>l)*(w>>l) cells, cell (y, x) at y*(w>>l) + x); img_bytes = parts * (Dp/8) * 16 * (2 N + N1 + N2 + N3).
 *           region = [part][k-octet][cell][8] IEEE fp16, Dp = D rounded up to 32 (rows D .. Dp-1 zero),
 *           parts = 1 (SF_PRECISION_F16: the value rounded to nearest) or 2 (SF_PRECISION_F16X3: hi, lo of split_operand.h split8()).
 *       Levels 1..3 are pooled in fp32 from the fp32 level below (vertical pair, horizontal pair, times 0.25) and rounded to the
 *       operand format ONCE.  Every frame is packed per side and pair (a frame shared by two pairs is packed twice: the result
 *       is bitwise the same whichever way f2 is handed over).  Every byte of the workspace is written.
 *   sf_corr_direct_ws_bytes: B * pairs * img_bytes -- exactly that many bytes suffice (0 for an unsupported precision or grid).
 *   sf_corr_direct_lookup: coords / channel order l*81 + a*9 + b' / sampling rule / NaN, infinite and far coordinates exactly as
 *       sf_corr_lookup (a scaled coordinate not strictly inside (-1e6, 1e6) samples zero; exactly zero where all four taps lie
 *       outside; -0.0 is 0).  out: fp32 planes [324][h*w] per image (stride out_img_stride floats); out_koct: fp16 k-octet planes
 *       [41][h*w][8] per image (rows 324..327 zero), bitwise fp16(out) of the same launch.  At least one of the two.
 *       A workgroup takes 16 consecutive source pixels; per level it walks the bounding box of their clipped windows in chunks of
 *       16 cells on v_mfma_f32_16x16x32_f16 (chunks no pixel needs are skipped): with smooth flow about twice the needed products,
 *       with arbitrary coordinates up to pixels x level cells.  Enqueues on `stream` only: no allocation, no synchronisation.
 *   precision: SF_PRECISION_F16 (one product, fp32 accumulation: the class of the blocked fp16 volume) or SF_PRECISION_F16X3 (three
 *       products: the class of the blocked fp32 volume); anything else SF_ERR_UNSUPPORTED, as is D > 256.  Cells are never rounded
 *       to fp16 and never stored, so the values are NOT bitwise the volume routes'; both are held to float64.
 *   SF_ERR_BAD_ARG: null pointers (both outputs NULL included), a grid below 8 x 8, ws not 16-byte aligned or ws_bytes too small,
 *       out_koct not 16-byte aligned or its stride no multiple of 8 halves.  f1, f2, coords and out need 4-byte alignment, every
 *       stride is free.
 * Established by tests/test_gpu_corr_direct.py (grids 8 x 8 .. 24 x 40, D = 1 .. 256, B x pairs up to 2 x 2 and 1 x 3, noisy, uniform
 * random, all-dead and opposite-corner coordinates): every channel within the derived bound of tests/corr_direct_cases.py of float64;
 * the summation order of a cell is fixed (k-steps of 32 ascending; hi*hi, hi*lo, lo*hi per step), so a pixel's 324 values depend on
 * its own features and coordinates only: unchanged bitwise when its neighbours' coordinates change, image (b, t) of a batch bitwise
 * the call on that pair alone, placed runs bitwise the contiguous one, out alone / out_koct alone / both bitwise the same. */
int64_t sf_corr_direct_ws_bytes(int B, int pairs, int D, int h, int w, int precision);
int sf_corr_direct_pack(const float* f1, const float* f2, int64_t f_clip_stride, int64_t f_pair_stride,
                        void* ws, int64_t ws_bytes, int B, int pairs, int D, int h, int w, int precision, void* stream);
int sf_corr_direct_lookup(const void* ws, const float* coords, float* out, int64_t out_img_stride,
                          void* out_koct, int64_t out_koct_img_stride, int B, int pairs, int D, int h, int w,
                          int precision, void* stream);

/* ---- generic fused GEMM: every 1x1 conv / nn.Linear / einsum on the path ------------------------
 * C[z][m][n] = epilogue( alpha * ( sum_k A[z][m][k] * B[z][k][n] + bias[m] ) )
 * replaces: nn.Conv2d 1x1 in PCBlock4_Deep_nopool_res (update.py:18-28), convf1 (update.py:323),
 * to_qk/to_v (gma.py:48,82), einsum QK^T (gma.py:60) and attn@v (gma.py:97), timm Linear layers
 * (update.py:466-479), mask head (update.py:756-759; 3x3 conv as implicit GEMM). */
enum { SF_LAYOUT_K_MAJOR = 0,   /* A[k*lda + m]   /  B[k*ldb + n]   (rows of k)            */
       SF_LAYOUT_K_MINOR = 1,   /* A[m*lda + k]   /  B[n*ldb + k]   (k contiguous)          */
       SF_LAYOUT_SPLIT_F16 = 2,/* A only, split precisions: weights pre-split on the host into two IEEE fp16
                                    images A_hi/A_lo laid out in k-octet planes [K padded to 32 / 8][lda_h][8] with
                                    lda_h = M padded to 128 (zero padded): element (m,k) at ((k/8)*lda_h + m)*8 + k%8,
                                    w = hi + lo to ~22 bits.  16 bytes = one MFMA operand k-octet of one row, so a
                                    tile is moved to LDS by buffer_load ... lds without passing through registers */
       SF_LAYOUT_F16_K_MINOR = 3,  /* B only, split precisions: B points to IEEE fp16 values B[n*ldb + k]
                                    (ldb, strideB in halfs; ldb % 2 == 0); used as they are, no lo part:
                                    a*b = ah*b + al*b.  The stored attention matrix (sf_softmax_rows).   */
       SF_LAYOUT_F16_KOCT = 5,   /* B only, F16X2 / F16 with a SPLIT_F16 A.  The tiled kernels take it on the 128-row tile only, i.e. where
                                    M padded to 128 stays within 1.25 M (103 .. 128, 205 .. 256, 308 .. 384, 410 and up); every other M
                                    (96 and 192 among them) runs activation-stationary (64 < K <= 640) or is refused: IEEE fp16 in k-octet
                                    planes, element (k, n) at ((k/8)*ldb + n)*8 + k%8 (ldb = pixels per plane, strideB in
                                    halves; 16-byte aligned) -- what a producing sf_gemm stores with c_f16 = 2.  16 bytes =
                                    one MFMA operand octet of one pixel: the consumer moves its B tiles HBM/L2 -> LDS with
                                    buffer_load ... lds like the weights (no registers, no conversion, no ds_write).
                                    Octets past ceil(K/8) read as zero; rows K..8*ceil(K/8)-1 must be finite.          */
       /* (layout value 6 and c_f16 = 4 are retired since SF_VERSION 129: refused with SF_ERR_BAD_ARG, not to be reused) */
       SF_LAYOUT_F16_K_MAJOR = 4 };/* B only, SF_PRECISION_F16X2 with a SPLIT_F16 A: IEEE fp16 rows B[k*ldb + n]
                                    (ldb, strideB in halfs; N, ldb, strideB even) -- what a producing sf_gemm stores
                                    with c_f16 = 1.  Bit-identical to handing the fp32 values over (F16X2 rounds a
                                    B operand to fp16 on load), at half the bytes.                          */
enum { SF_PRECISION_FP32 = 0,   /* exact fp32: v_mfma_f32_32x32x2_f32, k-ordered fmaf chain          */
       SF_PRECISION_F16X3 = 1,  /* split precision: x = hi+lo (fp16 each); a*b = ah*bh + ah*bl + al*bh
                                    on v_mfma_f32_32x32x16_f16 with fp32 accumulation (~2^-22 relative)  */
       SF_PRECISION_F16X2 = 2,  /* A (weights) split hi+lo, B (activations) rounded once to fp16:
                                    a*b = ah*b + al*b, 2 MFMAs; error = the fp16 rounding of B (2^-11 rel.) */
       SF_PRECISION_F16 = 3 };  /* both operands rounded once to fp16, ONE f16 MFMA per product, fp32 accumulation: the
                                    arithmetic class of the reference's own deployment (fp16 autocast, demo.py:427-456).
                                    sf_corr_build_pyramid / sf_corr_lookup: every pyramid cell is also STORED as fp16
                                    (the "bf16/fp16 volume" configurations of BASELINE.json).  sf_gemm: needs SPLIT_F16
                                    weights (their hi image is the round-to-nearest fp16 of the scaled weight); an fp32
                                    A operand is treated as in F16X2 */
enum { SF_EPI_NONE = 0,         /* C = v                              v = alpha*(acc+bias)   */
       SF_EPI_GELU = 1,         /* C = gelu(v)                        exact erf GELU         */
       SF_EPI_RELU = 2,         /* C = max(v,0)                                              */
       SF_EPI_RES = 3,          /* C = R + v                                                 */
       SF_EPI_RES_GELU = 4,     /* C = gelu(R + v)                                           */
       SF_EPI_RES_GELU_DW1 = 5, /* t = gelu(R + v); C = gelu(t + dw_w[m]*t + dw_b[m])        */
       SF_EPI_AXPY = 6 };       /* C = R + gamma[0]*v     (gma.py:102)                       */

typedef struct SfGemm {
    const float* A; const float* B; float* C;
    const float* bias;            /* [M] or NULL */
    const float* R;               /* residual (same row/col addressing as C, own strides) or NULL */
    const float* dw_w; const float* dw_b;   /* [M] each, for SF_EPI_RES_GELU_DW1 */
    const float* gamma;           /* device scalar for SF_EPI_AXPY */
    int32_t M, N, K, batch;
    int64_t lda, ldb, ldc, ldr;
    int64_t strideA, strideB, strideC, strideR;   /* per batch index z (floats) */
    int32_t a_layout, b_layout;
    /* grouped rows (K_MAJOR B, and R): row k lives at (k / group)*group_stride + (k % group)*ld.
       group = 0 means "no grouping".  Used to read '(B T) C H W -> B (T C) H W' views in place. */
    int32_t b_group; int64_t b_group_stride;
    int32_t r_group; int64_t r_group_stride;
    /* implicit 3x3 conv (pad 1) on a K_MAJOR B: K = 9*Cin, k = tap*Cin + c, tap = ky*3+kx; needs h*w == N */
    int32_t conv3x3, h, w;
    float alpha;
    int32_t epilogue;
    int32_t precision;            /* SF_PRECISION_* */
    const void* A_hi; const void* A_lo;   /* SF_LAYOUT_SPLIT_F16 operand (shared by all batch indices) */
    int64_t lda_h;                /* rows per k-octet plane of A_hi/A_lo (M padded to 128) */
    int32_t a_padded;             /* K_MAJOR fp32 A is zero padded to [K up to 32][M up to 128]: no bounds checks */
    /* split-K (the split precisions F16X3 / F16X2 / F16; refused in FP32): the K range is cut into k_splits <= 16 slices of
       whole k-tiles, slice s writes its partial product (epilogue must be SF_EPI_NONE, no bias) to C + s*split_stride;
       combine with sf_splitk_combine. */
    int32_t k_splits; int64_t split_stride;
    /* optional scratch (caller-owned).  If given (>= auto_split_max * batch * M * N floats... see sf_gemm_split_ws_floats)
       and k_splits == 0, the library may split K on its own for small grids with deep K (split precisions only; FP32 ignores
       the scratch, and so do conv3x3, c_f16, r_f16 and problems the activation-stationary kernel takes): partial products
       go to the scratch and a second kernel applies bias / epilogue.  Results are deterministic. */
    float* split_ws; int64_t split_ws_floats;
    /* c_f16 = 1 (split precisions, 16-byte-aligned C, N % 4 == 0, ldc % 4 == 0): C points to IEEE fp16 storage, results are
       rounded to nearest and stored as halves (ldc, strideC in halves): the K-major fp16 operand of the next sf_gemm.
       c_f16 = 2: the same values in k-octet planes (SF_LAYOUT_F16_KOCT; ldc = pixels per plane, strideC in halves,
       8*ceil(M/8) rows are written: the caller provides room for them).
       c_f16 = 3: C is written in fp32 as usual AND a second time as fp16 k-octet planes at C16 (ldc pixels per plane,
       strideC16 halves between images; same alignment rules as c_f16 = 1 for C and c_f16 = 2 for C16; every epilogue).
       Only rows < M are written to C16: a last, partial octet keeps its other rows. */
    int32_t c_f16;
    void* C16; int64_t strideC16;
    /* r_f16 = 2 (split precisions): the residual R is not fp32 planes but an fp16 k-octet image (SF_LAYOUT_F16_KOCT: element
       (m, n) at ((m/8)*ldr + n)*8 + m%8, ldr = pixels per plane >= N, strideR in halves and % 8 == 0, 16-byte aligned, no
       grouping) -- e.g. the tensor that was this block's GEMM operand, read a second time as the residual without an fp32
       copy of it ever having been written (correlation features).  The tiled kernels take it with SF_EPI_RES_GELU_DW1 and
       the vector epilogue only (the alignment rules of c_f16 = 1 for C; c_f16 != 2); the activation-stationary kernel with
       every residual epilogue (RES, RES_GELU, RES_GELU_DW1, AXPY), every output format and no alignment rule for C, at
       K <= 512. */
    int32_t r_f16;
    /* SPLIT_F16 weights: the k extent the A_hi / A_lo planes are zero-padded to is K rounded up to a multiple of a_k_pad
       (0 or 32: the minimum the tiled kernels need; 128: what the activation-stationary kernel needs -- streamflow_amd
       packs 128).  Any other multiple of 32 promises at least the minimum and is taken as such; a value that is negative or
       no multiple of 32 is refused (SF_ERR_BAD_ARG).  Nothing past [K so padded][lda_h] is read, and of the lda_h rows of a
       plane only the first M padded to 128 (lda_h may be larger, a multiple of 128). */
    int32_t a_k_pad;
    /* kernel family: SF_ALGO_AUTO picks per problem; the other two force one (tests, A/B timing) and fail when it cannot run */
    int32_t algo;
} SfGemm;
enum { SF_ALGO_AUTO = 0,
       SF_ALGO_TILED = 1,     /* 128 x 128 / 128 x 256 output tiles, operands staged per k-tile (csrc/gemm_split.hip) */
       SF_ALGO_BSTAT = 2 };   /* activation-stationary: a wave keeps the K values of its 32 pixels in registers and the weights
                                 stream past them through LDS (csrc/gemm_bstat.hip): F16X2 / F16, SPLIT_F16 weights with
                                 a_k_pad = 128, 64 < K <= 640 (with an fp32 residual K <= 384, with a k-octet one K <= 512), B as
                                 fp32 planes / fp16 rows / k-octets, C as fp32 planes and / or k-octets (c_f16 0, 2, 3), no
                                 implicit 3x3.  It loads fp16 rows (SF_LAYOUT_F16_K_MAJOR) half by half: N, ldb and strideB may be
                                 odd and B needs 2-byte alignment only -- the tiled kernels refuse those (even N / ldb / strideB,
                                 4-byte aligned B) */

/* floats of scratch that let sf_gemm auto-split a problem of this size (0 if it never would) */
int64_t sf_gemm_split_ws_floats(int M, int N, int K, int batch);

/* Established for SPLIT_F16 weights by tests/test_gpu_gemm_packed.py (every kernel family, one to three products, against float64;
 * the case lists and the dispatch rules they cover: tests/gemm_packed_cases.py, held against sf_gemm_route on the CPU):
 *   placement: ldb > N, ldc > N, ldr > N, gaps between images and between row groups, and bases off the allocation's start hold
 *       for fp32 planes, fp16 rows and the k-octet forms of B, C (c_f16 = 2), C16 and R (r_f16 = 2) alike.  Only [z][m < M][n < N]
 *       is written -- c_f16 = 2 also writes the rows up to the end of the last octet (finite values), c_f16 = 3 leaves them alone
 *       -- and no operand is.  Dense, pitched and (where the format allows less than 16 bytes) unaligned placements of one
 *       problem give bitwise the same result, vector and scalar epilogue included; five runs are bitwise equal.
 *   the B-direct kernel takes a k-octet B where ceil(N / 256) * ceil(M / 128) * batch >= 384 and M >= 205 (see SF_LAYOUT_F16_KOCT
 *       for the M it has a tile for) or M in 103 .. 128 with K <= 192; below that the 128 x 128 DMA tile runs the same problem.
 *   activation-stationary: any N >= 1 (a wave owns its pixels' whole K: pixels [0, n) of a run at N > n are bitwise the run at
 *       n), any M <= 1024, odd N / ldb / strideB for fp32 planes and fp16 rows. */
int sf_gemm(const SfGemm* g, void* stream);

/* Which kernel sf_gemm would launch for this descriptor, without launching anything (no GPU needed, pointers are looked at for
 * their alignment only).  It runs sf_gemm's own validation and dispatch code -- every launch site reports its identity instead of
 * launching -- so a refused descriptor gets the same return code and sf_last_error() text as from sf_gemm, and `out` is then
 * left alone. */
enum { SF_GEMM_FAMILY_FP32_TILED = 1,   /* csrc/gemm.hip: exact fp32 tiles                                                   */
       SF_GEMM_FAMILY_SPLIT_TILED = 2,  /* csrc/gemm_split.hip: operands staged through registers; told apart by (a_layout,
                                           b_layout): fp32 / SPLIT_F16 A x fp32 / fp16-rows / stored-fp16 K-minor B          */
       SF_GEMM_FAMILY_KOCT_DMA = 3,     /* SPLIT_F16 A x k-octet B, both by LDS-DMA, 128 x 128 tile                          */
       SF_GEMM_FAMILY_BDIRECT = 4,      /* SPLIT_F16 A x k-octet B, 128 x 256 tile, B straight into registers                */
       SF_GEMM_FAMILY_BSTAT = 5,        /* csrc/gemm_bstat.hip: activation-stationary, general epilogue                      */
       SF_GEMM_FAMILY_BSTAT_GELU = 6 }; /* activation-stationary, software-pipelined GELU -> k-octets                        */
typedef struct SfGemmRoute {
    int32_t family;               /* SF_GEMM_FAMILY_* */
    int32_t a_layout, b_layout;   /* of the descriptor */
    int32_t tile_rows;            /* rows of the workgroup tile: 32 / 64 / 128; 0 for the activation-stationary kernels */
    int32_t products;             /* MFMA products per element: 1 / 2 / 3 (1 for exact fp32) */
    int32_t nks, res;             /* activation-stationary: k-steps of 16 the instantiation holds (8 / 16 / 24 / 32 / 40) and its
                                     residual form (0 none, 1 fp32 planes, 2 k-octets; 0 for the pipelined-GELU kernel) */
    int32_t msplit, n_main;       /* activation-stationary: row ranges per pixel tile (1 .. 4) and the pixel tiles that run whole */
    int32_t k_splits;             /* slices when the library splits K on its own through split_ws (the second, epilogue kernel is
                                     implied), else 0 */
} SfGemmRoute;
int sf_gemm_route(const SfGemm* g, SfGemmRoute* out);

/* out[i] = R[i] + gamma[0] * sum_s partial[s*split_stride + i]  for n_img images of rows*P floats each
 * (image strides in floats): the AXPY epilogue of gma.py:102 applied after a split-K attn @ v. */
int sf_splitk_combine(const float* partial, int64_t split_stride, int k_splits, int64_t part_img_stride,
                      const float* R, int64_t r_img_stride, const float* gamma, float* out,
                      int64_t out_img_stride, int n_img, int64_t floats_per_img, void* stream);

/* ---- a6' + a7 fused: GMA aggregation without the N x N matrix (demo.py:235-258; == gma.py:53-65 + 91-104) ----------
 * out[img][d][p] = mf[img][d][p] + gamma[0] * sum_j softmax_j(scale * <q_p, k_j>) * v[img][d][j]     (heads = 1, dim 128)
 * The reference's demo recomputes softmax(q k^T) v in every refinement iteration (flash_attn_func or a naive einsum)
 * instead of keeping the attention matrix; this is that path: online softmax, logits never leave the CU.
 *   sf_gma_flash_pack_qk: once per clip.  qk [n_img][256][P] fp32 (rows 0..127 = q, 128..255 = k: the to_qk output,
 *       gma.py:57) -> fp16 (hi, lo) operand images in `ws` (q pre-scaled by scale * log2 e).  stats_qk_products = 1 / 2 / 3
 *       additionally runs the logits once (with that many products) and stores every query's softmax statistics (row
 *       maximum, 1 / row sum) in `ws`: q and k do not change over the refinement loop, so the per-iteration kernel can
 *       skip its running maximum, accumulator rescale and row sum (use_stats below; -21 % per iteration).  0 = none.
 *   sf_gma_flash_aggregate: every iteration.  v [n_img][128][P] (to_v output), mf and out [n_img][128][P] planes with
 *       image strides in floats; packs v into `ws`, then one fused kernel.  qk_products = MFMA products per logit:
 *       3 = split precision (q_hi k_hi + q_lo k_hi + q_hi k_lo, fp32-class logits), 2 = k rounded to fp16,
 *       1 = q and k rounded to fp16 (the arithmetic of the reference's fp16 flash-attn path).  Softmax weights and v
 *       enter the second contraction as fp16 (like the materialised matrix of sf_softmax_rows), accumulation is fp32.
 *       use_stats = 1: use the statistics stored by pack_qk, which must have been called with stats_qk_products ==
 *       qk_products (same logits); 0: self-contained online softmax.
 *       out_koct (optional): `out` a second time, rounded to fp16, as k-octet planes [16][P][8] per image
 *       (SF_LAYOUT_F16_KOCT, image stride in halves) -- the operand format of the GEMM that reads it next.
 * ws: caller-owned scratch of sf_gma_flash_ws_bytes(n_img, P) bytes, 16-byte aligned; must persist from pack_qk to the
 * last aggregate of the clip.
 * Established by tests/test_gpu_attn_kernels.py (P = 1 .. 641, image strides beyond dense, bases off the allocation):
 *   sf_gma_flash_ws_bytes: exactly that many bytes suffice for every call below (nothing is read or written past them).
 *   sf_gma_flash_pack_qk: writes `ws` only; every call (re)writes the header that names P and stats_qk_products.
 *   sf_gma_flash_aggregate: use_stats = 1 with statistics of another product count, of another P (same rounded-up size), or of
 *       stats_qk_products = 0 gives NaN in EVERY element of out and out_koct, never a silent result; image z of a batch is bitwise
 *       the call on image z alone (n_img on the same side of the key-range split); the pipelined and the plain kernel agree
 *       bitwise; out_koct is bitwise fp16(out); gamma = 0 returns mf exactly; a NaN in mf or in one query stays at that pixel.
 *   sf_gma_flash_aggregate_f16v: bitwise sf_gma_flash_aggregate on fp32 planes whose rounding to fp16 gives those rows.
 *   sf_gma_flash_project_v: for operands whose products and sums are exact in fp32, bitwise the aggregate of those v planes. */
int64_t sf_gma_flash_ws_bytes(int n_img, int P);
int sf_gma_flash_pack_qk(const float* qk, int64_t qk_img_stride, void* ws, int64_t ws_bytes, int n_img, int P,
                         float scale, int stats_qk_products, void* stream);
int sf_gma_flash_aggregate(void* ws, int64_t ws_bytes, const float* v, int64_t v_img_stride, const float* mf,
                           int64_t mf_img_stride, const float* gamma, float* out, int64_t out_img_stride,
                           void* out_koct, int64_t out_koct_img_stride, int n_img, int P, int qk_products, int use_stats,
                           void* stream);
/* The same with v as fp16 ROWS [n_img][128][P] (v_img_stride in halves: sf_gemm's c_f16 = 1 output of the to_v layer in the
 * config-2 presets): v enters the second contraction as fp16 either way, the to_v GEMM writes and the pack reads half the bytes. */
int sf_gma_flash_aggregate_f16v(void* ws, int64_t ws_bytes, const void* v_f16, int64_t v_img_stride, const float* mf,
                                int64_t mf_img_stride, const float* gamma, float* out, int64_t out_img_stride,
                                void* out_koct, int64_t out_koct_img_stride, int n_img, int P, int qk_products,
                                int use_stats, void* stream);
/* to_v (core/gma.py:93: v = to_v(fmap), 1x1 conv 128 -> 128, no bias) AND the v pack in one launch: v = fp16(alpha * W_v x) written
 * straight into the packed v planes of ws, from operands in the formats they already have -- x_koct: the k-octet fp16 copy of the
 * motion features [16][ldx][8] per image (SF_LAYOUT_F16_KOCT; x_koct_img_stride in halves, ldx = pixels per octet row >= P);
 * w_hi / w_lo: the split weight planes [128 / 8][lda_h = 128][8] of sf_gemm's SF_LAYOUT_SPLIT_F16 (products = 1: w_hi alone,
 * 2: w_hi + w_lo); alpha: 1 / the weights' power-of-two pre-scale.  A following sf_gma_flash_aggregate* call takes v == NULL
 * ("the v planes of ws are current").  The activation enters as fp16 (the config-2 arithmetic class). */
int sf_gma_flash_project_v(void* ws, int64_t ws_bytes, const void* x_koct, int64_t x_koct_img_stride, int64_t ldx,
                           const void* w_hi, const void* w_lo, int lda_h, float alpha, int products, int n_img, int P,
                           void* stream);

/* ---- a6 + a7 with the attention weights KEPT (core/gma.py:53-65 computes `attn` once per clip, gma.py:99-102 multiplies it every
 * iteration): the fused path above recomputes softmax(q k^T) in every iteration; q and k do not change over the refinement loop, so
 * the weights can be stored once -- as fp16, unnormalised (exp2 of the logit minus the stored row maximum: bit for bit what the fused
 * kernel multiplies), in the register image of the second contraction's B operand ([key tile of 64][query tile of 32][4] x 1 KB per
 * image, an opaque format between the two calls below) -- and every iteration only streams them past v:
 * half the matrix-core work, no exponentials, HBM-bound (n_img * Ppad^2 * 2 bytes per iteration, Ppad = P rounded up to 128).
 *   sf_gma_stored_p_bytes: size of `pbuf` (caller-owned, 16-byte aligned, persists over the clip's iterations).
 *   sf_gma_stored_image_ok: 1 when an image of P pixels can be stored at all, 0 otherwise: sf_gma_flash_store_p and
 *       sf_gma_stored_aggregate refuse an image whose stored weights (Ppad^2 * 2 bytes plus the read-ahead) reach 4 GiB or whose
 *       packed planes reach 1 GiB, whatever n_img is.  A caller sizes with both: the total with _p_bytes, each image with this.
 *   sf_gma_flash_store_p: once per clip, after sf_gma_flash_pack_qk(stats_qk_products = qk_products): writes pbuf.
 *   sf_gma_stored_aggregate: every iteration; out = mf + gamma / rowsum * v P^T.  v as in sf_gma_flash_aggregate (v_f16 = 1: fp16
 *       rows; v == NULL: the v planes of ws are current, sf_gma_flash_project_v).  With the same ws the result is bit-identical to
 *       sf_gma_flash_aggregate(use_stats = 1).  Weights stored by another pack call / product count poison the result (NaN).
 *   Established by tests/test_gpu_attn_kernels.py: sf_gma_stored_p_bytes bytes suffice exactly; sf_gma_flash_store_p writes pbuf and the
 *   header of ws only; sf_gma_stored_aggregate without a store_p behind the last pack_qk, after a pack_qk for another P or with
 *   stats_qk_products = 0, gives NaN in every element of out and out_koct -- split and unsplit key range alike. */
int64_t sf_gma_stored_p_bytes(int n_img, int P);
int sf_gma_stored_image_ok(int P);
int sf_gma_flash_store_p(void* ws, int64_t ws_bytes, void* pbuf, int64_t pbuf_bytes, int n_img, int P, int qk_products,
                         void* stream);
int sf_gma_stored_aggregate(void* ws, int64_t ws_bytes, const void* pbuf, int64_t pbuf_bytes, const void* v, int v_f16,
                            int64_t v_img_stride, const float* mf, int64_t mf_img_stride, const float* gamma, float* out,
                            int64_t out_img_stride, void* out_koct, int64_t out_koct_img_stride, int n_img, int P, void* stream);

/* ---- a8: one FFN pair of an SK block in ONE launch (core/update.py:14-16, 30-36; csrc/ffn_pair.hip) ---------------------------
 * y = W2 gelu(W1 x + b1) + b2 with the 1.5 C hidden tensor kept in registers (the two-launch form writes and re-reads it).
 * X: the input as fp16 k-octet planes [K1/8][ldx][8] per image (SF_LAYOUT_F16_KOCT; strideX in halves), N pixels, `batch` images.
 * wstream: both layers' weights as ONE stream of 1-KB MFMA fragments in consumption order, built by the host
 *   (streamflow_amd.ops.PackedPair): per 32 hidden rows  2 * ceil(K1/32) * pm1 fragments of W1 (16 rows x 32 k each: lane
 *   (row, kq) = 8 halves W1[row][32 s + 8 kq ..]; with pm = 2 the `lo` fragment precedes the `hi` one), then ceil(M2/16) * pm2
 *   fragments of W2 whose 32 columns are ordered  k = 8 kq + i <-> hidden row 4 kq + i (i < 4) | 16 + 4 kq + i - 4 (i >= 4),
 *   zero-padded to sf_ffn_pair_frags(K1, M2, pm1, pm2) fragments.  Weights pre-scaled by a power of two per layer (alpha1 / alpha2
 *   undo it; bias1 / bias2 carry the same scale), rows / columns beyond H, K1, M2 zero.
 * mode 0 (an ffn2 pair): out = y, or gelu(y) with gelu_out, to C (fp32 planes [M2][ldc], optional) and / or C16 (fp16 k-octet
 *   planes [M2/8][ldc16][8], optional; c16_partial: rows >= M2 of the last octet are not written).
 * mode 1 (an ffn1 pair, M2 == K1): x1 = gelu(x + y); x2 = gelu(x1 + dw_w * x1 + dw_b)  (update.py:31-32: residual, then the
 *   depthwise 1x1 layer of conv_list); C16 = x2 as fp16 ROWS [M2][ldc16].  The residual is the fp16 operand itself.
 * Shapes built: the SK blocks of the update block (C = 128 / 256 / 324) and the flow head (384 / 256 / 128 -> 2 (T - 1) rows); see the
 * dispatch table in csrc/ffn_pair.hip.
 * N: any pixel count > 0 -- no multiple of the tile (64 or 128 pixels) or of 4 is required: a lane past N neither loads nor stores.
 * Every ld* >= N; columns [N, ld), the gaps between images and groups and the rows >= K1 of X's last octet are never part of a
 * result (the latter must be finite) and nothing outside [image][row < M2][pixel < N] is written, except the rows >= M2 of C16's
 * last octet when c16_partial = 0 (they receive 0). */
typedef struct SfFfnPair {
    const void* X; int64_t strideX; int64_t ldx;
    const void* wstream; int64_t wstream_bytes;
    const float* bias1; const float* bias2; const float* dw_w; const float* dw_b;
    float* C; int64_t strideC; int64_t ldc;
    void* C16; int64_t strideC16; int64_t ldc16;
    int32_t N, batch, K1, H, M2, pm1, pm2, mode, gelu_out, c16_partial;
    float alpha1, alpha2;
    int32_t x_group; int64_t x_group_stride;   /* x_group > 0: X's K1 rows are x_group-row slices (a multiple of 32 that divides K1) of
                                                  consecutive groups x_group_stride halves apart -- the flow head's '(B T) C -> B (T C)'
                                                  view of the hidden state (update.py:775) without a copy; 0: plain planes */
    const float* R32; int64_t strideR32, ldr32, r32_group_stride;   /* mode 1, optional: the residual x from fp32 planes [M2][ldr32]
                                                  (grouped like X: groups r32_group_stride floats apart) instead of the fp16 operand */
} SfFfnPair;
int sf_ffn_pair(const SfFfnPair* p, void* stream);
int sf_ffn_pair_frags(int K1, int M2, int pm1, int pm2);

/* ---- a8, back half: pw -> GELU -> ffn2.0 -> GELU -> ffn2.2 of an SK block in ONE launch (core/update.py:35-36 with ffn2 of
 * update.py:14-16; csrc/sk_tail.hip) ------------------------------------------------------------------------------------------
 * y = W3 gelu(W2 gelu(W1' x3 + b1) + b2) + b3,  W1' = pw + I (the residual of `x + pw(x)` folded into the weights).  x4 and the
 * 1.5 C hidden stay in registers (the three-launch form writes and re-reads both).
 * X: x3 as fp16 ROWS [C][ldx] per image (what sf_dwconv_res_gelu_f16in writes; strideX in halves), N pixels, `batch` images.
 * wstream: ONE stream of 1-KB fragments (32 rows x 16 k: lane (row m, k-half) = 8 halves W[32 t + m][k(8 khalf + i)]; pm = 2:
 *   the `lo` fragment precedes the `hi` one) in consumption order (streamflow_amd.ops.PackedTail):
 *     for t = 0 .. C/32 - 1: W1' row tile t, k-steps 0 .. C/16 - 1 (natural column order), zero-padded to a multiple of 16 fragments;
 *     for th = 0 .. H/32 - 1: W2 row tile th, k-steps 0 .. C/16 - 1; then for s = 0, 1: W3 row tiles 0 .. ceil(M2/32) - 1 at the
 *       k-step (th, s) of the hidden rows; zero-padded to a multiple of 16 fragments;
 *   the columns of a k-step (t, s) of W2 and W3 are ordered  k = 8 khalf + i <-> input row 32 t + 16 s + (i & 3) + 8 (i >> 2) + 4 khalf
 *   (the accumulator layout of the producing tile).  sf_sk_tail_frags(C, H, M2, pm) fragments in all (0: shape not built).
 *   Weights pre-scaled by a power of two per layer (alpha* = 1 / scale, bias* carry the scale).
 * Y (fp32 planes [M2][ldy], optional) and / or Y16 (fp16 k-octet planes, optional; y16_partial = 1: rows >= M2 of the last octet
 * are left alone).  gelu_out: y = gelu(...).  Built for (C, M2) = (256, 192), (256, 126), (384, 6), (128, 64), H % 32 == 0, H <= 576,
 * pm = 1 / 2; anything else: SF_ERR_BAD_ARG (the caller keeps the three launches).
 * N: any pixel count > 0 (no multiple of the 128-pixel tile or of 4); X needs no alignment beyond its element (2 bytes), ldx / ldy /
 * ldy16 >= N; nothing outside [image][row < M2][pixel < N] is written, except the rows >= M2 of Y16's last octet when y16_partial = 0
 * (they receive 0). */
typedef struct SfSkTail {
    const void* X; int64_t strideX; int64_t ldx;
    const void* wstream; int64_t wstream_bytes;
    const float* bias1; const float* bias2; const float* bias3;
    float* Y; int64_t strideY; int64_t ldy;
    void* Y16; int64_t strideY16; int64_t ldy16;
    int32_t N, batch, C, H, M2, pm, gelu_out, y16_partial;
    float alpha1, alpha2, alpha3;
} SfSkTail;
int sf_sk_tail(const SfSkTail* p, void* stream);
int sf_sk_tail_frags(int C, int H, int M2, int pm);
/* The stream's unit structure (what the host packer needs besides the order above): returns sf_sk_tail_frags(); *stage = fragments per
 * stage (every unit is zero-padded to a multiple of it), *group = hidden tiles th per phase-2 unit, *pw_one_unit = 1 when the C/32 pw row
 * tiles form ONE unit instead of a unit each.  The one layout that ships: *stage = 16, *group = 1, *pw_one_unit = 0, always (the
 * 32-fragment / grouped variant measured 1 % slower on the step and was removed).  Any pointer may be NULL. */
int sf_sk_tail_layout(int C, int H, int M2, int pm, int* stage, int* group, int* pw_one_unit);

/* ---- a10: the temporal transformer block in ONE launch (core/update.py:459-484,502-513 -> timm Block; called at update.py:770;
 * csrc/temporal.hip) ---------------------------------------------------------------------------------------------------------
 * tokens of one pixel = its TT = T - 1 frames x C = 128 channels:  x += proj(softmax(C^-1/2 q k^T) v), (q, k, v) = qkv(LN1 x);
 * x += fc2(gelu(fc1(LN2 x))) -- the unfused form is sf_layernorm_cm, sf_gemm, sf_temporal_attn, sf_gemm, sf_layernorm_cm, sf_gemm,
 * sf_gemm.  Here every intermediate stays in registers (a wave owns 16 pixels x TT frames).
 * X16: the tokens as fp16 k-octet planes [C/8][ldx][8] per image, image = clip * TT + frame (strideX in halves); they are the
 *   operand AND the residual.  B clips of N pixels.
 * wstream: the four layers' weights as ONE stream of 1-KB fragments (16 rows x 32 k: lane (row, kq) = 8 halves W[row][k(8 kq ..)];
 *   with pm = 2 the `lo` fragment precedes the `hi` one) in consumption order (streamflow_amd.ops.PackedTemporal):
 *     q and k rows of qkv: row tile m = 0 .. 15, k-step s = 0 .. 3 (natural column order);
 *     then for p = 0 .. 3: v row tiles 16 + 2 p, 16 + 2 p + 1 (x 4 k-steps), then proj row tiles 0 .. 7 at k-step p;
 *     then for h = 0 .. 7: fc1 row tiles 2 h, 2 h + 1 (x 4 k-steps), then fc2 row tiles 0 .. 7 at k-step h;
 *   the columns of a k-step of proj, fc1 and fc2 are ordered  k = 8 kq + i <-> input row 4 kq + i (i < 4) | 16 + 4 kq + i - 4
 *   (i >= 4) of that k-step's 32 rows (the accumulator layout of the producing tiles).  sf_temporal_block_frags(pm) fragments.
 *   Weights pre-scaled by a power of two per layer: alpha_* = 1 / scale; bias_* carry the scale; ss_proj / ss_fc2 = the scale of
 *   proj / fc2 (the residual enters their accumulators).  qkv has no bias (timm: qkv_bias = False).
 * Y (fp32 planes [C][ldy], optional) and / or Y16 (their fp16 k-octet copy, optional): image stride strideY floats / strideY16 halves.
 * Built for C = 128, H = 256 (mlp_ratio 2), TT = 1 .. 3, pm = 1 / 2; anything else: SF_ERR_UNSUPPORTED (the caller keeps the
 * seven launches).  Arithmetic: activations enter every product as fp16; fp32 accumulation, LayerNorm, softmax and GELU. */
typedef struct SfTemporalBlock {
    const void* X16; int64_t strideX, ldx;
    const void* wstream; int64_t wstream_bytes;
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *bias_proj, *bias_fc1, *bias_fc2;
    float* Y; int64_t strideY, ldy;
    void* Y16; int64_t strideY16, ldy16;
    int32_t N, B, TT, C, H, pm;
    float alpha_qkv, alpha_proj, alpha_fc1, alpha_fc2, ss_proj, ss_fc2, eps, scale;
} SfTemporalBlock;
int sf_temporal_block(const SfTemporalBlock* p, void* stream);
int sf_temporal_block_frags(int pm);

/* ---- f2: mask head, second layer + convex upsampling in ONE launch (core/update.py:756-759,777 + core/models/streamflow.py:82-93;
 * csrc/mask_upsample.hip) ------------------------------------------------------------------------------------------------------
 * out[n][c][8 y + i][8 x + j] = sum_k softmax_k(mask[n][64 k + 8 i + j][y][x]) * 8 flow[n][c][y + k / 3 - 1][x + k % 3 - 1]  (0 outside),
 * mask = alpha * (W x + bias) with W the 576 x 256 weights of mask.2 and alpha = 0.25 / (the weights' power-of-two pre-scale): the
 * unfused form is sf_gemm (mask.2) + sf_upsample_flow, with the 576-channel mask written and read back in between.
 * X16: relu(mask.0(net)) as fp16 k-octet planes [256/8][ldx][8] per image (strideX in halves) -- sf_gemm's c_f16 = 3 copy;
 * wstream: the weights as 1-KB fragments (16 rows x 32 k, lane (row, kq) = 8 halves W[row][32 s + 8 kq ..]; pm = 2: `lo` before `hi`)
 *   in the order row tile 0 .. 35, k-step 0 .. 7 (streamflow_amd.ops.PackedMask): sf_mask_upsample_frags(pm) fragments;
 * bias: 576 floats carrying the pre-scale (or NULL); flow [n][2][h][w] fp32; out [n][2][8h][8w] fp32, 16-byte aligned. */
typedef struct SfMaskUpsample {
    const void* X16; int64_t strideX, ldx;
    const void* wstream; int64_t wstream_bytes;
    const float* bias; const float* flow; float* out;
    int32_t n_img, h, w, K, M, pm;
    float alpha;
} SfMaskUpsample;
int sf_mask_upsample(const SfMaskUpsample* p, void* stream);
int sf_mask_upsample_frags(int pm);

/* ---- row softmax (gma.py:63): x [rows][cols] ----------------------------------------------------
 * out_f16 == NULL: in place.  Otherwise the weights are written as IEEE fp16 to out_f16 [rows][cols] (x is then
 * scratch): the attention matrix is re-read by every refinement iteration's attn @ v and that read is HBM-bound,
 * so the split-precision modes store it in half the bytes (SF_LAYOUT_F16_K_MINOR below). */
int sf_softmax_rows(float* x, int64_t rows, int cols, void* out_f16, void* stream);

/* ---- depthwise KxK conv + bias + residual + GELU  (update.py:33-34 with kernel in {7,15}) -------
 * y = gelu(x + dwconv(x) + b);  plane (img, c) of x is the [h][w] map at x + img*x_img_stride + c*h*w
 * (same for y with y_img_stride); wgt [C][K][K], bias [C].  x and y must not overlap.
 * precision SF_PRECISION_FP32: fp32 FMA stencil on the VALU.  Split precisions: every kernel row is a banded
 * Toeplitz GEMM on the matrix cores with fp32 accumulation.  SF_PRECISION_F16X3: (hi, lo) fp16 halves of both
 * operands, three products.  SF_PRECISION_F16X2: sf_gemm's f16x2 arithmetic -- weights hi + lo, the activation
 * enters the products rounded to fp16 (two products).  SF_PRECISION_F16: the weights are rounded once to fp16 as well (one
 * product; a single-product layer of the mixed preset).  The residual x is exact in the stencil and where x arrives as fp16
 * rows through registers; on the matrix cores it is read back from the staged halves: hi + lo of the truncating split in
 * SF_PRECISION_F16X3 (|x - (hi + lo)| <= 2^-20 |x|, as the correlation builds), hi + lo of the round-to-nearest split in the
 * two- and one-product forms on fp32 input (2^-22 |x|); the DMA form of sf_dwconv_res_gelu_f16in at two products has no
 * separate residual, its centre tap is the split of fp32(w_centre + 1).
 * y_f16 = 1: y receives IEEE fp16 planes of the same [img][c][h][w] order, y_img_stride counted in halves -- the
 * hand-over to a GEMM that reads them as SF_LAYOUT_F16_K_MAJOR (the engine's pw layer in the f16x2 mode, whose
 * residual is folded into its weights so that x3 has no other reader).
 *
 * Established by tests/test_gpu_dwconv_kernels.py (both entry points; tests/dwconv_cases.py restates the dispatch):
 *   Shapes.  ksize 7 or 15, h * w < 2^30.  The stencil (SF_PRECISION_FP32, and SF_PRECISION_F16X3 at ksize 7) takes
 *   w <= 880 (ksize 15) / w <= 1620 (ksize 7) at every h whose strips fit the launch grid: its strip is as tall as 512 threads
 *   allow, shortened until rows plus halo fit 64 KB of LDS, and more than 65535 strips are refused (tested up to h = 1000).
 *   The matrix-core kernel (every other combination) takes w up to 480 (ksize 15) / 704 (ksize 7) at h = 16, at most 65535
 *   strips, and planes whose outputs span at most 2^31 - 1 bytes: it addresses a plane with 32-bit byte offsets.  With fp16
 *   input the plane may also hold at most 2^30 bytes (the offset the DMA form uses for "outside the plane"; the rule is applied
 *   to the register form as well).  Tested with up to 15 images and 640 channels; n_img * C (the stencil's grid) is not checked.
 *   Anything else, a y_f16 other than 0 / 1, a precision outside the enum, null pointers and non-positive sizes are refused
 *   with SF_ERR_BAD_ARG before anything is written.
 *   Placement.  Any 4-byte (fp16: 2-byte) aligned base and any image stride that keeps the images apart.  Alignment only selects
 *   the access width and never the values: 16-byte aligned rows (w % 4 == 0, x_img_stride % 4 == 0) are staged with 16-byte loads
 *   by the matrix-core kernel, 16-byte (fp16: 8-byte) aligned rows of y are stored four at a time by the stencil, and both are
 *   bitwise the element-wise run.  fp16 rows with w % 8 == 0, x_img_stride % 8 == 0 and a 16-byte aligned base take the DMA form
 *   where two staged planes rounded up to 4 KB fit LDS; every such placement is bitwise the dense one.  The DMA form and the
 *   register form differ within 2^-9 max|y| + 2.5e-5 (the fold of the residual into the centre tap).
 *   Batches.  Image z of a batch is bitwise the call on image z alone, for every number of images per workgroup.
 *   Operand range.  The split precisions hold x in fp16 halves: |x| must stay below the fp16 maximum (65504).  A NaN or +inf
 *   at one pixel (y0, x0) of x, or in the two- and one-product forms a finite value beyond that range, changes outputs of that
 *   plane only: in the stencil exactly the K x K footprint, on the matrix cores exactly rows y0 - K/2 .. y0 + K/2 of every
 *   16-column tile whose 32-column window (columns 16 t - 8 .. 16 t + 23) holds x0 -- the window is multiplied by a band with
 *   structural zeros, and 0 * inf = NaN.  (SF_PRECISION_F16X3 keeps 1e5 finite, its split truncates, and changes the footprint
 *   alone.)  NO OUTPUT IS NaN in either kernel: both GELU forms clamp their argument with max / med3, which return the other
 *   operand for a NaN, so a NaN or -inf pre-activation leaves as a number within the form's absolute error of zero, and +inf
 *   as +inf.  A caller that needs to see non-finite input must check x itself.
 *   GELU.  fp16 output of the two- and one-product forms uses the polynomial GELU of csrc/sf_common.h (5.2e-5 absolute up to
 *   a pre-activation of 8, 6.6e-6 of it beyond); everything else the erf form (1.3e-6, 3e-7 of the pre-activation beyond 4). */
int sf_dwconv_res_gelu(const float* x, int64_t x_img_stride, const float* wgt, const float* bias, void* y,
                       int64_t y_img_stride, int y_f16, int n_img, int C, int h, int w, int ksize, int precision,
                       void* stream);
/* The same layer with x ALSO as fp16 rows [img][c][h][w] (both strides in halves): the config-2 hand-over of an SK block's
 * x2 (written by sf_gemm with c_f16 = 1) and x3.  precision SF_PRECISION_F16X2 or SF_PRECISION_F16 only.  The convolution
 * input and the residual are the fp16 value itself (what the two-product arithmetic multiplies anyway; the residual loses
 * the 2^-12 relative rounding of x2, which x3's own fp16 rounding already has).  Rows of whole, 16-byte aligned octets
 * (w % 8 == 0) are staged HBM/L2 -> LDS by DMA, double-buffered over the images of a workgroup; other widths through
 * registers. */
int sf_dwconv_res_gelu_f16in(const void* x_f16, int64_t x_img_stride, const float* wgt, const float* bias, void* y_f16,
                             int64_t y_img_stride, int n_img, int C, int h, int w, int ksize, int precision, void* stream);

/* ---- LayerNorm over channels of channel-major planes (update.py:462-463,481-483) --------------
 * x,y [n_img][C][P] (image strides given in floats), normalises each (img,p) column over C.
 * y_koct (optional, C = 128 / 256): the result as fp16 k-octet planes (SF_LAYOUT_F16_KOCT, image stride in halves) for
 * a consumer that is an sf_gemm; y may then be NULL. */
int sf_layernorm_cm(const float* x, int64_t x_img_stride, const float* gamma, const float* beta,
                    float* y, int64_t y_img_stride, void* y_koct, int64_t y_koct_img_stride, int n_img, int C, int P,
                    float eps, void* stream);

/* ---- per-pixel attention over the T-1 tokens (timm Attention core, update.py:466-474) ----------
 * qkv [B*TT][3*C][P] (rows [q|k|v]) -> out [B*TT][C][P]; softmax(q k^T / sqrt(C)) v over t.
 * out_koct (optional, C % 32 == 0): the result as fp16 k-octet planes [B*TT][C/8][P][8] (SF_LAYOUT_F16_KOCT); out may
 * then be NULL.  C % 4 == 0.  TT = 1..7; a TT outside that range returns SF_ERR_UNSUPPORTED.  TT = 4..7 is what clips of
 * T >= 5 frames run: sf_temporal_block stops at TT = 3.  Both forms (this one and sf_temporal_attn_f16in) are tested over TT = 1..7
 * (tests/test_gpu_glue_kernels.py). */
int sf_temporal_attn(const float* qkv, float* out, void* out_koct, int B, int TT, int C, int P, void* stream);
/* The same with qkv as fp16 ROWS [B*TT][3C][P] (what sf_gemm writes with c_f16 = 1): the config-2 hand-over -- the qkv GEMM
 * writes and this kernel reads half the bytes; scores, softmax and the weighted sum stay fp32. */
int sf_temporal_attn_f16in(const void* qkv_f16, float* out, void* out_koct, int B, int TT, int C, int P, void* stream);

/* ---- fp32 planes -> fp16 k-octet planes (no reference counterpart: an operand format of sf_gemm) -----------------
 * x [n_img][rows][P] fp32 (x_img_stride in floats) -> y [n_img][ceil(rows/8)][P][8] IEEE fp16 (y_img_stride in halves),
 * element (r, p) at ((r / 8) * P + p) * 8 + r % 8; rows past `rows` in a last, partial octet are left untouched (they
 * must be finite: zero-initialise the planes once): SF_LAYOUT_F16_KOCT, the
 * image sf_gemm moves to LDS by DMA.  Used once per clip for the static context features; tensors produced inside
 * the loop get their k-octet copy from the producing kernel (SfGemm.C16). */
int sf_pack_koct(const float* x, int64_t x_img_stride, int n_img, int rows, int P, void* y, int64_t y_img_stride,
                 void* stream);

/* ---- measurement aid (no reference counterpart) -----------------------------------------------------------------
 * One wave that reads the shader-cycle counter and the constant 100 MHz counter for `spin_us` microseconds (sleeping in
 * between) and writes out[0] = shader cycles, out[1] = 100 MHz ticks that passed: launched on a side stream while the hot path
 * replays, it gives the clock the chip SUSTAINS under that load (MI355X clocks to its power budget; bench.py prices the
 * matrix-core roof at 2.4 GHz as the guide prescribes and quotes this clock next to it).  out: two int64 in device memory. */
int sf_clock_probe(int64_t* out, int spin_us, void* stream);

/* ---- context split (streamflow.py:119-122): cnets [n_img][2*hdim][P] ->
 * nets = tanh(first half) (written with nets_img_stride), inps = relu(second half). */
int sf_context_split(const float* cnets, float* nets, int64_t nets_img_stride, float* inps,
                     int64_t inps_img_stride, int n_img, int hdim, int P, void* stream);

/* ---- flow bookkeeping (streamflow.py:133,138) ----------------------------------------------------
 * coords1 += delta (if delta != NULL); flow = coords1 - grid; flow written to up to two places, and (flow_koct != NULL)
 * as fp16 into rows flow_koct_row (x), flow_koct_row + 1 (y) of k-octet planes (SF_LAYOUT_F16_KOCT, image stride in
 * halves): the flow rows of the k-octet copy of the motion features. */
int sf_flow_update(float* coords1, const float* delta, float* flow_a, int64_t flow_a_img_stride,
                   float* flow_b, int64_t flow_b_img_stride, void* flow_koct, int64_t flow_koct_img_stride,
                   int flow_koct_row, int n_img, int h, int w, void* stream);

/* ---- f1: Twins_CSC encoder (core/encoders/twins_csc.py:59-85 over timm's twins_svt_large stages 1-2) -----------------
 * Token planes [n_img][C][N]: N = H*W tokens of the (T*h) x w grid of a clip, channel = head*32 + d (head dim 32).
 * Linear layers / strided convs of the encoder use sf_gemm, LayerNorms sf_layernorm_cm; these three are the rest.
 * sf_window_attn: timm LocallyGroupedAttn core.  qkv [n_img][3C][H*W] (rows q | k | v, the qkv Linear output) ->
 *     out [n_img][C][H*W] = softmax(q k^T / sqrt(32)) v inside non-overlapping ws x ws windows.  Windows reaching past
 *     the grid are completed with zero tokens, whose k and v are qkv_bias (timm pads after the norm, before the Linear).
 * sf_window_attn_mfma: the same on the matrix cores, one wave per (window, head); precision as sf_subsample_attn_mfma.
 * sf_subsample_attn: timm GlobalSubSampleAttn core.  q [n_img][C][N], kv [n_img][2C][M] (rows k | v) -> out [n_img][C][N].
 * sf_subsample_attn_mfma: the same contraction on the matrix cores (flash-style, transposed logits, no N x M tensor):
 *     precision SF_PRECISION_F16X3 = hi + lo fp16 split of q, k, the softmax weights and v (3 products per contraction,
 *     fp32-class), SF_PRECISION_F16X2 / SF_PRECISION_F16 = every operand rounded once to fp16 (1 product); fp32
 *     accumulation, softmax statistics in fp32.  ws: sf_subsample_attn_ws_bytes(n_img, heads, M) bytes, 16-byte aligned
 *     (the packed k / v operand images; scratch, dead when the call's kernels have run).
 *     sf_window_attn_mfma, qkv_koct = 1 (one-product classes only): qkv points to fp16 k-octet planes [3C/8][H*W][8] (the
 *     qkv sf_gemm's c_f16 = 2 output; image stride in halves) instead of fp32 planes.
 *     Both *_mfma cores: out_koct (optional) = the result as fp16 k-octet planes [C/8][N][8] (SF_LAYOUT_F16_KOCT, image
 *     stride in halves): the B operand image of the proj sf_gemm that consumes it; out may then be NULL.
 * sf_dwconv3x3_res: timm PosConv: y = x + depthwise3x3(x) + b on [n_img][C][H][W]; w [C][9].
 * Established by tests/test_gpu_attn_kernels.py (ws 2..7, grids from 1 x 1, N and M on either side of 32 / 64 / 128 / 256):
 *   sf_window_attn: heads must be a multiple of 4 (as for sf_window_attn_mfma), out may not be NULL; writes the H*W tokens of out only.
 *   sf_window_attn_mfma: out alone, out_koct alone and both give bitwise the same values (out_koct = fp16(out));
 *       SF_PRECISION_F16X2 and SF_PRECISION_F16 are bitwise the same; qkv_koct = 1 rounds the bias tokens' k and v to fp16.
 *   sf_subsample_attn_ws_bytes: exactly that many bytes suffice; sf_subsample_attn_mfma writes nothing else outside its outputs.
 *   sf_subsample_attn_mfma: the output requests and the two one-product classes agree bitwise as for sf_window_attn_mfma.
 *   All four: image z of a batch is bitwise the call on image z alone, whatever the image strides. */
int sf_window_attn(const float* qkv, int64_t qkv_img_stride, const float* qkv_bias, float* out, int64_t out_img_stride,
                   int n_img, int C, int heads, int H, int W, int ws, void* stream);
int sf_window_attn_mfma(const void* qkv, int64_t qkv_img_stride, int qkv_koct, const float* qkv_bias, float* out,
                        int64_t out_img_stride, void* out_koct, int64_t out_koct_img_stride, int n_img, int C, int heads,
                        int H, int W, int ws, int precision, void* stream);
int sf_subsample_attn(const float* q, int64_t q_img_stride, const float* kv, int64_t kv_img_stride, float* out,
                      int64_t out_img_stride, int n_img, int C, int heads, int N, int M, void* stream);
int64_t sf_subsample_attn_ws_bytes(int n_img, int heads, int M);
int sf_subsample_attn_mfma(const float* q, int64_t q_img_stride, const float* kv, int64_t kv_img_stride, float* out,
                           int64_t out_img_stride, void* out_koct, int64_t out_koct_img_stride, int n_img, int C, int heads,
                           int N, int M, void* ws, int64_t ws_bytes, int precision, void* stream);
int sf_dwconv3x3_res(const float* x, int64_t x_img_stride, const float* w, const float* b, float* y,
                     int64_t y_img_stride, int n_img, int C, int H, int W, void* stream);

/* ---- K12 convex upsampling (streamflow.py:82-93) -------------------------------------------------
 * flow [n][2][h][w], mask [n][9*64][h][w] -> out [n][2][8h][8w]. */
int sf_upsample_flow(const float* flow, const float* mask, float* out, int n, int h, int w, void* stream);

/* ---- f4: forward_interpolate  (core/utils/utils.py:34-62; warm start, evaluate_mf.py:305,362) ----
 * flow, out [n_img][2][h][w] (ch0 = dx, ch1 = dy).  Each source pixel is pushed along its flow; points landing
 * outside the open rectangle (0, w) x (0, h) are dropped; every grid pixel receives the flow of the nearest
 * remaining point (exact Euclidean nearest neighbour in float64, lowest source index on ties), zero if none is left.
 * Replaces scipy.interpolate.griddata(method='nearest') on the host. */
int sf_forward_interpolate(const float* flow, float* out, int n_img, int h, int w, void* stream);

/* ---- tiled inference: Gaussian-weighted blend of overlapping crops (evaluate_mf.py:985-1053, :919-982) ----------------
 * flows [n_clips * n_distinct][pairs][2][tile_h][tile_w] (the per-crop upsampled flows), weights [tile_h][tile_w] (one crop's
 * Gaussian patch), out [n_clips][pairs][2][out_h][out_w] = the window (out_y0, out_x0) of the img_h x img_w canvas.  Per pixel,
 * over the entries k of the crop sequence (origins tile_y/x[k], distinct crop tile_id[k]; duplicates included) that cover it and
 * in that order: acc = acc + f * w, wsum = wsum + w; out = acc / wsum -- each operation rounded on its own in fp32, subnormals
 * kept (bitwise the reference's F.pad accumulation on the CPU). */
#define SF_TILE_MAX 64
typedef struct SfTilePlan {
    int32_t n_seq, n_distinct;
    int32_t tile_h, tile_w;
    int32_t img_h, img_w;
    int32_t out_y0, out_x0, out_h, out_w;
    int32_t tile_y[SF_TILE_MAX], tile_x[SF_TILE_MAX], tile_id[SF_TILE_MAX];
} SfTilePlan;
int sf_tile_blend(const float* flows, const float* weights, float* out, const SfTilePlan* plan, int n_clips, int pairs,
                  void* stream);

/* ---- flow colour-wheel images (core/utils/flow_viz.py: flow_to_image; demo.py vis_flow, the submission writers) --------
 * flows [n][2][h][w] fp32 (ch0 = u, ch1 = v) -> out [n][h][w][3] uint8 (RGB, or BGR with bgr != 0), the Middlebury wheel of
 * Baker et al. with 55 entries.  Every field is normalised by its OWN maximum radius (written to rad_max_ws[n], which stays
 * readable after the call), or by fixed_rad_max when that is >= 0 (rad_max_ws may then be null and no reduction is launched).
 * At most three kernels on `stream` (the first clears rad_max_ws), no host synchronisation: safe inside graph capture.
 *
 * Per-call clears, here and in every entry point below: whatever an entry point resets per call (accumulators, status and key
 * words, the slots bits are ORed into) it resets with a KERNEL on `stream`, never with hipMemsetAsync: a memset node of a captured
 * graph cleared only a part of its bytes from the second replay on (ROCm 7.0), a kernel node replays as captured.  "Cleared by the
 * call itself" therefore holds eagerly, on any stream, inside a capture and on every replay; tests/test_gpu_media_state.py runs
 * every media entry point in used buffers, on a side stream and as a replayed graph.
 *
 * Arithmetic (the reference's numpy arithmetic for float32 input, except for its libm's float32 arctan2):
 *   fp32, every operation rounded on its own, subnormals kept, correctly rounded division and square root:
 *     [clip_flow >= 0: u, v clamped to [0, clip_flow] first -- np.clip(flow, 0, clip_flow): NEGATIVE components become 0]
 *     rad = sqrt(u u + v v), m = max over the field, d = m + 1e-5f, u' = u / d, v' = v / d, rad' = sqrt(u' u' + v' v')
 *     angle = fp32(atan2(-(double)v', -(double)u'))   (the fp64 arctangent rounded once; the negation keeps the sign of zero:
 *             v = +0, u > 0 gives -pi = wheel entry 0, v = -0 gives +pi = entry 54)
 *     a = angle / (float)pi, fk = (a + 1) / 2 * 54, k0 = floor(fk), k1 = k0 + 1 (55 -> 0)
 *   fp64 (numpy's float32 - int32 is float64): f = fk - k0 (exact), c0 = wheel[k0] / 255, c1 = wheel[k1] / 255,
 *     col = (1 - f) c0 + f c1,
 *     col = rad' <= 1 ? 1 - rad' (1 - col) : col * 0.75   (the second branch is reachable with fixed_rad_max only),
 *     byte = floor(255 col).
 * A pixel with a non-finite component does not enter the maximum and is painted (0, 0, 0) (the reference is undefined there);
 * an all-zero field is white.  Limits: n, h, w > 0, h * w < 2^30, n <= 65535. */
int sf_flow_to_image(const float* flows, uint8_t* out, float* rad_max_ws, int n, int h, int w, float clip_flow,
                     float fixed_rad_max, int bgr, void* stream);

/* ---- Spring scoring (evaluate_mf.py:50-102 validate_spring_mf) -----------------------------------------------------------
 * Scores one predicted field against one ground-truth field and ADDS the result into acc[SF_SCORE_LEN] (fp64, on the device).
 *   pred: fp32 planes [2][h][w]: u at pred[y * pred_row_stride + x], v at the same + pred_ch_stride (a view into a padded output
 *         needs no copy).
 *   gt:   fp32 interleaved [gt_h][gt_w][2] (read_flo5's array); pixel (y, x) is scored against gt[step * y][step * x], step = 1
 *         or 2 (2 = the reference's flow[::2, ::2], mf_datasets.py:189-190); gt_h > step (h - 1), gt_w > step (w - 1).
 *   ws:   scratch of SF_SCORE_WS_BYTES bytes (per-block partials); it is not read by later calls.
 * Per pixel, fp32 with every operation rounded on its own (no contraction; correctly rounded square root):
 *   e = sqrt((pu - gu)(pu - gu) + (pv - gv)(pv - gv)),  valid = !isnan(gu + gv),  mag = sqrt(gu gu + gv gv).
 * Entries (counts are exact in fp64 below 2^53; NaN compares false):
 *   PIXELS         pixels                       SUM_EPE        sum of e (fp64; NaN if any e is NaN)
 *   LT1 / LT3 / LT5  pixels with e < 1 / 3 / 5    GT1            pixels with e > 1
 *   VALID          valid pixels                 SUM_EPE_VALID  sum of e over valid pixels
 *   S0_10, S0_10_GT1     valid & mag < 10,          and of those e > 1
 *   S10_40, S10_40_GT1   valid & 10 <= mag < 40,    and of those e > 1
 *   S40, S40_GT1         valid & mag >= 40,         and of those e > 1
 * Deterministic: per-block partials summed in a fixed order by a second one-block kernel, no atomics; repeated calls give bitwise
 * equal accumulators.  Two kernels on `stream`, no host synchronisation.  Limits: h, w > 0, h * w < 2^30. */
enum {
    SF_SCORE_PIXELS = 0, SF_SCORE_SUM_EPE = 1, SF_SCORE_LT1 = 2, SF_SCORE_LT3 = 3, SF_SCORE_LT5 = 4, SF_SCORE_GT1 = 5,
    SF_SCORE_VALID = 6, SF_SCORE_SUM_EPE_VALID = 7, SF_SCORE_S0_10 = 8, SF_SCORE_S0_10_GT1 = 9, SF_SCORE_S10_40 = 10,
    SF_SCORE_S10_40_GT1 = 11, SF_SCORE_S40 = 12, SF_SCORE_S40_GT1 = 13, SF_SCORE_LEN = 14
};
#define SF_SCORE_WS_BYTES (1024 * SF_SCORE_LEN * 8)
int sf_flow_score(const float* pred, int64_t pred_ch_stride, int64_t pred_row_stride, const float* gt, int gt_h, int gt_w,
                  int step, int h, int w, double* acc, void* ws, int64_t ws_bytes, void* stream);

/* ---- Sintel / KITTI scoring, a batch of fields per call (evaluate_mf.py:106-142, :468-503, :549-592) --------------------------
 * Scores n_fields (1 .. SF_SCORE_BATCH_MAX) predicted fields of one size h x w, field i against its own ground truth, and ADDS
 * the result of field i into row i of acc[n_fields][SF_EVAL_LEN] (fp64, on the device).  `f` is a HOST table that travels in the
 * kernel arguments (entries at and above n_fields are not looked at); nothing is uploaded.
 *   pred[i]: fp32 planes [2][h][w]: u at pred[i][y * pred_row_stride + x], v at the same + pred_ch_stride (strides in floats,
 *            shared by all fields: windows of the model's padded outputs, slices of one tensor).
 *   gt[i]:   the ground truth as its decoder left it, dense:
 *            SF_GT_FLO32    fp32 [h][w][2] = (u, v) (a .flo file); valid = !isnan(gu + gv);
 *            SF_GT_KITTI16  uint16 [h][w][3] = (u, v, valid) samples of a KITTI flow_occ PNG, decoded here:
 *                           gu = ((float)s0 - 32768) / 64, gv likewise (exact in fp32), valid = s2 != 0.
 *   mask[i]: NULL for every field, or for every field uint8 [h][w], the bytes of a Sintel occlusions PNG: a pixel is occluded when
 *            its byte is 255, non-occluded otherwise (the reference's astype(uint8) // 255 as bool).
 *   ws:      scratch of sf_flow_score_batch_ws_bytes(n_fields, h, w) bytes (per-block partials); it is not read by later calls.
 * Per pixel, fp32 with every operation rounded on its own (no contraction; correctly rounded square root and division):
 *   e = sqrt((pu - gu)(pu - gu) + (pv - gv)(pv - gv)),  mag = sqrt(gu gu + gv gv),
 *   outlier = valid && e > 3 && e / mag > 0.05   (IEEE for mag = 0: e / 0 = inf is an outlier, 0 / 0 = NaN is not).
 * Entries of a row (counts are exact in fp64 below 2^53; NaN compares false):
 *   PIXELS         pixels                       SUM_EPE        sum of e (fp64; NaN if any e is NaN)
 *   LT1 / LT3 / LT5  pixels with e < 1 / 3 / 5
 *   VALID          valid pixels                 SUM_EPE_VALID  sum of e over valid pixels          OUTLIER  outlier pixels
 *   OCC            occluded pixels              SUM_EPE_OCC    sum of e over them      (these four stay as they are
 *   NOC            non-occluded pixels          SUM_EPE_NOC    sum of e over them       without masks)
 * Vector loads (16 bytes of a prediction plane, 16 / 8 of fp32 and 8 / 4 of 16-bit ground truth, 4 mask bytes) where pointers,
 * strides and w allow them, element loads otherwise.  Deterministic: per-block partials summed in a fixed order by a second kernel
 * (one block per field), no atomics, a grid that depends on (n_fields, h, w) alone; repeated calls give bitwise equal accumulators.
 * Two kernels on `stream`, no host synchronisation.
 * SF_ERR_BAD_ARG before any launch for: a null f, acc or ws; n_fields outside 1 .. SF_SCORE_BATCH_MAX; an unknown gt_kind;
 * h, w <= 0 or h * w >= 2^30; pred_row_stride < w or pred_ch_stride == 0; ws_bytes too small; acc or ws not 8-byte aligned; a null
 * pred[i] or gt[i]; a pred[i] or gt[i] not aligned to its element size (4; 4 or 2); masks for some fields only.
 * sf_flow_score_batch_ws_bytes returns SF_ERR_BAD_ARG for n_fields, h, w outside the limits above. */
#define SF_SCORE_BATCH_MAX 32
enum { SF_GT_FLO32 = 0, SF_GT_KITTI16 = 1 };
enum {
    SF_EVAL_PIXELS = 0, SF_EVAL_SUM_EPE = 1, SF_EVAL_LT1 = 2, SF_EVAL_LT3 = 3, SF_EVAL_LT5 = 4, SF_EVAL_VALID = 5,
    SF_EVAL_SUM_EPE_VALID = 6, SF_EVAL_OUTLIER = 7, SF_EVAL_OCC = 8, SF_EVAL_SUM_EPE_OCC = 9, SF_EVAL_NOC = 10,
    SF_EVAL_SUM_EPE_NOC = 11, SF_EVAL_LEN = 12
};
typedef struct SfScoreFields {
    const float* pred[SF_SCORE_BATCH_MAX];
    const void* gt[SF_SCORE_BATCH_MAX];
    const uint8_t* mask[SF_SCORE_BATCH_MAX];
} SfScoreFields;
int64_t sf_flow_score_batch_ws_bytes(int n_fields, int h, int w);
int sf_flow_score_batch(const SfScoreFields* f, int n_fields, int64_t pred_ch_stride, int64_t pred_row_stride, int gt_kind, int h,
                        int w, double* acc, void* ws, int64_t ws_bytes, void* stream);

/* ---- video clips: uint8 frames -> clip batches, per-pair outputs -> flows in video order (demo.py:502-534) ---------------------
 * The clip schedule of the reference's read_video_and_group_predict, in closed form (streamflow_amd.demo.group_clips states the
 * same thing as a list): a video of n frames in clips of T has nc = ceil((n - 1) / (T - 1)) clips; clip c starts at frame
 * s(c) = min(c (T - 1), n - T); pair j (frames j -> j + 1, 0 <= j < n - 1) belongs to clip c(j) = min(j / (T - 1), nc - 1) and is
 * that clip's slot j - s(c(j)).  Only the last clip can overlap its predecessor; the slots it repeats belong to the earlier clip.
 * Both entry points compute the schedule in the kernel: no table is uploaded, one launch each, no host synchronisation.
 *
 * sf_frames_to_clips: `frames` holds the frames frame0 .. frame0 + n_buf - 1 of the video as uint8, byte (f, y, x, ch) at
 *   frames + (f - frame0) frame_stride + y row_stride + x px_stride + ch ch_stride (strides in bytes, >= 0: HWC is (3 H W, 3 W, 3, 1),
 *   CHW is (3 H W, W, 1, H W), views of larger buffers are fine).  For the clips first_clip .. first_clip + n_clips - 1:
 *     out[c'][t][ch][y][x] = lut[ frame s(first_clip + c') + t at (clamp(y - pad_top, 0, H - 1), clamp(x - pad_left, 0, W - 1), ch) ]
 *   out fp32 [n_clips][T][3][Hp][Wp], 16-byte aligned; lut: DEVICE table of 256 floats (the normalisation, built by the caller with
 *   the model's own expression, so the kernel does no arithmetic on pixel values).  SF_ERR_BAD_ARG before any launch for: null
 *   pointers, T < 2, n < T, clips outside 0 .. nc - 1, a clip whose frames fall outside the buffer, Hp / Wp not multiples of 8 or
 *   smaller than the frame plus pad, negative strides, n_clips T > 65535, Hp Wp >= 2^30, a misaligned out.
 *
 * sf_clips_to_flows: pairs->p[k] is the model's output for slot k of every clip of the batch, [n_clips][2][Hp][Wp] addressed as
 *   p[k] + c' clip_stride + ch ch_stride + y row_stride + x (strides in floats; all slots share them).  For the pairs
 *   pair0 .. pair0 + n_pairs - 1 of the video:  out[j - pair0][ch][y][x] = p[j - s(c(j))][c(j) - first_clip][ch][y + pad_top][x + pad_left]
 *   out fp32 [n_pairs][2][H][W] contiguous.  float4 accesses where strides, pad_left, W and the pointers allow, scalar otherwise.
 *   SF_ERR_UNSUPPORTED for T - 1 > SF_VIDEO_MAX_PAIRS; SF_ERR_BAD_ARG for null pointers (pairs->p[0 .. T - 2] included), T < 2,
 *   n < T, pairs outside 0 .. n - 2, a pair whose clip is outside first_clip .. first_clip + n_clips - 1, row_stride < W + pad_left,
 *   n_pairs > 32767. */
#define SF_VIDEO_MAX_PAIRS 8
typedef struct SfPairPtrs {
    const float* p[SF_VIDEO_MAX_PAIRS];
} SfPairPtrs;
int sf_frames_to_clips(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, int64_t px_stride, int64_t ch_stride,
                       int frame0, int n_buf, int n, int T, int first_clip, int n_clips, int H, int W, int pad_top, int pad_left,
                       int Hp, int Wp, const float* lut, float* out, void* stream);
int sf_clips_to_flows(const SfPairPtrs* pairs, int64_t clip_stride, int64_t ch_stride, int64_t row_stride, int n, int T,
                      int first_clip, int n_clips, int pair0, int n_pairs, int H, int W, int pad_top, int pad_left, float* out,
                      void* stream);

/* ---- forward-backward consistency: occlusion classes and backward warping, a batch of fields per call -------------------------
 * The consistency check of Sundaram et al. 2010 with the constants' roles as in UnFlow (Meister et al. 2018).  Both entry points
 * share one coordinate rule.  For pixel (y, x) of field i with flow (u, v), fp32, every operation rounded on its own:
 *     px = (float)x + u,  py = (float)y + v,
 *     inside = px >= 0 && px <= (float)(w - 1) && py >= 0 && py <= (float)(h - 1)        (false for NaN; made BEFORE any conversion
 *              to an integer, so NaN, +-Inf and huge flows never form an address),
 *     x0 = floorf(px), fx = px - x0, x1 = min(x0 + 1, w - 1), likewise y0, fy, y1,
 *     sample(A) = (1 - fy) * ((1 - fx) * A[y0][x0] + fx * A[y0][x1]) + fy * ((1 - fx) * A[y1][x0] + fx * A[y1][x1])   in this order.
 *
 * sf_flow_consistency: n forward and n backward fields of one size h x w, fp32 planes: u of field i at
 *   fwd + i fwd_field_stride + y fwd_row_stride + x, v at the same + fwd_ch_stride (strides in floats; bwd likewise: slices of
 *   predict_video's outputs and views into padded buffers need no copy).  Inside:
 *     bu = sample(bwd u), bv = sample(bwd v),  dx = u + bu, dy = v + bv,  lhs = dx dx + dy dy,
 *     rhs = alpha * ((u u + v v) + (bu bu + bv bv)) + beta,
 *   class VISIBLE if inside && lhs <= rhs; OCCLUDED if inside && !(lhs <= rhs) (a NaN among the taps included); OUTSIDE otherwise.
 *   cls:   uint8 [n][h][w] dense; the byte of a pixel is code_visible / code_occluded / code_outside (255 / 0 / 128 gives a mask
 *          image, 0 / 1 / 2 codes, without a second pass).
 *   stats: fp64 [n][SF_FBC_LEN] on the device; row i is ADDED to (counts are exact in fp64 below 2^53):
 *            PIXELS    pixels                         VISIBLE / OCCLUDED / OUTSIDE   pixels of each class
 *            SUM_FB    sum of sqrtf(lhs) over visible pixels
 *            SUM_MAG   sum of sqrtf(u u + v v) over the pixels where that magnitude is finite in fp32 (NaN, Inf and flows whose
 *                      square overflows stay out)     FINITE   their number
 *   ws:    scratch of sf_flow_consistency_ws_bytes(n, h, w) bytes (per-block partials); it is not read by later calls.
 *   Consecutive lanes take consecutive pixels (coalesced element loads and stores for any strides and alignment, measured faster
 *   than four pixels per lane with 16-byte accesses); the taps of the backward field are element loads (a gather).
 *
 * sf_warp_frames: n source frames (in a video: the frames j + 1), uint8 with 3 channels, byte (i, y, x, ch) at
 *   src + i src_frame_stride + y src_row_stride + x src_px_stride + ch src_ch_stride (bytes, >= 0, as sf_frames_to_clips: HWC, CHW
 *   and views), warped back by field i of `flows` (planes addressed as fwd above):
 *     val = sample((float)src channel),   out[i][y][x][ch] = (uint8)floorf(val + 0.5f) inside, 0 outside;   out uint8 [n][h][w][3] dense.
 *   cls (sf_flow_consistency's map for the same flows) and ref (the frames j, strides as src) are optional and come together; with
 *   them row i of stats fp64 [n][SF_WARP_LEN] is ADDED to: SUM_ABS = sum over inside pixels whose class byte is code_visible, and
 *   over the three channels, of fabsf(val - (float)ref byte); TERMS = the number of terms.  ws: sf_warp_frames_ws_bytes(n, h, w)
 *   bytes; stats and ws may be NULL without cls / ref.  float4 loads of the flow planes where pointer and strides allow, three 4-byte
 *   stores per four pixels where w % 4 == 0 and out is 4-byte aligned; element accesses otherwise.
 *
 * Both: one main launch (grid: blocks per field x n) and, with stats, one finish launch (a block per field sums the per-block
 * partials in a fixed order); no atomics; the grid depends on (n, h, w) alone, so repeated calls give bitwise equal rows.  Enqueued
 * on `stream`, no host synchronisation.
 * SF_ERR_BAD_ARG before any launch for: null pointers (cls without ref or the reverse; stats or ws missing where they are needed);
 * h, w <= 0, h * w >= 2^30, n outside 1 .. 65535; a flow row stride < w, a zero channel stride, negative field / byte strides; NaN
 * alpha or beta; flow pointers not 4-byte, stats / ws not 8-byte aligned; ws_bytes too small.  The *_ws_bytes functions return
 * SF_ERR_BAD_ARG for n, h, w outside the limits. */
enum {
    SF_FBC_PIXELS = 0, SF_FBC_VISIBLE = 1, SF_FBC_OCCLUDED = 2, SF_FBC_OUTSIDE = 3, SF_FBC_SUM_FB = 4, SF_FBC_SUM_MAG = 5,
    SF_FBC_FINITE = 6, SF_FBC_LEN = 7
};
enum { SF_WARP_SUM_ABS = 0, SF_WARP_TERMS = 1, SF_WARP_LEN = 2 };
int64_t sf_flow_consistency_ws_bytes(int n, int h, int w);
int sf_flow_consistency(const float* fwd, int64_t fwd_field_stride, int64_t fwd_ch_stride, int64_t fwd_row_stride, const float* bwd,
                        int64_t bwd_field_stride, int64_t bwd_ch_stride, int64_t bwd_row_stride, int n, int h, int w, float alpha,
                        float beta, uint8_t code_visible, uint8_t code_occluded, uint8_t code_outside, uint8_t* cls, double* stats,
                        void* ws, int64_t ws_bytes, void* stream);
int64_t sf_warp_frames_ws_bytes(int n, int h, int w);
int sf_warp_frames(const uint8_t* src, int64_t src_frame_stride, int64_t src_row_stride, int64_t src_px_stride, int64_t src_ch_stride,
                   const float* flows, int64_t flow_field_stride, int64_t flow_ch_stride, int64_t flow_row_stride, int n, int h, int w,
                   uint8_t* out, const uint8_t* cls, uint8_t code_visible, const uint8_t* ref, int64_t ref_frame_stride,
                   int64_t ref_row_stride, int64_t ref_px_stride, int64_t ref_ch_stride, double* stats, void* ws, int64_t ws_bytes,
                   void* stream);

/* ---- frame interpolation: forward splatting with integer weights, a batch of frame pairs per call --------------------------------
 * sf_frame_interp: for n pairs of one size h x w the frame at time t = num / den (0 < num < den <= 64) between frame A (the frames
 *   j, time 0) and frame B (the frames j + 1, time 1).  A, B: uint8 with 3 channels, byte (i, y, x, ch) at a + i a_frame_stride +
 *   y a_row_stride + x a_px_stride + ch a_ch_stride (bytes, >= 0, as sf_warp_frames' src; b likewise with its own strides).  fwd: the
 *   flows A -> B, bwd: the flows B -> A, fp32 planes addressed as sf_flow_consistency's.  cls_f / cls_b: optional, together: the class
 *   maps uint8 [n][h][w] sf_flow_consistency wrote for (fwd, bwd) and for (bwd, fwd); code_visible / code_occluded are the bytes that
 *   mean visible / occluded there.  imp_vis, imp_occ, imp_other: integer importances 1 .. 16 of a source pixel whose class byte is
 *   code_visible / code_occluded / anything else; without class maps every source pixel has imp_vis.
 *
 *   Splat, for side A with flow = fwd, ts = (float)num / (float)den, and for side B with flow = bwd, ts = (float)(den - num) /
 *   (float)den (both quotients computed in fp32 on the host).  Source pixel (x, y) of a side with flow (u, v), fp32, every
 *   operation rounded on its own:
 *     px = (float)x + ts * u,  py = (float)y + ts * v,
 *     the pixel contributes only if  px > -1 && px < (float)w && py > -1 && py < (float)h   (false for NaN, +-Inf, 1e30; made BEFORE
 *       any conversion to an integer, so such flows never form an address),
 *     x0 = (int)floorf(px), fx = px - floorf(px), wx1 = (int)floorf(fx * 64 + 0.5f) in 0 .. 64, wx0 = 64 - wx1; likewise y0, wy0, wy1,
 *     tap (x0 + a, y0 + b), a, b in {0, 1}, has the integer weight wt = wxa * wyb (the four sum to exactly 4096) and contributes only
 *       if wt != 0 and its position lies inside [0, w) x [0, h):
 *         W += wt * imp,   C[ch] += wt * imp * byte[ch]      in the tap's four unsigned 64-bit accumulators of this side.
 *   Integer sums do not depend on the order of arrival: the result is bitwise reproducible from run to run and for any grid.  (2^30
 *   source pixels of the largest weight, importance and byte on one target sum to less than 2^54.)
 *   Resolve, per target pixel, integer division throughout; every byte is the exact rational value rounded ONCE, half up (<= 255).
 *   A side is present if its W > 0.  Only A / only B: out = (2 C[ch] + W) / (2 W) of that side, cover 1 / 2.  Both present, cover
 *   0: with N = (den - num) CA[ch] WB + num CB[ch] WA and D = den WA WB (up to 2^108: 128-bit products),
 *   out = (2 N + D) / (2 D) -- the blend of the two means as ONE quotient; the sides are not rounded to bytes first, which would
 *   round twice and leave the byte up to a whole level from the real-valued result.  Neither (a hole), cover 3:
 *   out = (a (den - num) + b num + den / 2) / den of the co-located bytes a, b of A and B.
 *   out:   uint8 [n][h][w][3] dense.   cover: optional uint8 [n][h][w] dense, the codes above.
 *   stats: fp64 [n][SF_INTERP_LEN] on the device; row i is ADDED to: PIXELS, then the pixels of each cover code (BOTH, A_ONLY, B_ONLY,
 *          HOLES); exact counts.
 *   ws:    sf_frame_interp_ws_bytes(n, h, w) = 2 * 4 * 8 * n * h * w bytes of accumulators (planar: uint64 [n][side][W, C0, C1,
 *          C2][h][w]) plus the per-block partial rows of the stats; cleared by the call itself, not read by later calls.
 *   Launches: a clear of the accumulators (a kernel on the stream), the splat (grid: blocks per pair x n x 2 sides; a wave owns 256 consecutive
 *   pixels of a row, lane l the pixels l + 64 j, so for smooth flows an atomic wave-instruction covers 512 contiguous bytes; plain
 *   no-return 64-bit integer atomic adds in global memory, at most 128 added bytes per source pixel and side), the resolve (blocks
 *   per pair x n) and the stats finish (a block per pair sums the partials in a fixed order).  The grid depends on (n, h, w) alone.
 *   Enqueued on `stream`, no host synchronisation.
 *   SF_ERR_BAD_ARG before any launch for: a null a, b, fwd, bwd, out, stats or ws; cls_f without cls_b or the reverse; h, w <= 0,
 *   h * w >= 2^30, n outside 1 .. 65535; num, den outside 0 < num < den <= 64; a flow row stride < w, a zero channel stride, negative
 *   field / byte strides; an importance outside 1 .. 16; flow pointers not 4-byte, stats / ws not 8-byte aligned; ws_bytes too small.
 *   sf_frame_interp_ws_bytes returns SF_ERR_BAD_ARG for n, h, w outside the limits.
 * sf_frame_interp_phases: the same call restricted to the launches named by `phases`, a mask of 1 = clear, 2 = splat, 4 = resolve
 *   and finish (7 = sf_frame_interp); for timing the parts (tools/frame_interp_bench.py).  The exception to the workspace rule
 *   above: without the clear (bit 1) the splat ADDS to whatever the accumulators in `ws` hold, and without the splat the resolve
 *   reads what earlier calls left there, so the caller must keep `ws`, n, h and w unchanged between the calls of one sequence, and
 *   only the sequence clear, splat, resolve (in one call or several) gives sf_frame_interp's result. */
enum {
    SF_INTERP_PIXELS = 0, SF_INTERP_BOTH = 1, SF_INTERP_A_ONLY = 2, SF_INTERP_B_ONLY = 3, SF_INTERP_HOLES = 4, SF_INTERP_LEN = 5
};
int64_t sf_frame_interp_ws_bytes(int n, int h, int w);
int sf_frame_interp(const uint8_t* a, int64_t a_frame_stride, int64_t a_row_stride, int64_t a_px_stride, int64_t a_ch_stride,
                    const uint8_t* b, int64_t b_frame_stride, int64_t b_row_stride, int64_t b_px_stride, int64_t b_ch_stride,
                    const float* fwd, int64_t fwd_field_stride, int64_t fwd_ch_stride, int64_t fwd_row_stride, const float* bwd,
                    int64_t bwd_field_stride, int64_t bwd_ch_stride, int64_t bwd_row_stride, int n, int h, int w, int num, int den,
                    const uint8_t* cls_f, const uint8_t* cls_b, uint8_t code_visible, uint8_t code_occluded, int imp_vis, int imp_occ,
                    int imp_other, uint8_t* out, uint8_t* cover, double* stats, void* ws, int64_t ws_bytes, void* stream);
int sf_frame_interp_phases(const uint8_t* a, int64_t a_frame_stride, int64_t a_row_stride, int64_t a_px_stride, int64_t a_ch_stride,
                           const uint8_t* b, int64_t b_frame_stride, int64_t b_row_stride, int64_t b_px_stride, int64_t b_ch_stride,
                           const float* fwd, int64_t fwd_field_stride, int64_t fwd_ch_stride, int64_t fwd_row_stride,
                           const float* bwd, int64_t bwd_field_stride, int64_t bwd_ch_stride, int64_t bwd_row_stride, int n, int h,
                           int w, int num, int den, const uint8_t* cls_f, const uint8_t* cls_b, uint8_t code_visible,
                           uint8_t code_occluded, int imp_vis, int imp_occ, int imp_other, uint8_t* out, uint8_t* cover, double* stats,
                           void* ws, int64_t ws_bytes, int phases, void* stream);

/* ---- resize: separable resampling of uint8 frames and fp32 flow planes with caller-built tables (csrc/resize.hip) -----------------
 * Running the model at a chosen resolution: frames are resampled to the working size, the flows back to the frames' own grid.  The
 * coefficient tables are built by the caller on the host (streamflow_amd.resize.coeff_table: a few hundred doubles per axis, the
 * filters' sin / polynomial evaluated in float64 once per (in, out, filter)) and passed as DEVICE pointers; the kernels do the
 * per-pixel arithmetic only.  Per axis, for an output of `out` positions from an input of `in`:
 *     bounds int32 [out][2]:  (first tap, tap count), 0 <= first, first + count <= in, count <= ksize,
 *     k      [out][ksize]:    the coefficient of tap first + i at [o][i]; entries past the count are not read.
 *
 * sf_resize_u8: n frames uint8 with 3 channels, byte (i, y, x, ch) at src + i frame_stride + y row_stride + x px_stride +
 *   ch ch_stride (bytes, >= 0, as sf_warp_frames' src: HWC, CHW and views need no copy), from H x W to h x w; out uint8
 *   [n][h][w][3] dense (the layout sf_frames_to_clips' fast path reads).  k is int32, the coefficients scaled by 2^22.  This is
 *   Pillow's ImagingResample for 8-bit images:
 *     a horizontal pass runs only if w != W:  t[i][y][x][ch] = clip8(2^21 + sum_j src[i][y][first_x(x) + j][ch] * kx[x][j]),  y < H,
 *     then a vertical pass only if h != H:    out[i][y][x][ch] = clip8(2^21 + sum_j t[i][first_y(y) + j][x][ch] * ky[y][j]),
 *     clip8(ss) = clamp(ss >> 22, 0, 255) (arithmetic shift); the sums are 32-bit integers; the intermediate t is uint8
 *     [n][H][w][3] in `ws`; with one pass its result goes straight to out, with none the call is a copy into the dense layout.
 *   ws: sf_resize_u8_ws_bytes(n, H, W, h, w) = 3 n H w bytes when both passes run, else 0 (ws may then be NULL); 4-byte aligned.
 *   Tables of an axis that has no pass are not read and may be NULL.
 * sf_resize_f32: n fields of two fp32 planes, u of field i at src + i field_stride + y row_stride + x, v at the same + ch_stride
 *   (floats, as sf_flow_consistency's fwd), from H x W to h x w; out fp32 [n][2][h][w] dense.  k is fp32 (the float64 table rounded
 *   once).  The same two passes in fp32, every product and every sum rounded on its own, in tap order from acc = 0:
 *     acc = acc + v[first + j] * k[o][j],  j = 0 .. count - 1;   the intermediate is fp32 [n][2][H][w] in `ws`;
 *   on the final store (of whichever pass is last, or of the copy) channel 0 is multiplied by sx and channel 1 by sy (flows resized
 *   to another grid are in that grid's pixels: sx = w / W, sy = h / H; 1 for plain resampling).  Every tap inside a position's
 *   bounds is multiplied, zero coefficients included: where the output is NaN is a function of the table and of where the input is
 *   not finite, nothing else.  ws: sf_resize_f32_ws_bytes(n, H, W, h, w) = 8 n H w bytes when both passes run, else 0.
 *
 * Addressing: no address depends on pixel data.  The only data-dependent indices are the tables' first + j: each is clamped into
 * [0, in - 1] in the kernel and the count into [0, ksize], so no table content can form an address outside the image; a wrong table
 * gives wrong pixels and nothing else.
 * Launches: one per pass (memory-bound work), one copy launch when neither axis changes.  Horizontal: a block owns 64 output
 * columns for 16 rows and stages its 64 table rows in LDS; a thread owns one output pixel.  Vertical: a block owns (part of) one
 * output row, its coefficients are wave-uniform; u8: a thread owns four consecutive bytes of the packed 3 w-byte row, with dword
 * loads and stores where the source is packed (px_stride 3, ch_stride 1), 3 w % 4 == 0 and src, its row / frame strides, are
 * 4-byte aligned, byte accesses otherwise.  Enqueued on `stream`, no host synchronisation, nothing allocated.
 * SF_ERR_BAD_ARG before any launch for: a null src or out, a null table of an axis that has a pass, a null ws where one is needed;
 * H, W, h, w <= 0; H W, h w or H w >= 2^30; n outside 1 .. 65535 (u8) / 1 .. 32767 (f32); ksize of an axis that has a pass outside
 * 1 .. SF_RESIZE_MAX_KSIZE (97: a 16-fold reduction with the 3-lobe filter, 2 * 48 + 1 taps); negative byte strides (u8), a row
 * stride < W, a zero channel stride, a negative field stride (f32); out, ws or a table not 4-byte aligned (f32: src too); ws_bytes
 * too small.  The *_ws_bytes functions return SF_ERR_BAD_ARG for n, H, W, h, w outside the limits. */
#define SF_RESIZE_MAX_KSIZE 97
int64_t sf_resize_u8_ws_bytes(int n, int H, int W, int h, int w);
int sf_resize_u8(const uint8_t* src, int64_t frame_stride, int64_t row_stride, int64_t px_stride, int64_t ch_stride, int n, int H, int W,
                 int h, int w, const int32_t* bounds_x, const int32_t* kx, int ksize_x, const int32_t* bounds_y, const int32_t* ky,
                 int ksize_y, uint8_t* out, void* ws, int64_t ws_bytes, void* stream);
int64_t sf_resize_f32_ws_bytes(int n, int H, int W, int h, int w);
int sf_resize_f32(const float* src, int64_t field_stride, int64_t ch_stride, int64_t row_stride, int n, int H, int W, int h, int w,
                  const int32_t* bounds_x, const float* kx, int ksize_x, const int32_t* bounds_y, const float* ky, int ksize_y, float sx,
                  float sy, float* out, void* ws, int64_t ws_bytes, void* stream);

/* ---- PNG frames: row unfiltering of inflated IDAT streams (PNG specification, section 9; flow_io.read_png on the host) ----------
 * The host inflates (zlib); the device undoes the row filters of a whole batch of equally shaped images in one launch, so the
 * decoded frames are born where sf_frames_to_clips and sf_flow_score_batch read them.
 *
 * sf_png_unfilter: scan + i scan_image_stride is the inflated IDAT stream of image i: h rows of 1 + w bpp bytes, dense, each with
 *   its filter-type byte first (rows therefore start at arbitrary byte addresses; nothing is assumed about alignment).  bpp is the
 *   PNG filter distance = bytes per pixel: 1, 2, 3, 4, 6 or 8 (8 / 16-bit grey, grey + alpha, RGB, RGBA).  The reconstructed byte x
 *   of row y goes to out[i out_image_stride + y out_row_stride + x], with swap16 != 0 to ... + (x ^ 1) (16-bit samples in host
 *   order; needs an even bpp).  Every byte of the h x (w bpp) view is written, nothing outside it.  Filter types 0 .. 4 = None, Sub,
 *   Up, Average ((a + b) >> 1 on 9 bits), Paeth (ties a, b, c), all mod 256; a = c = 0 in the first bpp bytes of a row, b = c = 0 in
 *   row 0.  A filter byte above 4 is treated as type 0 (flow_io.png_scanlines rejects such files before anything is uploaded).
 *   One workgroup per image walks it in bands of SF_PNG_BAND_ROWS rows, a thread per row, one pixel per step along the
 *   anti-diagonals; the row handed from band to band lives in LDS, hence SF_PNG_MAX_ROW_BYTES.  No data passes between workgroups
 *   and every loop's trip count depends on (h, w) alone.  One launch, no host synchronisation.
 *   SF_ERR_BAD_ARG before any launch for: null pointers, n_images outside 1 .. 65535, h or w < 1, a bpp outside the set above, swap16
 *   with an odd bpp, scan_image_stride < h (1 + w bpp), out_row_stride < w bpp, out_image_stride < (h - 1) out_row_stride + w bpp,
 *   h (1 + w bpp) >= 2^31.  SF_ERR_UNSUPPORTED for w bpp > SF_PNG_MAX_ROW_BYTES. */
#define SF_PNG_BAND_ROWS 256
#define SF_PNG_MAX_ROW_BYTES 40960 /* 5120 pixels of 16-bit RGBA; the kernel keeps one row of this size and 4 KiB more in LDS */
int sf_png_unfilter(const uint8_t* scan, int64_t scan_image_stride, int n_images, int h, int w, int bpp, uint8_t* out,
                    int64_t out_image_stride, int64_t out_row_stride, int swap16, void* stream);

/* ---- PNG output: adaptive row filter and Huffman-only deflate of a batch of device images (RFC 1950 / 1951; PNG specification 9, 12.8) --
 * sf_png_encode: image i is h rows of w bpp bytes at img + i img_image_stride + y img_row_stride (bpp as for sf_png_unfilter; with
 *   swap16 != 0 the 16-bit samples are in host order and are filtered and written big-endian; needs an even bpp).  out + i
 *   out_image_stride receives a complete zlib stream and out_bytes[i] (device memory) its length:
 *     `78 01`; one dynamic-Huffman block per band of SF_PNG_ENC_BAND_ROWS scanlines, literals and end-of-block only, BFINAL on the
 *     last; the big-endian Adler-32 of the scanlines.
 *   A scanline is the filter-type byte and the w bpp filtered bytes; the type of a row is the one whose filtered bytes have the
 *   smallest sum of min(v, 256 - v) (libpng's heuristic), ties to the lowest type; row 0 has a zero row above it.
 *   A block: BFINAL, BTYPE = 2, HLIT = 0, HDIST = 1, HCLEN = 15; 19 code-length code lengths; 257 literal / end-of-block lengths and two
 *   distance lengths of 1 (as zlib writes a block without matches), each as its own code-length symbol 0 .. 15 (no repeat codes: a
 *   header is at most 1887 bits against some 100 KB of scanlines); the literals; the end-of-block.  Code lengths are at most 15
 *   (literals) and 7 (code-length alphabet) bits, codes canonical.  Lengths: the used symbols ranked by (frequency, symbol); Huffman's
 *   algorithm on two queues, a leaf taken when its weight is <= the front node's; leaves per depth, depths above the limit counted at
 *   the limit; while the Kraft sum exceeds 1, one code leaves the limit and one code of the deepest shorter length becomes two codes
 *   one bit longer; lengths handed out along the rank, longest first.  If the literal table costs more bits than the fixed table
 *   (8 bits for 0 .. 254, 9 for 255 and end-of-block) that table is used.  A band always has two used symbols (a byte and the
 *   end-of-block), so a band of one value gets two 1-bit codes.  tests/png_encode_cases.py restates all of it; the output equals that
 *   restatement byte for byte, and two runs are bitwise equal.
 *   SF_PNG_ENC_BAND_ROWS = 32: the stream size is flat over 8 .. 64 rows (-0.4 % .. +0.4 % of zlib's Z_HUFFMAN_ONLY on smooth
 *   436 x 1024 images); 32 rows make 14 blocks of a 436-row frame, enough workgroups per image, with a header below
 *   0.3 % of a block.
 * sf_png_encode_bound(h, w, bpp): no stream is longer, whatever the image holds: 2 + ceil((nb 1896 + 9 h (1 + w bpp)) / 8) + 4 rounded
 *   up to a multiple of 4, nb = ceil(h / SF_PNG_ENC_BAND_ROWS): a header is at most 17 + 57 + 259 x 7 = 1887 bits, and the literals
 *   of a band of N bytes at most 9 N + 9 bits because the fixed table above replaces a costlier one.  -1 for a shape sf_png_encode
 *   refuses with SF_ERR_BAD_ARG.  The bytes of a slot between the stream's end and the bound are unspecified (the call clears them
 *   itself: `out` need not be zeroed); nothing beyond the bound is written.
 * sf_png_encode_ws_bytes: the workspace (filtered scanlines, per-band tables); -1 for a refused shape or n_images.
 * One clear launch and four more (filter: a wave per row; tables: a workgroup per band; offsets: a thread per image; pack: a workgroup
 *   per band, bits ORed in with vector atomics); dependencies between workgroups are launch boundaries and every trip count depends
 *   on (n_images, h, w, bpp) alone.  No host synchronisation.
 *   SF_ERR_BAD_ARG before any launch for: null pointers, n_images outside 1 .. 65535, h or w < 1, a bpp outside the set, swap16 with an
 *   odd bpp, h (1 + w bpp) >= 2^31, img_row_stride < w bpp, img_image_stride < (h - 1) img_row_stride + w bpp, out_image_stride below
 *   the bound, out or out_image_stride not a multiple of 4, out_bytes not 8-byte aligned, ws_bytes too small.  SF_ERR_UNSUPPORTED for
 *   w bpp > SF_PNG_MAX_ROW_BYTES.
 * sf_flow_to_kitti16: flow [n][2][h][w] fp32 -> out [n][h][w][3] uint16 in host order = (64 u + 32768, 64 v + 32768, 1), flow_io.kitti_encode
 *   for float32 input: the product (exact) and the sum are rounded to fp32 one after the other, the result is truncated.  Values
 *   below 0 and NaN give 0, values of 65535 or more give 65535.  Limits: n <= 65535, h * w < 2^30. */
#define SF_PNG_ENC_BAND_ROWS 32
int64_t sf_png_encode_bound(int h, int w, int bpp);
int64_t sf_png_encode_ws_bytes(int n_images, int h, int w, int bpp);
int sf_png_encode(const uint8_t* img, int64_t img_image_stride, int64_t img_row_stride, int n_images, int h, int w, int bpp,
                  int swap16, uint8_t* out, int64_t out_image_stride, int64_t* out_bytes, void* ws, int64_t ws_bytes, void* stream);
int sf_flow_to_kitti16(const float* flow, uint16_t* out, int n, int h, int w, void* stream);

/* ---- JPEG output: baseline sequential DCT, Huffman coding (ITU-T T.81) of a batch of device images; the frames of a Motion-JPEG video ----
 * sf_jpeg_encode: image i is h rows of w pixels at img + i img_image_stride + y img_row_stride; channels = 3: interleaved R, G, B bytes
 *   (what sf_flow_to_image writes), channels = 1: grey.  qtables is HOST memory: [2][64] quantisation steps 1 .. 255 in natural (row-major)
 *   order, table 0 for luma / grey and table 1 for chroma; they are read before the call returns.  out + i out_image_stride receives
 *   image i's entropy-coded segment -- everything between the SOS header and EOI -- and out_bytes[i] (device memory) its length; the
 *   host writes the marker segments around it (jpeg_gpu.jpeg_file).  The format:
 *   Colour.  Grey is one component.  RGB becomes JFIF YCbCr (BT.601, full range) in 16-bit fixed point, >> arithmetic:
 *       Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *       Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16          (8421375 = 128 x 65536 + 32767)
 *       Cr = ( 32768 R - 27439 G -  5329 B + 8421375) >> 16
 *     all in 0 .. 255.  Sampling is 4:4:4: H = V = 1 for every component, an MCU is one 8 x 8 block per component in the order Y, Cb, Cr.
 *   Edges.  Where w or h is no multiple of 8 the last column / row is replicated.
 *   DCT.  s = sample - 128.  Table C[u][x] = round(2^13 sqrt 2 c(u) / 2 cos((2 x + 1) u pi / 16)), c(0) = 1 / sqrt 2, c(u) = 1 otherwise: the
 *     values 4096 (u = 0, 4: exact), 5681 4816 3218 1130 (cos of 1, 3, 5, 7 pi / 16), 5352 2217 (2, 6 pi / 16) with the cosines' signs;
 *     the factor sqrt 2 per pass makes the two passes give 2 F, and the DC coefficient exact.  Rows first:
 *     t[y][u] = (sum_x C[u][x] s[y][x] + 256) >> 9 (4 fraction bits, rounded half up); then columns: G[v][u] = sum_y C[v][y] t[y][u]
 *     = 2^18 F[v][u], not rounded.  All sums are exact in 32 bits: |G| < 2^29.
 *     Accuracy: G / 2^18 is within B = 0.3126 of the exact DCT coefficient.  With e = 2^-14 the table's rounding error relative to 2^13
 *     and A = max_u sum_x |sqrt 2 c(u) / 2 cos(..)| = 4: |t - sqrt 2 t_exact| <= 8 x 128 e + 2^-5 = 0.09375 =: d (table, then rounding),
 *     and |G / 2^17 - 2 F_exact| <= A d + 8 e (128 A + d) = 0.375 + 0.25005, half of which is B.
 *   Quantisation.  level = sign(G) ((|G| + (q << 17)) / (q << 18)), integer division: G / (2^18 q) rounded half away from zero, q the step of
 *     the component's table at that coefficient.  |level| <= 1024 for DC (a DC difference has category <= 11) and <= 1020 for AC
 *     (category <= 10): an AC basis function sums to zero and its absolute values sum to at most 8, so |F_exact| <= 4 (128 + 127).
 *   Entropy coding.  The four typical Huffman tables of T.81 Annex K.3 (K.3 / K.4 for DC, K.5 / K.6 for AC), luma tables for Y / grey and
 *     chroma tables for Cb, Cr; canonical codes as in Annex C.  A block: the DC difference to the previous block of the same component as
 *     category code + category bits (negative values: the low bits of value - 1); the AC levels along the zigzag scan as (run << 4 |
 *     category) code + category bits, ZRL (0xF0) for every 16 zeros in front of a level, EOB (0x00) unless coefficient 63 is non-zero.
 *     Bits are written MSB first.
 *   Restart intervals.  One interval per MCU row: DRI = ceil(w / 8).  The DC predictions are 0 at the start of each; each is padded to a
 *     byte with 1-bits; every 0xFF byte of it (a padded one too) is followed by 0x00; RSTm = FF D0+m, m = row mod 8, stands between
 *     intervals, none behind the last.  tests/jpeg_cases.py restates all of it; the output equals that restatement byte for byte, and two
 *     runs are bitwise equal.
 * sf_jpeg_encode_bound(h, w, channels): no segment is longer, whatever the image and the tables hold: ceil(h / 8) (2 I + 2) rounded up to a
 *   multiple of 4, I = ceil(ceil(w / 8) channels 1660 / 8).  A block has at most 1660 bits: the longest DC code (11 bits, chroma
 *   category 11) + 11 bits, and 63 AC levels of the longest AC code (16 bits) + 10 bits (a ZRL or EOB is cheaper than the levels it
 *   stands for); I is an interval's bytes, doubled for stuffing, + 2 for its marker.  -1 for h or w outside 1 .. SF_JPEG_MAX_DIM or
 *   channels outside {1, 3}.  The bytes of a slot behind the segment are not written (`out` need not be cleared), nor anything beyond
 *   the bound.
 * sf_jpeg_encode_ws_bytes: the workspace (levels, the intervals before stuffing, their lengths and offsets); -1 for a refused shape or n.
 * Five launches (DCT: a thread per block; pack: a workgroup per interval, a thread per block and component, the bits ORed with vector
 *   atomics into workspace words the same workgroup cleared; 0xFF count; offsets: a thread per image; gather with stuffing: plain byte
 *   stores); dependencies between workgroups are launch boundaries.  No host synchronisation.
 *   SF_ERR_BAD_ARG before any launch for: null pointers, n_images outside 1 .. 65535, h or w < 1, channels outside {1, 3}, a table entry
 *   outside 1 .. 255, img_row_stride < w channels, img_image_stride < (h - 1) img_row_stride + w channels, out_image_stride below the
 *   bound, out or out_image_stride not a multiple of 4, out_bytes not 8-byte aligned, ws_bytes too small.  SF_ERR_UNSUPPORTED for h or w
 *   above SF_JPEG_MAX_DIM (checked after the first five of these). */
#define SF_JPEG_MAX_DIM 8192 /* the bound of an 8192 x 8192 x 3 image stays below 2^31; 2160 x 3840 video frames fit */
int64_t sf_jpeg_encode_bound(int h, int w, int channels);
int64_t sf_jpeg_encode_ws_bytes(int n_images, int h, int w, int channels);
int sf_jpeg_encode(const uint8_t* img, int64_t img_image_stride, int64_t img_row_stride, int n_images, int h, int w, int channels,
                   const uint16_t* qtables, uint8_t* out, int64_t out_image_stride, int64_t* out_bytes, void* ws, int64_t ws_bytes,
                   void* stream);

/* ---- JPEG input: baseline files of one geometry -> device images (csrc/jpeg_decode.hip; the host's marker walk is jpeg_gpu.parse) ----
 * sf_jpeg_decode: n_images files of ONE geometry -- h, w, components (1: grey, 3: YCbCr), luma sampling hs x vs in {1x1, 2x1, 2x2} with
 *   chroma at 1 x 1 (4:4:4, 4:2:2, 4:2:0; grey: 1 x 1) -- from their entropy-coded bytes to pixels.  Baseline sequential DCT (SOF0), 8 bit,
 *   Huffman, one interleaved scan; whatever else a file may be is the host parser's to refuse.  All pointers but `stream` are device
 *   memory:
 *   data     data_bytes bytes: the entropy-coded bytes of all files, still stuffed (FF 00), any alignment.
 *   desc     n_intervals rows of SF_JPEG_DESC_WORDS int64, one per restart interval: in_off, in_len (the interval is data[in_off ..
 *            in_off + in_len): no RSTm marker, no fill bytes), image, first_mcu, n_mcus (the MCUs first_mcu .. first_mcu + n_mcus - 1 of
 *            that image, counted in scan order: rows of ceil(w / 8 hs) MCUs), table_set.  A file without DRI is one interval with all
 *            its MCUs.  The intervals of an image must cover each of its MCUs once.
 *   tables   n_table_sets records of SF_JPEG_TABLE_SET_BYTES = 3 x 608 bytes, de-duplicated by the host: per component (3 slots, the
 *            unused ones of a grey file are not read) 64 quantisation steps as bytes in NATURAL (row-major) order, then the DC and the
 *            AC Huffman specification, each 16 BITS bytes + 256 HUFFVAL bytes (fixed stride: entries past the sum of BITS are ignored).
 *   out      image i at out + i out_image_stride + y out_row_stride, w pixels of out_channels bytes: 3: R, G, B (a grey file's sample
 *            three times, as datasets.read_frame does for grey PNGs), 1: the grey sample (components = 1 only).
 *   status   one int32 per image: 0, or the SF_JPEG_* word of its failed interval with the lowest row number in desc, or
 *            SF_JPEG_BAD_DESC where the clean intervals do not cover the image's MCUs.  (A row whose `image` is out of range is
 *            reported at the nearest image.)  A failed image leaves unspecified pixels inside its own slot; the other images of the
 *            batch are not affected.
 *   The arithmetic, all integer (>> arithmetic); tests/jpeg_decode_cases.py restates it, and on every file of tests/golden/jpeg_decode
 *   that restatement, this entry point and libjpeg-turbo (through PIL) agree bit for bit:
 *   Entropy decoding.  T.81 F.2.2: canonical codes from BITS / HUFFVAL (Annex C), MSB first; a DC difference of category s <= 11 on top
 *     of the component's prediction, which starts at 0 in every interval; AC symbols run << 4 | size along the zigzag scan with size
 *     <= 10, ZRL (F0) and EOB (00).  Coefficient k of component c is multiplied by the c's step k and stored as int16 in natural
 *     order.  Bounds: every dequantised coefficient has |c| <= 2048 and the 64 of a block sum |c| <= 18432, else
 *     SF_JPEG_COEF_RANGE.  No file made from 8-bit samples gets there: the exact DCT of samples - 128 has |F| <= 1024 and sum |F| <=
 *     8 ||s||_2 <= 8192, a quantiser that rounds to the nearest level or towards zero gives 0 or at most |F| + q / 2 <= 2 |F|, q <=
 *     255.  The per-coefficient bound X = 2048 alone does NOT keep the inverse DCT inside 32 bits (64 coefficients of 2048 with the
 *     signs of one sample's basis reach 1.74 x 2^31 in the second pass); with both bounds no intermediate of either pass passes
 *     0.88 x 2^31 (csrc/jpeg_decode_core.h has the derivation, tests/jpeg_decode_cases.idct_bounds() recomputes it from the
 *     data flow of the transform, not from samples).
 *   Inverse DCT.  libjpeg's jidctint.c "islow" exactly, in 32-bit integers, CONST_BITS = 13, PASS1_BITS = 2, the constants 2446 3196
 *     4433 6270 7373 9633 12299 15137 16069 16819 20995 25172 = FIX(0.298631336) .. FIX(3.072711026).  One pass on in[0 .. 7]:
 *       even: z1 = (in2 + in6) 4433, tmp2 = z1 - in6 15137, tmp3 = z1 + in2 6270, tmp0 = (in0 + in4) << 13, tmp1 = (in0 - in4) << 13,
 *             tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2
 *       odd:  t0 = in7, t1 = in5, t2 = in3, t3 = in1; z1 = t0 + t3, z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3, z5 = (z3 + z4) 9633;
 *             t0 *= 2446, t1 *= 16819, t2 *= 25172, t3 *= 12299; z1 *= -7373, z2 *= -20995, z3 = z3 (-16069) + z5, z4 = z4 (-3196) + z5;
 *             t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4
 *       out0 / out7 = tmp10 +- t3, out1 / out6 = tmp11 +- t2, out2 / out5 = tmp12 +- t1, out3 / out4 = tmp13 +- t0.
 *     Columns first, descaled (x + 1024) >> 11; then rows, descaled (x + 2^17) >> 18, + 128, clamped to 0 .. 255.
 *   Chroma upsampling.  libjpeg's "fancy" triangle filters on the cw = ceil(w / hs) x ch = ceil(h / vs) real samples of a chroma plane
 *     (the block padding is never read).  2 x 1: output 2 i = (3 c[i] + c[i - 1] + 1) >> 2, output 2 i + 1 = (3 c[i] + c[i + 1] + 2) >> 2,
 *     output 0 = c[0], output 2 cw - 1 = c[cw - 1].  2 x 2: for output row y the chroma row r = y / 2 and its nearer neighbour n = r - 1
 *     (y even) or r + 1 (y odd), clamped to 0 .. ch - 1; t[i] = 3 c[r][i] + c[n][i]; output 2 i = (3 t[i] + t[i - 1] + 8) >> 4, output
 *     2 i + 1 = (3 t[i] + t[i + 1] + 7) >> 4, output 0 = (4 t[0] + 8) >> 4, output 2 cw - 1 = (4 t[cw - 1] + 7) >> 4.
 *     As in libjpeg (jinit_upsampler), a plane of cw <= 2 samples (w <= 4) is too narrow for the filters: its samples are replicated
 *     instead, out[y][x] = c[y / vs][x / 2].
 *   Colour.  Cb' = Cb - 128, Cr' = Cr - 128: R = Y + ((91881 Cr' + 32768) >> 16), G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16),
 *     B = Y + ((116130 Cb' + 32768) >> 16), each clamped to 0 .. 255.
 *   Safety.  For ANY bytes in data, desc and tables every read of `data` stays inside the interval's [in_off, in_off + in_len), every
 *     write of the entropy stage inside the workspace blocks of the interval's own MCUs, and an interval ends within 8 in_len symbol
 *     decodes + in_len refill steps + min(6 n_mcus, 8 in_len + 1) block stores (csrc/jpeg_decode_core.h argues both; the same core
 *     runs under the host sanitizers as csrc/host/jpeg_decode_host_main.cpp).  Two runs are bitwise equal.
 * sf_jpeg_decode_ws_bytes: the workspace (int16 coefficients [image][component][block row][block column][64], the components' uint8
 *   planes padded to whole blocks, two words per image); -1 for a refused shape or n_images.
 * One clear launch (the two words per image) and four more (entropy: one wave per interval; status: a thread per image; inverse DCT: a
 *   thread per block; upsampling and colour: a thread per pixel); dependencies between workgroups are launch boundaries: no flags, no
 *   spinning, no host synchronisation.
 *   SF_ERR_BAD_ARG before anything is enqueued for: null pointers, data_bytes < 0, n_intervals outside 1 .. 2^26, n_table_sets or
 *   n_images outside 1 .. 65535, h or w < 1, components outside {1, 3}, a sampling outside the list above, out_channels outside {1, 3}
 *   or 1 with 3 components, out_row_stride < w out_channels, out_image_stride < (h - 1) out_row_stride + w out_channels, desc not
 *   8-byte, status not 4-byte or ws not 16-byte aligned, ws_bytes too small.  SF_ERR_UNSUPPORTED for h or w above SF_JPEG_MAX_DIM
 *   (checked after the sampling and channel checks).  What desc and tables hold is checked on the device. */
#define SF_JPEG_DESC_WORDS 6
#define SF_JPEG_TABLE_SET_BYTES 1824
enum {
    SF_JPEG_OK = 0,
    SF_JPEG_BAD_CODE = 1,      /* bits that are no code of the table */
    SF_JPEG_BAD_RUN = 2,       /* a run past coefficient 63, a ZRL with no coefficient left to follow it, a run / size symbol baseline lacks */
    SF_JPEG_BAD_CATEGORY = 3,  /* DC category above 11 or AC category above 10 */
    SF_JPEG_TRUNCATED = 4,     /* the interval's input ends inside an MCU */
    SF_JPEG_NOT_CONSUMED = 5,  /* behind the last MCU more than 7 bits remain, or the remaining bits are not all 1 */
    SF_JPEG_BAD_DESC = 6,      /* a descriptor outside the buffers, images, MCUs or table sets; intervals that do not cover the image */
    SF_JPEG_COEF_RANGE = 7,    /* a dequantised coefficient beyond 2048, or a block whose absolute values sum beyond 18432 */
    SF_JPEG_BAD_TABLE = 8,     /* a Huffman specification with more than 256 codes, or more codes of a length than it has patterns */
    SF_JPEG_BAD_MARKER = 9     /* an FF byte inside an interval that is not followed by 00 */
};
int64_t sf_jpeg_decode_ws_bytes(int n_images, int h, int w, int components, int hs, int vs);
int sf_jpeg_decode(const uint8_t* data, int64_t data_bytes, const int64_t* desc, int n_intervals, const uint8_t* tables, int n_table_sets,
                   int n_images, int h, int w, int components, int hs, int vs, uint8_t* out, int64_t out_image_stride,
                   int64_t out_row_stride, int out_channels, int32_t* status, void* ws, int64_t ws_bytes, void* stream);

/* sf_jpeg_decode_split: sf_jpeg_decode with LONG intervals decoded in parallel.  sf_jpeg_decode gives every restart interval one wave,
 *   and a file without DRI -- what PIL, ffmpeg's default, cameras and capture cards write -- is one interval.  Here an interval with
 *   in_len >= split_min_bytes takes the split route: a thread per segment of segment_bytes bytes of its UNSTUFFED stream, by the
 *   self-synchronising method of Klein and Wiseman as Weissenberger and Schmidt applied it to JPEG.  The other intervals take
 *   sf_jpeg_decode's wave route.  split_min_bytes = 0 splits every interval; a value above data_bytes makes the call sf_jpeg_decode's
 *   (the same launches).  All arguments up to `status` are sf_jpeg_decode's; segment_bytes is a power of two in 8 .. 4096.
 *   The unstuffed stream.  The interval's bytes without the 00 of every FF 00, up to the first FF that is the interval's last byte or
 *     has another byte than 00 behind it: the usable stream ends there, and running out of bits is then SF_JPEG_BAD_MARKER instead of
 *     SF_JPEG_TRUNCATED.  Segment s is bits [8 s segment_bytes, 8 min((s + 1) segment_bytes, length)) of it; an empty stream has one
 *     (empty) segment.
 *   A state is (bit, slot, k): the offset of the next symbol's first bit in the unstuffed stream, the block slot inside the MCU (the hs vs
 *     luma blocks, then Cb, then Cr; grey: slot 0 only) and the zigzag index of the next coefficient, k = 0: the next symbol is a DC
 *     symbol.  A step decodes one symbol with the checks of sf_jpeg_decode's entropy decoding, in their order.  A walk of a segment
 *     goes from a state to the first symbol boundary at or behind the segment's last bit, or stops in front of a symbol the stream has
 *     no bits left for.
 *   The lenient rule.  The walks that only look for the boundaries store nothing, and ANY error (no code, a run past 63, a category
 *     baseline lacks) ends the current block ONE BIT behind the failed symbol's first bit; decoding goes on with the next slot's DC
 *     symbol.  A speculative chain therefore never dies (a dead one would let the truth advance one segment per round only), and from
 *     a true state on a valid stream the walk takes exactly the strict steps.  It counts the blocks it ends.
 *   The rounds.  Every segment is first walked from (its first bit, 0, 0).  Then, per window of 256 segments in stream order: the window's
 *     first segment enters with the previous window's final exit, the interval's first with (0, 0, 0); each round sets segment k's entry to
 *     segment k - 1's exit of the round before, and the segments whose entry changed walk again; until a round changes nothing, which is
 *     at most the window's segment count, by induction from its first segment.  The fixed point is the serial decoder's states; a
 *     prefix sum of the block counts gives every segment the ordinal of the block its entry lies in.
 *   The strict walk.  From its true entry every segment decodes for real: AC coefficients dequantised into their blocks, the RAW DC
 *     difference into coefficient 0, and only while the block's ordinal is below n_mcus x blocks per MCU -- for ANY input every write
 *     stays inside the interval's own MCUs.  The walk that ends the last block makes sf_jpeg_decode's closing check (at most 7 bits left,
 *     all 1; SF_JPEG_BAD_MARKER where the stream ends at a marker); the last segment's walk reports SF_JPEG_TRUNCATED / BAD_MARKER where
 *     the stream ends in front of the last block.  Then, per component in scan order, 64-bit prefix sums of the DC differences give the
 *     predictions: |pred| <= 2048 and |pred q| <= 2048 as in sf_jpeg_decode, the dequantised DC into coefficient 0, and the block's
 *     sum |c| <= 18432.
 *   Status of a split interval: every error has the key (ordinal of its block in the interval) << 6 | phase << 4 | word -- phase 0 the DC
 *     range checks, 1 an entropy error (an AC coefficient beyond 2048 included), 2 the block's sum; the closing check has the
 *     interval's block count as its ordinal, a Huffman specification that is none key SF_JPEG_BAD_TABLE alone -- and the interval's word
 *     is that of the SMALLEST key: the first error in stream order, the only one that means anything, since the segments behind it hold
 *     garbage by construction.  It enters the image's status exactly as a wave's word does.
 *   Contract.  An image's status is 0 exactly when sf_jpeg_decode's is, and then its pixels are bitwise sf_jpeg_decode's.  A nonzero word
 *     is the split route's own: sf_jpeg_decode's depends on how far its bit buffer had read ahead (a marker behind the last MCU), which is
 *     not reproduced.  Two runs are bitwise equal.
 *   Launches.  sf_jpeg_decode's clear and four launches, plus -- unless split_min_bytes > data_bytes -- two clear launches (the coefficient
 *     area, since two segments may each write their own coefficients of one block; the keys and the workgroup map, which lie side by side) and seven launches in
 *     front of the wave launch, which skips the split intervals: plan (one workgroup scans desc on the device: which intervals split,
 *     their first workgroup of 256 segment slots and their share of the unstuffed area, by exclusive scans; the host never reads desc
 *     and sizes grids and areas from the bounds data_bytes / (256 segment_bytes) + n_intervals workgroups and data_bytes + 16 n_intervals
 *     bytes, which intervals that do not overlap always fit -- one that does not fit takes the wave route), unstuff (a workgroup per
 *     split interval: count per chunk, scan, copy), the speculative walks (a thread per segment), the rounds (a workgroup per split
 *     interval), the strict walks (a thread per segment), the DC sums (a workgroup per split interval and component), the interval
 *     words.  Dependencies between workgroups are launch boundaries: no flags, no spinning, no host synchronisation.
 *   Safety.  For ANY bytes in data, desc and tables: `data` is read inside an interval's [in_off, in_off + in_len) only, every write of
 *     the entropy stage stays inside the workspace and, for coefficients, inside the blocks of the interval's own MCUs; every walk
 *     consumes at least one bit per step and ends within 8 segment_bytes + 27 bits, and a window's rounds are at most its segments + 1
 *     (csrc/jpeg_sync_core.h and csrc/jpeg_decode.hip argue both; the same functions run under the host sanitizers as
 *     csrc/host/jpeg_sync_host_main.cpp).
 * sf_jpeg_decode_split_ws_bytes: sf_jpeg_decode_ws_bytes plus the split route's areas; -1 for what sf_jpeg_decode_ws_bytes refuses,
 *   data_bytes outside 0 .. 2^40, n_intervals outside 1 .. 2^26, a segment_bytes outside its set, or 2^31 workgroups and more.
 *   SF_ERR_BAD_ARG before anything is enqueued for sf_jpeg_decode's list, segment_bytes outside its set, split_min_bytes < 0 and
 *   ws_bytes too small; SF_ERR_UNSUPPORTED as there. */
int64_t sf_jpeg_decode_split_ws_bytes(int n_images, int h, int w, int components, int hs, int vs, int64_t data_bytes, int n_intervals,
                                      int segment_bytes);
int sf_jpeg_decode_split(const uint8_t* data, int64_t data_bytes, const int64_t* desc, int n_intervals, const uint8_t* tables,
                         int n_table_sets, int n_images, int h, int w, int components, int hs, int vs, uint8_t* out,
                         int64_t out_image_stride, int64_t out_row_stride, int out_channels, int32_t* status, int segment_bytes,
                         int64_t split_min_bytes, void* ws, int64_t ws_bytes, void* stream);

/* ---- Spring .flo5 output: the HDF5 filters shuffle -> deflate of a batch of flow fields, chunk by chunk (flo5.flo5_file frames them) ---
 * sf_flo5_encode: field i is two planes, element (ch, y, x) at flow + i field_stride + ch ch_stride + y row_stride + x (strides in
 *   floats; an unpadded view of a padded field goes in as it is).  The HDF5 dataset is float32 [h][w][2] in chunks of
 *   (rows_per_chunk, w, 2): nchunks = ceil(h / rows_per_chunk), chunk c starts at row c rows_per_chunk and has N = rows_per_chunk w 2
 *   elements, element (y w + x) 2 + ch the BIT PATTERN of flow[ch][c rows_per_chunk + y][x] (NaN payloads, -0.0, infinities and
 *   denormals pass unchanged), rows past h zero bits (libhdf5 stores edge chunks at full size).  HDF5's shuffle filter: byte j N + e
 *   of the shuffled chunk is byte j (little-endian) of element e.  The slot out + (i nchunks + c) out_chunk_stride receives one
 *   complete zlib stream and out_bytes[i nchunks + c] (device memory) its length:
 *     `78 01`; for each byte plane j = 0 .. 3 in turn one block per segment of at most SF_FLO5_BLOCK_BYTES bytes (no block straddles two
 *     planes), BFINAL on the last block of plane 3; the big-endian Adler-32 of the 4 N shuffled bytes.
 *   A block is what sf_png_encode writes for a band (above): the same header fields, length-limited Huffman construction and canonical
 *   codes, no repeat codes, the fixed 8 / 9-bit table wherever the dynamic table costs more.  tests/flo5_encode_cases.py restates the
 *   format; the output equals that restatement byte for byte, and two runs are bitwise equal.
 *   SF_FLO5_BLOCK_BYTES = 65536: see DESIGN.md 9.8 for the stream sizes at 16 / 64 / 256 KiB.
 * sf_flo5_chunk_bound(rows_per_chunk, w): no stream is longer: 2 + ceil((nblk 1896 + 9 x 4 N) / 8) + 4 rounded up to a multiple of 4,
 *   nblk = 4 ceil(N / SF_FLO5_BLOCK_BYTES); -1 for rows_per_chunk or w < 1 or 4 N >= 2^31.  The bytes of a slot between the stream's end
 *   and the bound are unspecified (the call clears them itself: `out` need not be zeroed); nothing beyond the bound is written.
 * sf_flo5_encode_ws_bytes: the workspace (the shuffled chunks, per-block tables); -1 for a shape or n sf_flo5_encode refuses.
 * One clear launch and four more (shuffle: a thread per 4 elements; tables: a workgroup per block; offsets: a thread per chunk; pack: a
 *   workgroup per block, bits ORed in with vector atomics); dependencies between workgroups are launch boundaries and every trip
 *   count depends on (n, h, w, rows_per_chunk) alone.  No host synchronisation.
 *   SF_ERR_BAD_ARG before any launch for: null pointers, n outside 1 .. 65535, h, w or rows_per_chunk < 1, nchunks > 64 (the container
 *   writes a single B-tree leaf), 4 N >= 2^31, row_stride < w, ch_stride < (h - 1) row_stride + w, field_stride < ch_stride +
 *   (h - 1) row_stride + w, flow not 4-byte aligned, out_chunk_stride below the bound, out or out_chunk_stride not a multiple of 4,
 *   out_bytes not 8-byte aligned, ws_bytes too small. */
#define SF_FLO5_BLOCK_BYTES 65536
int64_t sf_flo5_chunk_bound(int rows_per_chunk, int w);
int64_t sf_flo5_encode_ws_bytes(int n, int h, int w, int rows_per_chunk);
int sf_flo5_encode(const float* flow, int64_t field_stride, int64_t ch_stride, int64_t row_stride, int n, int h, int w,
                   int rows_per_chunk, uint8_t* out, int64_t out_chunk_stride, int64_t* out_bytes, void* ws, int64_t ws_bytes,
                   void* stream);

/* ---- Spring .flo5 input: a batch of zlib streams inflated on the device, and the inflated chunks put together (csrc/flo5_decode.hip) ----
 * sf_inflate: n independent zlib streams (RFC 1950 / 1951) -> bytes; generic, it knows nothing of HDF5.  desc (device memory) holds
 *   SF_INFLATE_DESC_WORDS int64 per stream: in_off, in_len, out_off, out_len, flags.  The stream is in[in_off .. in_off + in_len) (any
 *   alignment; bytes behind the stream's end are ignored) and must inflate to EXACTLY out_len bytes, written to out[out_off ..
 *   out_off + out_len) (out_len < 2^31; slots of different streams must not overlap).  flags & SF_INFLATE_STORED: no stream, the in_len
 *   bytes are the data and are copied (an HDF5 chunk whose filter mask skips deflate).  One wave per stream; every block type, repeat
 *   codes, codes up to 15 bits, distances up to 32 768, overlapping matches, any number of blocks; the zlib header and the Adler-32
 *   trailer are verified, a preset dictionary is refused.  status[i] (device memory) receives 0 or one of SF_INFLATE_* below; a failed
 *   stream leaves unspecified bytes inside its own slot and nothing anywhere else.  For ANY input bytes every read stays inside the
 *   stream's input range and every write inside its slot, and the kernel ends within 8 in_len + out_len decode steps (DESIGN.md 9.9;
 *   the decoder core, csrc/inflate_core.h, runs under the host sanitizers as csrc/host/inflate_host_main.cpp).  Two runs are bitwise
 *   equal.  No workspace, one launch, no host synchronisation.
 *   SF_ERR_BAD_ARG before the launch for: null pointers, n outside 1 .. SF_INFLATE_MAX_STREAMS, negative in_bytes / out_bytes, desc not
 *   8-byte or status not 4-byte aligned.  What desc holds is checked on the device: SF_INFLATE_BAD_SLOT.
 * sf_flo5_assemble: the chunks of n files of ONE geometry -> out [n][h][w][2] float32 bit patterns (read_flo5's array).  The dataset is
 *   (h, w, 2) little-endian float32 in chunks of (ch, cw, cc), cc 1 or 2; slot s is the chunk_stride bytes at chunks + s chunk_stride,
 *   of which the first 4 ch cw cc are one inflated chunk (byte-shuffled -- byte j of element e at j N + e -- when shuffle != 0).
 *   grid (device memory, int32 [n][ceil(h / ch)][ceil(w / cw)][2 / cc]) names the slot of every chunk, or -1 (any value outside
 *   0 .. n_slots - 1) for a chunk the file does not store: its elements are 0.0, the fill value.  Edge chunks lose their padding.
 *   A thread per pixel; one launch.  SF_ERR_BAD_ARG for: null pointers, n or h outside 1 .. 65535, w, ch, cw < 1, cc not 1 or 2,
 *   4 ch cw cc >= 2^31, n_slots < 0, chunk_stride below 4 ch cw cc or no multiple of 4, chunks / grid not 4-byte or out not 8-byte
 *   aligned. */
#define SF_INFLATE_DESC_WORDS 5
#define SF_INFLATE_STORED 1
#define SF_INFLATE_MAX_STREAMS 16777216
enum {
    SF_INFLATE_OK = 0,
    SF_INFLATE_BAD_HEADER = 1,       /* CM != 8, CINFO > 7 or the check bits */
    SF_INFLATE_TRUNCATED = 2,        /* the input ends inside the stream */
    SF_INFLATE_BAD_BLOCK_TYPE = 3,   /* BTYPE 3 */
    SF_INFLATE_BAD_CODE_LENGTHS = 4, /* over-subscribed or incomplete set, HLIT / HDIST out of range, bad repeat, no end-of-block code */
    SF_INFLATE_BAD_SYMBOL = 5,       /* bits that are no code; literal/length 286 / 287; distance 30 / 31 */
    SF_INFLATE_BAD_DISTANCE = 6,     /* a distance before the start of the output */
    SF_INFLATE_OUTPUT_LONG = 7,      /* more output than out_len */
    SF_INFLATE_OUTPUT_SHORT = 8,     /* less output than out_len */
    SF_INFLATE_BAD_ADLER = 9,        /* the trailer does not match the output */
    SF_INFLATE_BAD_STORED_LEN = 10,  /* a stored block whose NLEN is not ~LEN */
    SF_INFLATE_PRESET_DICT = 11,     /* FDICT set */
    SF_INFLATE_BAD_SLOT = 12         /* the stream's input or output range lies outside the buffers, or out_len >= 2^31 */
};
int sf_inflate(const uint8_t* in, int64_t in_bytes, const int64_t* desc, int n, uint8_t* out, int64_t out_bytes, int32_t* status,
               void* stream);
int sf_flo5_assemble(const uint8_t* chunks, int64_t chunk_stride, int n_slots, const int32_t* grid, int n, int h, int w, int ch, int cw,
                     int cc, int shuffle, float* out, void* stream);

/* ---- video stabilisation: a camera motion per flow field by reweighted least squares, frames rendered through affine maps ---------
 * Coordinates and model.  For a field of h x w, fp32, every operation rounded on its own:
 *     cx = (float)(w - 1) * 0.5f,  cy = (float)(h - 1) * 0.5f,  s = 2.0f / (float)max(w - 1, h - 1, 1),
 *     xn = ((float)x - cx) * s,    yn = ((float)y - cy) * s.
 *   A model is six numbers a0 .. a5, pixels of displacement at normalised coordinates: u ~ a0 + a1 xn + a2 yn, v ~ a3 + a4 xn + a5 yn.
 *   kind: SF_MOTION_TRANSLATION (a1 = a2 = a4 = a5 = 0), SF_MOTION_SIMILARITY (a1 = a5, a4 = -a2), SF_MOTION_AFFINE.
 *
 * sf_motion_moments: one weighting pass over n fields of one size; flow planes addressed as sf_flow_consistency's fwd (strides in
 *   floats).  Only pixels with y % step == 0 && x % step == 0 take part.  Per pixel, fp32, in this order:
 *     valid = fabsf(u) <= max_mag && fabsf(v) <= max_mag                                                    (false for NaN)
 *     wc    = 1 without cls; with cls (uint8 [n][h][w] dense, as sf_flow_consistency writes it) w_visible / w_occluded / w_outside where
 *             the pixel's byte is code_visible / code_occluded / code_outside (tested in this order), 0 for any other byte
 *     without a model  wt = wc;   with model (fp32 [n][6]) and inv_c2 (fp32 [n]), which come together:
 *       pu = a0 + (a1 xn + a2 yn),  pv = a3 + (a4 xn + a5 yn),  ru = u - pu,  rv = v - pv,  r2 = ru ru + rv rv,  t = r2 inv_c2,
 *       wr = t < 1 ? (1 - t) (1 - t) : 0          (Tukey's biweight; 0 for NaN),       wt = wc wr
 *     invalid pixels: wt = 0.
 *   NaN, Inf and huge flows are ordinary inputs with defined results (weight 0); nothing forms an address from them.
 *   moments: fp64 [n][SF_MOT_LEN], WRITTEN (not added to).  With W = (double)wt and X, Y, U, V the doubles of xn, yn, u, v, over the
 *   pixels with wt > 0, every product rounded on its own in fp64:
 *     S1 = sum W,  SX = sum W X,  SY = sum W Y,  SXX = sum (W X) X,  SXY = sum (W X) Y,  SYY = sum (W Y) Y,
 *     SU = sum W U,  SXU = sum (W X) U,  SYU = sum (W Y) U,  SV = sum W V,  SXV = sum (W X) V,  SYV = sum (W Y) V,
 *     SQQ = sum W (U U + V V),   N = the number of those pixels (exact).
 *   ws: sf_motion_moments_ws_bytes(n, h, w, step) bytes.  A main launch (grid: blocks per field x n) and a finish launch (a block per
 *   field sums the per-block partials in a fixed order); no atomics; the grid depends on (n, h, w, step) alone, so repeated calls
 *   give bitwise equal rows.
 *
 * sf_motion_solve: moments fp64 [n][SF_MOT_LEN] -> models, fp64, a thread per field.  With M = [S1 SX SY; SX SXX SXY; SY SXY SYY],
 *   bu = (SU, SXU, SYU), bv = (SV, SXV, SYV):
 *     S1 > 0 is false (NaN included): the model is zero, status SF_MOT_EMPTY, rss = 0.
 *     TRANSLATION:  a0 = SU / S1,  a3 = SV / S1.
 *     SIMILARITY (a1 = a5 = a, a2 = b, a4 = -b):  D = (SXX + SYY) - (SX SX + SY SY) / S1,
 *                   a = ((SXU + SYV) - (SX SU + SY SV) / S1) / D,   b = ((SYU - SXV) - (SY SU - SX SV) / S1) / D,
 *                   a0 = ((SU - a SX) - b SY) / S1,   a3 = ((SV + b SX) - a SY) / S1.
 *     AFFINE:       M = L L' (Cholesky: l00 = sqrt(S1), l10 = SX / l00, l20 = SY / l00, d1 = SXX - l10 l10, l11 = sqrt(d1),
 *                   l21 = (SXY - l20 l10) / l11, d2 = (SYY - l20 l20) - l21 l21, l22 = sqrt(d2)); (a0, a1, a2) = M^-1 bu and
 *                   (a3, a4, a5) = M^-1 bv by forward and backward substitution with the one factor.
 *     A pivot (D; d1, d2) that is not > 2^-40 S1: the TRANSLATION model instead, status SF_MOT_DEGENERATE.
 *   The scale of the next round, with p = the six numbers:  rss = max(0, (SQQ - 2 p.b) + p'Mp) / S1  (p.b = a0 SU + a1 SXU + a2 SYU +
 *   a3 SV + a4 SXV + a5 SYV; p'Mp = (a0 a1 a2) M (a0 a1 a2)' + (a3 a4 a5) M (a3 a4 a5)'),  c = max(c_floor, kappa sqrt(rss)),
 *   inv_c2 = (float)(1 / (c c)).
 *   Outputs per field: model64 fp64 [n][6], model32 fp32 [n][6] (the rounded copy, what a next sf_motion_moments reads), c fp64 [n],
 *   inv_c2 fp32 [n], status int32 [n].  One launch.
 *
 * sf_motion_fit: the whole chain of `rounds` rounds on `stream` without host synchronisation: round 0 weighs without a model, round
 *   r > 0 with round r - 1's fp32 model and inv_c2.  Two launches a round (the finish launch of a round also solves it).
 *   trace: fp64 [n][rounds][SF_MOT_TRACE_LEN], written: per round the moments (SF_MOT_TRACE_MOMENTS ..), the fp64 model
 *   (SF_MOT_TRACE_MODEL ..), c, inv_c2 (the float's value) and the status.  The last round's model is the result; the model the next
 *   round read is the fp32 rounding of the traced one.  ws: sf_motion_fit_ws_bytes(n, h, w, step) bytes.
 *
 * sf_warp_affine_u8: n source frames, uint8 with 3 channels, bytes addressed as sf_warp_frames' src (byte strides >= 0: HWC, CHW and
 *   views), rendered through inv_maps fp32 [n][6] (m0 .. m5 of frame i: output pixel -> source coordinate), fp32 in this order:
 *     sx = m0 (float)x + (m1 (float)y + m2),   sy = m3 (float)x + (m4 (float)y + m5),
 *     inside as in "forward-backward consistency" with (px, py) = (sx, sy).  Not inside (NaN included): the pixel counts as OUTSIDE, and
 *       SF_BORDER_CONSTANT:  the three fill bytes;
 *       SF_BORDER_REPLICATE: a NaN in sx or sy gives the fill bytes; else sx = fminf(fmaxf(sx, 0), (float)(w - 1)), sy likewise, and
 *                            the pixel is sampled there.
 *     sampled pixels: out = (uint8)floorf(sample((float)src channel) + 0.5f), sample() as there.
 *   out uint8 [n][h][w][3] dense; outside uint32 [n], WRITTEN: the number of OUTSIDE pixels per frame.  ws:
 *   sf_warp_affine_ws_bytes(n, h, w) bytes.  A main and a finish launch, no atomics, as above.
 *
 * SF_ERR_BAD_ARG before any launch for: null pointers (cls may be NULL; model without inv_c2 or the reverse); h, w <= 0, h * w >=
 * 2^30, n outside 1 .. 65535; a flow row stride < w, a zero channel stride, negative field / byte strides; step < 1; rounds outside
 * 1 .. SF_MOT_MAX_ROUNDS; an unknown kind or border; max_mag negative or NaN; a class weight negative, infinite or NaN; kappa negative,
 * infinite or NaN; c_floor <= 0, infinite or NaN; fp32 / uint32 pointers not 4-byte, fp64 pointers and the moments' ws not 8-byte
 * aligned; ws_bytes too small.  The *_ws_bytes functions return SF_ERR_BAD_ARG for n, h, w, step outside the limits. */
enum { SF_MOTION_TRANSLATION = 0, SF_MOTION_SIMILARITY = 1, SF_MOTION_AFFINE = 2 };
enum { SF_MOT_OK = 0, SF_MOT_DEGENERATE = 1, SF_MOT_EMPTY = 2 };
enum {
    SF_MOT_S1 = 0, SF_MOT_SX = 1, SF_MOT_SY = 2, SF_MOT_SXX = 3, SF_MOT_SXY = 4, SF_MOT_SYY = 5, SF_MOT_SU = 6, SF_MOT_SXU = 7,
    SF_MOT_SYU = 8, SF_MOT_SV = 9, SF_MOT_SXV = 10, SF_MOT_SYV = 11, SF_MOT_SQQ = 12, SF_MOT_N = 13, SF_MOT_LEN = 14
};
enum {
    SF_MOT_TRACE_MOMENTS = 0, SF_MOT_TRACE_MODEL = 14, SF_MOT_TRACE_C = 20, SF_MOT_TRACE_INV_C2 = 21, SF_MOT_TRACE_STATUS = 22,
    SF_MOT_TRACE_LEN = 23
};
#define SF_MOT_MAX_ROUNDS 16
enum { SF_BORDER_CONSTANT = 0, SF_BORDER_REPLICATE = 1 };
int64_t sf_motion_moments_ws_bytes(int n, int h, int w, int step);
int sf_motion_moments(const float* flows, int64_t field_stride, int64_t ch_stride, int64_t row_stride, int n, int h, int w,
                      const uint8_t* cls, uint8_t code_visible, uint8_t code_occluded, uint8_t code_outside, float w_visible,
                      float w_occluded, float w_outside, int step, float max_mag, const float* model, const float* inv_c2,
                      double* moments, void* ws, int64_t ws_bytes, void* stream);
int sf_motion_solve(const double* moments, int n, int kind, double kappa, double c_floor, double* model64, float* model32, double* c,
                    float* inv_c2, int32_t* status, void* stream);
int64_t sf_motion_fit_ws_bytes(int n, int h, int w, int step);
int sf_motion_fit(const float* flows, int64_t field_stride, int64_t ch_stride, int64_t row_stride, int n, int h, int w,
                  const uint8_t* cls, uint8_t code_visible, uint8_t code_occluded, uint8_t code_outside, float w_visible, float w_occluded,
                  float w_outside, int step, float max_mag, int kind, int rounds, double kappa, double c_floor, double* trace, void* ws,
                  int64_t ws_bytes, void* stream);
int64_t sf_warp_affine_ws_bytes(int n, int h, int w);
int sf_warp_affine_u8(const uint8_t* src, int64_t src_frame_stride, int64_t src_row_stride, int64_t src_px_stride, int64_t src_ch_stride,
                      const float* inv_maps, int n, int h, int w, int border, uint8_t fill0, uint8_t fill1, uint8_t fill2, uint8_t* out,
                      uint32_t* outside, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STREAMFLOW_HIP_H */
