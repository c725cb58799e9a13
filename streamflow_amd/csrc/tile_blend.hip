// Gaussian-weighted blend of tiled inference (reference evaluate_mf.py:1021-1035 / :951-962).
//
// The reference accumulates, for every crop k of its sequence, flows += F.pad(f_k * w) and count += F.pad(w) over the whole
// padded canvas, then divides.  Per pixel that is, over the crops that cover it and in the sequence's order,
//     acc = acc + f * w;   wsum = wsum + w;   out = acc / wsum
// (the zeros F.pad adds elsewhere leave acc and wsum bitwise unchanged: neither is ever -0).  One thread per output pixel (x fastest,
// coalesced loads of the crops and stores of the output), both channels at once; no atomics, no canvas, no zero fill.
//
// Bitwise agreement with the fp32 CPU arithmetic of the reference matters here: the crop corners carry weights of ~3e-43
// (subnormal) and a corner pixel covered by one crop only is fl(fl(f * w) / w), which differs from f by up to ~2e-3 px.  So every
// product, sum and quotient is rounded on its own and subnormals are kept: FMA contraction is switched off for this file by the
// pragma below (hipcc contracts a*b+c into v_fmac_f32 by default, and the __fmul_rn / __fadd_rn intrinsics of the HIP headers
// do not stop it: their bodies are plain operators compiled outside this pragma), the fp32 division is the correctly rounded
// v_div_scale / v_div_fmas / v_div_fixup sequence (hipcc's default), and the library is built without denormal flushing or
// fast-math (.amdhsa_float_denorm_mode_32 3).
#include "sf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;

// flows [n_clips * n_distinct][pairs][2][th][tw], weights [th][tw], out [n_clips][pairs][2][out_h][out_w]
__global__ __launch_bounds__(kBlock) void tile_blend_kernel(const float* __restrict__ flows, const float* __restrict__ weights,
                                                            float* __restrict__ out, const SfTilePlan plan, int pairs) {
    const int npx = plan.out_h * plan.out_w;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= npx) return;
    const int img = blockIdx.y;                                   // clip * pairs + pair
    const int clip = img / pairs, pair = img % pairs;
    const int y = plan.out_y0 + t / plan.out_w, x = plan.out_x0 + t % plan.out_w;
    const int th = plan.tile_h, tw = plan.tile_w;
    const int64_t plane = (int64_t)th * tw;
    float acc0 = 0.0f, acc1 = 0.0f, wsum = 0.0f;
    for (int k = 0; k < plan.n_seq; ++k) {
        const int ly = y - plan.tile_y[k], lx = x - plan.tile_x[k];
        if (ly < 0 || ly >= th || lx < 0 || lx >= tw) continue;
        const int64_t p = (int64_t)ly * tw + lx;
        const float w = weights[p];
        const float* f = flows + (((int64_t)clip * plan.n_distinct + plan.tile_id[k]) * pairs + pair) * 2 * plane + p;
        acc0 = acc0 + f[0] * w;                                   // (contraction is off for this file: two roundings)
        acc1 = acc1 + f[plane] * w;
        wsum = wsum + w;
    }
    float* o = out + (int64_t)img * 2 * npx + t;
    o[0] = acc0 / wsum;                                           // (hipcc's fp32 division is correctly rounded by default)
    o[npx] = acc1 / wsum;
}

}  // namespace

extern "C" int sf_tile_blend(const float* flows, const float* weights, float* out, const SfTilePlan* plan, int n_clips,
                             int pairs, void* stream) {
    SF_REQUIRE(flows && weights && out && plan, "sf_tile_blend: null argument");
    const SfTilePlan& p = *plan;
    SF_REQUIRE(n_clips > 0 && pairs > 0 && n_clips * pairs <= 65535, "sf_tile_blend: bad clip / pair count %d x %d", n_clips, pairs);
    SF_REQUIRE(p.n_seq > 0 && p.n_seq <= SF_TILE_MAX, "sf_tile_blend: %d crops (1 .. %d allowed)", p.n_seq, SF_TILE_MAX);
    SF_REQUIRE(p.n_distinct > 0 && p.n_distinct <= p.n_seq, "sf_tile_blend: bad distinct crop count %d", p.n_distinct);
    SF_REQUIRE(p.tile_h > 0 && p.tile_w > 0 && p.img_h >= p.tile_h && p.img_w >= p.tile_w,
               "sf_tile_blend: crop %d x %d does not fit the canvas %d x %d", p.tile_h, p.tile_w, p.img_h, p.img_w);
    SF_REQUIRE(p.out_h > 0 && p.out_w > 0 && p.out_y0 >= 0 && p.out_x0 >= 0 && p.out_y0 + p.out_h <= p.img_h &&
                   p.out_x0 + p.out_w <= p.img_w,
               "sf_tile_blend: output crop outside the canvas");
    SF_REQUIRE((int64_t)p.img_h * p.img_w < (1 << 30), "sf_tile_blend: canvas too large");
    for (int k = 0; k < p.n_seq; ++k) {
        SF_REQUIRE(p.tile_y[k] >= 0 && p.tile_y[k] + p.tile_h <= p.img_h && p.tile_x[k] >= 0 && p.tile_x[k] + p.tile_w <= p.img_w,
                   "sf_tile_blend: crop %d at (%d, %d) leaves the canvas", k, p.tile_y[k], p.tile_x[k]);
        SF_REQUIRE(p.tile_id[k] >= 0 && p.tile_id[k] < p.n_distinct, "sf_tile_blend: crop %d maps to distinct crop %d of %d", k,
                   p.tile_id[k], p.n_distinct);
    }
    const int npx = p.out_h * p.out_w;
    hipLaunchKernelGGL(tile_blend_kernel, dim3(sf::ceil_div(npx, kBlock), n_clips * pairs), dim3(kBlock), 0, (hipStream_t)stream,
                       flows, weights, out, p, pairs);
    return sf::check_launch("sf_tile_blend");
}
