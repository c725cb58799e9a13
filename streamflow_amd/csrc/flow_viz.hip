// Flow colour-wheel images (reference core/utils/flow_viz.py: flow_to_image), the last step of the demo and of the
// submission writers: flows [n][2][h][w] fp32 -> [n][h][w][3] uint8 on the device, instead of a 16 MB copy per 1080p field to the
// host and ~0.3 s of numpy there.
//
// Two kernels.  flow_rad_max_kernel: the largest radius of every field (the reference normalises each call by its own maximum) --
// grid-stride loads, maximum within the wave by shuffles and within the block through LDS, blocks combined by a vector
// atomicMax on the bit pattern (radii are >= 0, so unsigned order is float order; a maximum does not depend on the order of
// combination, so the result is deterministic).  flow_colour_kernel: four consecutive pixels per thread, float4 loads from both
// planes and the 12 output bytes as three aligned dwords; fields whose pixel count is not a multiple of four (or unaligned
// pointers) take scalar loads and, where a thread's 12 bytes are not dword-aligned or run past the end, byte stores.
//
// The arithmetic contract is in include/streamflow_hip.h: fp32 with every operation rounded on its own up to the wheel
// position (FMA contraction is off for this file, as in tile_blend.hip; hipcc's fp32 division and square root are correctly
// rounded and the library keeps subnormals), the angle as the fp64 arctangent rounded once, fp64 from the wheel on, as numpy
// promotes.  -x keeps the sign of zero: v = +0 and v = -0 at u > 0 sit on the two sides of the wheel's one discontinuity.
#include "sf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kWheelN = 55;

// The Middlebury wheel (Baker et al., ICCV 2007): R -> Y -> G -> C -> B -> M -> R in 15 + 6 + 4 + 11 + 13 + 6 steps, five
// entries (R, G, B) per line.
// tests/test_flow_viz_cpu.py checks this table against streamflow_amd.flow_viz.make_colorwheel().
// clang-format off
__device__ const unsigned char kWheel[kWheelN * 3] = {
    255,   0,   0,  255,  17,   0,  255,  34,   0,  255,  51,   0,  255,  68,   0,
    255,  85,   0,  255, 102,   0,  255, 119,   0,  255, 136,   0,  255, 153,   0,
    255, 170,   0,  255, 187,   0,  255, 204,   0,  255, 221,   0,  255, 238,   0,
    255, 255,   0,  213, 255,   0,  170, 255,   0,  128, 255,   0,   85, 255,   0,
     43, 255,   0,    0, 255,   0,    0, 255,  63,    0, 255, 127,    0, 255, 191,
      0, 255, 255,    0, 232, 255,    0, 209, 255,    0, 186, 255,    0, 163, 255,
      0, 140, 255,    0, 116, 255,    0,  93, 255,    0,  70, 255,    0,  47, 255,
      0,  24, 255,    0,   0, 255,   19,   0, 255,   39,   0, 255,   58,   0, 255,
     78,   0, 255,   98,   0, 255,  117,   0, 255,  137,   0, 255,  156,   0, 255,
    176,   0, 255,  196,   0, 255,  215,   0, 255,  235,   0, 255,  255,   0, 255,
    255,   0, 213,  255,   0, 170,  255,   0, 128,  255,   0,  85,  255,   0,  43,
};
// clang-format on

__device__ __forceinline__ bool finite2(float u, float v) {
    return ((__float_as_uint(u) & 0x7fffffffu) < 0x7f800000u) && ((__float_as_uint(v) & 0x7fffffffu) < 0x7f800000u);
}

// np.clip(x, 0, c) by comparison: negative components become 0, -0.0 stays -0.0 (c < 0: no clamp)
__device__ __forceinline__ float clamp_flow(float x, float c) {
    if (c < 0.0f) return x;
    x = x < 0.0f ? 0.0f : x;
    return x > c ? c : x;
}

// squared radius of one pixel for the maximum: 0 for a pixel with a non-finite component.  The correctly rounded square root is
// monotonic, so max sqrt(s) = sqrt(max s) bit for bit: the root is taken once per thread, after its loop.
__device__ __forceinline__ float radius2_or_zero(float u, float v, float clip) {
    if (!finite2(u, v)) return 0.0f;
    u = clamp_flow(u, clip);
    v = clamp_flow(v, clip);
    return u * u + v * v;
}

template <bool kVec>
__global__ __launch_bounds__(kBlock) void flow_rad_max_kernel(const float* __restrict__ flows, float* __restrict__ rad_max, int npx,
                                                              float clip) {
    const int img = blockIdx.y;
    const float* pu = flows + (int64_t)img * 2 * npx;
    const float* pv = pu + npx;
    const int ngroups = (npx + 3) >> 2;
    float m = 0.0f;
    for (int q = blockIdx.x * kBlock + threadIdx.x; q < ngroups; q += gridDim.x * kBlock) {
        const int p = q << 2;
        if constexpr (kVec) {
            const float4 u = *reinterpret_cast<const float4*>(pu + p), v = *reinterpret_cast<const float4*>(pv + p);
            m = fmaxf(m, fmaxf(fmaxf(radius2_or_zero(u.x, v.x, clip), radius2_or_zero(u.y, v.y, clip)),
                               fmaxf(radius2_or_zero(u.z, v.z, clip), radius2_or_zero(u.w, v.w, clip))));
        } else {
            for (int j = 0; j < 4; ++j)
                if (p + j < npx) m = fmaxf(m, radius2_or_zero(pu[p + j], pv[p + j], clip));
        }
    }
    m = sqrtf(m);
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    __shared__ float s_m[kBlock / 64];
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kBlock / 64; ++k) m = fmaxf(m, s_m[k]);
        atomicMax(reinterpret_cast<unsigned int*>(rad_max) + img, __float_as_uint(m));       // m >= +0: unsigned order = float order
    }
}

// one pixel -> its three colour bytes in wheel order (R, G, B), packed into the low 24 bits
__device__ __forceinline__ unsigned int colour_px(float u, float v, float d, float clip, const double* __restrict__ wheel) {
    if (!finite2(u, v)) return 0u;
    u = clamp_flow(u, clip);
    v = clamp_flow(v, clip);
    const float un = u / d, vn = v / d;
    const float rad = sqrtf(un * un + vn * vn);
    const float angle = (float)atan2(-(double)vn, -(double)un);
    const float a = angle / 3.14159274101257324f;                        // (float)M_PI
    const float fk = (a + 1.0f) / 2.0f * 54.0f;                          // in [0, 54]
    const float k0f = floorf(fk);
    const int k0 = (int)k0f;
    const int k1 = k0 + 1 == kWheelN ? 0 : k0 + 1;
    const double f = (double)fk - (double)k0f;
    const double g = 1.0 - f, r = (double)rad;
    const bool inside = rad <= 1.0f;
    unsigned int rgb = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double col = g * wheel[k0 * 3 + c] + f * wheel[k1 * 3 + c];
        col = inside ? 1.0 - r * (1.0 - col) : col * 0.75;
        rgb |= (unsigned int)(int)floor(255.0 * col) << (8 * c);
    }
    return rgb;
}

template <bool kVec>
__global__ __launch_bounds__(kBlock) void flow_colour_kernel(const float* __restrict__ flows, uint8_t* __restrict__ out,
                                                             const float* __restrict__ rad_max, float fixed_rad_max, int npx,
                                                             float clip, int bgr) {
    __shared__ double s_wheel[kWheelN * 3];
    for (int i = threadIdx.x; i < kWheelN * 3; i += kBlock) s_wheel[i] = (double)kWheel[i] / 255.0;
    __syncthreads();
    const int img = blockIdx.y;
    const int q = blockIdx.x * kBlock + threadIdx.x;
    const int p = q << 2;
    if (p >= npx) return;
    const float m = fixed_rad_max >= 0.0f ? fixed_rad_max : rad_max[img];
    const float d = m + 1e-5f;
    const float* pu = flows + (int64_t)img * 2 * npx + p;
    const float* pv = pu + npx;
    uint8_t* o = out + ((int64_t)img * npx + p) * 3;
    const int left = npx - p;                                            // pixels of this thread that exist (>= 1)
    float u[4], v[4];
    if constexpr (kVec) {
        const float4 u4 = *reinterpret_cast<const float4*>(pu), v4 = *reinterpret_cast<const float4*>(pv);
        u[0] = u4.x, u[1] = u4.y, u[2] = u4.z, u[3] = u4.w;
        v[0] = v4.x, v[1] = v4.y, v[2] = v4.z, v[3] = v4.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            u[j] = j < left ? pu[j] : 0.0f;
            v[j] = j < left ? pv[j] : 0.0f;
        }
    }
    unsigned int c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = colour_px(u[j], v[j], d, clip, s_wheel);
        if (bgr) c[j] = ((c[j] & 0xffu) << 16) | (c[j] & 0xff00u) | (c[j] >> 16);
    }
    // 12 bytes c0 c0 c0 c1 | c1 c1 c2 c2 | c2 c3 c3 c3 (little endian)
    const unsigned int w0 = c[0] | (c[1] << 24), w1 = (c[1] >> 8) | (c[2] << 16), w2 = (c[2] >> 16) | (c[3] << 8);
    if (kVec || (left >= 4 && (reinterpret_cast<uintptr_t>(o) & 3u) == 0)) {
        unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
        o4[0] = w0, o4[1] = w1, o4[2] = w2;
    } else {
        const unsigned int w[3] = {w0, w1, w2};
        const int nbytes = (left < 4 ? left : 4) * 3;
#pragma unroll
        for (int b = 0; b < 12; ++b)
            if (b < nbytes) o[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
    }
}

}  // namespace

extern "C" int sf_flow_to_image(const float* flows, uint8_t* out, float* rad_max_ws, int n, int h, int w, float clip_flow,
                                float fixed_rad_max, int bgr, void* stream) {
    SF_REQUIRE(flows && out, "sf_flow_to_image: null argument");
    const bool fixed = fixed_rad_max >= 0.0f;
    SF_REQUIRE(fixed || rad_max_ws, "sf_flow_to_image: rad_max_ws is required without fixed_rad_max");
    SF_REQUIRE(fixed_rad_max == fixed_rad_max && clip_flow == clip_flow, "sf_flow_to_image: NaN clip_flow / fixed_rad_max");
    SF_REQUIRE(n > 0 && h > 0 && w > 0, "sf_flow_to_image: bad shape %d x %d x %d", n, h, w);
    SF_REQUIRE(n <= 65535, "sf_flow_to_image: %d fields in one call (at most 65535)", n);
    SF_REQUIRE((int64_t)h * w < (1 << 30), "sf_flow_to_image: field %d x %d too large", h, w);
    const int npx = h * w, ngroups = (npx + 3) / 4;
    const float clip = clip_flow >= 0.0f ? clip_flow : -1.0f;
    hipStream_t s = (hipStream_t)stream;
    // float4 loads need 16-byte aligned planes, the dword stores 4-byte aligned images
    const bool vec = npx % 4 == 0 && (reinterpret_cast<uintptr_t>(flows) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
    if (!fixed) {
        const int cleared = sf::fill_async("sf_flow_to_image (clear)", rad_max_ws, 0, (int64_t)sizeof(float) * n, s);
        if (cleared != SF_OK) return cleared;
        // at most 256 blocks per field (one per CU): one atomic per block on the field's slot, which all XCDs share
        const dim3 grid(sf::ceil_div(ngroups, kBlock) < 256 ? sf::ceil_div(ngroups, kBlock) : 256, n);
        if (vec) hipLaunchKernelGGL(flow_rad_max_kernel<true>, grid, dim3(kBlock), 0, s, flows, rad_max_ws, npx, clip);
        else hipLaunchKernelGGL(flow_rad_max_kernel<false>, grid, dim3(kBlock), 0, s, flows, rad_max_ws, npx, clip);
        const int st = sf::check_launch("sf_flow_to_image (maximum)");
        if (st != SF_OK) return st;
    }
    const dim3 grid(sf::ceil_div(ngroups, kBlock), n);
    if (vec) hipLaunchKernelGGL(flow_colour_kernel<true>, grid, dim3(kBlock), 0, s, flows, out, rad_max_ws, fixed_rad_max, npx, clip, bgr);
    else hipLaunchKernelGGL(flow_colour_kernel<false>, grid, dim3(kBlock), 0, s, flows, out, rad_max_ws, fixed_rad_max, npx, clip, bgr);
    return sf::check_launch("sf_flow_to_image");
}
