// The weight-stream ring of the fused chain kernels (ffn_pair.hip, sk_tail.hip, temporal.hip, mask_upsample.hip), and the two
// compile-time helpers every kernel with counted DMA waits needs (gemm_bstat.hip takes only those: its rings are its own).
//
// A chain kernel's weights are ONE host-packed stream of 1-KB MFMA fragments in consumption order.  The workgroup's waves pull it
// L2 -> LDS by DMA (buffer load to LDS), a stage of S fragments at a time, through a ring of RING stage-sized slots: while the
// MFMAs read stage gs out of its slot, stages gs + 1 .. gs + RING - 1 are in flight or landed, and ONE barrier per stage hands the
// slot just read to the request of stage gs + RING.
#pragma once
#include "sf_common.h"

#include <type_traits>

namespace sf {

template <int N>
__device__ __forceinline__ void wait_vm() {                 // s_waitcnt vmcnt(N) only (expcnt / lgkmcnt untouched)
    __builtin_amdgcn_s_waitcnt((N & 15) | 0x0F70 | ((N >> 4) << 14));
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {          // f(integral_constant<int, I>), ..., f(integral_constant<int, N - 1>)
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// S = fragments per stage, RING = slots, NW = waves of the workgroup (wave w moves pieces w, w + NW, ... of every stage).
// The kernel owns the LDS array (RING * S KB, 1-KB aligned) and hands over its base; per stage it runs
//     const char* sp = ring.begin();   ... MFMAs on *(f16x8*)(sp + i * 1024), i < S ...   ring.end();
// and, after the last stage, ring.drain() before the LDS is reused or released.
template <int S, int RING, int NW>
struct WeightRing {
    static_assert(RING >= 2 && S % NW == 0, "a stage is split evenly over the waves");
    static constexpr int kStage = S * 1024;
    static constexpr int kPieces = S / NW;                   // 1-KB pieces a wave moves per stage

    typedef __attribute__((address_space(3))) char* lds_ptr;

    __amdgpu_buffer_rsrc_t rw;
    lds_ptr lds;                                              // (an LDS-space pointer, not a generic one: hipcc then compiles the
                                                              // kernels exactly as with the ring written out in each of them)
    int last_stage, wave, lane;
    int gs = 0, slot = 0;                                     // stage being read, its slot

    // stage s = bytes [s * kStage, (s + 1) * kStage) of the stream; `bytes` is a whole number of stages (< 2^30, host-checked)
    __device__ __forceinline__ WeightRing(const void* stream, int64_t bytes, char* lds_base, int wave_, int lane_)
        : rw(__builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(stream), 0, (int)bytes, 0x00020000)), lds((lds_ptr)lds_base),
          last_stage((int)(bytes / kStage) - 1), wave(wave_), lane(lane_) {}

    // This wave's pieces of stage s into slot sl.  Stages requested past the end of the stream -- begin() keeps the request count
    // per stage constant, so that the counted wait of end() sees the same queue every trip -- re-read the LAST stage into a slot
    // nobody reads any more: the stage offset travels in the scalar offset, which the raw-buffer range check of gfx9 does not
    // cover, so "out of range: zeros" must not be relied on.
    __device__ __forceinline__ void issue(int s, int sl) const {
        const int sc = min(s, last_stage);
#pragma unroll
        for (int i = 0; i < kPieces; ++i) {
            const int piece = wave + NW * i;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, lds + sl * kStage + piece * 1024, 16,
                                                     lane * 16, sc * kStage + piece * 1024, 0, 0);
        }
    }

    // the first RING - 1 stages
    __device__ __forceinline__ void prologue() const {
#pragma unroll
        for (int i = 0; i < RING - 1; ++i) issue(i, i);
    }

    // Requests stage gs + RING - 1 into the slot every wave finished reading before the barrier that ended the previous stage;
    // returns this lane's 16 bytes of fragment 0 of the current stage (fragment i: + i * 1024).
    __device__ __forceinline__ const char* begin() const {
        issue(gs + RING - 1, slot == 0 ? RING - 1 : slot - 1);
        return (const char*)(lds + slot * kStage + lane * 16);
    }

    // Every fragment read of this stage must have EXECUTED before the barrier: the slot is refilled by whichever wave passes the
    // barrier first, and a read that was only issued (hipcc sinks the last MFMAs and their lgkmcnt waits below the s_barrier --
    // the builtin is no memory barrier to it) then races with the refill's DMA.  Seen as run-to-run differences
    // (tests/test_gpu_ffn_pair.py::test_ffn_pair_is_deterministic); the explicit drain removed them.
    __device__ __forceinline__ void end() {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        wait_vm<kPieces * (RING - 2)>();                     // this wave's pieces of the NEXT stage have landed (later ones fly on) ...
        __builtin_amdgcn_s_barrier();                        // ... everyone's; nobody reads this stage's slot any more
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        ++gs;
        slot = (slot == RING - 1) ? 0 : slot + 1;
    }

    // pieces requested past the end must land before the LDS is reused or released
    __device__ __forceinline__ void drain() const { wait_vm<0>(); }
};

}  // namespace sf
