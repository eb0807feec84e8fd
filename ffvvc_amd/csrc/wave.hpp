// Wave-level synchronisation and cross-lane moves shared by the gfx950 kernels.
#pragma once
#include "common.hpp"

namespace vvc355 {

// The lanes of a wave hand data to each other through LDS: the fence orders the accesses, the barrier keeps the compiler from moving
// code across the hand-over.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// a group of NT lanes `tid` = 0 .. NT - 1: inside one wave up to 64, the whole workgroup otherwise
template <int NT> __device__ __forceinline__ void group_sync()
{
    if (NT <= 64) wave_sync();
    else __syncthreads();
}

// DPP move with zero fill: lane <- the lane CTRL selects, 0 when that lane does not exist
template <int CTRL> __device__ __forceinline__ int dpp0(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
static constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141;          // quad_perm [1,0,3,2], [2,3,0,1]
static constexpr int kDppShr1 = 0x111, kDppShr2 = 0x112, kDppShl1 = 0x101, kDppQuad2 = 0xAA;   // quad_perm [2,2,2,2]
static constexpr int kDppShr4 = 0x114, kDppShr8 = 0x118;                                 // row_shr:4, row_shr:8

// a value of lane `src` (any lane, per lane): ds_bpermute, every lane of the wave active
__device__ __forceinline__ int lane_get(int v, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, v); }

} // namespace vvc355
