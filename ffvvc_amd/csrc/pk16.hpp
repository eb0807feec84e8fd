// Packed 16-bit and byte-permute vocabulary of the gfx950 kernels: a 32-bit register holds two 16-bit lanes, the even element in
// the low half.  Whatever two kernel files both need lives here; a selector or helper with one user stays in its file.
#pragma once
#include "common.hpp"

namespace vvc355 {

typedef short pk16 __attribute__((ext_vector_type(2)));
typedef unsigned short upk16 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ pk16 pk(uint32_t v) { return __builtin_bit_cast(pk16, v); }
__device__ __forceinline__ uint32_t un(pk16 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ upk16 upk(pk16 v) { return __builtin_bit_cast(upk16, v); }
__device__ __forceinline__ pk16 pk_splat(int v) { return pk16{ (short)v, (short)v }; }
__device__ __forceinline__ upk16 upk_splat(int v) { return upk16{ (unsigned short)v, (unsigned short)v }; }
__device__ __forceinline__ uint32_t pack16(int lo, int hi) { return (uint32_t)(lo & 0xffff) | ((uint32_t)hi << 16); }
__device__ __forceinline__ int pk_lo(pk16 v) { return v.x; }
__device__ __forceinline__ int pk_hi(pk16 v) { return v.y; }

// acc + a.lo * b.lo + a.hi * b.hi on signed halves (v_dot2_i32_i16)
__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int acc) { return __builtin_amdgcn_sdot2(pk(a), pk(b), acc, false); }

// Min / max come in two forms.  pk_min / pk_max leave the lowering to the compiler, which is what the bi-prediction tools were tuned
// with.  The compiler lowers min / max against small constants to compare + select per half, though: where that costs (the packed
// SAO and deblocking filters clip against splatted constants all the time) pk_min_pinned / pk_max_pinned pin the packed
// instructions.  The helpers below them (abs, clip) are the filters' and build on the pinned form.
__device__ __forceinline__ pk16 pk_max(pk16 a, pk16 b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ pk16 pk_min(pk16 a, pk16 b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ pk16 pk_min_pinned(pk16 a, pk16 b) { pk16 r; asm("v_pk_min_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ pk16 pk_max_pinned(pk16 a, pk16 b) { pk16 r; asm("v_pk_max_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ pk16 pk_abs(pk16 v) { return pk_max_pinned(v, pk_splat(0) - v); }
__device__ __forceinline__ pk16 pk_clip(pk16 v, pk16 lo, pk16 hi) { return pk_max_pinned(pk_min_pinned(v, hi), lo); }
__device__ __forceinline__ pk16 pk_clip_sym(pk16 v, int lim) { return pk_clip(v, pk_splat(-lim), pk_splat(lim)); }
__device__ __forceinline__ pk16 pk_sel(bool c, pk16 a, pk16 b) { return pk(c ? un(a) : un(b)); }
__device__ __forceinline__ pk16 pk_d2(pk16 a, pk16 b, pk16 c) { return pk_abs(a - b - b + c); }
__device__ __forceinline__ pk16 pk_sar(pk16 v, int n) { return v >> pk_splat(n); }

// ---- named v_perm_b32 selectors: one instruction each, whatever the halves that are not picked hold
// bytes 0, 1 of v -> the two 16-bit lanes (byte 0 in the low lane), zero-extended
__device__ __forceinline__ uint32_t widen_lo(uint32_t v) { return __builtin_amdgcn_perm(0, v, 0x0c010c00u); }
// bytes 2, 3 of v -> the two 16-bit lanes (byte 2 in the low lane), zero-extended
__device__ __forceinline__ uint32_t widen_hi(uint32_t v) { return __builtin_amdgcn_perm(0, v, 0x0c030c02u); }
// the low bytes of four 16-bit lanes: a's lanes -> bytes 0, 1, b's lanes -> bytes 2, 3 (the inverse of widen_lo / widen_hi)
__device__ __forceinline__ uint32_t narrow4(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x06040200u); }
// (low half of a) | (low half of b) << 16
__device__ __forceinline__ uint32_t pk_ll(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); }
// the same written so that wave-uniform operands stay on the scalar unit
__device__ __forceinline__ uint32_t upk_ll(uint32_t a, uint32_t b) { return (a & 0xffffu) | (b << 16); }
__device__ __forceinline__ uint32_t pk_l0(uint32_t a) { return a & 0xffffu; }
__device__ __forceinline__ uint32_t pk_0l(uint32_t a) { return a << 16; }
// (high half of a) | (high half of b) << 16
__device__ __forceinline__ uint32_t pk_hh(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }
// half h of a | (half h of b) << 16, h = 0 (pk_ll) or 1 (pk_hh) known only at run time: one permute with a selected selector
__device__ __forceinline__ uint32_t pk_half_pair(uint32_t a, uint32_t b, int h) { return __builtin_amdgcn_perm(b, a, h ? 0x07060302u : 0x05040100u); }
// (low half of lo_src) | (high half of hi_src), both where they were
__device__ __forceinline__ uint32_t lo_hi(uint32_t lo_src, uint32_t hi_src) { return __builtin_amdgcn_perm(hi_src, lo_src, 0x07060100u); }
// (high half of a) | (low half of b) << 16
__device__ __forceinline__ uint32_t hi_lo(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x05040302u); }
// the low half of v in both halves
__device__ __forceinline__ uint32_t pk_dup_lo(uint32_t v) { return __builtin_amdgcn_perm(0, v, 0x01000100u); }

// 8 consecutive samples as four registers of two 16-bit samples each, whatever the storage type
template <int BD> __device__ __forceinline__ void load8_pk(const typename Px<BD>::type *p, uint32_t (&d)[4])
{
    if (BD > 8) {
        const uint4 q = gld<uint4>(p);
        d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    } else {
        const uint2 q = gld<uint2>(p);
        d[0] = widen_lo(q.x); d[1] = widen_hi(q.x);
        d[2] = widen_lo(q.y); d[3] = widen_hi(q.y);
    }
}

} // namespace vvc355
