// The interpolation filters of the motion-compensation kernels: the tables, the read of one tap and the packed tap registers.  What
// mc_fused.hip and the two kernel headers it includes (mc_tools.hpp, mc_chroma_quad.hpp) share.
#pragma once
#include "common.hpp"
#include "pk16.hpp"

namespace vvc355 {

#define VVC355_TABLE(type, name, count) __device__ static const type d_tab_##name[count]
#include "tables.inc"
#undef VVC355_TABLE

__device__ __forceinline__ int tap_of(uint32_t lo, uint32_t hi, int k)      // signed byte k of the 8-byte tap vector
{
    const uint32_t v = k < 4 ? lo : hi;
    return (int)(int8_t)(v >> ((k & 3) * 8));
}

// Two adjacent outputs of an NTAP-tap filter from aligned sample pairs d[m] = (p[2m], p[2m+1]):
// out0 = sum f[k] p[k], out1 = sum f[k] p[k+1]; the pair beyond the last tap meets a zero.
template <int NTAP> struct Taps {
    static constexpr int NE = NTAP / 2, NO = NTAP / 2 + 1;
    uint32_t e[NE];     // (f0,f1) (f2,f3) ...
    uint32_t o[NO];     // (0,f0) (f1,f2) ... (f_last,0)
    __device__ __forceinline__ void set(uint32_t lo, uint32_t hi)
    {
        int f[NTAP];
#pragma unroll
        for (int k = 0; k < NTAP; k++) f[k] = tap_of(lo, hi, k);
#pragma unroll
        for (int m = 0; m < NE; m++) e[m] = pack16(f[2 * m], f[2 * m + 1]);
        o[0] = pack16(0, f[0]);
#pragma unroll
        for (int m = 1; m < NE; m++) o[m] = pack16(f[2 * m - 1], f[2 * m]);
        o[NE] = pack16(f[NTAP - 1], 0);
    }
    __device__ __forceinline__ void apply(const uint32_t (&d)[NO], int &out0, int &out1) const
    {
        int a = 0, b = 0;
#pragma unroll
        for (int m = 0; m < NE; m++) a = dot2(d[m], e[m], a);
#pragma unroll
        for (int m = 0; m < NO; m++) b = dot2(d[m], o[m], b);
        out0 = a; out1 = b;
    }
};

} // namespace vvc355
