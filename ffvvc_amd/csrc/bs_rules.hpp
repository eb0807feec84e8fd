// The boundary-strength rules' helpers, shared by the two kernels that derive bS: deblock_bs_kernel (loopfilter.hip, from the side tables)
// and bs_rec_kernel (bs_rec.hip, from the unit records).  The rules themselves are bs_rules_body.inc.
#pragma once
#include "common.hpp"
#include "../../include/vvc_mi355.h"

namespace vvc355 {

// boundary_strength (vvc_filter.c:308-372): the motion rule between two inter blocks.  pc / pn = reference POC lists of the
// slices the two blocks belong to (int32 [2][32]).
__device__ __forceinline__ bool mv_far(const int32_t *a, const int32_t *b) { return abs(a[0] - b[0]) >= 8 || abs(a[1] - b[1]) >= 8; }

__device__ __forceinline__ int bs_motion(const vvc355_mvfield &c, const vvc355_mvfield &n, const int *pc, const int *pn)
{
    if (c.pred_flag == 3 && n.pred_flag == 3) {
        const int c0 = gld<int>(pc + c.ref_idx[0]), c1 = gld<int>(pc + 32 + c.ref_idx[1]);
        const int n0 = gld<int>(pn + n.ref_idx[0]), n1 = gld<int>(pn + 32 + n.ref_idx[1]);
        if (c0 == n0 && c0 == c1 && n0 == n1)
            return (mv_far(n.mv[0], c.mv[0]) || mv_far(n.mv[1], c.mv[1])) && (mv_far(n.mv[1], c.mv[0]) || mv_far(n.mv[0], c.mv[1]));
        if (n0 == c0 && n1 == c1)
            return mv_far(n.mv[0], c.mv[0]) || mv_far(n.mv[1], c.mv[1]);
        if (n1 == c0 && n0 == c1)
            return mv_far(n.mv[1], c.mv[0]) || mv_far(n.mv[0], c.mv[1]);
        return 1;
    }
    if (c.pred_flag != 3 && n.pred_flag != 3) {
        const bool c_l0 = c.pred_flag & 1, n_l0 = n.pred_flag & 1;
        const int ra = gld<int>(pc + (c_l0 ? c.ref_idx[0] : 32 + c.ref_idx[1]));
        const int rb = gld<int>(pn + (n_l0 ? n.ref_idx[0] : 32 + n.ref_idx[1]));
        if (ra != rb)
            return 1;
        const int ax = c_l0 ? c.mv[0][0] : c.mv[1][0], ay = c_l0 ? c.mv[0][1] : c.mv[1][1];
        const int bx = n_l0 ? n.mv[0][0] : n.mv[1][0], by = n_l0 ? n.mv[0][1] : n.mv[1][1];
        return abs(ax - bx) >= 8 || abs(ay - by) >= 8;
    }
    return 1;
}

__device__ __forceinline__ vvc355_mvfield ld_mvf(const vvc355_mvfield *p)
{
    uint64_t w[3];
#pragma unroll
    for (int i = 0; i < 3; i++) w[i] = gld<uint64_t>((const uint64_t *)p + i);
    vvc355_mvfield r;
    __builtin_memcpy(&r, w, 24);
    return r;
}

} // namespace vvc355
