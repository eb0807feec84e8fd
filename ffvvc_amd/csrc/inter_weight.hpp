// What the inter stage drivers (inter_frame.hip, inter_cu.hip) share: the decoder's MvField as the kernels read it, and the weighted
// sample prediction parameters of a block, derive_weight_uni / derive_weight (libavcodec/vvc/vvc_inter.c:129-177).
#pragma once
#include "common.hpp"
#include "../../include/vvc_mi355.h"

namespace vvc355 {

struct MvFieldDev { int32_t mv[2][2]; int8_t ref_idx[2]; uint8_t hpel_if_idx, bcw_idx, pred_flag, ciip_flag, pad_[2]; };
static_assert(sizeof(MvFieldDev) == 24, "MvField layout (vvc_ctu.h:195-202)");
static_assert(sizeof(MvFieldDev) == sizeof(vvc355_mvfield), "vvc355_mvfield layout");

// The job fields weight_flag, denom, w0, w1, o0, o1 of component c for motion mv in slice sl: derive_weight for bi-predicted motion
// (pred_flag 3), derive_weight_uni otherwise.  Fields the reference leaves unset stay 0.
struct PredWeight { int16_t denom, w0, w1, o0, o1; uint8_t flag; };
__device__ __forceinline__ PredWeight derive_pred_weight(const vvc355_inter_slice *sl, const MvFieldDev &mv, int c, bool dmvr_flag, bool ciip_flag)
{
    PredWeight p = {};
    if (mv.pred_flag == 3) {
        // derive_weight (:149-177)
        const int weight_flag = sl->weighted_pred || (sl->weighted_bipred && !dmvr_flag);
        if ((weight_flag || mv.bcw_idx) && !(mv.bcw_idx && ciip_flag)) {
            const int bcw_w_lut[5] = { 4, 5, 3, 10, -2 };               // vvc_inter.c:29
            p.flag = 1;
            if (mv.bcw_idx) {
                p.denom = 2; p.w1 = (int16_t)bcw_w_lut[mv.bcw_idx]; p.w0 = (int16_t)(8 - p.w1);
            } else {
                p.denom = sl->log2_denom[c > 0];
                p.w0 = sl->weight[0][c][mv.ref_idx[0]]; p.w1 = sl->weight[1][c][mv.ref_idx[1]];
                p.o0 = sl->offset[0][c][mv.ref_idx[0]]; p.o1 = sl->offset[1][c][mv.ref_idx[1]];
            }
        }
    } else if (sl->weighted_pred || sl->weighted_bipred) {
        // derive_weight_uni (:129-146)
        const int lx = mv.pred_flag - 1;
        p.flag = 1;
        p.denom = sl->log2_denom[c > 0];
        p.w0 = sl->weight[lx][c][mv.ref_idx[lx]];
        p.o0 = sl->offset[lx][c][mv.ref_idx[lx]];
    }
    return p;
}

template <typename Job> __device__ __forceinline__ void set_pred_weight(Job &j, const PredWeight &p)
{
    j.weight_flag = p.flag;
    j.denom = p.denom; j.w0 = p.w0; j.w1 = p.w1; j.o0 = p.o0; j.o1 = p.o1;
}

} // namespace vvc355
