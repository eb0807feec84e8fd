// The per-sample tail of itransform (vvc_intra.c:449-475), shared by the chroma residual stage (intra.hip) and the transform epilogue of
// vvc355_inter_tb_pass (itx.hip).
#pragma once
#include "common.hpp"

namespace vvc355 {

// One residual sample on its way to add_residual.  joint as vvc355_recon_cmd.joint: bit 0 = pred_residual_joint (vvcdsp_template.c:65) with
// bit 1 the negative sign and bit 2 the shift; bit 3 = lmcs_scale_chroma's arithmetic (vvc_intra_template.c:431-447) with the unit's scale,
// applied after the sign / shift as add_residual_for_joint_coding_chroma does (vvc_intra.c:180-182).
template <int BD> __device__ __forceinline__ int resid_sample(int r, int joint, int scale)
{
    if (joint & 1)
        r = (r * ((joint & 2) ? -1 : 1)) >> ((joint >> 2) & 1);
    if (joint & 8) {
        const int c = clip_intp2(r, BD);
        r = c > 0 ? (c * scale + (1 << 10)) >> 11 : -((-c * scale + (1 << 10)) >> 11);
    }
    return r;
}

} // namespace vvc355
