/*
 * oracle/ref_shim.c — thin C surface over the reference decoder's own VVCDSPContext.
 *
 * TEST INFRASTRUCTURE ONLY.  Built by `make -C oracle ref` against the reference's static libraries into
 * oracle/_ref/libvvcref.so (never committed).  It exports one ref_<slot> per leaf slot with exactly the
 * orc_<slot> signature of vvc_oracle.h (leading `bd`, leading table indices), so the same ctypes table binds the
 * oracle, the product and the reference, plus the non-static helpers the oracle restates.
 *
 * The slots that take a populated VVCLocalContext (intra.intra_pred, intra.intra_cclm_pred, intra.lmcs_scale_chroma), the
 * availability functions and vvc_intra.c's static dequant / derive_transform_type / ilfnst_transform are in ref_shim_intra.c, the
 * library's second translation unit.  Not covered: the reference's callers (ff_vvc_reconstruct, the inter / filter drivers), which the
 * oracle restates as block and frame passes.
 */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "libavcodec/vvc/vvc_ctu.h"
#include "libavcodec/vvc/vvc_intra.h"
#include "libavcodec/vvc/vvc_itx_1d.h"
#include "libavcodec/vvc/vvcdsp.h"

#define REF_API __attribute__((visibility("default")))

static VVCDSPContext ctx[3];

__attribute__((constructor)) static void ref_init(void)
{
    for (int i = 0; i < 3; i++)
        ff_vvc_dsp_init(&ctx[i], 8 + 2 * i);
}

static const VVCDSPContext *C(int bd) { return &ctx[(bd - 8) >> 1]; }

/* table index of a block width: log2(width) - 1 */
static int wlog(int width) { int l = 0; while ((2 << l) < width) l++; return l > 6 ? 6 : l; }
/* SAO width class: 8, 16, 32, 48, ... 128 samples, the class of the width rounded up to a multiple of 8 (as the caller, vvc_filter.c, picks it) */
static int sao_class(int width) { const int k = ((width + 7) >> 3) - 1; return k < 2 ? k : (k >> 1) + 1; }

/* ---- in-loop filters ---- */
REF_API void ref_lmcs_filter(int bd, uint8_t *dst, ptrdiff_t dst_stride, int width, int height, const uint8_t *lut)
{
    C(bd)->lmcs.filter(dst, dst_stride, width, height, lut);
}
REF_API void ref_alf_filter_luma(int bd, uint8_t *dst, ptrdiff_t dst_stride, const uint8_t *src, ptrdiff_t src_stride,
    int width, int height, const int16_t *filter, const int16_t *clip, int vb_pos)
{
    C(bd)->alf.filter[0](dst, dst_stride, src, src_stride, width, height, filter, clip, vb_pos);
}
REF_API void ref_alf_filter_chroma(int bd, uint8_t *dst, ptrdiff_t dst_stride, const uint8_t *src, ptrdiff_t src_stride,
    int width, int height, const int16_t *filter, const int16_t *clip, int vb_pos)
{
    C(bd)->alf.filter[1](dst, dst_stride, src, src_stride, width, height, filter, clip, vb_pos);
}
REF_API void ref_alf_filter_cc(int bd, uint8_t *dst, ptrdiff_t dst_stride, const uint8_t *luma, ptrdiff_t luma_stride,
    int width, int height, int hs, int vs, const int16_t *filter, int vb_pos)
{
    C(bd)->alf.filter_cc(dst, dst_stride, luma, luma_stride, width, height, hs, vs, filter, vb_pos);
}
REF_API void ref_alf_classify(int bd, int *class_idx, int *transpose_idx, const uint8_t *src, ptrdiff_t src_stride,
    int width, int height, int vb_pos, int *gradient_tmp)
{
    C(bd)->alf.classify(class_idx, transpose_idx, src, src_stride, width, height, vb_pos, gradient_tmp);
}
REF_API void ref_alf_recon_coeff_and_clip(int bd, int16_t *coeff, int16_t *clip, const int *class_idx, const int *transpose_idx,
    int size, const int16_t *coeff_set, const uint8_t *clip_idx_set, const uint8_t *class_to_filt)
{
    C(bd)->alf.recon_coeff_and_clip(coeff, clip, class_idx, transpose_idx, size, coeff_set, clip_idx_set, class_to_filt);
}
REF_API void ref_sao_band_filter(int bd, uint8_t *dst, const uint8_t *src, ptrdiff_t dst_stride, ptrdiff_t src_stride,
    const int16_t *sao_offset_val, int sao_left_class, int width, int height)
{
    C(bd)->sao.band_filter[sao_class(width)](dst, src, dst_stride, src_stride, sao_offset_val, sao_left_class, width, height);
}
REF_API void ref_sao_edge_filter(int bd, uint8_t *dst, const uint8_t *src, ptrdiff_t dst_stride,
    const int16_t *sao_offset_val, int eo, int width, int height)
{
    C(bd)->sao.edge_filter[sao_class(width)](dst, src, dst_stride, sao_offset_val, eo, width, height);
}
REF_API void ref_sao_edge_restore(int bd, int variant, uint8_t *dst, const uint8_t *src, ptrdiff_t dst_stride, ptrdiff_t src_stride,
    const int16_t *offset_val, int eo_class, const int *borders, int width, int height,
    const uint8_t *vert_edge, const uint8_t *horiz_edge, const uint8_t *diag_edge)
{
    SAOParams sao;
    memset(&sao, 0, sizeof(sao));
    for (int c = 0; c < 3; c++) {               /* the same parameters in every component; the slot is called with c_idx 0 */
        memcpy(sao.offset_val[c], offset_val, sizeof(sao.offset_val[c]));
        sao.eo_class[c] = eo_class;
        sao.type_idx[c] = SAO_EDGE;
    }
    C(bd)->sao.edge_restore[variant](dst, src, dst_stride, src_stride, &sao, borders, width, height, 0, vert_edge, horiz_edge, diag_edge);
}
REF_API void ref_lf_filter_luma(int bd, int dir, uint8_t *pix, ptrdiff_t stride, const int32_t *beta, const int32_t *tc,
    const uint8_t *no_p, const uint8_t *no_q, const uint8_t *max_len_p, const uint8_t *max_len_q, int hor_ctu_edge)
{
    C(bd)->lf.filter_luma[dir](pix, stride, beta, tc, no_p, no_q, max_len_p, max_len_q, hor_ctu_edge);
}
REF_API void ref_lf_filter_chroma(int bd, int dir, uint8_t *pix, ptrdiff_t stride, const int32_t *beta, const int32_t *tc,
    const uint8_t *no_p, const uint8_t *no_q, const uint8_t *max_len_p, const uint8_t *max_len_q, int shift)
{
    C(bd)->lf.filter_chroma[dir](pix, stride, beta, tc, no_p, no_q, max_len_p, max_len_q, shift);
}
REF_API int ref_lf_ladf_level(int bd, int dir, const uint8_t *pix, ptrdiff_t stride)
{
    return C(bd)->lf.ladf_level[dir](pix, stride);
}

/* ---- inter prediction ---- */
REF_API void ref_put(int bd, int chroma, int vfrac, int hfrac, int16_t *dst, const uint8_t *src, ptrdiff_t src_stride,
    int height, const int8_t *hf, const int8_t *vf, int width)
{
    C(bd)->inter.put[chroma][wlog(width)][vfrac][hfrac](dst, src, src_stride, height, hf, vf, width);
}
REF_API void ref_put_uni(int bd, int chroma, int vfrac, int hfrac, uint8_t *dst, ptrdiff_t dst_stride,
    const uint8_t *src, ptrdiff_t src_stride, int height, const int8_t *hf, const int8_t *vf, int width)
{
    C(bd)->inter.put_uni[chroma][wlog(width)][vfrac][hfrac](dst, dst_stride, src, src_stride, height, hf, vf, width);
}
REF_API void ref_put_uni_w(int bd, int chroma, int vfrac, int hfrac, uint8_t *dst, ptrdiff_t dst_stride,
    const uint8_t *src, ptrdiff_t src_stride, int height, int denom, int wx, int ox,
    const int8_t *hf, const int8_t *vf, int width)
{
    C(bd)->inter.put_uni_w[chroma][wlog(width)][vfrac][hfrac](dst, dst_stride, src, src_stride, height, denom, wx, ox, hf, vf, width);
}
REF_API void ref_avg(int bd, uint8_t *dst, ptrdiff_t dst_stride, const int16_t *src0, const int16_t *src1, int width, int height)
{
    C(bd)->inter.avg(dst, dst_stride, src0, src1, width, height);
}
REF_API void ref_w_avg(int bd, uint8_t *dst, ptrdiff_t dst_stride, const int16_t *src0, const int16_t *src1, int width, int height,
    int denom, int w0, int w1, int o0, int o1)
{
    C(bd)->inter.w_avg(dst, dst_stride, src0, src1, width, height, denom, w0, w1, o0, o1);
}
REF_API void ref_put_ciip(int bd, uint8_t *dst, ptrdiff_t dst_stride, int width, int height,
    const uint8_t *inter, ptrdiff_t inter_stride, int intra_weight)
{
    C(bd)->inter.put_ciip(dst, dst_stride, width, height, inter, inter_stride, intra_weight);
}
REF_API void ref_put_gpm(int bd, uint8_t *dst, ptrdiff_t dst_stride, int width, int height,
    const int16_t *src0, const int16_t *src1, const uint8_t *weights, int step_x, int step_y)
{
    C(bd)->inter.put_gpm(dst, dst_stride, width, height, src0, src1, weights, step_x, step_y);
}
REF_API void ref_bdof_fetch_samples(int bd, int16_t *dst, const uint8_t *src, ptrdiff_t src_stride, int x_frac, int y_frac,
    int width, int height)
{
    C(bd)->inter.bdof_fetch_samples(dst, src, src_stride, x_frac, y_frac, width, height);
}
REF_API void ref_fetch_samples(int bd, int16_t *dst, const uint8_t *src, ptrdiff_t src_stride, int x_frac, int y_frac)
{
    C(bd)->inter.fetch_samples(dst, src, src_stride, x_frac, y_frac);
}
REF_API void ref_prof_grad_filter(int bd, int16_t *gradient_h, int16_t *gradient_v, ptrdiff_t gradient_stride,
    const int16_t *src, ptrdiff_t src_stride, int width, int height, int pad)
{
    C(bd)->inter.prof_grad_filter(gradient_h, gradient_v, gradient_stride, src, src_stride, width, height, pad);
}
REF_API void ref_apply_prof(int bd, int16_t *dst, const int16_t *src, const int16_t *diff_mv_x, const int16_t *diff_mv_y)
{
    C(bd)->inter.apply_prof(dst, src, diff_mv_x, diff_mv_y);
}
REF_API void ref_apply_prof_uni(int bd, uint8_t *dst, ptrdiff_t dst_stride, const int16_t *src,
    const int16_t *diff_mv_x, const int16_t *diff_mv_y)
{
    C(bd)->inter.apply_prof_uni(dst, dst_stride, src, diff_mv_x, diff_mv_y);
}
REF_API void ref_apply_prof_uni_w(int bd, uint8_t *dst, ptrdiff_t dst_stride, const int16_t *src,
    const int16_t *diff_mv_x, const int16_t *diff_mv_y, int denom, int wx, int ox)
{
    C(bd)->inter.apply_prof_uni_w(dst, dst_stride, src, diff_mv_x, diff_mv_y, denom, wx, ox);
}
REF_API void ref_apply_bdof(int bd, uint8_t *dst, ptrdiff_t dst_stride, int16_t *src0, int16_t *src1, int block_w, int block_h)
{
    C(bd)->inter.apply_bdof(dst, dst_stride, src0, src1, block_w, block_h);
}
REF_API int ref_sad(const int16_t *src0, const int16_t *src1, int dx, int dy, int block_w, int block_h)
{
    return ctx[0].inter.sad(src0, src1, dx, dy, block_w, block_h);
}
REF_API void ref_dmvr(int bd, int vfrac, int hfrac, int16_t *dst, const uint8_t *src, ptrdiff_t src_stride, int height,
    intptr_t mx, intptr_t my, int width)
{
    C(bd)->inter.dmvr[vfrac][hfrac](dst, src, src_stride, height, mx, my, width);
}

/* ---- inverse transform + residual ---- */
REF_API int ref_itx(int trh, int trv, int log2_w, int log2_h, int *coeffs, size_t nzw, size_t nzh,
    intptr_t log2_transform_range, intptr_t bd)
{
    if (trh < 0 || trh >= N_TX_TYPE || trv < 0 || trv >= N_TX_TYPE || log2_w < 0 || log2_w >= N_TX_SIZE || log2_h < 0 || log2_h >= N_TX_SIZE)
        return -1;
    if (!C((int)bd)->itx.itx[trh][trv][log2_w][log2_h])
        return -1;
    C((int)bd)->itx.itx[trh][trv][log2_w][log2_h](coeffs, nzw, nzh, log2_transform_range, bd);
    return 0;
}
REF_API void ref_add_residual(int bd, uint8_t *dst, const int *res, int width, int height, ptrdiff_t stride)
{
    C(bd)->itx.add_residual(dst, res, width, height, stride);
}
REF_API void ref_add_residual_joint(int bd, uint8_t *dst, const int *res, int width, int height, ptrdiff_t stride, int c_sign, int shift)
{
    C(bd)->itx.add_residual_joint(dst, res, width, height, stride, c_sign, shift);
}
REF_API void ref_pred_residual_joint(int *buf, int width, int height, int c_sign, int shift)
{
    ctx[0].itx.pred_residual_joint(buf, width, height, c_sign, shift);
}
REF_API void ref_transform_bdpcm(int *coeffs, int width, int height, int vertical, int log2_transform_range)
{
    ctx[0].itx.transform_bdpcm(coeffs, width, height, vertical, log2_transform_range);
}
REF_API void ref_inv_lfnst_1d(int *v, const int *u, int no_zero_size, int n_tr_s, int pred_mode_intra, int lfnst_idx,
    int log2_transform_range)
{
    ff_vvc_inv_lfnst_1d(v, u, no_zero_size, n_tr_s, pred_mode_intra, lfnst_idx, log2_transform_range);
}
/* type: 0 DCT2, 1 DST7, 2 DCT8; returns -1 when the reference has no 1-D kernel of that type and size */
REF_API int ref_inv_tx_1d(int type, int n, int *coeffs, ptrdiff_t stride, size_t nz)
{
    static const vvc_itx_1d_fn fn[3][7] = {
        { ff_vvc_inv_dct2_1, ff_vvc_inv_dct2_2, ff_vvc_inv_dct2_4, ff_vvc_inv_dct2_8, ff_vvc_inv_dct2_16, ff_vvc_inv_dct2_32, ff_vvc_inv_dct2_64 },
        { ff_vvc_inv_dst7_1, NULL, ff_vvc_inv_dst7_4, ff_vvc_inv_dst7_8, ff_vvc_inv_dst7_16, ff_vvc_inv_dst7_32, NULL },
        { ff_vvc_inv_dct8_1, NULL, ff_vvc_inv_dct8_4, ff_vvc_inv_dct8_8, ff_vvc_inv_dct8_16, ff_vvc_inv_dct8_32, NULL },
    };
    int l = 0;
    while ((1 << l) < n) l++;
    if (type < 0 || type > 2 || l > 6 || (1 << l) != n || !fn[type][l])
        return -1;
    fn[type][l](coeffs, stride, nz);
    return 0;
}

/* ---- intra leaf predictors (stride in pixels) and mode helpers ---- */
REF_API void ref_pred_planar(int bd, uint8_t *src, const uint8_t *top, const uint8_t *left, int w, int h, ptrdiff_t stride)
{
    C(bd)->intra.pred_planar(src, top, left, w, h, stride);
}
REF_API void ref_pred_dc(int bd, uint8_t *src, const uint8_t *top, const uint8_t *left, int w, int h, ptrdiff_t stride)
{
    C(bd)->intra.pred_dc(src, top, left, w, h, stride);
}
REF_API void ref_pred_v(int bd, uint8_t *src, const uint8_t *top, int w, int h, ptrdiff_t stride)
{
    C(bd)->intra.pred_v(src, top, w, h, stride);
}
REF_API void ref_pred_h(int bd, uint8_t *src, const uint8_t *left, int w, int h, ptrdiff_t stride)
{
    C(bd)->intra.pred_h(src, left, w, h, stride);
}
REF_API void ref_pred_angular_v(int bd, uint8_t *src, const uint8_t *top, const uint8_t *left, int w, int h, ptrdiff_t stride,
    int c_idx, int mode, int ref_idx, int filter_flag, int need_pdpc)
{
    C(bd)->intra.pred_angular_v(src, top, left, w, h, stride, c_idx, mode, ref_idx, filter_flag, need_pdpc);
}
REF_API void ref_pred_angular_h(int bd, uint8_t *src, const uint8_t *top, const uint8_t *left, int w, int h, ptrdiff_t stride,
    int c_idx, int mode, int ref_idx, int filter_flag, int need_pdpc)
{
    C(bd)->intra.pred_angular_h(src, top, left, w, h, stride, c_idx, mode, ref_idx, filter_flag, need_pdpc);
}
REF_API void ref_pred_mip(int bd, uint8_t *src, const uint8_t *top, const uint8_t *left, int w, int h, ptrdiff_t stride,
    int mode_id, int is_transpose)
{
    C(bd)->intra.pred_mip(src, top, left, w, h, stride, mode_id, is_transpose);
}
REF_API int ref_intra_pred_angle(int mode) { return ff_vvc_intra_pred_angle_derive(mode); }
REF_API int ref_intra_inv_angle(int angle) { return ff_vvc_intra_inv_angle_derive(angle); }
REF_API int ref_intra_nscale(int w, int h, int mode) { return ff_vvc_nscale_derive(w, h, mode); }
REF_API int ref_intra_need_pdpc(int w, int h, int bdpcm_flag, int mode, int ref_idx) { return ff_vvc_need_pdpc(w, h, (uint8_t)bdpcm_flag, mode, ref_idx); }
REF_API int ref_intra_ref_filter_flag(int mode) { return ff_vvc_ref_filter_flag_derive(mode); }
REF_API int ref_intra_mip_size_id(int w, int h) { return ff_vvc_get_mip_size_id(w, h); }
REF_API int ref_intra_wide_angle(int isp_split, int c_idx, int tb_width, int tb_height, int cb_width, int cb_height, int mode)
{
    CodingUnit cu;
    memset(&cu, 0, sizeof(cu));
    cu.isp_split_type = isp_split ? ISP_HOR_SPLIT : ISP_NO_SPLIT;
    cu.cb_width  = cb_width;
    cu.cb_height = cb_height;
    return ff_vvc_wide_angle_mode_mapping(&cu, tb_width, tb_height, c_idx, mode);
}
