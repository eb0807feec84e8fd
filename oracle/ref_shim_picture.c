/*
 * oracle/ref_shim_picture.c — prediction, reconstruction and inverse LMCS of a whole picture by the reference's own three calls.
 *
 * TEST INFRASTRUCTURE ONLY, fifth translation unit of oracle/_ref/libvvcref.so (see ref_shim.c).  Project code: it includes the
 * reference's headers from the tree at build time and calls functions the reference exports — ff_vvc_predict_inter, ff_vvc_reconstruct
 * (which calls ff_vvc_predict_ciip for a unit with ciip_flag itself) and ff_vvc_lmcs_filter, ff_videodsp_init — on ONE set of objects:
 * the VVCLocalContext / VVCFrameContext / SPS / PPS / picture header / SliceContexts / CTU table with CodingUnit and TransformUnit lists
 * that mir_recon_build (ref_shim_intra.c) wires from ref_recon_picture's description, completed here with what ref_shim_inter.c gives the
 * inter callers: fc->tab.mvf, fc->ref->tab_dmvr_mvf, the reference lists over the caller's reference planes, slice types and weight
 * tables, the forward and the inverse luma map, and cu->pu of every unit with inter luma, filled from the record at the unit's origin
 * (vvc355_inter_pu, vvc355_affine_cu, vvc355_gpm_cu, vvc355_ciip_cu).
 *
 * No slot of the ff_vvc_dsp_init table is replaced but intra.lmcs_scale_chroma, which mir_recon_build wraps to log the scales the
 * reference caches: intra.intra_pred and inter.put_ciip are the reference's own.
 *
 * Per CTU in raster order, lc->sc switched to the CTU's slice: ff_vvc_predict_inter, ff_vvc_reconstruct.  The planes are then copied to
 * recon_out; after that ff_vvc_lmcs_filter per CTU.  Returns 0, or -1 for what the objects cannot hold: the limits of ref_recon_picture
 * and of the four ref_*_picture entries, a destination that is not the description's planes, a record with no unit at its origin (or of
 * another size, kind or slice, or a second record for one unit), a unit with inter luma and no record, slice flags that disagree.
 */
#include <stdlib.h>
#include <string.h>

#include "libavutil/frame.h"
#include "libavcodec/videodsp.h"
#include "libavcodec/vvc/vvc_ctu.h"
#include "libavcodec/vvc/vvc_inter.h"
#include "libavcodec/vvc/vvc_intra.h"
#include "libavcodec/vvc/vvc_filter.h"

#include "vvc_oracle.h"
#include "../include/vvc_mi355.h"
#include "ref_shim_mir.h"

#define REF_API __attribute__((visibility("default")))
#define PTR(type, addr) ((type *)(uintptr_t)(addr))

_Static_assert(sizeof(MvField) == sizeof(orc_mv_field), "MvField layout");
_Static_assert(sizeof(orc_inter_frame) == sizeof(vvc355_inter_frame), "inter frame layout");

static H266RawPPS raw_pps;
static VVCFrame   cur;
static RefPicList rpl[2];
static VVCFrame   ref_frame[2][16];
static AVFrame    ref_av[2][16];

/* the unit with luma at (x0, y0) of the given size in the CTU that holds it, not yet claimed by a record, of the given slice; or NULL */
static CodingUnit *claim(const MirReconObjs *o, const MirReconPic *p, int x0, int y0, int w, int h, int slice)
{
    const int log2 = p->ctb_log2;
    int rs;

    if (x0 < 0 || y0 < 0 || w < 4 || h < 4 || w > 128 || h > 128 || (x0 & 3) || (y0 & 3) || (w & (w - 1)) || (h & (h - 1)) || x0 + w > p->width ||
        y0 + h > p->height || (x0 >> log2) != ((x0 + w - 1) >> log2) || (y0 >> log2) != ((y0 + h - 1) >> log2))
        return NULL;
    rs = (y0 >> log2) * o->ncx + (x0 >> log2);
    if (PTR(const int16_t, p->slice_idx)[rs] != slice)
        return NULL;
    for (CodingUnit *cu = o->ctus[rs].cus; cu; cu = cu->next)
        if (cu->x0 == x0 && cu->y0 == y0 && cu->tree_type != DUAL_TREE_CHROMA)
            return cu->cb_width == w && cu->cb_height == h && cu->pred_mode == MODE_INTER && !cu->pu.mi.num_sb_x ? cu : NULL;
    return NULL;
}

REF_API int ref_decode_picture(MirReconPic *p, const orc_inter_frame *f, const vvc355_affine_cu *aff, int n_aff, const vvc355_gpm_cu *gpm,
                               int n_gpm, const vvc355_ciip_cu *ciip, int n_ciip, const void *inv_lut, void *const recon_out[3])
{
    const orc_inter_pu *pus = PTR(const orc_inter_pu, f->pus);
    const MvField *mvf = PTR(const MvField, f->mvf);
    const int bd = p->bit_depth, n_comp = p->chroma_format_idc ? 3 : 1;
    const int hs = p->chroma_format_idc == 1 || p->chroma_format_idc == 2, vs = p->chroma_format_idc == 1;
    MirReconObjs o;
    int ret = -1;

    if (f->n_pus < 0 || (f->n_pus && !pus) || n_aff < 0 || (n_aff && !aff) || n_gpm < 0 || (n_gpm && !gpm) || n_ciip < 0 || (n_ciip && !ciip) ||
        !inv_lut || !recon_out || f->width != p->width || f->height != p->height || (f->width & 7) || (f->height & 7) ||
        f->chroma_format_idc != p->chroma_format_idc || f->pixel_shift != (bd > 8) || f->mvf_stride != f->width >> 2 || !f->mvf || !f->refs ||
        !f->slices || !f->dmvr_mvf || !f->lmcs_fwd_lut || f->hs != hs || f->vs != vs)
        return -1;
    for (int c = 0; c < n_comp; c++)
        if (f->dst[c] != p->plane[c] || f->dst_stride[c] != p->stride[c] || !recon_out[c])
            return -1;
    if (mir_recon_build(p, &o, 1))
        return -1;

    /* what ref_shim_inter.c's wire() adds to the picture */
    memset(&raw_pps, 0, sizeof(raw_pps));
    memset(&cur, 0, sizeof(cur));
    memset(rpl, 0, sizeof(rpl));
    memset(ref_frame, 0, sizeof(ref_frame));
    memset(ref_av, 0, sizeof(ref_av));
    o.pps->r             = &raw_pps;
    o.pps->ctb_count     = (uint32_t)o.n_ctb;
    o.pps->min_pu_width  = (uint16_t)(p->width >> 2);
    o.pps->min_pu_height = (uint16_t)(p->height >> 2);
    o.fc->ref            = &cur;
    o.fc->tab.mvf        = PTR(MvField, f->mvf);
    cur.tab_dmvr_mvf     = PTR(MvField, f->dmvr_mvf);
    ref_inter_wire_refs(PTR(const orc_ref_pic, f->refs), n_comp, rpl, ref_frame, ref_av);
    memcpy(o.fc->ps.lmcs.fwd_lut, PTR(const void, f->lmcs_fwd_lut), ((size_t)1 << bd) << (bd > 8));
    memcpy(o.fc->ps.lmcs.inv_lut, inv_lut, ((size_t)1 << bd) << (bd > 8));
    ff_videodsp_init(&o.fc->vdsp, bd);
    for (int s = 0; s < p->n_slices; s++) {
        const int used = o.sh[s].sh_lmcs_used_flag;
        if (ref_inter_wire_slice(PTR(const orc_inter_slice, f->slices) + s, 1, &o.sc[s], &o.sh[s], &raw_pps, rpl) || o.sh[s].sh_lmcs_used_flag != used)
            goto done;
    }

    /* cu->pu from the record at the unit's origin, as the four entries of ref_shim_inter.c fill it */
    for (int u = 0; u < f->n_pus; u++) {
        const orc_inter_pu *r = pus + u;
        CodingUnit *cu = claim(&o, p, r->x0, r->y0, r->cb_width, r->cb_height, r->slice);
        if (!cu || cu->ciip_flag || r->ciip_flag || !r->num_sb_x || !r->num_sb_y || r->cb_width % r->num_sb_x || r->cb_height % r->num_sb_y)
            goto done;
        cu->pu.mi.num_sb_x    = r->num_sb_x;
        cu->pu.mi.num_sb_y    = r->num_sb_y;
        cu->pu.mi.hpel_if_idx = r->hpel_if_idx;
        cu->pu.dmvr_flag      = r->dmvr_flag;
        cu->pu.bdof_flag      = r->bdof_flag;
    }
    for (int u = 0; u < n_aff; u++) {
        const vvc355_affine_cu *r = aff + u;
        CodingUnit *cu = claim(&o, p, r->x0, r->y0, r->cb_width, r->cb_height, r->slice);
        if (!cu || cu->ciip_flag || r->num_sb_x != r->cb_width >> 2 || r->num_sb_y != r->cb_height >> 2 || r->cb_width < 8 || r->cb_height < 8)
            goto done;
        cu->pu.inter_affine_flag = 1;
        cu->pu.mi.num_sb_x  = r->num_sb_x;
        cu->pu.mi.num_sb_y  = r->num_sb_y;
        cu->pu.mi.pred_flag = mvf[(r->y0 >> 2) * f->mvf_stride + (r->x0 >> 2)].pred_flag;
        for (int l = 0; l < 2; l++) {
            cu->pu.cb_prof_flag[l] = (r->prof_flags >> l) & 1;
            memcpy(cu->pu.diff_mv_x[l], r->diff_mv[l][0], sizeof(cu->pu.diff_mv_x[l]));
            memcpy(cu->pu.diff_mv_y[l], r->diff_mv[l][1], sizeof(cu->pu.diff_mv_y[l]));
        }
    }
    for (int u = 0; u < n_gpm; u++) {
        const vvc355_gpm_cu *r = gpm + u;
        CodingUnit *cu = claim(&o, p, r->x0, r->y0, r->cb_width, r->cb_height, r->slice);
        if (!cu || cu->ciip_flag || r->cb_width < 8 || r->cb_height < 8 || r->cb_width > 64 || r->cb_height > 64 || r->cb_width >= 8 * r->cb_height ||
            r->cb_height >= 8 * r->cb_width || r->partition_idx > 63)
            goto done;
        cu->pu.merge_gpm_flag    = 1;
        cu->pu.gpm_partition_idx = r->partition_idx;
        cu->pu.mi.num_sb_x = cu->pu.mi.num_sb_y = 1;               /* not read for such a unit: marks it claimed */
        memcpy(cu->pu.gpm_mv, r->gpm_mv, sizeof(cu->pu.gpm_mv));
        for (int i = 0; i < 2; i++) {
            const MvField *m = &cu->pu.gpm_mv[i];
            if ((m->pred_flag != PF_L0 && m->pred_flag != PF_L1) || m->ref_idx[m->pred_flag - PF_L0] < 0 || m->ref_idx[m->pred_flag - PF_L0] >= 16)
                goto done;
        }
    }
    for (int u = 0; u < n_ciip; u++) {
        const vvc355_ciip_cu *r = ciip + u;
        CodingUnit *cu = claim(&o, p, r->x0, r->y0, r->cb_width, r->cb_height, r->slice);
        if (!cu || !cu->ciip_flag || r->cb_width > 64 || r->cb_height > 64 || r->cb_width * r->cb_height < 64)
            goto done;
        cu->pu.mi.num_sb_x    = 1;
        cu->pu.mi.num_sb_y    = 1;
        cu->pu.mi.hpel_if_idx = r->hpel_if_idx & 1;
    }
    for (int rs = 0; rs < o.n_ctb; rs++) {
        const int s = o.fc->tab.slice_idx[rs];
        if (s < 0 || s >= p->n_slices)
            goto done;
        for (const CodingUnit *cu = o.ctus[rs].cus; cu; cu = cu->next)
            if (cu->pred_mode == MODE_INTER && cu->tree_type != DUAL_TREE_CHROMA && !cu->pu.mi.num_sb_x)
                goto done;                                          /* inter luma and no prediction unit */
    }

    ret = 0;
    for (int rs = 0; rs < o.n_ctb && !ret; rs++) {
        o.lc->sc = &o.sc[o.fc->tab.slice_idx[rs]];
        ret = ff_vvc_predict_inter(o.lc, rs);
        if (!ret)
            ret = ff_vvc_reconstruct(o.lc, rs, rs % o.ncx, rs / o.ncx);
    }
    if (ret)
        goto done;
    for (int c = 0; c < n_comp; c++)
        memcpy(recon_out[c], PTR(const void, p->plane[c]), (size_t)p->stride[c] * (size_t)(p->height >> (c ? vs : 0)));
    for (int rs = 0; rs < o.n_ctb; rs++) {
        o.lc->sc = &o.sc[o.fc->tab.slice_idx[rs]];
        ff_vvc_lmcs_filter(o.lc, (rs % o.ncx) << p->ctb_log2, (rs / o.ncx) << p->ctb_log2);
    }

done:
    mir_recon_free(&o);
    return ret;
}
