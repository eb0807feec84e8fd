/*
 * oracle/ref_shim_inter.c — the reference's inter prediction callers on whole pictures, driven from the stage drivers' descriptors.
 *
 * TEST INFRASTRUCTURE ONLY, fourth translation unit of oracle/_ref/libvvcref.so (see ref_shim.c).  Project code: it includes the
 * reference's headers from the tree at build time and calls functions the reference exports — ff_vvc_predict_inter (per CTU: pred_regular_blk,
 * pred_affine_blk, pred_gpm_blk with their callers' work: the DMVR search, edge emulation, derive_weight, derive_affine_mvc, the GPM weight
 * addressing, the forward luma map, set_dmvr_info), ff_vvc_dsp_init and ff_videodsp_init — on real VVCLocalContext / VVCFrameContext /
 * VVCSPS / VVCPPS / SliceContext / VVCFrame / AVFrame / CTU / CodingUnit objects.  fc->tab.mvf is the caller's MvField table,
 * fc->ref->tab_dmvr_mvf the caller's dmvr_mvf, rpl[l].ref[i] VVCFrames over the caller's reference planes, fc->frame the caller's
 * destination planes.  One CodingUnit per record, linked per CTU in list order; CTUs are walked in raster order and lc->sc is switched
 * per CTU to that CTU's slice.
 *
 * ref_ciip_picture calls ff_vvc_decode_neighbour per CTU and ff_vvc_predict_ciip per unit, with two slots of its own fc.vvcdsp table
 * replaced by callbacks of this file: intra.intra_pred does nothing, inter.put_ciip copies its `inter` operand into the unit's region of a
 * caller-supplied scratch (the layout vvc355_ciip_frame documents) and stores intra_weight per unit and component.  That is the inter
 * half exactly as the reference hands it to the blend; for luma that is after the forward map.
 *
 * The four entries take the host-address twin of the device descriptors (orc_inter_frame of vvc_oracle.h = vvc355_inter_frame; the
 * affine, GPM and CIIP records of include/vvc_mi355.h) and return 0, or -1 where a picture is outside what the real objects can hold:
 * sizes, a unit that crosses its CTU, two units of one CTU that name different slices (the reference keeps one SliceContext per CTU),
 * a slice with both weighted-prediction switches (a slice is P or B), a CIIP unit in the regular list (ff_vvc_predict_inter skips those),
 * mvf_stride != width / 4, memory.
 *
 * Slice headers.  weighted_pred means IS_P && pps_weighted_pred_flag, weighted_bipred IS_B && pps_weighted_bipred_flag: either PPS flag
 * is set when any slice of the picture has the switch, and each slice gets the type that makes its own pair come out (P, B, or I where
 * both are 0; predict_inter looks at the type nowhere else).  The weights go into sh.pwt (pps_wp_info_in_ph_flag = 0), which holds 15
 * entries per list: ref_idx 15 cannot be weighted by the reference.  Single-threaded: one set of objects, rewired by every call.
 */
#include <stdlib.h>
#include <string.h>

#include "libavutil/frame.h"
#include "libavcodec/videodsp.h"
#include "libavcodec/vvc/vvc_ctu.h"
#include "libavcodec/vvc/vvc_inter.h"

#include "vvc_oracle.h"
#include "../include/vvc_mi355.h"
#include "ref_shim_mir.h"

#define REF_API __attribute__((visibility("default")))
#define PTR(type, addr) ((type *)(uintptr_t)(addr))
#define MAX_SLICES 16
#define MAX_REFS   16

_Static_assert(sizeof(MvField) == sizeof(orc_mv_field), "MvField layout");
_Static_assert(sizeof(orc_inter_frame) == sizeof(vvc355_inter_frame), "inter frame layout");

static VVCLocalContext    lc;
static VVCFrameContext    fc;
static VVCSPS             sps;
static VVCPPS             pps;
static H266RawSPS         raw_sps;
static H266RawPPS         raw_pps;
static AVFrame            frame;
static VVCFrame           cur;
static SliceContext       sc[MAX_SLICES];
static H266RawSliceHeader raw_sh[MAX_SLICES];
static RefPicList         rpl[2];
static VVCFrame           ref_frame[2][MAX_REFS];
static AVFrame            ref_av[2][MAX_REFS];

/* both lists: an entry without a luma plane stays NULL, which pred_get_refs refuses */
void ref_inter_wire_refs(const orc_ref_pic *refs, int n_comp, RefPicList rl[2], VVCFrame fr[2][16], AVFrame av[2][16])
{
    for (int l = 0; l < 2; l++) {
        rl[l].nb_refs = MAX_REFS;
        for (int i = 0; i < MAX_REFS; i++) {
            const orc_ref_pic *rp = refs + l * 16 + i;
            if (!rp->plane[0])
                continue;
            for (int c = 0; c < n_comp; c++) {
                av[l][i].data[c]     = PTR(uint8_t, rp->plane[c]);
                av[l][i].linesize[c] = rp->stride[c];
            }
            fr[l][i].frame = &av[l][i];
            rl[l].ref[i] = &fr[l][i];
        }
    }
}

int ref_inter_wire_slice(const orc_inter_slice *in, int have_lut, SliceContext *s, H266RawSliceHeader *sh, H266RawPPS *rpps, RefPicList *rl)
{
    PredWeightTable *w = &s->sh.pwt;

    if (in->weighted_pred && in->weighted_bipred)
        return -1;
    if (in->lmcs_used && !have_lut)
        return -1;
    s->sh.r = sh;
    s->rpl  = rl;
    sh->sh_slice_type = in->weighted_pred ? VVC_SLICE_TYPE_P : in->weighted_bipred ? VVC_SLICE_TYPE_B : VVC_SLICE_TYPE_I;
    sh->sh_lmcs_used_flag = in->lmcs_used;
    if (in->weighted_pred)
        rpps->pps_weighted_pred_flag = 1;
    if (in->weighted_bipred)
        rpps->pps_weighted_bipred_flag = 1;
    w->log2_denom[0] = in->log2_denom[0];
    w->log2_denom[1] = in->log2_denom[1];
    for (int l = 0; l < 2; l++)
        for (int c = 0; c < 3; c++)
            for (int i = 0; i < MAX_WEIGHTS; i++) {
                w->weight[l][c][i] = in->weight[l][c][i];
                w->offset[l][c][i] = in->offset[l][c][i];
            }
    return 0;
}

/* the picture every entry shares: geometry, planes, MvField tables, reference lists, slice headers, forward map */
static int wire(int bd, const orc_inter_frame *f, int ctb_log2)
{
    const orc_ref_pic *refs = PTR(const orc_ref_pic, f->refs);
    const int n_comp = f->chroma_format_idc ? 3 : 1;

    if ((bd != 8 && bd != 10 && bd != 12) || f->width <= 0 || f->height <= 0 || f->width > 8192 || f->height > 8192 || (f->width & 7) ||
        (f->height & 7) || ctb_log2 < 5 || ctb_log2 > 7 || f->pixel_shift != (bd > 8) || f->mvf_stride != f->width >> 2 || !f->mvf ||
        !f->refs || !f->slices || f->chroma_format_idc > 3 || f->hs > 1 || f->vs > 1 ||
        f->hs != (f->chroma_format_idc == 1 || f->chroma_format_idc == 2) || f->vs != (f->chroma_format_idc == 1))
        return -1;
    memset(&lc, 0, sizeof(lc));
    memset(&fc, 0, sizeof(fc));
    memset(&sps, 0, sizeof(sps));
    memset(&pps, 0, sizeof(pps));
    memset(&raw_sps, 0, sizeof(raw_sps));
    memset(&raw_pps, 0, sizeof(raw_pps));
    memset(&frame, 0, sizeof(frame));
    memset(&cur, 0, sizeof(cur));
    memset(sc, 0, sizeof(sc));
    memset(raw_sh, 0, sizeof(raw_sh));
    memset(rpl, 0, sizeof(rpl));
    memset(ref_frame, 0, sizeof(ref_frame));
    memset(ref_av, 0, sizeof(ref_av));
    sps.r     = &raw_sps;
    pps.r     = &raw_pps;
    fc.ps.sps = &sps;
    fc.ps.pps = &pps;
    fc.frame  = &frame;
    fc.ref    = &cur;
    lc.fc     = &fc;

    raw_sps.sps_chroma_format_idc = f->chroma_format_idc;
    sps.width  = pps.width  = (uint16_t)f->width;
    sps.height = pps.height = (uint16_t)f->height;
    for (int c = 1; c < 3; c++) {
        sps.hshift[c] = f->hs;
        sps.vshift[c] = f->vs;
    }
    sps.bit_depth       = (uint8_t)bd;
    sps.pixel_shift     = bd > 8;
    sps.ctb_log2_size_y = (uint8_t)ctb_log2;
    sps.ctb_size_y      = (uint8_t)(1 << ctb_log2);
    pps.ctb_width     = (uint16_t)((f->width  + (1 << ctb_log2) - 1) >> ctb_log2);
    pps.ctb_height    = (uint16_t)((f->height + (1 << ctb_log2) - 1) >> ctb_log2);
    pps.ctb_count     = (uint32_t)pps.ctb_width * pps.ctb_height;
    pps.min_pu_width  = (uint16_t)(f->width >> 2);
    pps.min_pu_height = (uint16_t)(f->height >> 2);
    for (int c = 0; c < n_comp; c++) {
        if (!f->dst[c])
            return -1;
        frame.data[c]     = PTR(uint8_t, f->dst[c]);
        frame.linesize[c] = f->dst_stride[c];
    }
    fc.tab.mvf       = PTR(MvField, f->mvf);
    cur.tab_dmvr_mvf = PTR(MvField, f->dmvr_mvf);

    ref_inter_wire_refs(refs, n_comp, rpl, ref_frame, ref_av);
    if (f->lmcs_fwd_lut)
        memcpy(fc.ps.lmcs.fwd_lut, PTR(const void, f->lmcs_fwd_lut), ((size_t)1 << bd) << sps.pixel_shift);
    ff_vvc_dsp_init(&fc.vvcdsp, bd);
    ff_videodsp_init(&fc.vdsp, bd);
    return 0;
}

/* slice s of the caller's table -> sc[s]; -1 for a pair of switches no slice type produces */
static int wire_slice(const orc_inter_frame *f, int s, int have_lut)
{
    return ref_inter_wire_slice(PTR(const orc_inter_slice, f->slices) + s, have_lut, &sc[s], &raw_sh[s], &raw_pps, rpl);
}

typedef struct UnitHead { int x0, y0, w, h, slice; } UnitHead;

/* ---- CIIP capture: the two slots of fc.vvcdsp that ref_ciip_picture replaces with callbacks of its own */
static struct {
    const vvc355_ciip_cu *rec;     /* the unit being predicted */
    uint8_t *scratch;
    int32_t *weights;              /* [unit][3] */
    int64_t  scratch_len;          /* pixels */
    int      unit, c, failed;
} cap;

static void ciip_no_intra(const VVCLocalContext *l, int x0, int y0, int w, int h, int c_idx)
{
}

/* put_ciip as the reference calls it: Y, then (where the chroma is blended) Cb, Cr of the unit.  `inter` is the inter operand as the blend
 * would read it (luma: after the forward map); it goes to the unit's region in the layout of vvc355_ciip_frame, the plane is left alone */
static void ciip_capture(uint8_t *dst, ptrdiff_t dst_stride, int width, int height, const uint8_t *inter, ptrdiff_t inter_stride, int intra_weight)
{
    const vvc355_ciip_cu *r = cap.rec;
    const int c = cap.c++;
    const int ps = sps.pixel_shift;
    const int64_t off = (int64_t)r->scratch_off + (c ? r->cb_width * r->cb_height + (c - 1) * width * height : 0);

    if (c > 2 || off < 0 || off + (int64_t)width * height > cap.scratch_len) {
        cap.failed = 1;
        return;
    }
    for (int y = 0; y < height; y++)
        memcpy(cap.scratch + ((off + (int64_t)y * width) << ps), inter + y * inter_stride, (size_t)width << ps);
    cap.weights[3 * cap.unit + c] = intra_weight;
}

/* links cus[0..n) per CTU in list order, then for every CTU in raster order ff_vvc_predict_inter, or (ciip != NULL: the records)
 * ff_vvc_decode_neighbour and ff_vvc_predict_ciip per unit */
static int predict(const orc_inter_frame *f, CodingUnit *cus, const UnitHead *head, int n, const vvc355_ciip_cu *ciip)
{
    const int log2 = sps.ctb_log2_size_y;
    const int n_ctb = (int)pps.ctb_count;
    CTU *ctus = calloc((size_t)n_ctb, sizeof(*ctus));
    CodingUnit **tail = calloc((size_t)n_ctb, sizeof(*tail));
    int *slice = malloc((size_t)n_ctb * sizeof(*slice));
    int ok = ctus && tail && slice;

    for (int i = 0; ok && i < n_ctb; i++)
        slice[i] = -1;
    for (int u = 0; ok && u < n; u++) {
        const UnitHead *h = head + u;
        CodingUnit *cu = cus + u;
        int rs;
        if (h->x0 < 0 || h->y0 < 0 || h->w < 4 || h->h < 4 || h->w > 128 || h->h > 128 || (h->x0 & 3) || (h->y0 & 3) || (h->w & (h->w - 1)) ||
            (h->h & (h->h - 1)) || h->x0 + h->w > f->width || h->y0 + h->h > f->height || h->slice < 0 || h->slice >= MAX_SLICES ||
            (h->x0 >> log2) != ((h->x0 + h->w - 1) >> log2) || (h->y0 >> log2) != ((h->y0 + h->h - 1) >> log2)) {
            ok = 0;
            break;
        }
        rs = (h->y0 >> log2) * pps.ctb_width + (h->x0 >> log2);
        if (slice[rs] >= 0 && slice[rs] != h->slice) {
            ok = 0;
            break;
        }
        if (!sc[h->slice].sh.r && wire_slice(f, h->slice, f->lmcs_fwd_lut != 0)) {
            ok = 0;
            break;
        }
        slice[rs] = h->slice;
        cu->x0 = h->x0;
        cu->y0 = h->y0;
        cu->cb_width  = h->w;
        cu->cb_height = h->h;
        cu->pred_mode = MODE_INTER;
        cu->tree_type = SINGLE_TREE;
        cu->next = NULL;
        if (tail[rs])
            tail[rs]->next = cu;
        else
            ctus[rs].cus = cu;
        tail[rs] = cu;
    }
    if (ok) {
        fc.tab.ctus = ctus;
        for (int rs = 0; rs < n_ctb; rs++) {
            if (slice[rs] < 0)
                continue;
            lc.sc = &sc[slice[rs]];
            if (!ciip) {
                ff_vvc_predict_inter(&lc, rs);
                continue;
            }
            ff_vvc_decode_neighbour(&lc, (rs % pps.ctb_width) << log2, (rs / pps.ctb_width) << log2, rs % pps.ctb_width, rs / pps.ctb_width, rs);
            for (CodingUnit *cu = ctus[rs].cus; cu; cu = cu->next) {
                cap.unit = (int)(cu - cus);
                cap.rec  = ciip + cap.unit;
                cap.c    = 0;
                lc.cu    = cu;
                ff_vvc_predict_ciip(&lc);
            }
        }
        fc.tab.ctus = NULL;
    }
    free(ctus);
    free(tail);
    free(slice);
    return ok ? 0 : -1;
}

static int alloc_units(int n, CodingUnit **cus, UnitHead **head)
{
    *cus  = calloc((size_t)(n > 0 ? n : 1), sizeof(**cus));
    *head = calloc((size_t)(n > 0 ? n : 1), sizeof(**head));
    if (*cus && *head)
        return 0;
    free(*cus);
    free(*head);
    return -1;
}

/* ------------------------------------------------------------------ regular units: pred_regular_blk */
REF_API int ref_inter_picture(int bd, const orc_inter_frame *f, int ctb_log2)
{
    const orc_inter_pu *pus = PTR(const orc_inter_pu, f->pus);
    CodingUnit *cus;
    UnitHead *head;
    int err;

    if (f->n_pus < 0 || (f->n_pus && !f->pus) || wire(bd, f, ctb_log2) || alloc_units(f->n_pus, &cus, &head))
        return -1;
    err = 0;
    for (int u = 0; u < f->n_pus; u++) {
        const orc_inter_pu *p = pus + u;
        CodingUnit *cu = cus + u;
        head[u] = (UnitHead){ p->x0, p->y0, p->cb_width, p->cb_height, p->slice };
        /* CIIP units are not predicted by ff_vvc_predict_inter (pred_regular_blk skips them); DMVR needs its table */
        if (!p->num_sb_x || !p->num_sb_y || p->cb_width % p->num_sb_x || p->cb_height % p->num_sb_y || p->ciip_flag || (p->dmvr_flag && !f->dmvr_mvf))
            err = -1;
        cu->pu.mi.num_sb_x    = p->num_sb_x;
        cu->pu.mi.num_sb_y    = p->num_sb_y;
        cu->pu.mi.hpel_if_idx = p->hpel_if_idx;
        cu->pu.dmvr_flag      = p->dmvr_flag;
        cu->pu.bdof_flag      = p->bdof_flag;
    }
    if (!err)
        err = predict(f, cus, head, f->n_pus, NULL);
    free(cus);
    free(head);
    return err;
}

/* ------------------------------------------------------------------ affine units: pred_affine_blk */
REF_API int ref_affine_picture(int bd, const orc_inter_frame *f, int ctb_log2, const vvc355_affine_cu *rec, int n_cus)
{
    const MvField *mvf = PTR(const MvField, f->mvf);
    CodingUnit *cus;
    UnitHead *head;
    int err;

    if (n_cus < 0 || (n_cus && !rec) || wire(bd, f, ctb_log2) || alloc_units(n_cus, &cus, &head))
        return -1;
    err = 0;
    for (int u = 0; u < n_cus; u++) {
        const vvc355_affine_cu *r = rec + u;
        CodingUnit *cu = cus + u;
        head[u] = (UnitHead){ r->x0, r->y0, r->cb_width, r->cb_height, r->slice };
        if (r->x0 < 0 || r->y0 < 0 || r->x0 + r->cb_width > f->width || r->y0 + r->cb_height > f->height || r->num_sb_x != r->cb_width >> 2 ||
            r->num_sb_y != r->cb_height >> 2 || r->cb_width < 8 || r->cb_height < 8) {
            err = -1;
            break;
        }
        cu->pu.inter_affine_flag = 1;
        cu->pu.mi.num_sb_x   = r->num_sb_x;
        cu->pu.mi.num_sb_y   = r->num_sb_y;
        /* the unit's prediction direction, as the parser stores it beside the per-sub-block MvFields */
        cu->pu.mi.pred_flag  = mvf[(r->y0 >> 2) * f->mvf_stride + (r->x0 >> 2)].pred_flag;
        for (int l = 0; l < 2; l++) {
            cu->pu.cb_prof_flag[l] = (r->prof_flags >> l) & 1;
            memcpy(cu->pu.diff_mv_x[l], r->diff_mv[l][0], sizeof(cu->pu.diff_mv_x[l]));
            memcpy(cu->pu.diff_mv_y[l], r->diff_mv[l][1], sizeof(cu->pu.diff_mv_y[l]));
        }
    }
    if (!err)
        err = predict(f, cus, head, n_cus, NULL);
    free(cus);
    free(head);
    return err;
}

/* ------------------------------------------------------------------ geometric-partition units: pred_gpm_blk */
REF_API int ref_gpm_picture(int bd, const orc_inter_frame *f, int ctb_log2, const vvc355_gpm_cu *rec, int n_cus)
{
    CodingUnit *cus;
    UnitHead *head;
    int err;

    if (n_cus < 0 || (n_cus && !rec) || wire(bd, f, ctb_log2) || alloc_units(n_cus, &cus, &head))
        return -1;
    err = 0;
    for (int u = 0; u < n_cus; u++) {
        const vvc355_gpm_cu *r = rec + u;
        CodingUnit *cu = cus + u;
        head[u] = (UnitHead){ r->x0, r->y0, r->cb_width, r->cb_height, r->slice };
        /* the shapes the offset tables are indexed with: 8..64 per side; a part predicts from exactly one list */
        if (r->cb_width < 8 || r->cb_height < 8 || r->cb_width > 64 || r->cb_height > 64 || r->cb_width >= 8 * r->cb_height ||
            r->cb_height >= 8 * r->cb_width || r->partition_idx > 63)
            err = -1;
        cu->pu.merge_gpm_flag    = 1;
        cu->pu.gpm_partition_idx = r->partition_idx;
        memcpy(cu->pu.gpm_mv, r->gpm_mv, sizeof(cu->pu.gpm_mv));
        for (int i = 0; i < 2; i++) {
            const MvField *m = &cu->pu.gpm_mv[i];
            if ((m->pred_flag != PF_L0 && m->pred_flag != PF_L1) || m->ref_idx[m->pred_flag - PF_L0] < 0 ||
                m->ref_idx[m->pred_flag - PF_L0] >= MAX_REFS)
                err = -1;
        }
    }
    if (!err)
        err = predict(f, cus, head, n_cus, NULL);
    free(cus);
    free(head);
    return err;
}

/* ------------------------------------------------------------------ CIIP units: ff_vvc_predict_ciip, inter half only
 * scratch (pixels) and weights (int32 [n_cus][3], left as they are where the reference does not blend: 4:0:0, chroma 2 wide) receive what
 * put_ciip was handed; chroma of units with wc <= 2 lands on the plane, as in the reference. */
REF_API int ref_ciip_picture(int bd, const orc_inter_frame *f, int ctb_log2, const vvc355_ciip_cu *rec, int n_cus, const int16_t *slice_idx,
                             const uint16_t *col_bd, const uint16_t *row_bd, void *scratch, int scratch_len, int32_t *weights)
{
    CodingUnit *cus;
    UnitHead *head;
    int err;

    if (n_cus < 0 || (n_cus && !rec) || !slice_idx || !col_bd || !row_bd || !scratch || scratch_len < 0 || !weights || wire(bd, f, ctb_log2) ||
        alloc_units(n_cus, &cus, &head))
        return -1;
    fc.tab.slice_idx  = (int16_t *)(uintptr_t)slice_idx;
    pps.ctb_to_col_bd = (uint16_t *)(uintptr_t)col_bd;
    pps.ctb_to_row_bd = (uint16_t *)(uintptr_t)row_bd;
    fc.vvcdsp.intra.intra_pred = ciip_no_intra;
    fc.vvcdsp.inter.put_ciip   = ciip_capture;
    memset(&cap, 0, sizeof(cap));
    cap.scratch     = scratch;
    cap.scratch_len = scratch_len;
    cap.weights     = weights;
    err = 0;
    for (int u = 0; u < n_cus; u++) {
        const vvc355_ciip_cu *r = rec + u;
        CodingUnit *cu = cus + u;
        head[u] = (UnitHead){ r->x0, r->y0, r->cb_width, r->cb_height, r->slice };
        if (r->cb_width > 64 || r->cb_height > 64 || r->cb_width * r->cb_height < 64)
            err = -1;
        cu->ciip_flag = 1;
        cu->pu.mi.num_sb_x    = 1;
        cu->pu.mi.num_sb_y    = 1;
        cu->pu.mi.hpel_if_idx = r->hpel_if_idx & 1;
    }
    if (!err)
        err = predict(f, cus, head, n_cus, rec);
    if (cap.failed)
        err = -1;
    free(cus);
    free(head);
    return err;
}
