/*
 * oracle/ref_shim_filter.c — the reference's in-loop filter callers on whole pictures, driven from the oracle's descriptors.
 *
 * TEST INFRASTRUCTURE ONLY, third translation unit of oracle/_ref/libvvcref.so (see ref_shim.c).  Project code: it includes the
 * reference's headers from the tree at build time and calls functions the reference exports — ff_vvc_decode_neighbour,
 * ff_vvc_deblock_vertical / _horizontal (which derive the boundary strengths themselves), ff_vvc_sao_copy_ctb_to_hv +
 * ff_vvc_sao_filter, ff_vvc_alf_copy_ctu_to_hv + ff_vvc_alf_filter — on real VVCLocalContext / VVCFrameContext / VVCSPS / VVCPPS /
 * SliceContext objects whose fc->tab.* pointers are aimed at the caller's tables (orc_bs_frame / orc_deblock_frame / orc_sao_frame /
 * orc_alf_frame of vvc_oracle.h describe that very layout).  CTUs are walked in raster order, every stage over the whole picture
 * before the next (the order the reference's scheduler guarantees: all vertical edges of a CTU's neighbourhood before its
 * horizontal ones, vvc_thread.c).
 *
 * The three entries return 0, or -1 where a picture is outside what the real objects can hold (sizes, slice count, memory).
 *
 * ALF parameter sets.  The reference knows eight APS ids.  Per slice the shim installs seven VVCALF objects at ids 0..6 and leaves
 * id 7 NULL: object k carries the slice's luma set k (REF_ALF_LUMA_SETS = 7 luma sets per slice, sh_alf_aps_id_luma[k] = k); the
 * chroma filters live in object 0, the Cb cross-component filters in object 1 and the Cr ones in object 2, shared with the luma
 * sets there as a stream shares one APS between components.  A cc_coeff address of 0 selects id 7, the NULL entry the reference
 * tests for.  Single-threaded: one set of objects, rewired by every call.
 */
#include <stdlib.h>
#include <string.h>

#include "libavutil/frame.h"
#include "libavcodec/vvc/vvc_ctu.h"
#include "libavcodec/vvc/vvc_filter.h"

#include "vvc_oracle.h"

#define REF_API __attribute__((visibility("default")))
#define REF_ALF_LUMA_SETS 7

static VVCLocalContext    lc;
static VVCFrameContext    fc;
static SliceContext       sc;
static VVCSPS             sps;
static VVCPPS             pps;
static H266RawSPS         raw_sps;
static H266RawPPS         raw_pps;
static H266RawSliceHeader raw_sh;
static AVFrame            frame;
static VVCFrame           cur;

REF_API int ref_alf_luma_sets(void) { return REF_ALF_LUMA_SETS; }

#define PTR(type, addr) ((type *)(uintptr_t)(addr))

/* the geometry every stage shares; n_comp == 1 is 4:0:0 */
static int wire(int bd, int width, int height, int ctb_log2, int min_cb_log2, int hs, int vs, int n_comp,
                uint64_t slice_idx, uint64_t col_bd, uint64_t row_bd, int lfase, int lfate, int n_tiles,
                const uint64_t *plane, const int32_t *stride)
{
    if ((bd != 8 && bd != 10 && bd != 12) || width <= 0 || height <= 0 || width > 8192 || height > 8192 || ctb_log2 < 5 || ctb_log2 > 7 ||
        min_cb_log2 < 2 || min_cb_log2 > ctb_log2)
        return -1;
    memset(&lc, 0, sizeof(lc));
    memset(&fc, 0, sizeof(fc));
    memset(&sc, 0, sizeof(sc));
    memset(&sps, 0, sizeof(sps));
    memset(&pps, 0, sizeof(pps));
    memset(&raw_sps, 0, sizeof(raw_sps));
    memset(&raw_pps, 0, sizeof(raw_pps));
    memset(&raw_sh, 0, sizeof(raw_sh));
    memset(&frame, 0, sizeof(frame));
    memset(&cur, 0, sizeof(cur));
    sps.r     = &raw_sps;
    pps.r     = &raw_pps;
    sc.sh.r   = &raw_sh;
    fc.ps.sps = &sps;
    fc.ps.pps = &pps;
    fc.frame  = &frame;
    fc.ref    = &cur;
    lc.fc     = &fc;
    lc.sc     = &sc;

    raw_sps.sps_chroma_format_idc = (uint8_t)(n_comp == 1 ? 0 : hs && vs ? 1 : hs ? 2 : 3);
    sps.width  = pps.width  = (uint16_t)width;
    sps.height = pps.height = (uint16_t)height;
    for (int c = 1; c < 3; c++) {
        sps.hshift[c] = (uint8_t)hs;
        sps.vshift[c] = (uint8_t)vs;
    }
    sps.bit_depth          = (uint8_t)bd;
    sps.pixel_shift        = bd > 8;
    sps.qp_bd_offset       = (uint8_t)(6 * (bd - 8));
    sps.ctb_log2_size_y    = (uint8_t)ctb_log2;
    sps.ctb_size_y         = (uint8_t)(1 << ctb_log2);
    sps.min_cb_log2_size_y = (uint8_t)min_cb_log2;
    sps.min_cb_size_y      = (uint8_t)(1 << min_cb_log2);
    pps.ctb_width     = (uint16_t)((width  + (1 << ctb_log2) - 1) >> ctb_log2);
    pps.ctb_height    = (uint16_t)((height + (1 << ctb_log2) - 1) >> ctb_log2);
    pps.ctb_count     = (uint32_t)pps.ctb_width * pps.ctb_height;
    pps.min_cb_width  = (uint16_t)((width  + (1 << min_cb_log2) - 1) >> min_cb_log2);
    pps.min_cb_height = (uint16_t)((height + (1 << min_cb_log2) - 1) >> min_cb_log2);
    pps.min_pu_width  = pps.min_tu_width  = (uint16_t)(width >> 2);
    pps.min_pu_height = pps.min_tu_height = (uint16_t)(height >> 2);
    pps.ctb_to_col_bd = PTR(uint16_t, col_bd);
    pps.ctb_to_row_bd = PTR(uint16_t, row_bd);
    raw_pps.pps_loop_filter_across_slices_enabled_flag = (uint8_t)lfase;
    raw_pps.pps_loop_filter_across_tiles_enabled_flag  = (uint8_t)lfate;
    raw_pps.num_tiles_in_pic = (uint16_t)n_tiles;
    fc.tab.slice_idx = PTR(int16_t, slice_idx);
    for (int c = 0; c < n_comp; c++) {
        frame.data[c]     = PTR(uint8_t, plane[c]);
        frame.linesize[c] = stride[c];
    }
    ff_vvc_dsp_init(&fc.vvcdsp, bd);
    return 0;
}

/* calloc with room on both sides: the reference forms (and never reads) border-buffer addresses of CTU row / column -1 */
static uint8_t *slack_alloc(size_t size, size_t margin, uint8_t **base)
{
    *base = calloc(1, size + 2 * margin);
    return *base ? *base + margin : NULL;
}

typedef void (*ctu_fn)(int rx, int ry, int rs, void *arg);

static void for_each_ctu(ctu_fn fn, void *arg)
{
    for (int ry = 0; ry < pps.ctb_height; ry++)
        for (int rx = 0; rx < pps.ctb_width; rx++)
            fn(rx, ry, ry * pps.ctb_width + rx, arg);
}

/* ------------------------------------------------------------------ deblocking: boundary strengths + both edge directions */
typedef struct DeblockArg { RefPicListTab *rpl; int vertical; } DeblockArg;

static void deblock_ctu(int rx, int ry, int rs, void *arg)
{
    const DeblockArg *a = arg;
    const int x0 = rx << sps.ctb_log2_size_y, y0 = ry << sps.ctb_log2_size_y;

    sc.rpl = a->rpl[fc.tab.slice_idx[rs]].refPicList;
    ff_vvc_decode_neighbour(&lc, x0, y0, rx, ry, rs);
    if (a->vertical)
        ff_vvc_deblock_vertical(&lc, x0, y0);
    else
        ff_vvc_deblock_horizontal(&lc, x0, y0);
}

/* b: the side tables and the ten output tables; d: planes, QP tables, per-CTU offsets and LADF (its bs / max_len / tb_size_c / vertical
 * members are not read).  vertical_only != 0 stops after the vertical-edge pass. */
REF_API int ref_deblock_picture(int bd, const orc_bs_frame *b, const orc_deblock_frame *d, int n_slices, int vertical_only)
{
    static int32_t *no_tb_pos;
    static uint8_t *no_tb_u8;
    const int chroma = b->n_comp >= 3;
    const size_t n_tu = (size_t)(b->width >> 2) * (b->height >> 2);
    RefPicListTab *rpl, **rpl_tab;
    const int32_t *poc = PTR(const int32_t, b->ref_poc);
    const int16_t *slice_idx = PTR(const int16_t, b->slice_idx);
    DeblockArg arg;
    int n_ctb;

    if (n_slices < 1 || b->width != d->width || b->height != d->height || b->ctb_log2 != d->ctb_log2 || b->min_cb_log2 != d->min_cb_log2 ||
        b->min_tu_width != b->width >> 2 || b->min_pu_width != b->width >> 2 || d->min_tu_width != b->width >> 2 ||
        d->num_ladf_intervals > 5)
        return -1;
    if (wire(bd, b->width, b->height, b->ctb_log2, b->min_cb_log2, b->hs, b->vs, chroma ? 3 : 1, b->slice_idx, b->ctb_to_col_bd, b->ctb_to_row_bd,
             b->lfase, b->lfate, 1, d->plane, d->stride))
        return -1;
    if (b->min_cb_width != pps.min_cb_width || d->min_cb_width != pps.min_cb_width || b->ctb_width != pps.ctb_width || d->ctb_width != pps.ctb_width)
        return -1;
    n_ctb = (int)pps.ctb_count;
    for (int i = 0; i < n_ctb; i++)
        if (slice_idx[i] < 0 || slice_idx[i] >= n_slices)
            return -1;

    /* the ten output tables start from zero, as the reference clears them per picture */
    for (int dir = 0; dir < 2; dir++) {
        for (int c = 0; c < (chroma ? 3 : 1); c++)
            memset(PTR(uint8_t, b->bs[dir][c]), 0, n_tu);
        memset(PTR(uint8_t, b->max_len_p[dir]), 0, n_tu);
        memset(PTR(uint8_t, b->max_len_q[dir]), 0, n_tu);
    }
    for (int c = 0; c < 3; c++) {
        fc.tab.horizontal_bs[c] = PTR(uint8_t, b->bs[0][c]);
        fc.tab.vertical_bs[c]   = PTR(uint8_t, b->bs[1][c]);
        fc.tab.tu_coded_flag[c] = PTR(uint8_t, b->tu_coded_flag[c]);
    }
    fc.tab.horizontal_p = PTR(uint8_t, b->max_len_p[0]);
    fc.tab.horizontal_q = PTR(uint8_t, b->max_len_q[0]);
    fc.tab.vertical_p   = PTR(uint8_t, b->max_len_p[1]);
    fc.tab.vertical_q   = PTR(uint8_t, b->max_len_q[1]);
    fc.tab.tu_joint_cbcr_residual_flag = PTR(uint8_t, b->tu_joint_cbcr);
    for (int t = 0; t < 2; t++) {
        fc.tab.pcmf[t]      = PTR(uint8_t, b->pcmf[t]);
        fc.tab.tb_pos_x0[t] = PTR(int, b->tb_pos_x0[t]);
        fc.tab.tb_pos_y0[t] = PTR(int, b->tb_pos_y0[t]);
        fc.tab.tb_width[t]  = PTR(uint8_t, b->tb_width[t]);
        fc.tab.tb_height[t] = PTR(uint8_t, b->tb_height[t]);
    }
    if (!chroma) {
        /* 4:0:0: the reference still walks the chroma tree's position tables; give it tables in which no unit starts a block */
        int32_t *pos = realloc(no_tb_pos, n_tu * sizeof(*pos));
        uint8_t *u8;
        if (!pos)
            return -1;
        no_tb_pos = pos;
        u8 = realloc(no_tb_u8, n_tu);
        if (!u8)
            return -1;
        no_tb_u8 = u8;
        for (size_t i = 0; i < n_tu; i++)
            pos[i] = -4;
        memset(u8, 0, n_tu);
        fc.tab.tb_pos_x0[1] = fc.tab.tb_pos_y0[1] = pos;
        fc.tab.tb_width[1] = fc.tab.tb_height[1] = fc.tab.pcmf[1] = u8;
    }
    fc.tab.cb_pos_x[0]  = PTR(int, b->cb_pos_x);
    fc.tab.cb_pos_y[0]  = PTR(int, b->cb_pos_y);
    fc.tab.cb_width[0]  = PTR(uint8_t, b->cb_width);
    fc.tab.cb_height[0] = PTR(uint8_t, b->cb_height);
    fc.tab.msf = PTR(uint8_t, b->msf);
    fc.tab.iaf = PTR(uint8_t, b->iaf);
    fc.tab.mvf = PTR(MvField, b->mvf);
    fc.tab.qp[0]   = PTR(int8_t, d->qp_y);
    fc.tab.qp[1]   = PTR(int8_t, d->qp_c[0]);
    fc.tab.qp[2]   = PTR(int8_t, d->qp_c[1]);
    fc.tab.deblock = PTR(DBParams, d->db_params);

    raw_sps.sps_ladf_enabled_flag = d->ladf_enabled;
    raw_sps.sps_ladf_lowest_interval_qp_offset = d->ladf_lowest_qp_offset;
    sps.num_ladf_intervals = d->num_ladf_intervals;
    for (int i = 0; i < 4; i++)
        raw_sps.sps_ladf_qp_offset[i] = d->ladf_qp_offset[i];
    for (int i = 0; i < 5; i++)
        sps.ladf_interval_lower_bound[i] = (uint32_t)d->ladf_lower_bound[i];

    /* one pair of reference picture lists per slice; only the POCs are read (boundary_strength) */
    rpl     = calloc((size_t)n_slices, sizeof(*rpl));
    rpl_tab = calloc((size_t)n_ctb, sizeof(*rpl_tab));
    if (!rpl || !rpl_tab) {
        free(rpl);
        free(rpl_tab);
        return -1;
    }
    for (int s = 0; s < n_slices; s++)
        for (int l = 0; l < 2; l++) {
            RefPicList *list = &rpl[s].refPicList[l];
            list->nb_refs = VVC_MAX_REF_ENTRIES < 32 ? VVC_MAX_REF_ENTRIES : 32;
            for (int i = 0; i < list->nb_refs; i++)
                list->list[i] = poc[(s * 2 + l) * 32 + i];
        }
    for (int i = 0; i < n_ctb; i++)
        rpl_tab[i] = &rpl[slice_idx[i]];
    cur.rpl_tab = rpl_tab;

    arg.rpl = rpl;
    arg.vertical = 1;
    for_each_ctu(deblock_ctu, &arg);
    if (!vertical_only) {
        arg.vertical = 0;
        for_each_ctu(deblock_ctu, &arg);
    }
    free(rpl);
    free(rpl_tab);
    return 0;
}

/* ------------------------------------------------------------------ SAO, in place on src[] */
static void sao_copy_ctu(int rx, int ry, int rs, void *arg)
{
    ff_vvc_sao_copy_ctb_to_hv(&lc, rx, ry, ry == pps.ctb_height - 1);
}

static void sao_ctu(int rx, int ry, int rs, void *arg)
{
    const int x0 = rx << sps.ctb_log2_size_y, y0 = ry << sps.ctb_log2_size_y;
    ff_vvc_decode_neighbour(&lc, x0, y0, rx, ry, rs);
    ff_vvc_sao_filter(&lc, x0, y0);
}

REF_API int ref_sao_picture(int bd, const orc_sao_frame *f)
{
    const orc_sao_ctb *in = PTR(const orc_sao_ctb, f->sao);
    const int n_comp = f->n_comp >= 3 ? 3 : 1;
    uint8_t *base[6] = { 0 };
    SAOParams *sao;
    int ok = 1;

    /* no_tile_filter is num_tiles_in_pic > 1 with the tiles flag off; the flag alone is not read by SAO otherwise */
    if (wire(bd, f->width, f->height, f->ctb_log2, 2, f->hs, f->vs, n_comp, f->slice_idx, f->ctb_to_col_bd, f->ctb_to_row_bd,
             f->lfase, !f->no_tile_filter, f->no_tile_filter ? 2 : 1, f->src, f->src_stride))
        return -1;
    if (f->ctb_width != pps.ctb_width || f->ctb_height != pps.ctb_height)
        return -1;
    sao = calloc(pps.ctb_count, sizeof(*sao));
    if (!sao)
        return -1;
    for (uint32_t i = 0; i < pps.ctb_count; i++)
        for (int c = 0; c < 3; c++) {
            memcpy(sao[i].offset_val[c], in[i].offset_val[c], sizeof(sao[i].offset_val[c]));
            sao[i].type_idx[c]      = in[i].type_idx[c];
            sao[i].band_position[c] = in[i].band_position[c];
            sao[i].eo_class[c]      = in[i].eo_class[c];
        }
    fc.tab.sao = sao;
    for (int c = 0; c < n_comp; c++) {
        const size_t w = (size_t)(f->width >> sps.hshift[c]), h = (size_t)(f->height >> sps.vshift[c]);
        const size_t margin = (4 * (w + h) + 256) << 1;
        fc.tab.sao_pixel_buffer_h[c] = slack_alloc((2 * pps.ctb_height * w) << 1, margin, &base[2 * c]);
        fc.tab.sao_pixel_buffer_v[c] = slack_alloc((2 * pps.ctb_width * h) << 1, margin, &base[2 * c + 1]);
        ok = ok && fc.tab.sao_pixel_buffer_h[c] && fc.tab.sao_pixel_buffer_v[c];
    }
    if (ok) {
        for_each_ctu(sao_copy_ctu, NULL);
        for_each_ctu(sao_ctu, NULL);
    }
    for (int i = 0; i < 6; i++)
        free(base[i]);
    free(sao);
    return ok ? 0 : -1;
}

/* ------------------------------------------------------------------ ALF, in place on src[] */
static VVCALF alf_aps[REF_ALF_LUMA_SETS];

static void alf_copy_ctu(int rx, int ry, int rs, void *arg)
{
    ff_vvc_alf_copy_ctu_to_hv(&lc, rx << sps.ctb_log2_size_y, ry << sps.ctb_log2_size_y);
}

static void alf_install_slice(const orc_alf_slice *s)
{
    memset(alf_aps, 0, sizeof(alf_aps));
    for (int k = 0; k < REF_ALF_LUMA_SETS; k++) {
        fc.ps.alf_list[k] = &alf_aps[k];
        raw_sh.sh_alf_aps_id_luma[k] = (uint8_t)k;
        if (s->luma_coeff[k])
            memcpy(alf_aps[k].luma_coeff, PTR(const void, s->luma_coeff[k]), sizeof(alf_aps[k].luma_coeff));
        if (s->luma_clip_idx[k])
            memcpy(alf_aps[k].luma_clip_idx, PTR(const void, s->luma_clip_idx[k]), sizeof(alf_aps[k].luma_clip_idx));
    }
    fc.ps.alf_list[7] = NULL;
    raw_sh.sh_alf_aps_id_luma[7] = 0;
    raw_sh.sh_alf_aps_id_chroma  = 0;
    if (s->chroma_coeff)
        memcpy(alf_aps[0].chroma_coeff, PTR(const void, s->chroma_coeff), sizeof(alf_aps[0].chroma_coeff));
    if (s->chroma_clip_idx)
        memcpy(alf_aps[0].chroma_clip_idx, PTR(const void, s->chroma_clip_idx), sizeof(alf_aps[0].chroma_clip_idx));
    alf_aps[0].num_chroma_filters = ALF_NUM_FILTERS_CHROMA;
    /* cc_coeff is int16 [4][7]; VVCALF.cc_coeff[idx] has room for ALF_NUM_FILTERS_CC rows */
    raw_sh.sh_alf_cc_cb_aps_id = s->cc_coeff[0] ? 1 : 7;
    raw_sh.sh_alf_cc_cr_aps_id = s->cc_coeff[1] ? 2 : 7;
    for (int i = 0; i < 2; i++)
        if (s->cc_coeff[i]) {
            memcpy(alf_aps[1 + i].cc_coeff[i], PTR(const void, s->cc_coeff[i]), 4 * ALF_NUM_COEFF_CC * sizeof(int16_t));
            alf_aps[1 + i].num_cc_filters[i] = 4;
        }
}

static void alf_ctu(int rx, int ry, int rs, void *arg)
{
    const int x0 = rx << sps.ctb_log2_size_y, y0 = ry << sps.ctb_log2_size_y;
    alf_install_slice((const orc_alf_slice *)arg + fc.tab.slice_idx[rs]);
    ff_vvc_decode_neighbour(&lc, x0, y0, rx, ry, rs);
    ff_vvc_alf_filter(&lc, x0, y0);
}

REF_API int ref_alf_picture(int bd, const orc_alf_frame *f)
{
    const orc_alf_ctb *in = PTR(const orc_alf_ctb, f->alf);
    const int n_comp = f->n_comp >= 3 ? 3 : 1;
    uint8_t *base[12] = { 0 };
    ALFParams *alf;
    int ok = 1;

    if (wire(bd, f->width, f->height, f->ctb_log2, 2, f->hs, f->vs, n_comp, f->slice_idx, f->ctb_to_col_bd, f->ctb_to_row_bd,
             f->lfase, f->lfate, 1, f->src, f->src_stride))
        return -1;
    if (f->ctb_width != pps.ctb_width || f->ctb_height != pps.ctb_height)
        return -1;
    alf = calloc(pps.ctb_count, sizeof(*alf));
    if (!alf)
        return -1;
    for (uint32_t i = 0; i < pps.ctb_count; i++) {
        memcpy(alf[i].ctb_flag, in[i].ctb_flag, 3);
        alf[i].ctb_filt_set_idx_y = in[i].filt_set_idx_y;
        memcpy(alf[i].alf_ctb_filter_alt_idx, in[i].alt_idx, 2);
        memcpy(alf[i].ctb_cc_idc, in[i].cc_idc, 2);
        if (in[i].filt_set_idx_y >= 16 + REF_ALF_LUMA_SETS)
            ok = 0;
    }
    fc.tab.alf = alf;
    for (int c = 0; c < n_comp && ok; c++) {
        const size_t w = (size_t)(f->width >> sps.hshift[c]), h = (size_t)(f->height >> sps.vshift[c]);
        const size_t border = c ? ALF_BORDER_CHROMA : ALF_BORDER_LUMA;
        const size_t margin = (8 * (w + h) + 512) << 1;
        for (int i = 0; i < 2; i++) {
            fc.tab.alf_pixel_buffer_h[c][i] = slack_alloc((border * pps.ctb_height * w) << 1, margin, &base[4 * c + i]);
            fc.tab.alf_pixel_buffer_v[c][i] = slack_alloc((border * pps.ctb_width * h) << 1, margin, &base[4 * c + 2 + i]);
            ok = ok && fc.tab.alf_pixel_buffer_h[c][i] && fc.tab.alf_pixel_buffer_v[c][i];
        }
    }
    if (ok) {
        for_each_ctu(alf_copy_ctu, NULL);
        for_each_ctu(alf_ctu, PTR(void, f->slices));
    }
    for (int i = 0; i < 12; i++)
        free(base[i]);
    free(alf);
    return ok ? 0 : -1;
}
