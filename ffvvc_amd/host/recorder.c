/*
 * recorder.c — from parsed units to RECON commands and TB records (include/vvc_mi355_rec.h).
 *
 * vvc355_rec_ctu walks one CTU's coding units the way ff_vvc_reconstruct does (vvc_intra.c:498-527: per unit, per channel type, per
 * transform unit predict_intra then itransform) and leaves PENDING commands and blocks: everything INTEGRATION.md section 3 derives is
 * final there except KEEP of the scaled chroma blocks of inter units, which needs to know whether a neighbouring CTU — or, with CtbSizeY
 * 128, this one — holds an intra unit.  vvc355_rec_end_picture decides those, drops the RESID commands of the blocks that go to the batched
 * passes and the command lists of CTUs left with nothing but MARKs, groups the records (counting sort, CTUs in raster order, decoding order
 * inside a group), numbers the arena slots in list order and moves the packed groups into the same order.
 *
 * vvc355_rec_ctu_units is the same walk with two additions.  A CIIP unit gets its PRED + CIIP commands ahead of an inter unit's, every
 * coded block of it is KEEP, and it makes its CTU one that holds an intra unit.  And every unit leaves its unit records (vvc355_cu_rec,
 * vvc355_tu_rec, their QP bytes) and its motion records (vvc355_mvf_unit, and a vvc355_inter_pu / _affine_cu / _gpm_cu / _ciip_cu) in
 * recording order; vvc355_rec_end_picture puts them in raster CTU order and fills the running sums (first_job, scratch_off, link, the
 * ctu_first tables, the CIIP units' command indices).
 * Plain C11, no HIP, one thread at a time per object.
 */
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "vvc_mi355_rec.h"

enum { ST_IDLE, ST_BEGUN, ST_ENDED };
enum { L_INTRA, L_INTER, L_TS, N_LISTS };
enum { W_NO, W_YES, W_DEFERRED };
enum { M_NONE, M_WALK, M_UNITS };                /* which of the two CTU entries the picture goes through */
enum { U_CU, U_TU, U_MVF, U_INTER, U_AFFINE, U_GPM, U_CIIP, U_TUD, N_UNIT_LISTS };      /* U_TUD: the deblocking passes' transform-unit records */
enum { N_KEYS = 2 * VVC355_INTER_TB_BINS };      /* the largest key space of the three lists */
#define NO_SEQ 0xFFFFFFFFu

typedef struct rec_blk {
    union { vvc355_intra_tu a; vvc355_inter_tu e; vvc355_ts_tu s; } rec;     /* final but for coeff_off, KEEP and the joint bits */
    uint64_t groups;           /* packed: the side record's mask */
    uint64_t at;               /* packed: first group in the parse-order stream; else element offset in the raw int32 store */
    uint32_t seq;              /* its coding unit's number in recording order */
    int32_t  dep[2];           /* deferred: the CTUs holding the luma left of / above its unit's 64x64 unit, -1 = none */
    uint32_t slot;
    uint8_t  list, key, walk, sj, packed, n_elem_log2;
} rec_blk;

typedef struct rec_ctu {
    uint32_t cmd_first, cmd_n, blk_first, blk_n, intra_seq;
    uint8_t  seen, has_intra;
    uint8_t  kind;             /* set by end_picture: 0 no commands, 1 LIGHT, 2 the walk writes its luma */
    uint32_t u_first[N_UNIT_LISTS], u_n[N_UNIT_LISTS];     /* its ranges in the pending unit lists */
} rec_ctu;

/* a unit list: the records in recording order, and in raster CTU order after end_picture */
typedef struct rec_list {
    uint8_t *pend, *out;
    size_t pend_cap, out_cap, n, elem;
} rec_list;
static const size_t unit_elem[N_UNIT_LISTS] = { sizeof(vvc355_cu_rec), sizeof(vvc355_tu_rec), sizeof(vvc355_mvf_unit), sizeof(vvc355_inter_pu),
                                                sizeof(vvc355_affine_cu), sizeof(vvc355_gpm_cu), sizeof(vvc355_ciip_cu), sizeof(vvc355_tu_rec) };

struct vvc355_recorder {
    vvc355_rec_params p;
    int state, ncx, ncy, hs, vs, ls, tab_w, tab_h;
    uint32_t seq;
    rec_ctu *ctu;                 size_t ctu_cap;
    uint8_t *tab;                 size_t tab_cap;        /* IntraMipFlag, IntraPredModeY, CuPredMode per 4x4 luma samples, one after the other */
    vvc355_recon_cmd *pc;         size_t pc_cap, n_pc;   /* pending commands, resid = block index */
    rec_blk *blk;                 size_t blk_cap, n_blk;
    int16_t *tmp;                 size_t tmp_cap, n_tmp; /* packed groups in recording order (int16 elements) */
    int32_t *raw;                 size_t raw_cap, n_raw; /* int32 levels of the blocks that are not packed */
    /* the result's storage */
    vvc355_recon_cmd *cmds;       size_t cmds_cap, n_cmds;
    uint32_t *cmd_slot;           size_t cmd_slot_cap;
    vvc355_recon_ctu *out_ctu;    size_t out_ctu_cap;
    int32_t *order;               size_t order_cap;
    uint8_t *recs;                size_t recs_cap;       /* the three lists, 16 bytes a record, one after the other */
    vvc355_tb_levels *lv;         size_t lv_cap;
    uint32_t *fin;                size_t fin_cap;        /* final record index -> block */
    int16_t *levels;              size_t levels_cap;
    size_t n_rec;
    /* the unit entry */
    int mode;
    rec_list ul[N_UNIT_LISTS];
    int8_t *cu_qp, *cu_qp_out;    size_t cu_qp_cap, cu_qp_out_cap;
    int8_t *tu_qp, *tu_qp_out;    size_t tu_qp_cap, tu_qp_out_cap;      /* two bytes a record */
    int32_t *ctu_first[3];        size_t ctu_first_cap[3];              /* U_CU, U_TU, U_MVF */
    vvc355_rec_units_result units;
    int8_t *tud_qp, *tud_qp_out;  size_t tud_qp_cap, tud_qp_out_cap;    /* U_TUD's sidecar and its ctu_first table */
    int32_t *tud_first;           size_t tud_first_cap;
    vvc355_rec_deblock_tus deblock;
};

static int grow_(void **p, size_t *cap, size_t n, size_t elem)
{
    if (n <= *cap)
        return 0;
    size_t c = *cap ? *cap : 256;
    while (c < n)
        c *= 2;
    void *q = realloc(*p, c * elem);
    if (!q)
        return -1;
    *p = q;
    *cap = c;
    return 0;
}
#define GROW(ptr, cap, n) grow_((void **)&(ptr), &(cap), (n), sizeof(*(ptr)))

static int ilog2(int v)        /* v a power of two */
{
    int l = 0;
    while ((1 << l) < v)
        l++;
    return l;
}

static int pow2(int v)
{
    return v > 0 && !(v & (v - 1));
}

static int clip(int v, int lo, int hi)
{
    return v < lo ? lo : v > hi ? hi : v;
}

/* back to what vvc355_rec_begin_picture left */
static void restart(vvc355_recorder *r)
{
    const size_t n = (size_t)r->ncx * r->ncy;
    memset(r->ctu, 0, n * sizeof(*r->ctu));
    for (size_t i = 0; i < n; i++)
        r->ctu[i].intra_seq = NO_SEQ;
    memset(r->tab, 0, 3 * (size_t)r->tab_w * r->tab_h);
    r->seq = 0;
    r->n_pc = r->n_blk = r->n_tmp = r->n_raw = r->n_cmds = r->n_rec = 0;
    for (int l = 0; l < N_UNIT_LISTS; l++)
        r->ul[l].n = 0;
    r->mode = M_NONE;
    r->state = ST_BEGUN;
}

static int refuse(vvc355_recorder *r, int code)
{
    restart(r);
    return code;
}

vvc355_recorder *vvc355_rec_create(void)
{
    return calloc(1, sizeof(vvc355_recorder));
}

void vvc355_rec_destroy(vvc355_recorder *r)
{
    if (!r)
        return;
    free(r->ctu); free(r->tab); free(r->pc); free(r->blk); free(r->tmp); free(r->raw);
    free(r->cmds); free(r->cmd_slot); free(r->out_ctu); free(r->order); free(r->recs); free(r->lv); free(r->fin); free(r->levels);
    for (int l = 0; l < N_UNIT_LISTS; l++) {
        free(r->ul[l].pend); free(r->ul[l].out);
    }
    free(r->cu_qp); free(r->cu_qp_out); free(r->tu_qp); free(r->tu_qp_out); free(r->tud_qp); free(r->tud_qp_out); free(r->tud_first);
    for (int l = 0; l < 3; l++)
        free(r->ctu_first[l]);
    free(r);
}

int vvc355_rec_begin_picture(vvc355_recorder *r, const vvc355_rec_params *p)
{
    if (!r || !p)
        return VVC355_REC_E_ARGS;
    r->state = ST_IDLE;
    if (p->width < 1 || p->width > 32767 || p->height < 1 || p->height > 32767 || p->ctb_log2 < 5 || p->ctb_log2 > 7 ||
        p->bit_depth < 8 || p->bit_depth > 16 || p->chroma_format_idc > 3)
        return VVC355_REC_E_PARAMS;
    r->p = *p;
    const int ctb = 1 << p->ctb_log2;
    r->ncx = (p->width + ctb - 1) >> p->ctb_log2;
    r->ncy = (p->height + ctb - 1) >> p->ctb_log2;
    r->hs = p->chroma_format_idc == 1 || p->chroma_format_idc == 2;
    r->vs = p->chroma_format_idc == 1;
    r->ls = p->ctb_log2 < 6 ? p->ctb_log2 : 6;         /* log2 of min(CtbSizeY, 64): the unit of the chroma scale */
    r->tab_w = (p->width + 3) >> 2;
    r->tab_h = (p->height + 3) >> 2;
    if (GROW(r->ctu, r->ctu_cap, (size_t)r->ncx * r->ncy) || GROW(r->tab, r->tab_cap, 3 * (size_t)r->tab_w * r->tab_h))
        return VVC355_REC_E_NOMEM;
    restart(r);
    return 0;
}

/* ---------------------------------------------------------------------------------------------------------------- one CTU */

static int push_cmd(vvc355_recorder *r, int kind, int c_idx, int x0, int y0, int w, int h, const vvc355_rec_cu *cu, vvc355_recon_cmd **out)
{
    if (GROW(r->pc, r->pc_cap, r->n_pc + 1))
        return VVC355_REC_E_NOMEM;
    vvc355_recon_cmd *c = &r->pc[r->n_pc++];
    memset(c, 0, sizeof(*c));
    c->kind = (uint8_t)kind;
    c->c_idx = (uint8_t)c_idx;
    c->x0 = (int16_t)x0, c->y0 = (int16_t)y0, c->w = (int16_t)w, c->h = (int16_t)h;
    c->cu_x0 = (int16_t)cu->x0, c->cu_y0 = (int16_t)cu->y0, c->cb_width = cu->w, c->cb_height = cu->h;
    if (out)
        *out = c;
    return 0;
}

/* 8.4.5.2.7, as the records' pred_mode_intra needs it */
static int wide_angle(int isp, int c_idx, int w, int h, int cb_w, int cb_h, int mode)
{
    const int nw = (!isp || c_idx) ? w : cb_w, nh = (!isp || c_idx) ? h : cb_h;
    const int r = abs(ilog2(nw) - ilog2(nh));
    const int hi = r > 1 ? 8 + 2 * r : 8, lo = r > 1 ? 60 - 2 * r : 60;
    if (nw > nh && mode >= 2 && mode < hi)
        return mode + 65;
    if (nh > nw && mode > lo && mode <= 66)
        return mode - 67;
    return mode;
}

/* derive_ilfnst_pred_mode_intra (vvc_intra.c:34-62) on the recorder's own tables */
static int lfnst_mode(const vvc355_recorder *r, const vvc355_rec_cu *cu, const vvc355_rec_tb *b)
{
    const size_t plane = (size_t)r->tab_w * r->tab_h;
    const uint8_t *imf = r->tab, *ipm = r->tab + plane, *cpm = r->tab + 2 * plane;
    int mode = b->c_idx ? cu->mode_c : cu->mode_y;
    if (b->c_idx == 0 && imf[(size_t)(b->y0 >> 2) * r->tab_w + (b->x0 >> 2)]) {
        mode = 0;
    } else if (mode >= 81 && mode <= 83) {
        const size_t at = (size_t)((b->y0 + ((b->h << r->vs) >> 1)) >> 2) * r->tab_w + ((b->x0 + ((b->w << r->hs) >> 1)) >> 2);
        mode = imf[at] ? 0 : cpm[at] != 1 ? 1 : ipm[at];
    }
    return wide_angle(cu->isp_type != 0, b->c_idx, b->w, b->h, cu->w, cu->h, mode);
}

/* derive_qp's clip (vvc_intra.c:277-310, ACT off) */
static int tb_qp(const vvc355_rec_params *p, const vvc355_rec_cu *cu, const vvc355_rec_tu *tu, int c_idx, int ts)
{
    int qp;
    if (c_idx == 0)
        qp = cu->qp[0] + p->qp_bd_offset;
    else
        qp = cu->qp[(tu->joint_cbcr_residual_flag && tu->coded_flag[1] && tu->coded_flag[2]) ? 3 : c_idx];
    return clip(qp, ts ? 4 + 6 * p->sps_min_qp_prime_ts : 0, 63 + p->qp_bd_offset);
}

static int ctu_of(const vvc355_recorder *r, int x, int y)
{
    return (y >> r->p.ctb_log2) * r->ncx + (x >> r->p.ctb_log2);
}

static int area_class(int s)
{
    return s <= 4 ? 0 : (s - 3) / 2;
}

/* one coded transform block: its record, its levels, and the RESID command(s) of a block the walk owns or may own */
static int record_block(vvc355_recorder *r, int slice_flags, const vvc355_rec_cu *cu, const vvc355_rec_tu *tu, const vvc355_rec_tb *b)
{
    const vvc355_rec_params *p = &r->p;
    const int c = b->c_idx, w = b->w, h = b->h, lw = ilog2(w), lh = ilog2(h), is_intra = cu->pred_mode == 1;
    const int dep = (slice_flags & VVC355_REC_SLICE_DEP_QUANT) != 0;
    const int scale = (c && (slice_flags & VVC355_REC_SLICE_LMCS) && p->ph_chroma_residual_scale_flag && w * h > 4) ? 8 : 0;
    const int jb = (tu->joint_cbcr_residual_flag && c) ? (1 | (p->ph_joint_cbcr_sign_flag ? 2 : 0) | ((tu->coded_flag[1] ^ tu->coded_flag[2]) & 1) << 2) : 0;
    const int qp = tb_qp(p, cu, tu, c, b->ts);
    const int x_c = b->x0 >> (c ? r->hs : 0), y_c = b->y0 >> (c ? r->vs : 0);
    const int nzw = b->max_x + 1, nzh = b->max_y + 1;
    /* bits 4 / 5 of the inter and ts records: the block's 64x64 unit minus the unit of its coding unit's origin */
    const int unit_d = ((b->x0 >> r->ls) > (cu->x0 >> r->ls) ? 16 : 0) | ((b->y0 >> r->ls) > (cu->y0 >> r->ls) ? 32 : 0);

    if (GROW(r->blk, r->blk_cap, r->n_blk + 1))
        return VVC355_REC_E_NOMEM;
    const uint32_t bi = (uint32_t)r->n_blk++;
    rec_blk *k = &r->blk[bi];
    memset(k, 0, sizeof(*k));
    k->seq = r->seq;
    k->sj = (uint8_t)(scale | jb);
    k->n_elem_log2 = (uint8_t)(lw + lh);
    k->dep[0] = k->dep[1] = -1;
    k->walk = (is_intra || cu->ciip_flag) ? W_YES : W_NO;       /* a CIIP unit's blocks: its CIIP commands overwrite what a batched pass added */
    if (k->walk == W_NO && scale) {
        const int xv = cu->x0 & ~((1 << r->ls) - 1), yv = cu->y0 & ~((1 << r->ls) - 1);
        k->walk = W_DEFERRED;
        if (xv > 0)
            k->dep[0] = ctu_of(r, xv - 1, yv);
        if (yv > 0)
            k->dep[1] = ctu_of(r, xv, yv - 1);
        if (k->dep[0] < 0 && k->dep[1] < 0)
            k->walk = W_NO;
    }
    if (b->ts) {
        const int bd = cu->bdpcm[c] != 0;
        vvc355_ts_tu *t = &k->rec.s;
        t->x0 = (int16_t)x_c, t->y0 = (int16_t)y_c;
        t->log2_w = (uint8_t)lw, t->log2_h = (uint8_t)lh, t->nzw = (uint8_t)nzw, t->nzh = (uint8_t)nzh, t->qp = (uint8_t)qp;
        t->flags = (uint8_t)(c | (bd ? VVC355_TS_TU_BDPCM : 0) | ((bd && (c ? cu->mode_c : cu->mode_y) == 50) ? VVC355_TS_TU_VERTICAL : 0) | unit_d);
        k->list = L_TS;
        k->key = (uint8_t)((c > 0) * VVC355_TS_TB_CLASSES + area_class(lw + lh));
    } else if (is_intra) {
        const int lf = cu->apply_lfnst[c] != 0;
        vvc355_intra_tu *t = &k->rec.a;
        t->log2_w = (uint8_t)lw, t->log2_h = (uint8_t)lh, t->nzw = (uint8_t)(lf ? 4 : nzw), t->nzh = (uint8_t)(lf ? 4 : nzh);
        t->c_idx = (uint8_t)c, t->qp = (uint8_t)qp;
        t->flags = (uint8_t)((dep ? VVC355_INTRA_TU_DEP_QUANT : 0) | (lf ? VVC355_INTRA_TU_LFNST : 0));
        t->tu_flags = (uint8_t)((p->mts_enabled ? VVC355_TU_MTS_ENABLED : 0) | (p->explicit_mts_intra ? VVC355_TU_EXPLICIT_MTS_INTRA : 0) |
                                (cu->isp_type ? VVC355_TU_ISP : 0) | VVC355_TU_INTRA | (cu->mip_flag ? VVC355_TU_MIP : 0));
        t->mts_idx = cu->mts_idx, t->lfnst_idx = cu->lfnst_idx;
        t->pred_mode_intra = (int8_t)(lf ? lfnst_mode(r, cu, b) : 0);
        k->list = L_INTRA;
        k->key = (uint8_t)area_class(lw + lh);
    } else {
        vvc355_inter_tu *t = &k->rec.e;
        t->x0 = (int16_t)x_c, t->y0 = (int16_t)y_c;
        t->log2_w = (uint8_t)lw, t->log2_h = (uint8_t)lh, t->nzw = (uint8_t)nzw, t->nzh = (uint8_t)nzh, t->qp = (uint8_t)qp;
        t->tu_flags = (uint8_t)((p->mts_enabled ? VVC355_TU_MTS_ENABLED : 0) | (cu->sbt_flag ? VVC355_TU_SBT : 0) |
                                (cu->sbt_horizontal ? VVC355_TU_SBT_HORIZONTAL : 0) | (cu->sbt_pos ? VVC355_TU_SBT_POS : 0));
        t->flags = (uint8_t)(c | (dep ? VVC355_INTER_TU_DEP_QUANT : 0) | unit_d);
        t->joint_mts = (uint8_t)(cu->mts_idx << 4);
        k->list = L_INTER;
        k->key = (uint8_t)((c > 0) * VVC355_INTER_TB_BINS + ((lw >= 2 && lh >= 2) ? (lw - 2) * 5 + (lh - 2) : 25));
    }

    /* the levels: packed into the recording-order stream, or copied as they are */
    const size_t n = (size_t)w * h;
    int groups = -1;
    if (p->pack_levels) {
        vvc355_tb_levels lv;
        if (GROW(r->tmp, r->tmp_cap, r->n_tmp + 16 * 64))
            return VVC355_REC_E_NOMEM;
        groups = vvc355_levels_pack(b->levels, lw, lh, r->tmp + r->n_tmp, &lv, 0);
        if (groups >= 0) {
            k = &r->blk[bi];
            k->packed = 1, k->groups = lv.groups, k->at = r->n_tmp / 16;
            r->n_tmp += 16 * (size_t)groups;
        }
    }
    if (groups < 0) {
        if (GROW(r->raw, r->raw_cap, r->n_raw + n))
            return VVC355_REC_E_NOMEM;
        memcpy(r->raw + r->n_raw, b->levels, n * sizeof(int32_t));
        r->blk[bi].at = r->n_raw;
        r->n_raw += n;
    }

    if (r->blk[bi].walk != W_NO) {
        vvc355_recon_cmd *cmd;
        int ret = push_cmd(r, VVC355_RECON_RESID, c, b->x0, b->y0, w, h, cu, &cmd);
        if (ret)
            return ret;
        cmd->resid = bi, cmd->joint = (uint8_t)scale;
        if (jb) {
            if ((ret = push_cmd(r, VVC355_RECON_RESID, 3 - c, b->x0, b->y0, w, h, cu, &cmd)))
                return ret;
            cmd->resid = bi, cmd->joint = (uint8_t)(scale | jb);
        }
    }
    return 0;
}

static int check_cu(const vvc355_recorder *r, int rs, const vvc355_rec_cu *cu, int units)
{
    const vvc355_rec_params *p = &r->p;
    const int ctb = 1 << p->ctb_log2, cx = (rs % r->ncx) << p->ctb_log2, cy = (rs / r->ncx) << p->ctb_log2;
    if (!pow2(cu->w) || !pow2(cu->h) || cu->w > 128 || cu->h > 128)
        return VVC355_REC_E_SIDE;
    if (cu->x0 < cx || cu->y0 < cy || cu->x0 + cu->w > cx + ctb || cu->y0 + cu->h > cy + ctb || cu->x0 + cu->w > p->width || cu->y0 + cu->h > p->height)
        return VVC355_REC_E_CU_RECT;
    if (cu->ciip_flag && !units)
        return VVC355_REC_E_CIIP;
    /* a CIIP unit is a single-tree inter unit: only such a unit gets the vvc355_ciip_cu its CIIP commands are paired with */
    if (cu->ciip_flag && (cu->pred_mode != 0 || cu->tree_type != 0 || cu->w < 4 || cu->h < 4 || cu->w > 64 || cu->h > 64 || cu->w * cu->h < 64))
        return VVC355_RECU_E_CIIP_SHAPE;
    if (cu->n_tus < 0 || (cu->n_tus > 0 && !cu->tus))
        return VVC355_REC_E_ARGS;
    for (int i = 0; i < cu->n_tus; i++) {
        const vvc355_rec_tu *tu = &cu->tus[i];
        if (tu->w < 1 || tu->h < 1 || tu->x0 < cu->x0 || tu->y0 < cu->y0 || tu->x0 + tu->w > cu->x0 + cu->w || tu->y0 + tu->h > cu->y0 + cu->h)
            return VVC355_REC_E_TB_RECT;
        if (tu->n_tbs < 0 || (tu->n_tbs > 0 && !tu->tbs))
            return VVC355_REC_E_ARGS;
        for (int j = 0; j < tu->n_tbs; j++) {
            const vvc355_rec_tb *b = &tu->tbs[j];
            if (b->c_idx > 2 || (b->c_idx && !p->chroma_format_idc))
                return VVC355_REC_E_C_IDX;
            if (!b->has_coeffs)
                continue;
            const int lim = b->ts ? 32 : 64;      /* transform skip is not coded above 32 */
            if (!pow2(b->w) || !pow2(b->h) || b->w > lim || b->h > lim || b->w * b->h < 4)
                return VVC355_REC_E_SIDE;
            const int lw = b->w << (b->c_idx ? r->hs : 0), lh = b->h << (b->c_idx ? r->vs : 0);
            if (b->x0 < cu->x0 || b->y0 < cu->y0 || b->x0 + lw > cu->x0 + cu->w || b->y0 + lh > cu->y0 + cu->h || b->max_x >= b->w || b->max_y >= b->h)
                return VVC355_REC_E_TB_RECT;
            if (!b->levels)
                return VVC355_REC_E_LEVELS;
        }
    }
    return 0;
}

/* predict_intra (vvc_intra.c:245-274) of transform unit i for one channel type, as commands */
static int record_predict(vvc355_recorder *r, const vvc355_rec_cu *cu, int i, int ch)
{
    const vvc355_rec_tu *tu = &cu->tus[i];
    vvc355_recon_cmd *cmd;
    int ret;
    if (cu->pred_mode != 1)
        return push_cmd(r, VVC355_RECON_MARK, ch, tu->x0, tu->y0, tu->w, tu->h, cu, NULL);
    if (ch == 0) {
        int w = tu->w;
        if (cu->isp_type == 2 && w < 4) {             /* vertical parts 1 or 2 wide: one prediction per 4 columns */
            if (i % (4 / w))
                return 0;
            w = 4;
        }
        if ((ret = push_cmd(r, VVC355_RECON_PRED, 0, tu->x0, tu->y0, w, tu->h, cu, &cmd)))
            return ret;
        cmd->mode = cu->mip_flag ? 0 : cu->mode_y;
        cmd->ref_idx = cu->ref_idx, cmd->is_mip = cu->mip_flag, cmd->mip_mode = cu->mip_mode, cmd->mip_transposed = cu->mip_transposed;
        cmd->isp_split = cu->isp_type != 0, cmd->bdpcm_flag = cu->bdpcm[0];
        return push_cmd(r, VVC355_RECON_MARK, 0, tu->x0, tu->y0, w, tu->h, cu, NULL);
    }
    if (cu->isp_type && i != cu->n_tus - 1)           /* ISP: chroma at the last partition, over the whole unit */
        return 0;
    const int x0 = cu->isp_type ? cu->x0 : tu->x0, y0 = cu->isp_type ? cu->y0 : tu->y0;
    const int w = cu->isp_type ? cu->w : tu->w, h = cu->isp_type ? cu->h : tu->h;
    if (cu->mode_c >= 81 && cu->mode_c <= 83) {
        if ((ret = push_cmd(r, VVC355_RECON_CCLM, 1, x0, y0, w, h, cu, &cmd)))
            return ret;
        cmd->mode = cu->mode_c;
    } else {
        const int direct = cu->mip_chroma_direct && cu->mip_flag;
        for (int c = 1; c <= 2; c++) {
            if ((ret = push_cmd(r, VVC355_RECON_PRED, c, x0, y0, w, h, cu, &cmd)))
                return ret;
            cmd->mode = cu->mode_c;
            cmd->is_mip = (uint8_t)direct, cmd->mip_mode = direct ? cu->mip_mode : 0, cmd->mip_transposed = direct ? cu->mip_transposed : 0;
            cmd->isp_split = cu->isp_type != 0, cmd->bdpcm_flag = cu->bdpcm[c];
        }
    }
    return push_cmd(r, VVC355_RECON_MARK, 1, x0, y0, w, h, cu, NULL);
}

/* ---------------------------------------------------------------------------------------------------------------- one CTU's unit records */

static int tiles16(int v)
{
    return (v + 15) >> 4;
}

/* a zeroed record at the end of pending list l, or NULL */
static void *unit_push(vvc355_recorder *r, int l)
{
    rec_list *L = &r->ul[l];
    L->elem = unit_elem[l];
    if (grow_((void **)&L->pend, &L->pend_cap, L->n + 1, L->elem))
        return NULL;
    void *p = L->pend + L->n++ * L->elem;
    memset(p, 0, L->elem);
    return p;
}

/* the record predicate of vvc355_mvf_unit_check (include/vvc_mi355.h) for a record the recorder is about to make: its pad_ is 0 and its link
 * is the recorder's own, which leaves the rules on sides, placement, kind and the affine / GPM bodies */
static int motion_ok(const vvc355_recorder *r, int rs, int x0, int y0, int w, int h, int kind, int aux, int pf, int gpm_pf0, int gpm_pf1)
{
    const int ctb = 1 << r->p.ctb_log2, ox = (rs % r->ncx) << r->p.ctb_log2, oy = (rs / r->ncx) << r->p.ctb_log2;
    if (w <= 0 || h <= 0 || ((w | h) & 3) || w > 128 || h > 128)
        return 0;
    if (x0 < 0 || y0 < 0 || ((x0 | y0) & 3) || x0 + w > r->p.width || y0 + h > r->p.height)
        return 0;
    if (x0 < ox || y0 < oy || x0 + w > ox + ctb || y0 + h > oy + ctb)
        return 0;
    if (kind == VVC355_MVF_AFFINE)
        return w >= 8 && h >= 8 && pow2(w) && pow2(h) && (aux == 1 || aux == 2) && (pf & 3);
    if (kind == VVC355_MVF_GPM)
        return w >= 8 && h >= 8 && w <= 64 && h <= 64 && w < 8 * h && h < 8 * w && aux <= 63 && (gpm_pf0 == 1 || gpm_pf0 == 2) && (gpm_pf1 == 1 || gpm_pf1 == 2);
    return kind == VVC355_MVF_PLAIN;
}

static int mvf_push(vvc355_recorder *r, int x0, int y0, int w, int h, int kind, int aux, const int32_t *body, int n_body, vvc355_mvf_unit **out)
{
    vvc355_mvf_unit *u = unit_push(r, U_MVF);
    if (!u)
        return VVC355_REC_E_NOMEM;
    u->x0 = (int16_t)x0, u->y0 = (int16_t)y0, u->w = (uint8_t)w, u->h = (uint8_t)h, u->kind = (uint8_t)kind, u->aux = (uint8_t)aux;
    if (body)
        memcpy(u->body, body, sizeof(int32_t) * (size_t)n_body);
    if (out)
        *out = u;
    return 0;
}

/* the unit records (set_cb_tab / set_tb_tab's call sites) and the motion records (vvc_mvs.c's three storage rules) of one coding unit */
static int record_unit(vvc355_recorder *r, int rs, int slice, const vvc355_rec_cu *cu, const vvc355_rec_pu *pu)
{
    const int chroma = r->p.chroma_format_idc != 0;
    const int inter = cu->pred_mode != 1 && cu->tree_type != 2;
    int ret;
    if (inter && (!pu || !pu->motion))
        return VVC355_RECU_E_ARGS;
    if (cu->tree_type != 2) {
        vvc355_cu_rec *c = unit_push(r, U_CU);
        if (!c || GROW(r->cu_qp, r->cu_qp_cap, r->ul[U_CU].n))
            return VVC355_REC_E_NOMEM;
        c->x0 = (int16_t)cu->x0, c->y0 = (int16_t)cu->y0, c->w = (uint8_t)cu->w, c->h = (uint8_t)cu->h;
        c->flags = inter ? (uint8_t)((pu->merge_subblock_flag != 0) | (pu->kind == VVC355_MVF_AFFINE) << 1) : 0;
        r->cu_qp[r->ul[U_CU].n - 1] = cu->qp[0];
    }
    for (int tree = cu->tree_type == 2; tree < 1 + (chroma && cu->tree_type != 1); tree++) {
        for (int i = 0; i < cu->n_tus; i++) {
            const vvc355_rec_tu *tu = &cu->tus[i];
            const int both = tu->joint_cbcr_residual_flag && tu->coded_flag[1] && tu->coded_flag[2];
            vvc355_tu_rec *t = unit_push(r, U_TU);
            if (!t || GROW(r->tu_qp, r->tu_qp_cap, 2 * r->ul[U_TU].n))
                return VVC355_REC_E_NOMEM;
            t->x0 = (int16_t)tu->x0, t->y0 = (int16_t)tu->y0, t->w = (uint8_t)tu->w, t->h = (uint8_t)tu->h;
            t->flags = tree ? (uint8_t)(0x80 | (tu->coded_flag[1] != 0) << 1 | (tu->coded_flag[2] != 0) << 2 | (tu->joint_cbcr_residual_flag != 0) << 3)
                            : (uint8_t)(tu->coded_flag[0] != 0);
            int8_t *q = r->tu_qp + 2 * (r->ul[U_TU].n - 1);
            q[0] = tree ? cu->qp[both ? 3 : 1] : 0, q[1] = tree ? cu->qp[both ? 3 : 2] : 0;
        }
    }
    /* The deblocking passes' records (vvc355_rec_deblock_tus): one per call site of set_tb_pos (vvc_ctu.c:379-401), bit 4 (pcmf, :1246) where
     * the unit is BDPCM-coded in that tree.  With ISP the chroma blocks belong to the last partition and cover the whole unit: ONE tree-1
     * record over the coding unit.  ISP partitions 1 or 2 samples wide (high) share a 4-sample column (row) of the tables: one tree-0
     * record per column (row), coded where any partition is. */
    const int isp = cu->isp_type != 0 && cu->n_tus > 0;
    const int thin_w = isp && cu->tus[0].w > 0 && cu->tus[0].w < 4, thin_h = isp && !thin_w && cu->tus[0].h > 0 && cu->tus[0].h < 4;
    const int per = thin_w ? 4 / cu->tus[0].w : thin_h ? 4 / cu->tus[0].h : 1;
    for (int tree = cu->tree_type == 2; tree < 1 + (chroma && cu->tree_type != 1); tree++) {
        const uint8_t pcm = (uint8_t)((cu->bdpcm[tree ? 1 : 0] != 0) << 4);
        const int step = tree ? 1 : per;
        for (int i = (tree && isp) ? cu->n_tus - 1 : 0; i < cu->n_tus; i += step) {
            const vvc355_rec_tu *tu = &cu->tus[i];
            const int both = tu->joint_cbcr_residual_flag && tu->coded_flag[1] && tu->coded_flag[2];
            vvc355_tu_rec *t = unit_push(r, U_TUD);
            if (!t || GROW(r->tud_qp, r->tud_qp_cap, 2 * r->ul[U_TUD].n))
                return VVC355_REC_E_NOMEM;
            t->x0 = (int16_t)tu->x0, t->y0 = (int16_t)tu->y0, t->w = (uint8_t)tu->w, t->h = (uint8_t)tu->h;
            if (tree) {
                if (isp)
                    t->x0 = (int16_t)cu->x0, t->y0 = (int16_t)cu->y0, t->w = (uint8_t)cu->w, t->h = (uint8_t)cu->h;
                t->flags = (uint8_t)(0x80 | (tu->coded_flag[1] != 0) << 1 | (tu->coded_flag[2] != 0) << 2 | (tu->joint_cbcr_residual_flag != 0) << 3 | pcm);
            } else {
                int coded = 0;
                for (int k = i; k < i + per && k < cu->n_tus; k++)
                    coded |= cu->tus[k].coded_flag[0] != 0;
                if (thin_w)
                    t->w = 4;
                if (thin_h)
                    t->h = 4;
                t->flags = (uint8_t)(coded | pcm);
            }
            int8_t *q = r->tud_qp + 2 * (r->ul[U_TUD].n - 1);
            q[0] = tree ? cu->qp[both ? 3 : 1] : 0, q[1] = tree ? cu->qp[both ? 3 : 2] : 0;
        }
    }
    if (cu->tree_type == 2)
        return 0;
    if (!inter)                                       /* ff_vvc_set_intra_mvf: a zero MvField over the unit */
        return motion_ok(r, rs, cu->x0, cu->y0, cu->w, cu->h, VVC355_MVF_PLAIN, 0, 0, 0, 0) ?
               mvf_push(r, cu->x0, cu->y0, cu->w, cu->h, VVC355_MVF_PLAIN, 0, NULL, 0, NULL) : VVC355_RECU_E_MOTION;

    vvc355_mvf_unit *u;
    if (pu->kind == VVC355_MVF_PLAIN) {
        const int nx = pu->num_sb_x, ny = pu->num_sb_y;
        if (cu->ciip_flag && (nx != 1 || ny != 1))
            return VVC355_RECU_E_CIIP_SHAPE;
        if (!nx || !ny || cu->w % nx || cu->h % ny)
            return VVC355_RECU_E_MOTION;
        const int sw = cu->w / nx, sh = cu->h / ny;
        if (!motion_ok(r, rs, cu->x0, cu->y0, cu->w, cu->h, VVC355_MVF_PLAIN, 0, 0, 0, 0) || ((sw | sh) & 3))
            return VVC355_RECU_E_MOTION;
        for (int sy = 0; sy < ny; sy++)
            for (int sx = 0; sx < nx; sx++) {
                if ((ret = mvf_push(r, cu->x0 + sx * sw, cu->y0 + sy * sh, sw, sh, VVC355_MVF_PLAIN, 0, pu->motion + 6 * (sy * nx + sx), 6, &u)))
                    return ret;
                if (cu->ciip_flag)
                    ((uint8_t *)u->body)[offsetof(vvc355_mvfield, ciip_flag)] = 1;
            }
        if (cu->ciip_flag) {
            vvc355_ciip_cu *c = unit_push(r, U_CIIP);
            if (!c)
                return VVC355_REC_E_NOMEM;
            c->x0 = (int16_t)cu->x0, c->y0 = (int16_t)cu->y0, c->cb_width = cu->w, c->cb_height = cu->h;
            c->hpel_if_idx = pu->hpel_if_idx, c->slice = (uint8_t)slice;
            c->cmd[0] = c->cmd[1] = c->cmd[2] = 0xFFFFFFFFu;
        } else {
            vvc355_inter_pu *c = unit_push(r, U_INTER);
            if (!c)
                return VVC355_REC_E_NOMEM;
            c->x0 = (int16_t)cu->x0, c->y0 = (int16_t)cu->y0, c->cb_width = cu->w, c->cb_height = cu->h;
            c->num_sb_x = (uint8_t)nx, c->num_sb_y = (uint8_t)ny, c->dmvr_flag = pu->dmvr_flag, c->bdof_flag = pu->bdof_flag;
            c->hpel_if_idx = pu->hpel_if_idx, c->slice = (uint8_t)slice;
        }
        return 0;
    }
    if (cu->ciip_flag)
        return VVC355_RECU_E_CIIP_SHAPE;
    if (pu->kind == VVC355_MVF_AFFINE) {
        const int pf = (pu->pred_flag & 3) | (pu->hpel_if_idx & 3) << 2 | (pu->bcw_idx & 15) << 4;
        if (!motion_ok(r, rs, cu->x0, cu->y0, cu->w, cu->h, VVC355_MVF_AFFINE, pu->motion_model_idc, pf, 0, 0))
            return VVC355_RECU_E_MOTION;
        if ((ret = mvf_push(r, cu->x0, cu->y0, cu->w, cu->h, VVC355_MVF_AFFINE, pu->motion_model_idc, pu->motion, 12, &u)))
            return ret;
        u->pf = (uint8_t)pf, u->ref_idx[0] = pu->ref_idx[0], u->ref_idx[1] = pu->ref_idx[1];
        u->link = (uint32_t)r->ul[U_AFFINE].n;        /* its number in recording order until end_picture */
        vvc355_affine_cu *c = unit_push(r, U_AFFINE);
        if (!c)
            return VVC355_REC_E_NOMEM;
        c->x0 = (int16_t)cu->x0, c->y0 = (int16_t)cu->y0, c->cb_width = cu->w, c->cb_height = cu->h;
        c->num_sb_x = (uint8_t)(cu->w >> 2), c->num_sb_y = (uint8_t)(cu->h >> 2), c->slice = (uint8_t)slice;
        return 0;
    }
    if (pu->kind == VVC355_MVF_GPM) {
        vvc355_mvfield part[2];
        memcpy(part, pu->motion, sizeof(part));
        if (!motion_ok(r, rs, cu->x0, cu->y0, cu->w, cu->h, VVC355_MVF_GPM, pu->gpm_partition_idx, 0, part[0].pred_flag, part[1].pred_flag))
            return VVC355_RECU_E_MOTION;
        if ((ret = mvf_push(r, cu->x0, cu->y0, cu->w, cu->h, VVC355_MVF_GPM, pu->gpm_partition_idx, pu->motion, 12, NULL)))
            return ret;
        vvc355_gpm_cu *c = unit_push(r, U_GPM);
        if (!c)
            return VVC355_REC_E_NOMEM;
        c->x0 = (int16_t)cu->x0, c->y0 = (int16_t)cu->y0, c->cb_width = cu->w, c->cb_height = cu->h;
        c->partition_idx = pu->gpm_partition_idx, c->slice = (uint8_t)slice;
        memcpy(c->gpm_mv, pu->motion, sizeof(c->gpm_mv));
        return 0;
    }
    return VVC355_RECU_E_MOTION;
}

/* ff_vvc_predict_ciip (vvc_inter.c:915) as commands: per present component the planar prediction and the blend with the inter part, which
 * vvc355_ciip_frame_build completes (resid, joint); chroma 2 wide or narrower is not blended (do_ciip, :590) */
static int record_ciip(vvc355_recorder *r, const vvc355_rec_cu *cu)
{
    int ret;
    for (int c = 0; c < (r->p.chroma_format_idc ? 3 : 1); c++) {
        if (c && (cu->w >> r->hs) <= 2)
            continue;
        if ((ret = push_cmd(r, VVC355_RECON_PRED, c, cu->x0, cu->y0, cu->w, cu->h, cu, NULL)) ||
            (ret = push_cmd(r, VVC355_RECON_CIIP, c, cu->x0, cu->y0, cu->w, cu->h, cu, NULL)))
            return ret;
    }
    return 0;
}

static int record_ctu(vvc355_recorder *r, int rs, int slice_flags, const vvc355_rec_cu *cus, int n_cus, int units, int slice, const vvc355_rec_pu *pus)
{
    if (!r)
        return VVC355_REC_E_ARGS;
    if (r->state != ST_BEGUN)
        return VVC355_REC_E_STATE;
    if (r->mode != M_NONE && r->mode != (units ? M_UNITS : M_WALK))
        return refuse(r, VVC355_RECU_E_MIXED);
    if (units && (slice < 0 || slice > 255))          /* the unit lists carry it in a byte */
        return refuse(r, VVC355_RECU_E_ARGS);
    if (n_cus < 0 || (n_cus > 0 && !cus))
        return refuse(r, VVC355_REC_E_ARGS);
    if (rs < 0 || rs >= r->ncx * r->ncy)
        return refuse(r, VVC355_REC_E_CTU_RANGE);
    if (r->ctu[rs].seen)
        return refuse(r, VVC355_REC_E_CTU_TWICE);
    int ret;
    for (int i = 0; i < n_cus; i++)
        if ((ret = check_cu(r, rs, &cus[i], units)))
            return refuse(r, ret);

    rec_ctu *t = &r->ctu[rs];
    r->mode = units ? M_UNITS : M_WALK;
    t->seen = 1;
    t->cmd_first = (uint32_t)r->n_pc, t->blk_first = (uint32_t)r->n_blk;
    for (int l = 0; l < N_UNIT_LISTS; l++)
        t->u_first[l] = (uint32_t)r->ul[l].n;
    const size_t plane = (size_t)r->tab_w * r->tab_h;
    const int chroma = r->p.chroma_format_idc != 0;
    for (int n = 0; n < n_cus; n++, r->seq++) {
        const vvc355_rec_cu *cu = &cus[n];
        if ((cu->pred_mode == 1 || cu->ciip_flag) && !t->has_intra)       /* the walk writes a CIIP unit's luma as it writes an intra unit's */
            t->has_intra = 1, t->intra_seq = r->seq;
        if (units && (ret = record_unit(r, rs, slice, cu, pus ? &pus[n] : NULL)))
            return refuse(r, ret);
        if (cu->ciip_flag && (ret = record_ciip(r, cu)))
            return refuse(r, ret);
        if (cu->tree_type != 2) {                     /* what the parser paints per 4x4 unit for the luma tree */
            for (int y = cu->y0 >> 2; y < (cu->y0 + cu->h + 3) >> 2; y++) {
                uint8_t *row = r->tab + (size_t)y * r->tab_w + (cu->x0 >> 2);
                const size_t len = (size_t)((cu->x0 + cu->w + 3) >> 2) - (cu->x0 >> 2);
                memset(row, cu->mip_flag, len);
                memset(row + plane, (uint8_t)cu->mode_y, len);
                memset(row + 2 * plane, cu->pred_mode, len);
            }
        }
        if (!cu->coded_flag) {
            for (int ch = 0; ch < 2; ch++)
                if ((ret = push_cmd(r, VVC355_RECON_MARK, ch, cu->x0, cu->y0, cu->w, cu->h, cu, NULL)))
                    return refuse(r, ret);
            continue;
        }
        for (int ch = cu->tree_type == 2; ch < 1 + (chroma && cu->tree_type != 1); ch++) {
            for (int i = 0; i < cu->n_tus; i++) {
                const vvc355_rec_tu *tu = &cu->tus[i];
                if ((ret = record_predict(r, cu, i, ch)))
                    return refuse(r, ret);
                for (int j = 0; j < tu->n_tbs; j++) {
                    const vvc355_rec_tb *b = &tu->tbs[j];
                    if ((b->c_idx > 0) == ch && b->has_coeffs && (ret = record_block(r, slice_flags, cu, tu, b)))
                        return refuse(r, ret);
                }
            }
        }
    }
    t = &r->ctu[rs];
    t->cmd_n = (uint32_t)r->n_pc - t->cmd_first, t->blk_n = (uint32_t)r->n_blk - t->blk_first;
    for (int l = 0; l < N_UNIT_LISTS; l++) {
        t->u_n[l] = (uint32_t)r->ul[l].n - t->u_first[l];
        if ((l <= U_MVF || l == U_TUD) && t->u_n[l] > 65535)           /* what the device passes read of one CTU's range */
            return refuse(r, VVC355_RECU_E_COUNT);
    }
    return 0;
}

int vvc355_rec_ctu(vvc355_recorder *r, int rs, int slice_flags, const vvc355_rec_cu *cus, int n_cus)
{
    return record_ctu(r, rs, slice_flags, cus, n_cus, 0, 0, NULL);
}

int vvc355_rec_ctu_units(vvc355_recorder *r, int rs, int slice_flags, int slice, const vvc355_rec_cu *cus, const vvc355_rec_pu *pus, int n_cus)
{
    return record_ctu(r, rs, slice_flags, cus, n_cus, 1, slice, pus);
}

/* ---------------------------------------------------------------------------------------------------------------- the picture */

static const int list_keys[N_LISTS] = { 5, 2 * VVC355_INTER_TB_BINS, 2 * VVC355_TS_TB_CLASSES };

/* the unit lists from recording order into raster CTU order, with what depends on that order: the ctu_first tables, the running job and
 * scratch sums, the affine records' numbers in the motion records that link them */
static int units_in_raster_order(vvc355_recorder *r)
{
    const int n_ctu = r->ncx * r->ncy, chroma = r->p.chroma_format_idc != 0;
    vvc355_rec_units_result *o = &r->units;
    memset(o, 0, sizeof(*o));
    for (int l = 0; l < N_UNIT_LISTS; l++) {
        rec_list *L = &r->ul[l];
        L->elem = unit_elem[l];
        if (grow_((void **)&L->out, &L->out_cap, L->n + 1, L->elem) || (l <= U_MVF && GROW(r->ctu_first[l], r->ctu_first_cap[l], (size_t)n_ctu + 1)))
            return -1;
    }
    if (GROW(r->cu_qp_out, r->cu_qp_out_cap, r->ul[U_CU].n + 1) || GROW(r->tu_qp_out, r->tu_qp_out_cap, 2 * r->ul[U_TU].n + 2) ||
        GROW(r->tud_qp_out, r->tud_qp_out_cap, 2 * r->ul[U_TUD].n + 2) || GROW(r->tud_first, r->tud_first_cap, (size_t)n_ctu + 1))
        return -1;
    size_t at[N_UNIT_LISTS] = { 0 };
    for (int rs = 0; rs < n_ctu; rs++) {
        const rec_ctu *t = &r->ctu[rs];
        if (t->u_n[U_CU])
            memcpy(r->cu_qp_out + at[U_CU], r->cu_qp + t->u_first[U_CU], t->u_n[U_CU]);
        if (t->u_n[U_TU])
            memcpy(r->tu_qp_out + 2 * at[U_TU], r->tu_qp + 2 * (size_t)t->u_first[U_TU], 2 * (size_t)t->u_n[U_TU]);
        if (t->u_n[U_TUD])
            memcpy(r->tud_qp_out + 2 * at[U_TUD], r->tud_qp + 2 * (size_t)t->u_first[U_TUD], 2 * (size_t)t->u_n[U_TUD]);
        r->tud_first[rs] = (int32_t)at[U_TUD];
        vvc355_mvf_unit *mv = (vvc355_mvf_unit *)r->ul[U_MVF].out + at[U_MVF];
        for (int l = 0; l < N_UNIT_LISTS; l++) {
            const rec_list *L = &r->ul[l];
            if (l <= U_MVF)
                r->ctu_first[l][rs] = (int32_t)at[l];
            if (t->u_n[l])
                memcpy(L->out + at[l] * L->elem, L->pend + t->u_first[l] * L->elem, t->u_n[l] * L->elem);
        }
        for (uint32_t i = 0; i < t->u_n[U_MVF]; i++)
            if (mv[i].kind == VVC355_MVF_AFFINE)
                mv[i].link = (uint32_t)at[U_AFFINE] + (mv[i].link - t->u_first[U_AFFINE]);
        for (int l = 0; l < N_UNIT_LISTS; l++)
            at[l] += t->u_n[l];
    }
    for (int l = 0; l <= U_MVF; l++)
        r->ctu_first[l][n_ctu] = (int32_t)at[l];
    r->tud_first[n_ctu] = (int32_t)at[U_TUD];
    r->deblock.tu = (const vvc355_tu_rec *)r->ul[U_TUD].out, r->deblock.tu_qp_c = r->tud_qp_out, r->deblock.ctu_first_tu = r->tud_first;
    r->deblock.n_tu = (int32_t)at[U_TUD], r->deblock.pad_ = 0;
    vvc355_inter_pu *pu = (vvc355_inter_pu *)r->ul[U_INTER].out;
    for (size_t i = 0; i < at[U_INTER]; i++) {
        pu[i].first_job = (uint32_t)o->n_inter_jobs;
        o->n_inter_jobs += pu[i].num_sb_x * pu[i].num_sb_y * tiles16(pu[i].cb_width / pu[i].num_sb_x) * tiles16(pu[i].cb_height / pu[i].num_sb_y);
    }
    vvc355_affine_cu *af = (vvc355_affine_cu *)r->ul[U_AFFINE].out;
    for (size_t i = 0; i < at[U_AFFINE]; i++) {
        af[i].first_job = (uint32_t)o->n_affine_jobs;
        o->n_affine_jobs += af[i].num_sb_x * af[i].num_sb_y;
    }
    vvc355_gpm_cu *gp = (vvc355_gpm_cu *)r->ul[U_GPM].out;
    for (size_t i = 0; i < at[U_GPM]; i++) {
        gp[i].first_job = (uint32_t)o->n_gpm_jobs;
        o->n_gpm_jobs += tiles16(gp[i].cb_width) * tiles16(gp[i].cb_height) + (chroma ? 2 * tiles16(gp[i].cb_width >> r->hs) * tiles16(gp[i].cb_height >> r->vs) : 0);
    }
    vvc355_ciip_cu *ci = (vvc355_ciip_cu *)r->ul[U_CIIP].out;
    for (size_t i = 0; i < at[U_CIIP]; i++) {
        const int w = ci[i].cb_width, h = ci[i].cb_height, wc = w >> r->hs, hc = h >> r->vs;
        ci[i].first_job = (uint32_t)o->n_ciip_jobs, ci[i].scratch_off = (uint32_t)o->ciip_scratch_len;
        o->n_ciip_jobs += tiles16(w) * tiles16(h) + (chroma ? 2 * tiles16(wc) * tiles16(hc) : 0);
        o->ciip_scratch_len += w * h + ((chroma && wc > 2) ? 2 * wc * hc : 0);
    }
    o->cu = (const vvc355_cu_rec *)r->ul[U_CU].out, o->cu_qp = r->cu_qp_out, o->tu = (const vvc355_tu_rec *)r->ul[U_TU].out, o->tu_qp_c = r->tu_qp_out;
    o->ctu_first_cu = r->ctu_first[U_CU], o->ctu_first_tu = r->ctu_first[U_TU], o->ctu_first_mvf = r->ctu_first[U_MVF];
    o->mvf = (const vvc355_mvf_unit *)r->ul[U_MVF].out;
    o->inter = pu, o->affine = af, o->gpm = gp, o->ciip = ci;
    o->n_cu = (int32_t)at[U_CU], o->n_tu = (int32_t)at[U_TU], o->n_mvf = (int32_t)at[U_MVF], o->n_inter = (int32_t)at[U_INTER];
    o->n_affine = (int32_t)at[U_AFFINE], o->n_gpm = (int32_t)at[U_GPM], o->n_ciip = (int32_t)at[U_CIIP];
    return 0;
}

int vvc355_rec_end_picture(vvc355_recorder *r, vvc355_rec_result *res)
{
    if (!r || !res)
        return VVC355_REC_E_ARGS;
    if (r->state != ST_BEGUN)
        return VVC355_REC_E_STATE;
    const int n_ctu = r->ncx * r->ncy;
    memset(res, 0, sizeof(*res));
    if (GROW(r->cmds, r->cmds_cap, r->n_pc + 1) || GROW(r->cmd_slot, r->cmd_slot_cap, r->n_pc + 1) || GROW(r->out_ctu, r->out_ctu_cap, (size_t)n_ctu) ||
        GROW(r->order, r->order_cap, (size_t)n_ctu) || GROW(r->recs, r->recs_cap, 16 * (r->n_blk + 1)) || GROW(r->lv, r->lv_cap, r->n_blk + 1) ||
        GROW(r->fin, r->fin_cap, r->n_blk + 1) || GROW(r->levels, r->levels_cap, r->n_tmp + 16))
        return refuse(r, VVC355_REC_E_NOMEM);

    /* KEEP of the deferred blocks, now that every CTU's units are known */
    for (size_t i = 0; i < r->n_blk; i++) {
        rec_blk *k = &r->blk[i];
        if (k->walk == W_DEFERRED) {
            int keep = 0, early = 0;
            for (int d = 0; d < 2; d++) {
                if (k->dep[d] >= 0 && r->ctu[k->dep[d]].has_intra) {
                    keep = 1;
                    early |= r->ctu[k->dep[d]].intra_seq < k->seq;
                }
            }
            k->walk = keep ? W_YES : W_NO;
            res->walk_scaled += keep;
            res->late_keep += keep && !early;
        }
        if (k->walk == W_YES)
            res->keep++;
        else if (k->sj & 8)
            res->batched_scaled++;
    }

    /* group: stable counting sort per list, CTUs in raster order */
    int32_t first[N_LISTS][N_KEYS + 1];
    memset(first, 0, sizeof(first));
    for (int rs = 0; rs < n_ctu; rs++)
        for (uint32_t i = 0; i < r->ctu[rs].blk_n; i++) {
            const rec_blk *k = &r->blk[r->ctu[rs].blk_first + i];
            first[k->list][k->key + 1]++;
        }
    int32_t n_list[N_LISTS], base[N_LISTS], next[N_LISTS][N_KEYS];
    for (int l = 0, b = 0; l < N_LISTS; l++) {
        for (int q = 0; q < list_keys[l]; q++)
            first[l][q + 1] += first[l][q];
        n_list[l] = first[l][list_keys[l]];
        base[l] = b;
        b += n_list[l];
        for (int q = 0; q < list_keys[l]; q++)
            next[l][q] = base[l] + first[l][q];
    }
    r->n_rec = r->n_blk;
    for (int rs = 0; rs < n_ctu; rs++)
        for (uint32_t i = 0; i < r->ctu[rs].blk_n; i++) {
            const uint32_t bi = r->ctu[rs].blk_first + i;
            r->fin[next[r->blk[bi].list][r->blk[bi].key]++] = bi;
        }

    /* slots, records, side records and the level stream, in list order */
    uint64_t slot = 0;
    uint32_t run = 0;
    for (size_t f = 0; f < r->n_rec; f++) {
        rec_blk *k = &r->blk[r->fin[f]];
        const int keep = k->walk == W_YES;
        k->slot = (uint32_t)slot;
        slot += (((uint64_t)1 << k->n_elem_log2) + 3) & ~(uint64_t)3;
        if (k->list == L_INTRA) {
            k->rec.a.coeff_off = k->slot;
        } else if (k->list == L_INTER) {
            k->rec.e.coeff_off = k->slot;
            k->rec.e.flags |= keep ? VVC355_INTER_TU_KEEP : 0;
            k->rec.e.joint_mts |= keep ? 0 : k->sj;
        } else {
            k->rec.s.coeff_off = k->slot;
            k->rec.s.flags |= keep ? VVC355_TS_TU_KEEP : 0;
            k->rec.s.joint = keep ? 0 : k->sj;
        }
        memcpy(r->recs + 16 * f, &k->rec, 16);
        vvc355_tb_levels *lv = &r->lv[f];
        lv->groups = 0, lv->first = run, lv->flags = VVC355_LEVELS_INT32;
        if (k->packed) {
            int n = 0;
            for (uint64_t g = k->groups; g; g &= g - 1)
                n++;
            memcpy(r->levels + 16 * (size_t)run, r->tmp + 16 * k->at, 32 * (size_t)n);
            lv->groups = k->groups, lv->flags = 0;
            run += (uint32_t)n;
        }
    }
    memset(r->levels + 16 * (size_t)run, 0, 32);

    if (r->mode != M_WALK && units_in_raster_order(r))
        return refuse(r, VVC355_REC_E_NOMEM);
    /* the CIIP unit whose commands come next: both are in raster CTU order; never past the list, whatever the commands say */
    vvc355_ciip_cu *ciip = (vvc355_ciip_cu *)r->ul[U_CIIP].out, *const ciip_end = ciip ? ciip + r->ul[U_CIIP].n : NULL;

    /* commands: CTUs in raster order; a CTU keeps its list when it holds an intra unit or a residual of the walk */
    r->n_cmds = 0;
    for (int rs = 0; rs < n_ctu; rs++) {
        const rec_ctu *t = &r->ctu[rs];
        vvc355_recon_ctu *o = &r->out_ctu[rs];
        const size_t start = r->n_cmds;
        int any_resid = 0;
        o->first_cmd = o->n_cmd = o->flags = 0;
        for (uint32_t i = 0; i < t->cmd_n; i++) {
            const vvc355_recon_cmd *c = &r->pc[t->cmd_first + i];
            uint32_t s = 0;
            if (c->kind == VVC355_RECON_RESID) {
                const rec_blk *k = &r->blk[c->resid];
                if (k->walk != W_YES)
                    continue;
                any_resid = 1;
                s = k->slot;
            } else if (c->kind == VVC355_RECON_CIIP) {   /* a CIIP unit's CTU keeps its list: the index is final */
                if (ciip < ciip_end && c->c_idx == 0 && ciip->cmd[0] != 0xFFFFFFFFu)
                    ciip++;
                if (ciip < ciip_end)
                    ciip->cmd[c->c_idx] = (uint32_t)r->n_cmds;
            }
            r->cmds[r->n_cmds] = *c;
            r->cmds[r->n_cmds].resid = s;
            r->cmd_slot[r->n_cmds++] = s;
        }
        if (t->has_intra || any_resid) {
            o->first_cmd = (uint32_t)start, o->n_cmd = (uint32_t)(r->n_cmds - start);
            r->ctu[rs].kind = t->has_intra ? 2 : 1;
        } else {
            r->n_cmds = start;
        }
    }
    for (int rs = 0; rs < n_ctu; rs++) {
        if (r->ctu[rs].kind != 1)
            continue;
        const int rx = rs % r->ncx, ry = rs / r->ncx;
        r->out_ctu[rs].flags = VVC355_RECON_CTU_LIGHT | ((rx && r->ctu[rs - 1].kind == 2) ? VVC355_RECON_CTU_LUMA_LEFT : 0) |
                               ((ry && r->ctu[rs - r->ncx].kind == 2) ? VVC355_RECON_CTU_LUMA_UP : 0);
    }

    res->cmds = r->cmds, res->ctus = r->out_ctu, res->order = r->order;
    res->n_cmds = (int32_t)r->n_cmds, res->n_ctus = n_ctu;
    res->n_work = vvc355_recon_order(r->out_ctu, r->ncx, r->ncy, r->order);
    res->n_intra = n_list[L_INTRA], res->n_inter = n_list[L_INTER], res->n_ts = n_list[L_TS];
    res->intra = (const vvc355_intra_tu *)r->recs;
    res->inter = (const vvc355_inter_tu *)(r->recs + 16 * (size_t)base[L_INTER]);
    res->ts = (const vvc355_ts_tu *)(r->recs + 16 * (size_t)base[L_TS]);
    res->intra_lv = r->lv, res->inter_lv = r->lv + base[L_INTER], res->ts_lv = r->lv + base[L_TS];
    res->levels = r->levels, res->n_levels = 16 * ((uint64_t)run + 1), res->arena_len = slot;
    for (int q = 0; q < 6; q++)
        res->class_first[q] = first[L_INTRA][q];
    for (int ch = 0; ch < 2; ch++) {
        for (int q = 0; q <= VVC355_INTER_TB_BINS; q++)
            res->bin_first[ch][q] = first[L_INTER][ch * VVC355_INTER_TB_BINS + q];
        for (int q = 0; q <= VVC355_TS_TB_CLASSES; q++)
            res->ts_first[ch][q] = first[L_TS][ch * VVC355_TS_TB_CLASSES + q];
    }
    r->state = ST_ENDED;
    return 0;
}

int vvc355_rec_units(const vvc355_recorder *r, vvc355_rec_units_result *out)
{
    if (!r)
        return VVC355_REC_E_ARGS;
    if (!out)
        return VVC355_RECU_E_ARGS;
    if (r->state != ST_ENDED)
        return VVC355_REC_E_STATE;
    if (r->mode == M_WALK)
        return VVC355_RECU_E_MIXED;
    *out = r->units;
    return 0;
}

int vvc355_rec_deblock_units(const vvc355_recorder *r, vvc355_rec_deblock_tus *out)
{
    if (!r)
        return VVC355_REC_E_ARGS;
    if (!out)
        return VVC355_RECU_E_ARGS;
    if (r->state != ST_ENDED)
        return VVC355_REC_E_STATE;
    if (r->mode == M_WALK)
        return VVC355_RECU_E_MIXED;
    *out = r->deblock;
    return 0;
}

int vvc355_rec_fill_arena(const vvc355_recorder *r, int32_t *arena)
{
    if (!r || !arena)
        return VVC355_REC_E_ARGS;
    if (r->state != ST_ENDED)
        return VVC355_REC_E_STATE;
    for (size_t f = 0; f < r->n_rec; f++) {
        const rec_blk *k = &r->blk[r->fin[f]];
        if (!k->packed)
            memcpy(arena + k->slot, r->raw + k->at, sizeof(int32_t) << k->n_elem_log2);
    }
    return 0;
}

int vvc355_rec_bind(vvc355_recorder *r, uint64_t arena_dev)
{
    if (!r)
        return VVC355_REC_E_ARGS;
    if (r->state != ST_ENDED)
        return VVC355_REC_E_STATE;
    for (size_t i = 0; i < r->n_cmds; i++)
        if (r->cmds[i].kind == VVC355_RECON_RESID)
            r->cmds[i].resid = arena_dev + 4 * (uint64_t)r->cmd_slot[i];
    return 0;
}
