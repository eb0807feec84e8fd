/*
 * oracle/ref_shim_intra.c — the static functions of the reference's vvc_intra.c, made callable, (second part of the file) the
 * slots that take a VVCLocalContext, called on real structs filled from the mirror context of include/vvc_mi355_ctx.h, and (third part)
 * ref_recon_picture: ff_vvc_reconstruct itself over a whole picture built from plain arrays.
 *
 * TEST INFRASTRUCTURE ONLY, second translation unit of oracle/_ref/libvvcref.so (see ref_shim.c).  The reference file is
 * compiled into this unit by the #include below, resolved at build time from the reference tree; its ten external names
 * are renamed first so that they do not collide with the copies in the reference's archive.  ref_dequant,
 * ref_derive_transform_type and ref_ilfnst_transform have exactly the orc_<slot> signatures of vvc_oracle.h: each fills real
 * VVCLocalContext / VVCFrameContext / VVCSPS / SliceContext / CodingUnit / TransformUnit / TransformBlock objects so that
 * the reference derives the flattened arguments itself, then calls the static function.
 *
 * Outside the domain a flattened argument list has no context that yields it; the functions then leave the block alone
 * (dequant) or return -1, so that a comparison fails loudly instead of comparing something else.
 */
#define ff_vvc_reconstruct             shimdup_reconstruct
#define ff_vvc_get_mip_size_id         shimdup_get_mip_size_id
#define ff_vvc_nscale_derive           shimdup_nscale_derive
#define ff_vvc_need_pdpc               shimdup_need_pdpc
#define ff_vvc_get_top_available       shimdup_get_top_available
#define ff_vvc_get_left_available      shimdup_get_left_available
#define ff_vvc_ref_filter_flag_derive  shimdup_ref_filter_flag_derive
#define ff_vvc_intra_pred_angle_derive shimdup_intra_pred_angle_derive
#define ff_vvc_intra_inv_angle_derive  shimdup_intra_inv_angle_derive
#define ff_vvc_wide_angle_mode_mapping shimdup_wide_angle_mode_mapping
#include "libavcodec/vvc/vvc_intra.c"

#define REF_API __attribute__((visibility("default")))

/* the flag bits of the flattened tu_flags argument (ORC_TU_* / VVC355_TU_*) */
enum { TU_MTS_ENABLED = 1, TU_EXPLICIT_MTS_INTRA = 2, TU_ISP = 4, TU_SBT = 8, TU_SBT_HORIZONTAL = 16, TU_SBT_POS = 32, TU_INTRA = 64, TU_MIP = 128 };

/* one set of real objects, wired together afresh by every call (the tests are single-threaded) */
#define TAB_W 64                                /* min_cb_width of the little picture behind the tables: 64 x 64 4x4 units */
static VVCLocalContext    lc;
static VVCFrameContext    fc;
static SliceContext       sc;
static VVCSPS             sps;
static VVCPPS             pps;
static H266RawSPS         raw_sps;
static H266RawSliceHeader raw_sh;
static VVCScalingList     sl;
static CodingUnit         cu;
static TransformUnit      tu;
static uint8_t            tab_imf[TAB_W * TAB_W], tab_ipm[TAB_W * TAB_W], tab_cpm[TAB_W * TAB_W];

/* the flat default matrix is filled once at decoder start-up by a static function of vvcdec.c (init_default_scale_m): every factor 16 */
__attribute__((constructor)) static void ref_intra_init(void)
{
    memset(ff_vvc_default_scale_m, 16, sizeof(ff_vvc_default_scale_m));
}

static TransformBlock *wire(int c_idx, int w, int h, int *coeffs)
{
    TransformBlock *tb;
    memset(&lc, 0, sizeof(lc));
    memset(&fc, 0, sizeof(fc));
    memset(&sc, 0, sizeof(sc));
    memset(&sps, 0, sizeof(sps));
    memset(&pps, 0, sizeof(pps));
    memset(&raw_sps, 0, sizeof(raw_sps));
    memset(&raw_sh, 0, sizeof(raw_sh));
    memset(&sl, 0, sizeof(sl));
    memset(&cu, 0, sizeof(cu));
    memset(&tu, 0, sizeof(tu));
    sps.r      = &raw_sps;
    sc.sh.r    = &raw_sh;
    fc.ps.sps  = &sps;
    fc.ps.pps  = &pps;
    fc.tab.imf = tab_imf;
    fc.tab.ipm = tab_ipm;
    fc.tab.cpm[0] = fc.tab.cpm[1] = tab_cpm;
    lc.fc = &fc;
    lc.sc = &sc;
    lc.cu = &cu;
    sps.min_cb_log2_size_y = 2;
    pps.min_cb_width       = TAB_W;
    tu.nb_tbs = 1;
    tb = &tu.tbs[0];
    tb->has_coeffs    = 1;
    tb->c_idx         = (uint8_t)c_idx;
    tb->tb_width      = w;
    tb->tb_height     = h;
    tb->log2_tb_width  = av_log2(w);
    tb->log2_tb_height = av_log2(h);
    tb->coeffs        = coeffs;
    return tb;
}

/*
 * The contexts behind one flattened argument list are not unique: the colour component, the prediction mode and joint
 * Cb-Cr coding only select which cu->qp[] entry and which scaling-list id the reference reads.  The shim walks through all
 * seven choices as a function of the arguments, so that every row of derive_qp and of derive_scale_m's id table is used,
 * and installs the given matrix and DC at the id the reference selects.
 */
REF_API void ref_dequant(int *coeffs, int log2_w, int log2_h, int min_x, int min_y, int max_x, int max_y, int qp, int ts,
    int dep_quant, int bit_depth, int log2_transform_range, const uint8_t *scale_matrix, int log2_matrix_size, int dc)
{
    static const int ids[2][3][6] = {          /* Table 38 (the id the reference will select; read here only to install the matrix there) */
        { { 0, 2, 8, 14, 20, 26 }, { 0, 3, 9, 15, 21, 21 }, { 0, 4, 10, 16, 22, 22 } },
        { { 0, 5, 11, 17, 23, 27 }, { 0, 6, 12, 18, 24, 24 }, { 1, 7, 13, 19, 25, 25 } },
    };
    const int max_log2 = log2_w > log2_h ? log2_w : log2_h;
    const int variant  = (qp + min_x + max_y + log2_w) % 7;
    const int inter    = variant < 6 ? variant / 3 : 0;
    const int c_idx    = variant < 6 ? variant % 3 : 1 + (qp & 1);
    const int jcbcr    = variant == 6;
    TransformBlock *tb;
    int id, qp_idx;

    if (max_log2 < 1 || max_log2 > 6 || log2_w < 0 || log2_h < 0)
        return;                                 /* no 1x1 transform block: the id table has no column for it */
    id = ids[inter][c_idx][max_log2 - 1];
    if (scale_matrix) {
        if (ts)
            return;                             /* transform skip never reads a scaling list (derive_scale_m) */
        if (log2_matrix_size != (id < 2 ? 1 : id < 8 ? 2 : 3))
            return;                             /* the matrix size follows from the block size */
        if (dc >= 0 && id < SL_START_16x16)
            return;                             /* only the 16x16 and larger matrices carry a DC value */
    }

    tb = wire(c_idx, 1 << log2_w, 1 << log2_h, coeffs);
    tb->ts         = (uint8_t)ts;
    tb->min_scan_x = min_x;
    tb->min_scan_y = min_y;
    tb->max_scan_x = max_x;
    tb->max_scan_y = max_y;

    sps.bit_depth            = (uint8_t)bit_depth;
    sps.qp_bd_offset         = (uint8_t)(6 * (bit_depth - 8));
    sps.log2_transform_range = (uint8_t)log2_transform_range;
    raw_sh.sh_dep_quant_used_flag = (uint8_t)dep_quant;
    cu.pred_mode = inter ? MODE_INTER : MODE_INTRA;
    if (jcbcr) {
        tu.joint_cbcr_residual_flag = 1;
        tu.coded_flag[CB] = tu.coded_flag[CR] = 1;
    }
    /* derive_qp: luma adds QpBdOffset to cu->qp[LUMA], chroma reads the primed value as it is */
    qp_idx = jcbcr ? JCBCR : c_idx;
    for (int i = 0; i < 4; i++)
        cu.qp[i] = -128;                        /* an entry the reference must not read */
    cu.qp[qp_idx] = (int8_t)(c_idx ? qp : qp - sps.qp_bd_offset);

    if (scale_matrix) {
        raw_sh.sh_explicit_scaling_list_used_flag = 1;
        fc.ps.sl = &sl;
        memcpy(sl.scaling_matrix_rec[id], scale_matrix, (size_t)1 << (2 * log2_matrix_size));
        if (id >= SL_START_16x16)               /* the reference always overrides there: "no DC" is the matrix's own first entry */
            sl.scaling_matrix_dc_rec[id - SL_START_16x16] = (uint8_t)(dc >= 0 ? dc : scale_matrix[0]);
    }
    dequant(&lc, &tu, tb);
}

REF_API int ref_derive_transform_type(int flags, int mts_idx, int lfnst_idx, int c_idx, int w, int h)
{
    enum TxType trh, trv;
    TransformBlock *tb = wire(c_idx, w, h, NULL);

    raw_sps.sps_mts_enabled_flag                = !!(flags & TU_MTS_ENABLED);
    raw_sps.sps_explicit_mts_intra_enabled_flag = !!(flags & TU_EXPLICIT_MTS_INTRA);
    cu.isp_split_type      = (flags & TU_ISP) ? ISP_HOR_SPLIT : ISP_NO_SPLIT;
    cu.sbt_flag            = !!(flags & TU_SBT);
    cu.sbt_horizontal_flag = !!(flags & TU_SBT_HORIZONTAL);
    cu.sbt_pos_flag        = !!(flags & TU_SBT_POS);
    cu.pred_mode           = (flags & TU_INTRA) ? MODE_INTRA : MODE_INTER;
    cu.intra_mip_flag      = !!(flags & TU_MIP);
    cu.lfnst_idx           = lfnst_idx;
    cu.mts_idx             = (MtsIdx)mts_idx;
    derive_transform_type(&fc, &lc, tb, &trh, &trv);
    return (int)trh | ((int)trv << 4);
}

/*
 * pred_mode_intra is what derive_ilfnst_pred_mode_intra returns, after the wide-angle mapping.  The shim undoes the mapping
 * (it is one-to-one for a given shape) and hands the reference the unmapped mode by one of the routes that function has,
 * chosen by the arguments: the luma mode of the coding unit, MIP (planar), a CCLM chroma block that takes the mode of the
 * collocated luma block (ipm), of a collocated MIP block (planar) or of a collocated IBC / palette block (DC), or a plain
 * chroma mode.  Returns the scan limit the reference leaves in the block (max_scan + 1), or -1 where the reference derives
 * another mode than the one given: the argument is then not reachable for that shape.
 */
enum { ROUTE_LUMA, ROUTE_LUMA_MIP, ROUTE_CCLM_IPM, ROUTE_CCLM_MIP, ROUTE_CCLM_IBC, ROUTE_CCLM_PLT, ROUTE_CHROMA, N_ROUTES };
static int route_calls[N_ROUTES];

/* calls of ref_ilfnst_transform that went by `route` (the enum above) and came out with the mode given, since the last reset (route < 0);
 * -1 for a route there is not.  A test reads it to see that a case list takes every branch of derive_ilfnst_pred_mode_intra. */
REF_API int ref_ilfnst_route_calls(int route)
{
    if (route < 0)
        memset(route_calls, 0, sizeof(route_calls));
    return route >= 0 && route < N_ROUTES ? route_calls[route] : -1;
}

REF_API int ref_ilfnst_transform(int *coeffs, int w, int h, int pred_mode_intra, int lfnst_idx, int log2_transform_range)
{
    const int unmapped = pred_mode_intra > 66 ? pred_mode_intra - 65 : pred_mode_intra < 0 ? pred_mode_intra + 67 : pred_mode_intra;
    const int route    = (pred_mode_intra + 16 + (w >> 2) + (h >> 1) + lfnst_idx) & 3;
    const int chroma   = route >= 2;
    const int hs = chroma ? (w >> 3) & 1 : 1, vs = chroma ? (h >> 3) & 1 : 1;       /* 4:2:0, 4:2:2, 4:4:4 and the transposed 4:2:2 geometry */
    const int x0 = 8 * ((pred_mode_intra + 16) & 7), y0 = 8 * (lfnst_idx + (w >> 4));
    TransformBlock *tb;
    int x_tb, y_tb, x_c, y_c, taken;

    if (w < 4 || h < 4 || w > 64 || h > 64 || unmapped < 0 || unmapped > 66)
        return -1;
    tb = wire(chroma ? 1 + (lfnst_idx & 1) : 0, w, h, coeffs);
    tb->x0 = x0;
    tb->y0 = y0;
    tb->max_scan_x = tb->max_scan_y = 3;
    sps.log2_transform_range = (uint8_t)log2_transform_range;
    sps.hshift[1] = sps.hshift[2] = (uint8_t)hs;
    sps.vshift[1] = sps.vshift[2] = (uint8_t)vs;
    cu.lfnst_idx = lfnst_idx;
    cu.pred_mode = MODE_INTRA;
    cu.isp_split_type = ISP_NO_SPLIT;
    cu.cb_width  = chroma ? w << hs : w;
    cu.cb_height = chroma ? h << vs : h;
    cu.intra_pred_mode_y = INTRA_VERT;          /* overwritten by the route that reads it */
    cu.intra_pred_mode_c = INTRA_HORZ;

    x_tb = x0 >> 2;
    y_tb = y0 >> 2;
    x_c  = (x0 + (w << hs >> 1)) >> 2;
    y_c  = (y0 + (h << vs >> 1)) >> 2;
    /* everywhere but at the positions the reference has to read, the tables say the opposite */
    memset(tab_imf, 1, sizeof(tab_imf));
    memset(tab_ipm, unmapped == INTRA_DC ? INTRA_PLANAR : INTRA_DC, sizeof(tab_ipm));
    memset(tab_cpm, MODE_IBC, sizeof(tab_cpm));
    tab_imf[y_tb * TAB_W + x_tb] = 0;
    tab_imf[y_c * TAB_W + x_c]   = 0;
    tab_cpm[y_c * TAB_W + x_c]   = MODE_INTRA;

    if (!chroma) {
        if (route == 1 && unmapped == INTRA_PLANAR) {
            tab_imf[y_tb * TAB_W + x_tb] = 1;                  /* MIP block: planar whatever the luma mode says */
            taken = ROUTE_LUMA_MIP;
        } else {
            cu.intra_pred_mode_y = unmapped;
            taken = ROUTE_LUMA;
        }
    } else if (route == 2) {
        cu.intra_pred_mode_c = INTRA_LT_CCLM + (h >> 2) % 3;
        if (unmapped == INTRA_PLANAR && (w & 8)) {
            tab_imf[y_c * TAB_W + x_c] = 1;                    /* collocated MIP block */
            tab_ipm[y_c * TAB_W + x_c] = INTRA_VERT;
            taken = ROUTE_CCLM_MIP;
        } else if (unmapped == INTRA_DC && (w & 24)) {
            tab_cpm[y_c * TAB_W + x_c] = (w & 8) ? MODE_IBC : MODE_PLT;
            tab_ipm[y_c * TAB_W + x_c] = INTRA_VERT;
            taken = (w & 8) ? ROUTE_CCLM_IBC : ROUTE_CCLM_PLT;
        } else {
            tab_ipm[y_c * TAB_W + x_c] = (uint8_t)unmapped;
            taken = ROUTE_CCLM_IPM;
        }
    } else {
        tab_imf[y_tb * TAB_W + x_tb] = 1;                      /* not read for chroma */
        cu.intra_pred_mode_c = unmapped;
        taken = ROUTE_CHROMA;
    }

    if (derive_ilfnst_pred_mode_intra(&lc, tb) != pred_mode_intra)
        return -1;
    route_calls[taken]++;
    ilfnst_transform(&lc, tb);
    return tb->max_scan_x == tb->max_scan_y ? tb->max_scan_x + 1 : -1;
}

/* ------------------------------------------------------------------ the slots that take a VVCLocalContext
 *
 * The callers hand over the plain-C mirror of include/vvc_mi355_ctx.h (what tests/ctx_mirror.py builds).  That header and the
 * reference's both define VVCLocalContext, so the layout is declared here once more under names of its own; ref_ctx_layout exports
 * sizes and offsets for the test that holds the three declarations together.  Every call copies the mirror member by member into
 * the real objects above and calls the real slot of the ff_vvc_dsp_init table, or the real availability function.
 */
#undef ff_vvc_get_top_available
#undef ff_vvc_get_left_available
int ff_vvc_get_top_available(const VVCLocalContext *lc, int x, int y, int target_size, int c_idx);          /* the archive's own copies */
int ff_vvc_get_left_available(const VVCLocalContext *lc, int x, int y, int target_size, int c_idx);

#define MIR_MAX_PARTS 1024
typedef struct MirArea { int x, y, w, h; } MirArea;
typedef struct MirCodingUnit {
    int      x0, y0, cb_width, cb_height;
    int      intra_pred_mode_y, intra_pred_mode_c;
    uint8_t  intra_luma_ref_idx, isp_split_type, mip_chroma_direct_flag;
    uint8_t  bdpcm_flag[3];
} MirCodingUnit;
typedef struct MirFrameContext {
    uint8_t *data[3];
    int      linesize[3];
    int      width, height;
    int      bit_depth;
    uint8_t  hshift[3], vshift[3];
    uint8_t  ctb_log2_size_y, min_cb_log2_size_y;
    int      min_cb_width;
    uint8_t  sps_entropy_coding_sync_enabled_flag, sps_chroma_vertical_collocated_flag;
    const uint8_t *imf, *imm, *imtf;
    struct {
        uint8_t  min_bin_idx, max_bin_idx;
        uint16_t pivot[17], chroma_scale_coeff[16];
    } lmcs;
} MirFrameContext;
typedef struct MirLocalContext {
    MirFrameContext *fc;
    const MirCodingUnit *cu;
    MirArea  ras[2][MIR_MAX_PARTS];
    int      num_ras[2];
    struct { int cand_up_left; } na;
    uint8_t  ctb_left_flag, ctb_up_flag;
    int      end_of_tiles_x;
    struct { int x_vpdu, y_vpdu, chroma_scale; } lmcs;
} MirLocalContext;

REF_API int ref_ctx_layout(int what)
{
    switch (what) {
    case 0:  return (int)sizeof(MirLocalContext);
    case 1:  return (int)sizeof(MirFrameContext);
    case 2:  return (int)sizeof(MirCodingUnit);
    case 3:  return (int)offsetof(MirLocalContext, num_ras);
    case 4:  return (int)offsetof(MirLocalContext, end_of_tiles_x);
    case 5:  return (int)offsetof(MirLocalContext, lmcs);
    case 6:  return (int)offsetof(MirFrameContext, imf);
    case 7:  return (int)offsetof(MirFrameContext, lmcs);
    case 8:  return (int)offsetof(MirCodingUnit, bdpcm_flag);
    default: return -1;
    }
}

static AVFrame frame;

static void load_ctx(const MirLocalContext *m)
{
    const MirFrameContext *mf = m->fc;
    const MirCodingUnit *mc = m->cu;

    wire(0, 4, 4, NULL);
    memset(&frame, 0, sizeof(frame));
    fc.frame = &frame;
    for (int c = 0; c < 3; c++) {
        frame.data[c]     = mf->data[c];
        frame.linesize[c] = mf->linesize[c];
        sps.hshift[c]     = mf->hshift[c];
        sps.vshift[c]     = mf->vshift[c];
        cu.bdpcm_flag[c]  = mc->bdpcm_flag[c];
    }
    sps.bit_depth          = (uint8_t)mf->bit_depth;
    sps.pixel_shift        = mf->bit_depth > 8;
    sps.ctb_log2_size_y    = mf->ctb_log2_size_y;
    sps.ctb_size_y         = 1 << mf->ctb_log2_size_y;
    sps.min_cb_log2_size_y = mf->min_cb_log2_size_y;
    raw_sps.sps_entropy_coding_sync_enabled_flag = mf->sps_entropy_coding_sync_enabled_flag;
    raw_sps.sps_chroma_vertical_collocated_flag  = mf->sps_chroma_vertical_collocated_flag;
    pps.width        = (uint16_t)mf->width;
    pps.height       = (uint16_t)mf->height;
    pps.min_cb_width = (uint16_t)mf->min_cb_width;
    fc.tab.imf  = (uint8_t *)mf->imf;
    fc.tab.imm  = (uint8_t *)mf->imm;
    fc.tab.imtf = (uint8_t *)mf->imtf;
    fc.ps.lmcs.min_bin_idx = mf->lmcs.min_bin_idx;
    fc.ps.lmcs.max_bin_idx = mf->lmcs.max_bin_idx;
    memcpy(fc.ps.lmcs.pivot, mf->lmcs.pivot, sizeof(mf->lmcs.pivot));
    memcpy(fc.ps.lmcs.chroma_scale_coeff, mf->lmcs.chroma_scale_coeff, sizeof(mf->lmcs.chroma_scale_coeff));
    ff_vvc_dsp_init(&fc.vvcdsp, mf->bit_depth);

    cu.x0 = mc->x0;
    cu.y0 = mc->y0;
    cu.cb_width  = mc->cb_width;
    cu.cb_height = mc->cb_height;
    cu.pred_mode = MODE_INTRA;
    cu.intra_pred_mode_y = mc->intra_pred_mode_y;
    cu.intra_pred_mode_c = mc->intra_pred_mode_c;
    cu.intra_luma_ref_idx     = mc->intra_luma_ref_idx;
    cu.isp_split_type         = mc->isp_split_type == 0 ? ISP_NO_SPLIT : mc->isp_split_type == 2 ? ISP_VER_SPLIT : ISP_HOR_SPLIT;
    cu.mip_chroma_direct_flag = mc->mip_chroma_direct_flag;

    for (int t = 0; t < 2; t++) {
        lc.num_ras[t] = m->num_ras[t] < MIR_MAX_PARTS ? m->num_ras[t] : MIR_MAX_PARTS;
        for (int i = 0; i < lc.num_ras[t]; i++) {
            lc.ras[t][i].x = m->ras[t][i].x;
            lc.ras[t][i].y = m->ras[t][i].y;
            lc.ras[t][i].w = m->ras[t][i].w;
            lc.ras[t][i].h = m->ras[t][i].h;
        }
    }
    lc.na.cand_up_left   = m->na.cand_up_left;
    lc.ctb_left_flag     = m->ctb_left_flag;
    lc.ctb_up_flag       = m->ctb_up_flag;
    lc.end_of_tiles_x    = m->end_of_tiles_x;
    lc.lmcs.x_vpdu       = m->lmcs.x_vpdu;
    lc.lmcs.y_vpdu       = m->lmcs.y_vpdu;
    lc.lmcs.chroma_scale = m->lmcs.chroma_scale;
}

REF_API void ref_intra_pred_ctx(const MirLocalContext *m, int x0, int y0, int width, int height, int c_idx)
{
    load_ctx(m);
    fc.vvcdsp.intra.intra_pred(&lc, x0, y0, width, height, c_idx);
}

REF_API void ref_intra_cclm_pred_ctx(const MirLocalContext *m, int x0, int y0, int width, int height)
{
    load_ctx(m);
    fc.vvcdsp.intra.intra_cclm_pred(&lc, x0, y0, width, height);
}

/* the per-VPDU cache of the scale travels in and back through the mirror, so that no call depends on the one before it */
REF_API void ref_lmcs_scale_chroma_ctx(MirLocalContext *m, int *dst, const int *coeff, int width, int height, int x0_cu, int y0_cu)
{
    load_ctx(m);
    fc.vvcdsp.intra.lmcs_scale_chroma(&lc, dst, coeff, width, height, x0_cu, y0_cu);
    m->lmcs.x_vpdu       = lc.lmcs.x_vpdu;
    m->lmcs.y_vpdu       = lc.lmcs.y_vpdu;
    m->lmcs.chroma_scale = lc.lmcs.chroma_scale;
}

REF_API int ref_top_available(const MirLocalContext *m, int x, int y, int target_size, int c_idx)
{
    load_ctx(m);
    return ff_vvc_get_top_available(&lc, x, y, target_size, c_idx);
}

REF_API int ref_left_available(const MirLocalContext *m, int x, int y, int target_size, int c_idx)
{
    load_ctx(m);
    return ff_vvc_get_left_available(&lc, x, y, target_size, c_idx);
}

/* ------------------------------------------------------------------ the RECON walk of a whole picture: ff_vvc_reconstruct itself
 *
 * ref_recon_picture builds, from plain arrays, the objects the reference's RECON stage reads — SPS / PPS / picture header / one
 * SliceContext per slice, the CTU table with CodingUnit and TransformUnit lists allocated through ff_refstruct_allocz (the reference
 * frees them), and the tables the parser paints per coding unit (imf, imm, imtf, ipm, cpm) — and calls the reference's own
 * ff_vvc_reconstruct (compiled into this unit as shimdup_reconstruct) for every CTU in raster order.  The planes are reconstructed in
 * place; they hold the inter prediction where a unit is not intra.  The levels are copied: the reference transforms them in place.
 *
 * One slot of the table is replaced: intra.lmcs_scale_chroma becomes a callback that calls the real slot and then appends what the
 * reference cached in lc->lmcs (x_vpdu, y_vpdu, chroma_scale) to the caller's log.
 *
 * Every member of the arrays is an int32 (addresses: uint64), so that a numpy record array mirrors them without padding rules.
 * Returns what ff_vvc_reconstruct returned last (0), or -1 for a picture these objects cannot hold: a unit with ciip_flag
 * (ff_vvc_predict_ciip needs the inter machinery), more than MIR_MAX_SLICES slices, a transform unit with more than three blocks,
 * a block beyond 64 samples, a unit outside its CTU.
 *
 * The wiring is mir_recon_build / mir_recon_free (declared in ref_shim_mir.h with the arrays), shared with ref_decode_picture of
 * ref_shim_picture.c, which completes the same objects with the inter machinery and takes units with ciip_flag.
 */
#include "libavcodec/refstruct.h"
#include "ref_shim_mir.h"

REF_API int ref_recon_layout(int what)
{
    switch (what) {
    case 0:  return (int)sizeof(MirReconPic);
    case 1:  return (int)sizeof(MirReconCu);
    case 2:  return (int)sizeof(MirReconTu);
    case 3:  return (int)sizeof(MirReconTb);
    case 4:  return (int)offsetof(MirReconPic, stride);
    case 5:  return (int)offsetof(MirReconPic, n_slices);
    default: return -1;
    }
}

static SliceContext         rc_sc[MIR_MAX_SLICES];
static H266RawSliceHeader   rc_sh[MIR_MAX_SLICES];
static H266RawPictureHeader rc_ph;
static MirReconPic         *rc_pic;
static void (*rc_real_scale)(VVCLocalContext *lc, int *dst, const int *coeff, int w, int h, int x0_cu, int y0_cu);

static void rc_scale_hook(VVCLocalContext *l, int *dst, const int *coeff, int w, int h, int x0_cu, int y0_cu)
{
    int32_t *log = (int32_t *)(uintptr_t)rc_pic->scale_log;
    rc_real_scale(l, dst, coeff, w, h, x0_cu, y0_cu);
    if (log && rc_pic->n_scale_log < rc_pic->scale_log_cap) {
        int32_t *e = log + 3 * rc_pic->n_scale_log;
        e[0] = l->lmcs.x_vpdu;
        e[1] = l->lmcs.y_vpdu;
        e[2] = l->lmcs.chroma_scale;
    }
    rc_pic->n_scale_log++;                      /* counts on past the capacity: the caller sees that the log was too short */
}

static void rc_paint(uint8_t *tab, int pitch, const MirReconCu *m, int v)
{
    for (int y = m->y0 >> 2; y < (m->y0 + m->h + 3) >> 2; y++)
        memset(tab + y * pitch + (m->x0 >> 2), v, (size_t)((m->w + 3) >> 2));
}

int mir_recon_build(MirReconPic *p, MirReconObjs *o, int ciip)
{
    const int ctb = 1 << p->ctb_log2, ncx = (p->width + ctb - 1) >> p->ctb_log2, ncy = (p->height + ctb - 1) >> p->ctb_log2;
    const int pitch = (p->width + 3) >> 2, units = pitch * ((p->height + 3) >> 2);
    const int hs = p->chroma_format_idc == 1 || p->chroma_format_idc == 2, vs = p->chroma_format_idc == 1;
    const int32_t *first = (const int32_t *)(uintptr_t)p->ctu_first_cu;
    const MirReconCu *cus = (const MirReconCu *)(uintptr_t)p->cus;
    const MirReconTu *tus = (const MirReconTu *)(uintptr_t)p->tus;
    const MirReconTb *tbs = (const MirReconTb *)(uintptr_t)p->tbs;
    uint8_t *tabs = NULL;
    int *levels = NULL;
    CTU *ctus = NULL;

    memset(o, 0, sizeof(*o));
    p->n_scale_log = 0;
    if (p->n_slices < 1 || p->n_slices > MIR_MAX_SLICES || p->ctb_log2 < 5 || p->ctb_log2 > 7 || p->chroma_format_idc < 0 || p->chroma_format_idc > 3 ||
        (p->bit_depth != 8 && p->bit_depth != 10 && p->bit_depth != 12))
        return -1;

    wire(0, 4, 4, NULL);
    memset(&frame, 0, sizeof(frame));
    memset(rc_sc, 0, sizeof(rc_sc));
    memset(rc_sh, 0, sizeof(rc_sh));
    memset(&rc_ph, 0, sizeof(rc_ph));
    rc_pic = p;
    fc.frame = &frame;
    for (int c = 0; c < 3; c++) {
        frame.data[c]     = (uint8_t *)(uintptr_t)p->plane[c];
        frame.linesize[c] = p->stride[c];
        sps.hshift[c]     = (uint8_t)(c ? hs : 0);
        sps.vshift[c]     = (uint8_t)(c ? vs : 0);
    }
    sps.width = pps.width = (uint16_t)p->width;
    sps.height = pps.height = (uint16_t)p->height;
    sps.bit_depth            = (uint8_t)p->bit_depth;
    sps.pixel_shift          = p->bit_depth > 8;
    sps.qp_bd_offset         = (uint8_t)(6 * (p->bit_depth - 8));
    sps.log2_transform_range = (uint8_t)p->log2_transform_range;
    sps.ctb_log2_size_y      = (uint8_t)p->ctb_log2;
    sps.ctb_size_y           = (uint8_t)ctb;
    sps.min_cb_log2_size_y   = 2;
    raw_sps.sps_chroma_format_idc                 = (uint8_t)p->chroma_format_idc;
    raw_sps.sps_entropy_coding_sync_enabled_flag  = (uint8_t)p->wpp;
    raw_sps.sps_chroma_vertical_collocated_flag   = (uint8_t)p->collocated;
    raw_sps.sps_mts_enabled_flag                  = (uint8_t)p->mts_enabled;
    raw_sps.sps_explicit_mts_intra_enabled_flag   = (uint8_t)p->explicit_mts_intra;
    raw_sps.sps_explicit_mts_inter_enabled_flag   = (uint8_t)p->explicit_mts_inter;
    raw_sps.sps_min_qp_prime_ts                   = (uint8_t)p->min_qp_prime_ts;
    pps.min_cb_width  = (uint16_t)pitch;
    pps.ctb_width     = (uint16_t)ncx;
    pps.ctb_height    = (uint16_t)ncy;
    pps.ctb_to_col_bd = (uint16_t *)(uintptr_t)p->col_bd;
    pps.ctb_to_row_bd = (uint16_t *)(uintptr_t)p->row_bd;
    rc_ph.ph_joint_cbcr_sign_flag       = (uint8_t)p->joint_cbcr_sign;
    rc_ph.ph_chroma_residual_scale_flag = (uint8_t)p->chroma_residual_scale;
    fc.ps.ph.r = &rc_ph;
    fc.ps.lmcs.min_bin_idx = (uint8_t)p->lmcs_min_bin_idx;
    fc.ps.lmcs.max_bin_idx = (uint8_t)p->lmcs_max_bin_idx;
    for (int i = 0; i < 17; i++)
        fc.ps.lmcs.pivot[i] = (uint16_t)p->lmcs_pivot[i];
    for (int i = 0; i < 16; i++)
        fc.ps.lmcs.chroma_scale_coeff[i] = (uint16_t)p->lmcs_chroma_scale_coeff[i];
    for (int s = 0; s < p->n_slices; s++) {
        rc_sc[s].sh.r = &rc_sh[s];
        rc_sh[s].sh_dep_quant_used_flag = (uint8_t)((const int32_t *)(uintptr_t)p->slice_dep_quant)[s];
        rc_sh[s].sh_lmcs_used_flag      = (uint8_t)((const int32_t *)(uintptr_t)p->slice_lmcs_used)[s];
    }
    fc.tab.slice_idx = (int16_t *)(uintptr_t)p->slice_idx;
    ff_vvc_dsp_init(&fc.vvcdsp, p->bit_depth);
    rc_real_scale = fc.vvcdsp.intra.lmcs_scale_chroma;
    fc.vvcdsp.intra.lmcs_scale_chroma = rc_scale_hook;

    tabs   = calloc(6, (size_t)units);
    levels = malloc(sizeof(int) * (size_t)(p->n_levels > 0 ? p->n_levels : 1));
    ctus   = calloc((size_t)(ncx * ncy), sizeof(*ctus));
    if (!tabs || !levels || !ctus)
        goto done;
    memcpy(levels, (const void *)(uintptr_t)p->levels, sizeof(int) * (size_t)(p->n_levels > 0 ? p->n_levels : 0));
    fc.tab.imf  = tabs;
    fc.tab.imm  = tabs + units;
    fc.tab.imtf = tabs + 2 * units;
    fc.tab.ipm  = tabs + 3 * units;
    fc.tab.cpm[0] = tabs + 4 * units;
    fc.tab.cpm[1] = tabs + 5 * units;
    fc.tab.ctus = ctus;

    /* the units: lists per CTU, and what the parser paints per unit (set_cu_tabs, vvc_ctu.c) */
    for (int rs = 0; rs < ncx * ncy; rs++) {
        CodingUnit **link = &ctus[rs].cus;
        for (int i = first[rs]; i < first[rs + 1]; i++) {
            const MirReconCu *m = &cus[i];
            CodingUnit *u;
            TransformUnit **tlink;
            if ((m->ciip_flag && (!ciip || m->pred_mode || m->tree_type)) || m->n_tus < 0 || m->w < 1 || m->h < 1 || m->x0 < 0 || m->y0 < 0 || m->x0 + m->w > p->width || m->y0 + m->h > p->height ||
                (m->x0 >> p->ctb_log2) != rs % ncx || (m->y0 >> p->ctb_log2) != rs / ncx || m->w > ctb || m->h > ctb)
                goto done;
            u = ff_refstruct_allocz(sizeof(*u));
            if (!u)
                goto done;
            *link = u;
            link = &u->next;
            u->tree_type = m->tree_type == 1 ? DUAL_TREE_LUMA : m->tree_type == 2 ? DUAL_TREE_CHROMA : SINGLE_TREE;
            u->ch_type   = m->tree_type == 2;
            u->x0 = m->x0; u->y0 = m->y0; u->cb_width = m->w; u->cb_height = m->h;
            u->pred_mode  = m->pred_mode ? MODE_INTRA : MODE_INTER;
            u->coded_flag = (uint8_t)m->coded_flag;
            u->ciip_flag  = (uint8_t)m->ciip_flag;
            u->sbt_flag = (uint8_t)m->sbt_flag; u->sbt_horizontal_flag = (uint8_t)m->sbt_horizontal; u->sbt_pos_flag = (uint8_t)m->sbt_pos;
            u->lfnst_idx = m->lfnst_idx;
            u->mts_idx   = (MtsIdx)m->mts_idx;
            u->intra_luma_ref_idx = (uint8_t)m->ref_idx;
            u->intra_mip_flag     = (uint8_t)m->mip_flag;
            u->isp_split_type     = m->isp_type == 1 ? ISP_HOR_SPLIT : m->isp_type == 2 ? ISP_VER_SPLIT : ISP_NO_SPLIT;
            u->num_intra_subpartitions = m->num_isp;
            u->intra_pred_mode_y  = m->mode_y;
            u->intra_pred_mode_c  = m->mode_c;
            u->mip_chroma_direct_flag = m->mip_chroma_direct;
            for (int c = 0; c < 3; c++) {
                u->bdpcm_flag[c]       = m->bdpcm[c];
                u->apply_lfnst_flag[c] = m->apply_lfnst[c];
            }
            for (int k = 0; k < 4; k++)
                u->qp[k] = (int8_t)m->qp[k];
            if (m->tree_type != 2) {
                rc_paint(fc.tab.imf, pitch, m, m->mip_flag);
                rc_paint(fc.tab.imm, pitch, m, m->mip_mode);
                rc_paint(fc.tab.imtf, pitch, m, m->mip_transposed);
                rc_paint(fc.tab.ipm, pitch, m, m->mode_y);
                rc_paint(fc.tab.cpm[0], pitch, m, u->pred_mode);
            }
            if (m->tree_type != 1)
                rc_paint(fc.tab.cpm[1], pitch, m, u->pred_mode);
            tlink = &u->tus.head;
            for (int j = m->first_tu; j < m->first_tu + m->n_tus; j++) {
                const MirReconTu *mt = &tus[j];
                TransformUnit *t;
                if (mt->n_tbs < 0 || mt->n_tbs > VVC_MAX_SAMPLE_ARRAYS)
                    goto done;
                t = ff_refstruct_allocz(sizeof(*t));
                if (!t)
                    goto done;
                *tlink = t;
                tlink = &t->next;
                u->tus.tail = t;
                t->x0 = mt->x0; t->y0 = mt->y0; t->width = mt->w; t->height = mt->h;
                t->joint_cbcr_residual_flag = (uint8_t)mt->joint;
                for (int c = 0; c < 3; c++)
                    t->coded_flag[c] = (uint8_t)mt->coded_flag[c];
                t->nb_tbs = (uint8_t)mt->n_tbs;
                for (int k = 0; k < mt->n_tbs; k++) {
                    const MirReconTb *mb = &tbs[mt->first_tb + k];
                    TransformBlock *b = &t->tbs[k];
                    if (mb->w < 1 || mb->h < 1 || mb->w > 64 || mb->h > 64 || mb->c_idx < 0 || mb->c_idx > 2 ||
                        (mb->has_coeffs && ((mb->w & (mb->w - 1)) || (mb->h & (mb->h - 1)))) ||         /* the uncoded part of an SBT unit may be 3/4 of a side */
                        mb->level_off < 0 || mb->level_off + mb->w * mb->h > p->n_levels || mb->max_x >= mb->w || mb->max_y >= mb->h || mb->min_x < 0 || mb->min_y < 0)
                        goto done;
                    b->has_coeffs = (uint8_t)mb->has_coeffs;
                    b->c_idx = (uint8_t)mb->c_idx;
                    b->ts    = (uint8_t)mb->ts;
                    b->x0 = mb->x0; b->y0 = mb->y0;
                    b->tb_width = mb->w; b->tb_height = mb->h;
                    b->log2_tb_width = av_log2(mb->w); b->log2_tb_height = av_log2(mb->h);
                    b->min_scan_x = mb->min_x; b->min_scan_y = mb->min_y; b->max_scan_x = mb->max_x; b->max_scan_y = mb->max_y;
                    b->coeffs = levels + mb->level_off;
                }
            }
        }
    }

    o->lc = &lc; o->fc = &fc; o->sps = &sps; o->pps = &pps; o->sc = rc_sc; o->sh = rc_sh;
    o->ctus = ctus; o->ncx = ncx; o->n_ctb = ncx * ncy; o->tabs = tabs; o->levels = levels;
    return 0;

done:
    o->ctus = ctus; o->n_ctb = ncx * ncy; o->tabs = tabs; o->levels = levels;
    mir_recon_free(o);
    return -1;
}

void mir_recon_free(MirReconObjs *o)
{
    if (o->ctus)
        for (int rs = 0; rs < o->n_ctb; rs++)
            ff_vvc_ctu_free_cus(&o->ctus[rs]);
    free(o->ctus);
    free(o->levels);
    free(o->tabs);
    memset(o, 0, sizeof(*o));
    rc_pic = NULL;
}

REF_API int ref_recon_picture(MirReconPic *p)
{
    MirReconObjs o;
    int ret = 0;

    if (mir_recon_build(p, &o, 0))
        return -1;
    for (int rs = 0; rs < o.n_ctb && !ret; rs++) {
        const int s = fc.tab.slice_idx[rs];
        if (s < 0 || s >= p->n_slices) {
            ret = -1;
            break;
        }
        lc.sc = &rc_sc[s];
        ret = shimdup_reconstruct(&lc, rs, rs % o.ncx, rs / o.ncx);
    }
    mir_recon_free(&o);
    return ret;
}
