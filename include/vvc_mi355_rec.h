/*
 * vvc_mi355_rec.h — the recorder: from a decoder's parsed units to the inputs of the RECON walk and the three TB record passes.
 *
 * Host C (ffvvc_amd/host/recorder.c, linked into libvvc_mi355.so), no device work.  A decoder hands over every CTU's coding units as it
 * parses them; at the end of the picture the recorder has derived, by the rules of INTEGRATION.md section 3,
 *   the per-CTU command lists (MARK / PRED / CCLM / RESID, one command per reference call in the reference's order), the CTU table with
 *   the LIGHT / LUMA_LEFT / LUMA_UP flags and the ticket order of vvc355_recon_order;
 *   the three grouped record lists vvc355_intra_tu / vvc355_inter_tu / vvc355_ts_tu with their first-tables, the vvc355_tb_levels paired
 *   with them by index and the int16 level stream;
 *   the arena slot of every block, and which chroma residuals stay with the walk (KEEP).
 *
 * KEEP is decided in vvc355_rec_end_picture, over the whole picture: a scaled chroma block of an inter unit stays with the walk when the CTU
 * that holds the luma left of or above its unit's 64x64 unit contains an intra unit.  CTUs arrive in any order (tiles, wavefront), and with
 * CtbSizeY 128 that CTU can be the block's own, so the answer can depend on units parsed later.
 *
 * With vvc355_rec_ctu_units in place of vvc355_rec_ctu the same walk also takes CIIP units (their PRED + CIIP commands, the vvc355_ciip_cu
 * list; every coded block of such a unit is KEEP, and their CTU counts as one that holds an intra unit) and records, from one
 * vvc355_rec_pu per coding unit, what the deblocking and motion side of a picture reads: the vvc355_cu_rec / vvc355_tu_rec lists with their
 * QP sidecars, the vvc355_mvf_unit list, and the vvc355_inter_pu / vvc355_affine_cu / vvc355_gpm_cu lists with their running job sums, all
 * grouped per CTU in raster order whatever the order of the calls (vvc355_rec_units after vvc355_rec_end_picture; the transform-unit
 * records for the deblocking passes from vvc355_rec_deblock_units).
 * Of the statistics, keep counts a CIIP unit's blocks; walk_scaled and late_keep count what the neighbour rule above keeps, as before.
 *
 * Out of scope here: scaling lists, ACT; SAO / ALF / deblocking parameters stay with the caller.
 *
 * Threads: a recorder object is used by ONE thread at a time.  A decoder that parses CTUs on several threads serialises its
 * vvc355_rec_ctu / vvc355_rec_ctu_units calls (or keeps one recorder per picture and a lock around it); different recorder objects are independent.
 */
#ifndef VVC_MI355_REC_H
#define VVC_MI355_REC_H

#include "vvc_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- input: the project's own flat PODs, filled by in-tree glue from whatever the parser keeps.  Read during vvc355_rec_ctu only: the
 * recorder copies what it needs (levels included), the caller may reuse its memory as soon as the call returns. */

/* one transform block; 32 bytes, no implicit padding */
typedef struct vvc355_rec_tb {
    const int32_t *levels;     /* w * h int32 levels, row-major, as residual coding left them; read with has_coeffs only */
    int32_t  x0, y0;           /* LUMA coordinates (tb->x0, tb->y0) */
    int16_t  w, h;             /* the component's samples (tb_width, tb_height) */
    uint8_t  c_idx, ts, has_coeffs, pad0_;
    uint8_t  min_x, min_y, max_x, max_y;   /* the scan window; the records' nzw / nzh are max_x + 1 / max_y + 1 */
    uint32_t pad1_;
} vvc355_rec_tb;

/* one transform unit; 32 bytes, no implicit padding */
typedef struct vvc355_rec_tu {
    const vvc355_rec_tb *tbs;
    int32_t  n_tbs;
    int32_t  x0, y0;           /* luma samples */
    int16_t  w, h;
    uint8_t  coded_flag[3];
    uint8_t  joint_cbcr_residual_flag;
    uint32_t pad_;
} vvc355_rec_tu;

/* one coding unit; 56 bytes, no implicit padding */
typedef struct vvc355_rec_cu {
    const vvc355_rec_tu *tus;  /* in decoding order */
    int32_t  n_tus;
    int32_t  x0, y0;           /* luma samples */
    int16_t  w, h;             /* cb_width, cb_height */
    uint8_t  pred_mode;        /* 0 inter, 1 intra (MODE_INTRA); other values count as not intra */
    uint8_t  tree_type;        /* 0 single, 1 dual-tree luma, 2 dual-tree chroma */
    uint8_t  coded_flag, ciip_flag;
    int8_t   mode_y, mode_c;   /* intra_pred_mode_y / intra_pred_mode_c as parsed (before the wide-angle mapping) */
    uint8_t  ref_idx;          /* intra_luma_ref_idx */
    uint8_t  mip_flag, mip_mode, mip_transposed, mip_chroma_direct;
    uint8_t  isp_type;         /* 0 none, 1 horizontal, 2 vertical split */
    uint8_t  bdpcm[3];
    uint8_t  lfnst_idx, apply_lfnst[3], mts_idx;
    uint8_t  sbt_flag, sbt_horizontal, sbt_pos;
    int8_t   qp[4];            /* cu->qp[LUMA, CB, CR, JOINT_CBCR] */
    uint8_t  pad_[5];
} vvc355_rec_cu;

/* a picture's parameters; 48 bytes, no implicit padding */
typedef struct vvc355_rec_params {
    int32_t  width, height;    /* luma samples, 1..32767 */
    uint8_t  ctb_log2;         /* 5..7 */
    uint8_t  bit_depth;        /* 8..16 */
    uint8_t  log2_transform_range;
    uint8_t  chroma_format_idc;            /* 0..3 */
    int8_t   qp_bd_offset;     /* 6 * (bit_depth - 8) */
    uint8_t  sps_min_qp_prime_ts;
    uint8_t  mts_enabled, explicit_mts_intra, explicit_mts_inter;   /* the last is not read today: no VVC355_TU_* bit carries it, an inter
                                                                     * unit's mts_idx is 0 without it */
    uint8_t  ph_joint_cbcr_sign_flag, ph_chroma_residual_scale_flag;
    uint8_t  pack_levels;      /* 1 = vvc355_levels_pack per block (blocks it declines stay VVC355_LEVELS_INT32); 0 = every block int32 in the arena */
    uint8_t  pad_[28];
} vvc355_rec_params;

enum { VVC355_REC_SLICE_DEP_QUANT = 1, VVC355_REC_SLICE_LMCS = 2 };    /* slice_flags: sh_dep_quant_used_flag, sh_lmcs_used_flag */

/* ---- output: HOST pointers into the recorder's own buffers, valid until the next vvc355_rec_begin_picture (or _destroy) */
typedef struct vvc355_rec_result {
    const vvc355_recon_cmd *cmds;          /* RESID commands carry their arena slot (int32 elements) in `resid` until vvc355_rec_bind */
    const vvc355_recon_ctu *ctus;          /* n_ctus = ctb_width * ctb_height entries, raster order */
    const int32_t *order;                  /* n_work entries: vvc355_recon_order's */
    const vvc355_intra_tu *intra;          /* grouped by area class, see class_first */
    const vvc355_inter_tu *inter;          /* luma then chroma, grouped by shape bin, see bin_first */
    const vvc355_ts_tu *ts;                /* luma then chroma, grouped by area class, see ts_first */
    const vvc355_tb_levels *intra_lv, *inter_lv, *ts_lv;   /* paired with the lists by index; with pack_levels 0 every entry is {0, 0, INT32} */
    const int16_t *levels;                 /* the level stream: the lists' groups in list order (intra, inter, ts), then one group of zeros */
    uint64_t n_levels;                     /* int16 elements of `levels`, the closing group included */
    uint64_t arena_len;                    /* int32 elements: every block has a slot, a multiple of 4 elements long, back to back */
    int32_t  n_cmds, n_ctus, n_work;
    int32_t  n_intra, n_inter, n_ts;
    int32_t  class_first[6];
    int32_t  bin_first[2][VVC355_INTER_TB_BINS + 1];
    int32_t  ts_first[2][VVC355_TS_TB_CLASSES + 1];
    int32_t  keep;             /* blocks whose add stays with the walk (a RESID command each, two for a joint unit) */
    int32_t  batched_scaled;   /* scaled chroma blocks the TB passes add through the scale table */
    int32_t  walk_scaled;      /* scaled chroma blocks of inter units kept in the walk */
    int32_t  late_keep;        /* of walk_scaled: blocks recorded before the first intra unit of every CTU that keeps them in the walk —
                                * what a decision taken while parsing would have got wrong.  Depends on the order of the vvc355_rec_ctu calls. */
} vvc355_rec_result;

/* what the calls return for input they refuse.  A refused vvc355_rec_ctu or vvc355_rec_end_picture leaves the recorder as
 * vvc355_rec_begin_picture left it: the picture's CTUs are recorded again. */
enum {
    VVC355_REC_E_ARGS = -1,        /* a null recorder, parameter block, unit list or result */
    VVC355_REC_E_STATE = -2,       /* no picture begun (or, for fill_arena / bind, no picture ended) */
    VVC355_REC_E_PARAMS = -3,      /* picture parameters outside the ranges above */
    VVC355_REC_E_CTU_RANGE = -4,   /* a CTU index outside the grid */
    VVC355_REC_E_CTU_TWICE = -5,   /* a CTU given twice */
    VVC355_REC_E_CU_RECT = -6,     /* a coding unit outside its CTU or the picture */
    VVC355_REC_E_TB_RECT = -7,     /* a transform unit or transform block outside its coding unit, or a scan window outside its block */
    VVC355_REC_E_SIDE = -8,        /* a side that is not a power of two, or above 64 for a coded block / 128 for a coding unit */
    VVC355_REC_E_C_IDX = -9,       /* c_idx above 2, or a chroma block at 4:0:0 */
    VVC355_REC_E_LEVELS = -10,     /* a coded block without levels */
    VVC355_REC_E_CIIP = -11,       /* a CIIP unit given to vvc355_rec_ctu: vvc355_rec_ctu_units records those */
    VVC355_REC_E_NOMEM = -12
};

typedef struct vvc355_recorder vvc355_recorder;

vvc355_recorder *vvc355_rec_create(void);
void vvc355_rec_destroy(vvc355_recorder *rec);
/* Starts a picture (dropping one that was begun and not ended).  The object is reusable: its buffers grow and are kept. */
int vvc355_rec_begin_picture(vvc355_recorder *rec, const vvc355_rec_params *params);
/* One CTU's coding units in decoding order; rs = its raster index; once per CTU, CTUs in any order.  A CTU that is never given has no
 * commands and counts as holding no intra unit. */
int vvc355_rec_ctu(vvc355_recorder *rec, int rs, int slice_flags, const vvc355_rec_cu *cus, int n_cus);
/* Derives everything and fills *result; returns 0.  The picture is then ended: the next call of the cycle is vvc355_rec_begin_picture. */
int vvc355_rec_end_picture(vvc355_recorder *rec, vvc355_rec_result *result);
/* After end_picture: writes the int32 levels of the blocks that are not packed into their slots of `arena` (HOST, arena_len elements) and
 * nothing else. */
int vvc355_rec_fill_arena(const vvc355_recorder *rec, int32_t *arena);
/* After end_picture: turns the RESID commands' slots into addresses inside the DEVICE arena at arena_dev (may be called again with another
 * base: the slots are kept aside). */
int vvc355_rec_bind(vvc355_recorder *rec, uint64_t arena_dev);

/* ---- the unit entry: CIIP units, unit records and motion records (recorder.c, the same object and the same cycle) */

/* one prediction unit, paired with cus[i] by index and not read for intra units (pred_mode 1) or units of the chroma tree; 32 bytes, no
 * implicit padding.  `motion` is read during the call only:
 *   VVC355_MVF_PLAIN   num_sb_x * num_sb_y vvc355_mvfield (6 int32 each), row-major over the sub-blocks; one for an ordinary unit
 *   VVC355_MVF_AFFINE  mi->mv[list][cp] as x, y: int32 [2][3][2]
 *   VVC355_MVF_GPM     pu->gpm_mv[0], pu->gpm_mv[1]: two vvc355_mvfield */
typedef struct vvc355_rec_pu {
    const int32_t *motion;
    uint8_t  kind;             /* VVC355_MVF_PLAIN / _AFFINE / _GPM */
    uint8_t  merge_subblock_flag;
    uint8_t  num_sb_x, num_sb_y;           /* PLAIN: the sub-block grid (1, 1 for an ordinary unit); other kinds: not read */
    uint8_t  dmvr_flag, bdof_flag, hpel_if_idx, bcw_idx;
    uint8_t  pred_flag;        /* AFFINE: mi->pred_flag; other kinds carry it in their MvFields */
    uint8_t  motion_model_idc; /* AFFINE: 1 or 2 */
    uint8_t  gpm_partition_idx;
    int8_t   ref_idx[2];       /* AFFINE */
    uint8_t  pad_[11];
} vvc355_rec_pu;

/* HOST pointers into the recorder's buffers, with the lifetime of vvc355_rec_result.  Every list is in raster CTU order, decoding order
 * inside a CTU; the ctu_first_* tables have n_ctus + 1 entries. */
typedef struct vvc355_rec_units_result {
    const vvc355_cu_rec *cu;               /* one per coding unit of the luma or single tree; flags = merge_subblock_flag | affine << 1 */
    const int8_t *cu_qp;                   /* paired by index: qp[0] */
    const vvc355_tu_rec *tu;               /* a tree-0 record per transform unit of a luma / single-tree unit, then (chroma formats) a tree-1
                                            * record per transform unit of a chroma / single-tree unit, unit by unit.  NOT what the deblocking
                                            * passes need where a unit is BDPCM- or ISP-coded: vvc355_rec_deblock_units below */
    const int8_t *tu_qp_c;                 /* [n_tu][2]; read for tree-1 records: qp[1], qp[2], or qp[3] twice for a joint unit with both flags */
    const int32_t *ctu_first_cu, *ctu_first_tu;
    const vvc355_mvf_unit *mvf;            /* intra unit: PLAIN, zero body; PLAIN: one per sub-block; AFFINE (link = its affine_cu); GPM */
    const int32_t *ctu_first_mvf;
    const vvc355_inter_pu *inter;          /* PLAIN inter units that are not CIIP */
    const vvc355_affine_cu *affine;        /* prof_flags and diff_mv zero: vvc355_mvf_unit_pass writes them */
    const vvc355_gpm_cu *gpm;
    const vvc355_ciip_cu *ciip;            /* in command order; cmd[] = indices into vvc355_rec_result.cmds */
    int32_t  n_cu, n_tu, n_mvf, n_inter, n_affine, n_gpm, n_ciip;
    int32_t  n_inter_jobs, n_affine_jobs, n_gpm_jobs, n_ciip_jobs;     /* the totals of the running first_job sums */
    int32_t  ciip_scratch_len;             /* pixels: the total of the running scratch_off sum */
} vvc355_rec_units_result;

/* refusals of the unit entry; the recorder is then as vvc355_rec_begin_picture left it, as after any refusal */
enum {
    VVC355_RECU_E_ARGS = -21,        /* an inter unit without pus, or without motion; slice outside 0..255; a null result */
    VVC355_RECU_E_MIXED = -22,       /* vvc355_rec_ctu and vvc355_rec_ctu_units in one picture; vvc355_rec_units after a picture of vvc355_rec_ctu */
    VVC355_RECU_E_CIIP_SHAPE = -23,  /* a CIIP unit with a side outside 4..64 or an area below 64, or one that is not a single-tree PLAIN inter unit of one
                                      * sub-block */
    VVC355_RECU_E_MOTION = -24,      /* a motion record vvc355_mvf_unit_check would reject (sides, placement, kind, the affine and GPM rules), or a
                                      * sub-block grid that does not divide the unit */
    VVC355_RECU_E_COUNT = -25        /* more than 65535 records of a kind in one CTU */
};

/* vvc355_rec_ctu that also accepts CIIP units and records the unit and motion lists.  slice = the index the inter drivers' slices[] use;
 * pus may be null when no unit of the CTU is inter.  A picture goes through ONE of the two entries. */
int vvc355_rec_ctu_units(vvc355_recorder *rec, int rs, int slice_flags, int slice, const vvc355_rec_cu *cus, const vvc355_rec_pu *pus, int n_cus);
/* After a vvc355_rec_end_picture that returned 0, for a picture recorded through vvc355_rec_ctu_units: fills *out; returns 0. */
int vvc355_rec_units(const vvc355_recorder *rec, vvc355_rec_units_result *out);

/* The transform-unit records for vvc355_tab_fill_pass, vvc355_deblock_bs_rec_pass and vvc355_deblock_qp_rec_pass, by the call sites of
 * set_tb_pos / set_tb_tab / set_qp_c_tab (vvc_ctu.c:379-401, :1241-1250).  They differ from vvc355_rec_units_result.tu in three rules, each
 * of which changes a boundary strength or a chroma QP (whole decoded pictures against the reference found them):
 *   - bit 4 (pcm) is set where bdpcm[] of the tree's component is: two neighbouring BDPCM blocks get strength 0;
 *   - an ISP unit has ONE tree-1 record, over the whole coding unit, with its last partition's flags and QPs (the chroma blocks belong to that
 *     partition and cover the unit);
 *   - ISP partitions 1 or 2 samples wide (high) share a 4-sample column (row) of the tables, and the passes skip rectangles that are no
 *     multiples of 4: one tree-0 record per column (row), 4 wide (high), coded where any of its partitions is.
 * Use them with vvc355_rec_units_result's cu, cu_qp and ctu_first_cu.  HOST pointers with the lifetime of vvc355_rec_result; 32 bytes. */
typedef struct vvc355_rec_deblock_tus {
    const vvc355_tu_rec *tu;
    const int8_t *tu_qp_c;                 /* [n_tu][2], as vvc355_rec_units_result.tu_qp_c */
    const int32_t *ctu_first_tu;           /* n_ctus + 1 entries */
    int32_t  n_tu, pad_;
} vvc355_rec_deblock_tus;
/* Same conditions and refusals as vvc355_rec_units. */
int vvc355_rec_deblock_units(const vvc355_recorder *rec, vvc355_rec_deblock_tus *out);

#ifdef __cplusplus
}
#endif
#endif /* VVC_MI355_REC_H */
