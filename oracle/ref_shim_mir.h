/*
 * oracle/ref_shim_mir.h — what the translation units of oracle/_ref/libvvcref.so share: the plain arrays a whole picture is described
 * with (ref_recon_picture of ref_shim_intra.c, ref_decode_picture of ref_shim_picture.c) and the helpers that turn them, and the inter
 * frame of ref_shim_inter.c, into the reference's objects.  TEST INFRASTRUCTURE ONLY.  Project code: it is included after the
 * reference's headers, which the including file resolves from the reference tree at build time.
 *
 * Every member of the arrays is an int32 (addresses: uint64), so that a numpy record array mirrors them without padding rules.
 */
#ifndef REF_SHIM_MIR_H
#define REF_SHIM_MIR_H

#include <stdint.h>

#include "libavutil/frame.h"
#include "libavcodec/vvc/vvc_ctu.h"

#include "vvc_oracle.h"

#define MIR_MAX_SLICES 8
typedef struct MirReconTb { int32_t c_idx, x0, y0, w, h, ts, has_coeffs, min_x, min_y, max_x, max_y, level_off; } MirReconTb;
typedef struct MirReconTu { int32_t x0, y0, w, h, coded_flag[3], joint, first_tb, n_tbs; } MirReconTu;
typedef struct MirReconCu {
    int32_t x0, y0, w, h, pred_mode, tree_type, mode_y, mode_c;
    int32_t ref_idx, mip_flag, mip_mode, mip_transposed, mip_chroma_direct, isp_type, num_isp, bdpcm[3];
    int32_t lfnst_idx, apply_lfnst[3], mts_idx, sbt_flag, sbt_horizontal, sbt_pos, coded_flag, ciip_flag, qp[4];
    int32_t first_tu, n_tus;
} MirReconCu;
typedef struct MirReconPic {
    uint64_t plane[3];
    uint64_t slice_idx, col_bd, row_bd;            /* int16 per CTB; uint16 per CTB column (+1) / row (+1) */
    uint64_t slice_dep_quant, slice_lmcs_used;     /* int32 per slice */
    uint64_t ctu_first_cu, cus, tus, tbs, levels;  /* int32 [n_ctb + 1]; MirReconCu / Tu / Tb arrays; int32 level arena */
    uint64_t scale_log;                            /* int32 [scale_log_cap][3], or 0 */
    int32_t  stride[3];
    int32_t  width, height, bit_depth, chroma_format_idc, ctb_log2;
    int32_t  wpp, collocated, mts_enabled, explicit_mts_intra, explicit_mts_inter;
    int32_t  log2_transform_range, min_qp_prime_ts, joint_cbcr_sign, chroma_residual_scale;
    int32_t  lmcs_min_bin_idx, lmcs_max_bin_idx, lmcs_pivot[17], lmcs_chroma_scale_coeff[16];
    int32_t  n_slices, n_levels, scale_log_cap, n_scale_log;
} MirReconPic;

/* The objects mir_recon_build wires from a MirReconPic (the one set ref_shim_intra.c keeps; single-threaded).  ctus[rs].cus are lists
 * allocated through ff_refstruct_allocz: ff_vvc_reconstruct frees a CTU's list itself, mir_recon_free whatever is still linked. */
typedef struct MirReconObjs {
    VVCLocalContext    *lc;
    VVCFrameContext    *fc;
    VVCSPS             *sps;
    VVCPPS             *pps;
    SliceContext       *sc;                        /* [MIR_MAX_SLICES], sc[s].sh.r = &sh[s] */
    H266RawSliceHeader *sh;
    CTU                *ctus;
    int                 ncx, n_ctb;
    uint8_t            *tabs;
    int                *levels;
} MirReconObjs;

/* ref_shim_intra.c: 0, or -1 for a picture the objects cannot hold (nothing is left allocated then).  ciip: units with ciip_flag are
 * taken (as the parser leaves them: planar, reference line 0, no MIP) instead of refused. */
int  mir_recon_build(MirReconPic *p, MirReconObjs *o, int ciip);
void mir_recon_free(MirReconObjs *o);

/* ref_shim_inter.c: rpl[l].ref[i] -> fr[l][i] -> av[l][i] over the planes of refs[l * 16 + i] (an entry without a luma plane stays NULL),
 * and one slice header from its vvc355_inter_slice twin: -1 for a pair of switches no slice type produces or LMCS without a map */
void ref_inter_wire_refs(const orc_ref_pic *refs, int n_comp, RefPicList rpl[2], VVCFrame fr[2][16], AVFrame av[2][16]);
int  ref_inter_wire_slice(const orc_inter_slice *in, int have_lut, SliceContext *s, H266RawSliceHeader *sh, H266RawPPS *raw_pps, RefPicList *rpl);

#endif
