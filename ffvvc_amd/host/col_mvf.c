/*
 * col_mvf.c — the parser-side half of the hand-back of collocated motion (include/vvc_mi355.h, vvc355_col_mvf_pass).
 *
 * Called on the entries vvc355_download_async brought back, before the parser derives a temporal candidate from the picture
 * (temporal_luma_motion_vector, vvc_mvs.c:220-245; sb_temproal_luma_motion, :1016-1022): unpacks an entry, or puts a picture's entries
 * where the reference's TAB_MVF reads find them.  Plain C11, no HIP: linked into libvvc_mi355.so like levels_pack.c.
 */
#include "vvc_mi355.h"

void vvc355_col_mv_unpack(const vvc355_col_mv *e, int32_t mv[2][2], int8_t ref_idx[2], uint8_t *pred_flag)
{
    const uint8_t pf = (e->w[0][1] >> 19) & 3;

    for (int l = 0; l < 2; l++) {
        const int used = (pf >> l) & 1;
        for (int k = 0; k < 2; k++) {
            const int32_t v = (int32_t)(e->w[l][k] & 0x7FFFF);
            mv[l][k] = used ? v - ((v & 0x40000) << 1) : 0;             /* 19 bits, signed */
        }
        ref_idx[l] = used ? (int8_t)((e->w[l][0] >> 19) & 0x1F) : -1;
    }
    *pred_flag = pf;
}

void vvc355_col_mvf_scatter(const vvc355_col_mv *col, int col_stride, int width, int height, void *tab_mvf, int min_pu_width)
{
    vvc355_mvfield *tab = (vvc355_mvfield *)tab_mvf;
    const int gw = (width + 7) >> 3, gh = (height + 7) >> 3;

    for (int gy = 0; gy < gh; gy++) {
        for (int gx = 0; gx < gw; gx++) {
            vvc355_mvfield *m = tab + (size_t)(2 * gy) * min_pu_width + 2 * gx;
            vvc355_col_mv_unpack(col + (size_t)gy * col_stride + gx, m->mv, m->ref_idx, &m->pred_flag);
        }
    }
}
