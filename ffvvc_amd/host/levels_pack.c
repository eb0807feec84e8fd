/*
 * levels_pack.c — the parser-side packer of coefficient levels (include/vvc_mi355.h, vvc355_tb_levels).
 *
 * Called per transform block right after residual coding (ff_vvc_residual_coding), on the int32 levels the parser has just written:
 * appends the block's coded 4x4 groups to the picture's int16 level stream and fills its side record.  Plain C11, no HIP: it is
 * linked into libvvc_mi355.so so that a decoder needs nothing else to produce what vvc355_itx_*_batch_lv read.
 */
#include "vvc_mi355.h"

int vvc355_levels_pack(const int32_t *coeffs, int log2_w, int log2_h, int16_t *out, vvc355_tb_levels *lv, uint32_t first)
{
    const int w = 1 << log2_w, h = 1 << log2_h;
    const int gw = ((w < 32 ? w : 32) + 3) >> 2, gh = ((h < 32 ? h : 32) + 3) >> 2;
    uint64_t groups = 0;

    lv->groups = 0;
    lv->first = first;
    lv->flags = VVC355_LEVELS_INT32;
    /* validate first, so that a block that stays on the int32 path leaves nothing in the stream */
    for (int y = 0; y < h; y++) {
        for (int x = 0; x < w; x++) {
            const int32_t c = coeffs[y * w + x];
            if (!c)
                continue;
            if (c < INT16_MIN || c > INT16_MAX)
                return VVC355_LEVELS_E_RANGE;
            if (x >= 32 || y >= 32)
                return VVC355_LEVELS_E_ZERO_OUT;
            groups |= 1ull << ((y >> 2) * gw + (x >> 2));
        }
    }
    int n = 0;
    for (int gy = 0; gy < gh; gy++) {
        for (int gx = 0; gx < gw; gx++) {
            if (!(groups >> (gy * gw + gx) & 1))
                continue;
            int16_t *g = out + 16 * n++;
            for (int s = 0; s < 16; s++) {
                const int x = 4 * gx + (s & 3), y = 4 * gy + (s >> 2);
                g[s] = (int16_t)(x < w && y < h ? coeffs[y * w + x] : 0);
            }
        }
    }
    lv->groups = groups;
    lv->flags = 0;
    return n;
}
