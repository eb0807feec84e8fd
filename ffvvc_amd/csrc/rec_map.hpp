// Unit records -> LDS maps of a CTU's 4x4 units: shared by tabfill_kernel (tabfill.hip), bs_rec_kernel (bs_rec.hip) and qp_rec_kernel
// (qp_rec.hip).
#pragma once
#include "common.hpp"

namespace vvc355 {

static constexpr int kMaxUnits = 32 * 32;          // 128x128 CTU in 4x4 units
static constexpr uint16_t kNoRec = 0xffff;

// a well-formed record of the CTU at (ox, oy): sizes positive multiples of 4, position a multiple of 4, the rectangle inside the CTU
__device__ __forceinline__ bool rec_inside(int x0, int y0, int w, int h, int ox, int oy, int ctb)
{
    return w > 0 && h > 0 && !((w | h | x0 | y0) & 3) && x0 >= ox && y0 >= oy && x0 + w <= ox + ctb && y0 + h <= oy + ctb;
}

// CTU rs's range in a record array of n records: [first, last) clamped to the array and to the 65535 records a map entry can name
__device__ __forceinline__ void ctu_range(const int *firsts, int rs, int n, int &r0, int &r1)
{
    r0 = r1 = 0;
    if (!firsts || n <= 0)
        return;
    r0 = min(max(gld<int>(firsts + rs), 0), n);
    r1 = min(max(gld<int>(firsts + rs + 1), r0), min(n, r0 + 65535));
}

__device__ __forceinline__ int abs_rec(uint16_t idx, int base) { return idx == kNoRec ? -1 : base + (int)idx; }

// records [first, last) of one kind -> map[unit within the CTU] = record index - first.  `map_tree1` != 0: the records carry a tree bit
// (flags bit 7) and those of tree 1 go to that map.  Sixteen lanes per record; widths are powers of two in every partitioning a decoder
// produces (the general case keeps the division).  CHECKED: a record that is malformed (a size of zero, a size or a position that is no multiple
// of 4, a rectangle not inside the CTU) is skipped before it paints anything; without it the records are trusted.  TREE1_ONLY: the
// records of tree 0 paint nothing and `map` is not used.
template <typename REC, bool CHECKED = false, bool TREE1_ONLY = false>
__device__ __forceinline__ void map_records(uint16_t *map, uint16_t *map_tree1, uint2 *heads, const REC *recs, int first, int last, int ox, int oy, int lw)
{
    const int sub = threadIdx.x & 15;
    // the records' heads (x0 y0 | w h flags pad: the same 8 bytes for all three record kinds) come in through LDS, 1024 at a time with one
    // coalesced round trip, so that the painting passes below (sixteen records per pass) do not each wait for a global load
    for (int c0 = first; c0 < last; c0 += kMaxUnits) {
        const int nc = min(kMaxUnits, last - c0);
        __syncthreads();
        for (int i = threadIdx.x; i < nc; i += 256)
            heads[i] = gld<uint2>(recs + c0 + i);
        __syncthreads();
        for (int k = threadIdx.x >> 4; k < nc; k += 16) {
            const uint2 head = heads[k];
            const int r = c0 + k;
            const int x0 = (int16_t)(head.x & 0xffff), y0 = (int16_t)(head.x >> 16), w = head.y & 0xff, h = (head.y >> 8) & 0xff, flags = (head.y >> 16) & 0xff;
            if constexpr (CHECKED) {
                if (!rec_inside(x0, y0, w, h, ox, oy, 4 << lw))
                    continue;
            }
            if constexpr (TREE1_ONLY) {
                if (!(flags >> 7))
                    continue;
            }
            uint16_t *m = (map_tree1 && (flags >> 7)) ? map_tree1 : map;
            const int ux = (x0 - ox) >> 2, uy = (y0 - oy) >> 2, uw = w >> 2, n = uw * (h >> 2);
            const int base = (uy << lw) + ux;
            if ((uw & (uw - 1)) == 0) {
                const int lg = __builtin_ctz(uw | 64);
                for (int i = sub; i < n; i += 16)
                    m[base + ((i >> lg) << lw) + (i & (uw - 1))] = (uint16_t)(r - first);
            } else {
                for (int i = sub; i < n; i += 16) {
                    const int dy = i / uw, dx = i - dy * uw;
                    m[base + (dy << lw) + dx] = (uint16_t)(r - first);
                }
            }
        }
    }
}

} // namespace vvc355
