// Boundary strengths and luma maximum filter lengths straight from the unit records (vvc355_deblock_bs_rec_pass).
//
// vvc355_tab_fill_pass + vvc355_deblock_bs_pass carry every coding-unit and transform-unit record through 20 per-unit tables in HBM
// (about 62 bytes per 4x4 unit) only so that the second kernel can read them back, one lane per unit.  Here the two meet in one kernel: the
// records are inverted into LDS maps as tabfill_kernel does (rec_map.hpp), and the lane of a unit reads the records it needs through the
// maps and runs the rules of deblock_bs_kernel on them (bs_rules_body.inc: one copy of the rules, shared as text).  The side tables never
// exist; the MvField table stays an input (the inter stage needs it anyway).
//
// One workgroup per CTU, 256 lanes, one launch, no device scratch.
//   paint   the CTU's coding-unit, tree-0 and tree-1 records -> map[3][32 x 32] (record index relative to the CTU's first record), sixteen
//           lanes per record, heads staged through LDS.  The P side of the CTU's first unit column / row lies in the left / upper CTU: a
//           one-unit halo (halo_l / halo_t, 32 entries per map) is painted from THOSE CTUs' record ranges, one lane per record, only by the
//           records that touch the shared edge.  A halo index is relative to its own CTU's first record: the gather keeps the two bases
//           apart.  The upper-left corner is never asked for.
//   gather  one lane per unit, rows of 32 units: own records and the P-side records of both directions as 8-byte loads that neighbouring
//           lanes share, three MvFields and the prediction flag at the transform unit's origin from the mvf table, then the rules.
// LDS: 3 x 1024 + 2 x 3 x 32 uint16 + 1024 uint2 heads = 14.7 KB.
//
// Unlike tabfill_kernel this kernel does not trust its records: a malformed record paints nothing (rec_map.hpp, CHECKED), a map entry
// without a record is never dereferenced, the CTU's record ranges are clamped to the arrays, and a unit whose records are missing — or
// whose P side's are — gets zeros (see include/vvc_mi355.h).
#include "common.hpp"
#include "runtime.hpp"
#include "rec_map.hpp"
#include "bs_rules.hpp"
#include "../../include/vvc_mi355.h"
#include "stage_checks.hpp"

namespace vvc355 {

static constexpr int kHalo = 32;                   // units along one side of a 128x128 CTU

// The halo of one neighbouring CTU at (nx, ny): its records [first, last) that are well-formed and end on the edge it shares with the
// current CTU paint their index (relative to `first`) along that edge.  vertical = 1: the left CTU, its right-most unit column, indexed
// by unit row; 0: the upper CTU, its bottom unit row, indexed by unit column.  One lane per record, heads read once, coalesced.
template <typename REC>
__device__ __forceinline__ void paint_halo(uint16_t *halo, uint16_t *halo_tree1, const REC *recs, int first, int last, int nx, int ny, int ctb, int vertical)
{
    for (int r = first + (int)threadIdx.x; r < last; r += 256) {
        const uint2 head = gld<uint2>(recs + r);
        const int x0 = (int16_t)(head.x & 0xffff), y0 = (int16_t)(head.x >> 16), w = head.y & 0xff, h = (head.y >> 8) & 0xff, flags = (head.y >> 16) & 0xff;
        if (!rec_inside(x0, y0, w, h, nx, ny, ctb))
            continue;
        if ((vertical ? x0 + w - nx : y0 + h - ny) != ctb)
            continue;
        uint16_t *m = (halo_tree1 && (flags >> 7)) ? halo_tree1 : halo;
        const int u0 = (vertical ? y0 - ny : x0 - nx) >> 2, n = (vertical ? h : w) >> 2;
        for (int i = 0; i < n; i++)
            m[u0 + i] = (uint16_t)(r - first);
    }
}

// (256, 8): 64 VGPRs, so that the 8 workgroups per CU of an 8K picture (2040 CTUs on 256 CUs) are resident at once
__global__ __launch_bounds__(256, 8) void bs_rec_kernel(const vvc355_bs_rec_frame *__restrict__ fp)
{
    __shared__ uint16_t map[3][kMaxUnits];             // coding unit, transform unit tree 0, tree 1
    __shared__ uint16_t halo_l[3][kHalo], halo_t[3][kHalo];
    __shared__ uint2 heads[kMaxUnits];
    const vvc355_bs_rec_frame F = load_uniform(fp);
    const int rs = blockIdx.x, ry = rs / F.ctb_width, rx = rs - ry * F.ctb_width;
    const int ctb_log2 = F.ctb_log2, ctb = 1 << ctb_log2;
    const int lw = ctb_log2 - 2, side = 1 << lw, n_units = side * side;
    const int ox = rx << ctb_log2, oy = ry << ctb_log2;
    for (int i = threadIdx.x; i < 3 * kMaxUnits / 2; i += 256)
        ((uint32_t *)map)[i] = 0xffffffffu;
    if (threadIdx.x < 3 * kHalo / 2) {
        ((uint32_t *)halo_l)[threadIdx.x] = 0xffffffffu;
        ((uint32_t *)halo_t)[threadIdx.x] = 0xffffffffu;
    }
    __syncthreads();
    const int *fcu = (const int *)F.ctu_first_cu, *ftu = (const int *)F.ctu_first_tu;
    const vvc355_cu_rec *cus = (const vvc355_cu_rec *)F.cu;
    const vvc355_tu_rec *tus = (const vvc355_tu_rec *)F.tu;
    // [0] this CTU, [1] the upper one, [2] the left one: the first record of each kind, the base of the indices its map / halo holds
    int cu_base[3] = { 0, 0, 0 }, tu_base[3] = { 0, 0, 0 };
    int cu_end[3] = { 0, 0, 0 }, tu_end[3] = { 0, 0, 0 };
    // all three CTUs' ranges are asked for before the first is used: one round trip, not three
    ctu_range(fcu, rs, F.n_cu, cu_base[0], cu_end[0]);
    ctu_range(ftu, rs, F.n_tu, tu_base[0], tu_end[0]);
    if (ry > 0) {
        ctu_range(fcu, rs - F.ctb_width, F.n_cu, cu_base[1], cu_end[1]);
        ctu_range(ftu, rs - F.ctb_width, F.n_tu, tu_base[1], tu_end[1]);
    }
    if (rx > 0) {
        ctu_range(fcu, rs - 1, F.n_cu, cu_base[2], cu_end[2]);
        ctu_range(ftu, rs - 1, F.n_tu, tu_base[2], tu_end[2]);
    }
    // the halo first: its head loads have no barrier in front of them, so they overlap with each other
    if (ry > 0) {
        paint_halo(halo_t[0], (uint16_t *)nullptr, cus, cu_base[1], cu_end[1], ox, oy - ctb, ctb, 0);
        paint_halo(halo_t[1], halo_t[2], tus, tu_base[1], tu_end[1], ox, oy - ctb, ctb, 0);
    }
    if (rx > 0) {
        paint_halo(halo_l[0], (uint16_t *)nullptr, cus, cu_base[2], cu_end[2], ox - ctb, oy, ctb, 1);
        paint_halo(halo_l[1], halo_l[2], tus, tu_base[2], tu_end[2], ox - ctb, oy, ctb, 1);
    }
    map_records<vvc355_cu_rec, true>(map[0], (uint16_t *)nullptr, heads, cus, cu_base[0], cu_end[0], ox, oy, lw);
    map_records<vvc355_tu_rec, true>(map[1], map[2], heads, tus, tu_base[0], tu_end[0], ox, oy, lw);
    __syncthreads();

    // slice and tile numbers as deblock_bs_kernel reads them; a CTU edge is the only place where they can differ
    const int16_t *slice = (const int16_t *)F.slice_idx;
    const int my_slice = gld<int16_t>(slice + rs);
    const int ctb_slice[2] = { ry > 0 ? (int)gld<int16_t>(slice + rs - F.ctb_width) : my_slice, rx > 0 ? (int)gld<int16_t>(slice + rs - 1) : my_slice };
    const int16_t *row_bd = (const int16_t *)F.ctb_to_row_bd, *col_bd = (const int16_t *)F.ctb_to_col_bd;
    const int ctb_tile_edge[2] = { ry > 0 && gld<int16_t>(row_bd + ry) != gld<int16_t>(row_bd + ry - 1),
                                   rx > 0 && gld<int16_t>(col_bd + rx) != gld<int16_t>(col_bd + rx - 1) };
    const vvc355_mvfield *mvf = (const vvc355_mvfield *)F.mvf;
    const int mpw = F.mvf_pitch, pw = F.width >> 2, ph = F.height >> 2;                // picture size in units
    const bool chroma = F.n_comp == 3;

    for (int i = threadIdx.x; i < n_units; i += 256) {
        const int dy = i >> lw, dx = i & (side - 1);
        const int ux = (ox >> 2) + dx, uy = (oy >> 2) + dy;
        if (ux >= pw || uy >= ph)
            continue;
        const int x = ux * 4, y = uy * 4;
        const int off = uy * F.unit_pitch + ux;
        // ---- the unit's own records
        const int q_cu = abs_rec(map[0][i], cu_base[0]), q_t0 = abs_rec(map[1][i], tu_base[0]), q_t1 = chroma ? abs_rec(map[2][i], tu_base[0]) : -1;
        vvc355_tu_rec r0 = {}, r1 = {};
        if (q_t0 >= 0)
            r0 = gld<vvc355_tu_rec>(tus + q_t0);
        if (q_t1 >= 0)
            r1 = gld<vvc355_tu_rec>(tus + q_t1);
        if (chroma) {
            if (F.tb_width_c)
                gst<uint8_t>((uint8_t *)F.tb_width_c + off, (uint8_t)(r1.w >> F.hs));          // in chroma samples; 0 without a tree-1 record
            if (F.tb_height_c)
                gst<uint8_t>((uint8_t *)F.tb_height_c + off, (uint8_t)(r1.h >> F.vs));
        }
        // the coding unit at the luma transform unit's origin: the same CTU (a painted record lies inside it)
        int o_cu = -1;
        if (q_t0 >= 0)
            o_cu = abs_rec(map[0][(((r0.y0 - oy) >> 2) << lw) + ((r0.x0 - ox) >> 2)], cu_base[0]);
        const bool complete = q_cu >= 0 && q_t0 >= 0 && o_cu >= 0 && (!chroma || q_t1 >= 0);
        if (!complete) {
#pragma unroll
            for (int d = 0; d < 2; d++) {
                gst<uint8_t>((uint8_t *)F.bs[d][0] + off, (uint8_t)0);
                gst<uint8_t>((uint8_t *)F.max_len_p[d] + off, (uint8_t)0);
                gst<uint8_t>((uint8_t *)F.max_len_q[d] + off, (uint8_t)0);
                if (chroma) {
                    gst<uint8_t>((uint8_t *)F.bs[d][1] + off, (uint8_t)0);
                    gst<uint8_t>((uint8_t *)F.bs[d][2] + off, (uint8_t)0);
                }
            }
            continue;
        }
        // ---- the P side per direction ([0] above, [1] left): through the map, or through the halo with the other CTU's bases
        const int has_n[2] = { uy > 0, ux > 0 };
        bool ok[2];                                    // the entries of (unit, direction) are derived; otherwise they are written as 0
        vvc355_tu_rec p0[2], p1[2];
        int sb_p[2];
#pragma unroll
        for (int d = 0; d < 2; d++) {
            const bool inside = d ? dx > 0 : dy > 0;
            const int j = d ? i - 1 : i - side, e = d ? dy : dx, b = inside ? 0 : d + 1;
            int p_cu = q_cu, p_t0 = q_t0, p_t1 = q_t1;
            if (has_n[d]) {
                const uint16_t (*hl)[kHalo] = d ? halo_l : halo_t;
                p_cu = abs_rec(inside ? map[0][j] : hl[0][e], cu_base[b]);
                p_t0 = abs_rec(inside ? map[1][j] : hl[1][e], tu_base[b]);
                p_t1 = chroma ? abs_rec(inside ? map[2][j] : hl[2][e], tu_base[b]) : -1;
            }
            ok[d] = p_cu >= 0 && p_t0 >= 0 && (!chroma || p_t1 >= 0);
            if (!ok[d])
                p_cu = q_cu, p_t0 = q_t0, p_t1 = q_t1;          // any record that exists: what the rules make of it is not stored
            p0[d] = gld<vvc355_tu_rec>(tus + p_t0);
            p1[d] = r1;
            if (p_t1 >= 0)
                p1[d] = gld<vvc355_tu_rec>(tus + p_t1);
            sb_p[d] = gld<vvc355_cu_rec>(cus + p_cu).flags & 3;          // MergeSubblockFlag | InterAffineFlag
        }
        const vvc355_mvfield curr = ld_mvf(mvf + uy * mpw + ux);
        const vvc355_mvfield neigh[2] = { ld_mvf(mvf + (uy - has_n[0]) * mpw + ux), ld_mvf(mvf + uy * mpw + ux - has_n[1]) };
        const int t0[2][2] = { { r0.y0, r0.x0 }, { r1.y0, r1.x0 } };                  // [tree][dir]
        const int size_q[2] = { r0.h, r0.w }, size_p[2] = { p0[0].h, p0[1].w };
        // pcm0, cbf0, pcm1, cbf1, cbf2, joint: here / on the P side
        const int fq[6] = { (r0.flags >> 4) & 1, r0.flags & 1, (r1.flags >> 4) & 1, (r1.flags >> 1) & 1, (r1.flags >> 2) & 1, (r1.flags >> 3) & 1 };
        int fn[2][6];
#pragma unroll
        for (int d = 0; d < 2; d++) {
            fn[d][0] = (p0[d].flags >> 4) & 1; fn[d][1] = p0[d].flags & 1;
            fn[d][2] = (p1[d].flags >> 4) & 1; fn[d][3] = (p1[d].flags >> 1) & 1; fn[d][4] = (p1[d].flags >> 2) & 1; fn[d][5] = (p1[d].flags >> 3) & 1;
        }
        const int n_slice[2] = { dy == 0 ? ctb_slice[0] : my_slice, dx == 0 ? ctb_slice[1] : my_slice };
        const int tile_edge[2] = { dy == 0 && ctb_tile_edge[0], dx == 0 && ctb_tile_edge[1] };
        // ---- the coding unit at the transform unit's origin
        const vvc355_cu_rec oc = gld<vvc355_cu_rec>(cus + o_cu);
        const bool is_intra = gld<uint8_t>((const uint8_t *)(mvf + (r0.y0 >> 2) * mpw + (r0.x0 >> 2)) + 20) == 0;
        const int cb0[2] = { oc.y0, oc.x0 }, cb_size[2] = { oc.h, oc.w };
        const bool sb_cu = !is_intra && (oc.flags & 3);
        // ---- the rules
#define BS_RULES_OUT(tab, v) gst<uint8_t>((uint8_t *)(tab) + off, (uint8_t)(ok[dir] ? (v) : 0))
#include "bs_rules_body.inc"
#undef BS_RULES_OUT
    }
}

} // namespace vvc355

// the frame as the header states it: every refusal before any HIP call
int vvc355::bs_rec_check(const vvc355_bs_rec_frame *f)
{
    if (!f)
        return VVC355_BS_REC_E_FRAME;
    if (f->width <= 0 || f->height <= 0 || (f->width & 3) || (f->height & 3))
        return VVC355_BS_REC_E_SIZE;
    if (f->ctb_log2 < 5 || f->ctb_log2 > 7)
        return VVC355_BS_REC_E_CTB;
    const int ctb = 1 << f->ctb_log2;
    if (f->ctb_width != (f->width + ctb - 1) >> f->ctb_log2 || f->ctb_height != (f->height + ctb - 1) >> f->ctb_log2)
        return VVC355_BS_REC_E_GRID;
    if (f->unit_pitch < f->width / 4 || f->mvf_pitch < f->width / 4)
        return VVC355_BS_REC_E_PITCH;
    if (f->n_comp != 1 && f->n_comp != 3)
        return VVC355_BS_REC_E_COMP;
    if (f->hs > 1 || f->vs > 1)
        return VVC355_BS_REC_E_SHIFT;
    if (f->n_cu < 0 || f->n_tu < 0)
        return VVC355_BS_REC_E_COUNT;
    if ((f->n_cu > 0 && (!f->cu || !f->ctu_first_cu)) || (f->n_tu > 0 && (!f->tu || !f->ctu_first_tu)))
        return VVC355_BS_REC_E_RECORDS;
    if (!f->mvf || !f->ref_poc || !f->slice_idx || !f->ctb_to_col_bd || !f->ctb_to_row_bd)
        return VVC355_BS_REC_E_TABLES;
    for (int d = 0; d < 2; d++) {
        if (!f->bs[d][0] || !f->max_len_p[d] || !f->max_len_q[d])
            return VVC355_BS_REC_E_OUTPUT;
        if (f->n_comp == 3 && (!f->bs[d][1] || !f->bs[d][2]))
            return VVC355_BS_REC_E_OUTPUT;
    }
    return 0;
}

extern "C" int vvc355_deblock_bs_rec_pass(void *stream, const vvc355_bs_rec_frame *frame_dev, const vvc355_bs_rec_frame *frame_host)
{
    const int err = frame_dev ? vvc355::bs_rec_check(frame_host) : VVC355_BS_REC_E_FRAME;
    if (err)
        return err;
    hipLaunchKernelGGL(vvc355::bs_rec_kernel, dim3(frame_host->ctb_width * frame_host->ctb_height), dim3(256), 0, (hipStream_t)stream, frame_dev);
    HIP_CHECK(hipGetLastError());
    return 0;
}
