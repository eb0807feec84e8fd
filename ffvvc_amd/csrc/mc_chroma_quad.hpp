// Chroma bi-prediction of FOUR Cb/Cr pairs per wave for gfx950: the 4:2:0 8x8 blocks of four consecutive sub-blocks, one pair per
// 16-lane group.  Used by mc_fused.hip's chroma bi-prediction kernel; the one-pair path there stays the path of everything else.
//
// The stage is bound by VALU issue, and what the one-pair path issues is mostly overhead paid per wave for 128 samples: clamped
// 2-byte loads, partly filled passes, a descriptor unpacked on the scalar unit.  Here a wave produces 512 samples:
//
//  * The decision is wave-uniform (chroma_quad returns false before it has written anything, the caller then runs the old
//    path): all four pairs pass the old pair test, are 4:2:0 8x8, and the 12 x 11 samples fetched per reference and plane lie
//    inside the plane.  A pair's values (motion, planes, weights, destinations) are per-lane values of its group.
//  * ONE fetch per reference and plane.  With dmvr every read is clamped to the 11 x 11 window of the unrefined block
//    (emulated_edge_dmvr, vvc_inter.c:61-88); without, the window is the 11 x 11 samples around the block at its motion.  A
//    lane owns one quarter row (4 samples: one 8-byte load, one ds_write_b64).  A read at window index u + d (d = refined minus
//    unrefined integer position, |d| <= 2, anything else takes the old path) is LDS index clamp(u + d, 0, 10): columns through
//    replicated pad columns, rows through replicated rows of the intermediate.
//  * The zero-fraction filter {0, 64, 0, 0} makes copy / h / v / hv one formula, as in mc_tools.hpp: 64 s >> (bd - 8) =
//    s << (14 - bd) and (64 t) >> 6 = t, and for v only ((sum f s) << (14 - bd)) >> 6 = (sum f s) >> (bd - 8).  All exact.
//    A whole-sample position takes entry 0 of filter set 0 whatever the job's set: the other sets' entry 0 is a real filter,
//    and the reference copies at a zero fraction without looking at the set.
//  * h pass: a lane owns one reference and plane and one output pair, 11 rows; v pass: a lane owns one plane and column, both
//    references, 8 rows.  v_dot2 on aligned pairs; the parity of d is folded into the tap registers (two sets of three).
//  * Epilogue: avg is w_avg with weights 1, denom 0 and offsets 0, so one formula per lane with its plane's weights.
#pragma once
#include "common.hpp"
#include "pk16.hpp"
#include "wave.hpp"
#include "mc_filters.hpp"
#include "../../include/vvc_mi355.h"

namespace vvc355 {

static constexpr int kQwP = 20;         // window pitch in samples: 2 pad + window columns 0..10 at LDS columns 4..14 + 5 pad (8-byte rows)
static constexpr int kQwC0 = 4;         // LDS column of window column 0
static constexpr int kQwRows = 11;
static constexpr int kQtP = 16;         // intermediate, transposed: [column][row], window row r at row r + 2, rows 0..1 and 13..15 replicated

struct QuadGroupLds {
    union {                             // the intermediate lies in the windows' bytes: the h pass reads all of its input, syncs, then stores
        uint16_t win[4][kQwRows * kQwP];    // [reference * 2 + plane]
        int16_t tmpT[4][8 * kQtP];
    };
};
struct QuadLds { QuadGroupLds g[4]; };  // 7 040 bytes per wave

// Two adjacent outputs of a 4-tap filter from three aligned sample pairs d[m] = (p[2m], p[2m + 1]).  Even start: out0 = sum f[k] p[k],
// out1 = sum f[k] p[k + 1]; odd start (the wanted samples begin at p[1]): out0 = sum f[k] p[k + 1], out1 = sum f[k] p[k + 2].
struct QuadTaps {
    uint32_t a[3], b[3];
    __device__ __forceinline__ void set(uint32_t f4, bool odd)
    {
        const int f0 = (int8_t)f4, f1 = (int8_t)(f4 >> 8), f2 = (int8_t)(f4 >> 16), f3 = (int8_t)(f4 >> 24);
        const uint32_t e0 = pack16(f0, f1), e1 = pack16(f2, f3);
        const uint32_t o0 = pack16(0, f0), o1 = pack16(f1, f2), o2 = pack16(f3, 0);
        a[0] = odd ? o0 : e0; a[1] = odd ? o1 : e1; a[2] = odd ? o2 : 0u;
        b[0] = odd ? 0u : o0; b[1] = odd ? e0 : o1; b[2] = odd ? e1 : o2;
    }
    __device__ __forceinline__ void apply(uint32_t d0, uint32_t d1, uint32_t d2, int &out0, int &out1) const
    {
        out0 = dot2(d2, a[2], dot2(d1, a[1], dot2(d0, a[0], 0)));
        out1 = dot2(d2, b[2], dot2(d1, b[1], dot2(d0, b[0], 0)));
    }
};

__device__ __forceinline__ int lo16s(uint32_t v) { return (int)(int16_t)(v & 0xffff); }
__device__ __forceinline__ int hi16s(uint32_t v) { return (int)v >> 16; }
__device__ __forceinline__ const uint8_t *ptr64(uint32_t lo, uint32_t hi) { return (const uint8_t *)(((uint64_t)hi << 32) | lo); }

// jobs[ia .. ia + 7] must exist.  Returns false (wave-uniform, nothing written) when the wave has to take the one-pair path.
template <int BD>
__device__ __forceinline__ bool chroma_quad(const vvc355_bipred_job *jobs, int ia, QuadLds &LQ, int lane)
{
    using px_t = typename Px<BD>::type;
    static_assert(sizeof(vvc355_bipred_job) == 104, "descriptor layout: dword indices below");
#define VVC355_QUAD_AT(field, byte) static_assert(offsetof(vvc355_bipred_job, field) == (byte), "descriptor layout: " #field)
    VVC355_QUAD_AT(dst, 0); VVC355_QUAD_AT(ref0, 8); VVC355_QUAD_AT(ref1, 16); VVC355_QUAD_AT(rec, 24);
    VVC355_QUAD_AT(dst_stride, 32); VVC355_QUAD_AT(ref0_stride, 36); VVC355_QUAD_AT(ref1_stride, 40); VVC355_QUAD_AT(mv, 44);
    VVC355_QUAD_AT(x, 60); VVC355_QUAD_AT(y, 62); VVC355_QUAD_AT(w, 64); VVC355_QUAD_AT(h, 66); VVC355_QUAD_AT(pic_w, 68); VVC355_QUAD_AT(pic_h, 70);
    VVC355_QUAD_AT(denom, 72); VVC355_QUAD_AT(w0, 74); VVC355_QUAD_AT(w1, 76); VVC355_QUAD_AT(o0, 78); VVC355_QUAD_AT(o1, 80);
    VVC355_QUAD_AT(chroma, 82); VVC355_QUAD_AT(hs, 83); VVC355_QUAD_AT(vs, 84); VVC355_QUAD_AT(dmvr, 85); VVC355_QUAD_AT(bdof, 86);
    VVC355_QUAD_AT(hf_idx, 87); VVC355_QUAD_AT(vf_idx, 88); VVC355_QUAD_AT(weight_flag, 89); VVC355_QUAD_AT(pred_flag, 90);
#undef VVC355_QUAD_AT
    const int grp = lane >> 4, l = lane & 15;

    // ---- both descriptors of the group's pair, dwords 0..23 (8-byte loads: the descriptors are 8-byte aligned)
    // 0-1 dst, 2-3 ref0, 4-5 ref1, 6-7 rec, 8-10 strides, 11-14 mv, 15 x|y, 16 w|h, 17 pic_w|pic_h, 18 denom|w0, 19 w1|o0,
    // 20 o1|chroma|hs, 21 vs|dmvr|bdof|hf_idx, 22 vf_idx|weight_flag|pred_flag
    uint32_t a[24], b[24];
    {
        const uint8_t *pa = (const uint8_t *)(jobs + ia + 2 * grp), *pb = pa + sizeof(vvc355_bipred_job);
#pragma unroll
        for (int i = 0; i < 12; i++) {
            const uint2 va = gld<uint2>(pa + 8 * i), vb = gld<uint2>(pb + 8 * i);
            a[2 * i] = va.x; a[2 * i + 1] = va.y;
            b[2 * i] = vb.x; b[2 * i + 1] = vb.y;
        }
    }
    // the pair test of the one-pair path (bi-predicted chroma jobs of one sub-block), 4:2:0, 8x8
    bool ok = a[6] == b[6] && a[7] == b[7];
#pragma unroll
    for (int k = 11; k <= 17; k++) ok = ok && a[k] == b[k];
    const uint32_t pfa = (a[22] >> 16) & 0xff, pfb = (b[22] >> 16) & 0xff;
    ok = ok && ((a[20] ^ b[20]) >> 16) == 0 && ((a[20] >> 16) & 0xff) != 0 && (a[20] >> 24) == 1 &&      // chroma, hs
         ((a[21] ^ b[21]) & 0xff00ffffu) == 0 && (a[21] & 0xff) == 1 &&                                  // vs, dmvr, hf_idx
         ((a[22] ^ b[22]) & 0xff) == 0 &&                                                                // vf_idx
         !(pfa == 1 || pfa == 2) && !(pfb == 1 || pfb == 2) && a[16] == (8u | (8u << 16));               // bi-predicted, 8x8

    int mv[4] = { (int)a[11], (int)a[12], (int)a[13], (int)a[14] };
    const uint8_t *rec = ptr64(a[6], a[7]);
    if (ok && rec) {
#pragma unroll
        for (int k = 0; k < 4; k++) mv[k] = gld<int>(rec + 4 * k);                   // written by the luma launch
    }
    const int x = lo16s(a[15]), y = hi16s(a[15]), pic_w = lo16s(a[17]), pic_h = hi16s(a[17]);
    const bool dmvr = ((a[21] >> 8) & 0xff) != 0;
    int bx[2], by[2], dx[2], dy[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int ox = x + (mv[2 * i] >> 5), oy = y + (mv[2 * i + 1] >> 5);
        bx[i] = dmvr ? x + ((int)a[11 + 2 * i] >> 5) : ox;                           // the unrefined block: its window is all that is read
        by[i] = dmvr ? y + ((int)a[12 + 2 * i] >> 5) : oy;
        dx[i] = ox - bx[i];
        dy[i] = oy - by[i];
        // fetched: columns bx - 1 .. bx + 10 (three 4-sample loads), rows by - 1 .. by + 9
        ok = ok && (unsigned)(dx[i] + 2) <= 4u && (unsigned)(dy[i] + 2) <= 4u &&
             bx[i] >= 1 && bx[i] + 10 < pic_w && by[i] >= 1 && by[i] + 9 < pic_h;
    }
    if (!__all(ok))
        return false;

    QuadGroupLds &L = LQ.g[grp];
    const int q = l >> 2, ref = q >> 1, second = q & 1;          // fetch and h pass: the lane's reference and plane
    // ---- fetch: lane -> quarter row k of (reference, plane) q, 11 rows; k = 3 re-reads quarter 2 and fills the right pad
    {
        const int k = l & 3;
        const uint8_t *plane = second ? (ref ? ptr64(b[4], b[5]) : ptr64(b[2], b[3])) : (ref ? ptr64(a[4], a[5]) : ptr64(a[2], a[3]));
        const int stride = (int)(second ? (ref ? b[10] : b[9]) : (ref ? a[10] : a[9]));
        const int fx0 = (ref ? bx[1] : bx[0]) - 1 + 4 * min(k, 2), fy0 = (ref ? by[1] : by[0]) - 1;
        const uint8_t *p = plane + row_off(fy0, stride) + fx0 * (int)sizeof(px_t);
        uint2 v[kQwRows];
#pragma unroll
        for (int r = 0; r < kQwRows; r++) {
            if (BD > 8) {
                v[r] = gld<uint2>(p);
            } else {
                const uint32_t s = gld<uint32_t>(p);
                v[r] = make_uint2(widen_lo(s), widen_hi(s));
            }
            p += stride;
        }
        uint16_t *wq = L.win[q] + kQwC0 + 4 * k;
#pragma unroll
        for (int r = 0; r < kQwRows; r++) {
            uint2 d = v[r];
            const uint32_t rep = pk_dup_lo(d.y);                                     // window column 10 twice
            if (k >= 2) d.y = rep;                                                   // column 11 is past the window
            if (k == 3) d.x = rep;
            *(uint2 *)(wq + r * kQwP) = d;
            if (k == 0)
                *(uint32_t *)(wq + r * kQwP - 2) = pk_dup_lo(d.x);                   // left pad: column 0 twice
        }
        wave_sync();
    }
    const uint32_t hf_idx = a[21] >> 24, vf_idx = a[22] & 0xff;

    // ---- h pass: lane -> (reference, plane) q, outputs 2 xp and 2 xp + 1, rows 0..10 -> tmpT[q][x][r + 2] and the replicated rows
    {
        const int xp = l & 3, d = ref ? dx[1] : dx[0], fx = (ref ? mv[2] : mv[0]) & 31;
        QuadTaps t;
        t.set(gld<uint32_t>(d_tab_inter_chroma_filters + (fx ? hf_idx * 32 + fx : 0) * 4), d & 1);      // whole sample: {0, 64, 0, 0} of set 0
        // tap 0 of output x reads window column x + d: LDS column 2 xp + 4 + d, rounded down to a pair (2 .. 12, reads end at 17)
        const uint32_t *rp = (const uint32_t *)(L.win[q] + 2 * xp + kQwC0 + d - (d & 1));
        int t0[kQwRows], t1[kQwRows];
#pragma unroll
        for (int r = 0; r < kQwRows; r++) {
            int o0, o1;
            t.apply(rp[r * (kQwP / 2)], rp[r * (kQwP / 2) + 1], rp[r * (kQwP / 2) + 2], o0, o1);
            t0[r] = o0 >> (BD - 8);                                                  // put[..] stores int16: pack16 narrows
            t1[r] = o1 >> (BD - 8);
        }
        wave_sync();                                                                 // every lane has read its window rows: their bytes are free
        uint4 *c0 = (uint4 *)(L.tmpT[q] + (2 * xp) * kQtP), *c1 = (uint4 *)(L.tmpT[q] + (2 * xp + 1) * kQtP);
        c0[0] = make_uint4(pack16(t0[0], t0[0]), pack16(t0[0], t0[1]), pack16(t0[2], t0[3]), pack16(t0[4], t0[5]));
        c0[1] = make_uint4(pack16(t0[6], t0[7]), pack16(t0[8], t0[9]), pack16(t0[10], t0[10]), pack16(t0[10], t0[10]));
        c1[0] = make_uint4(pack16(t1[0], t1[0]), pack16(t1[0], t1[1]), pack16(t1[2], t1[3]), pack16(t1[4], t1[5]));
        c1[1] = make_uint4(pack16(t1[6], t1[7]), pack16(t1[8], t1[9]), pack16(t1[10], t1[10]), pack16(t1[10], t1[10]));
        wave_sync();
    }

    // ---- v pass: lane -> plane, column xo, both references, rows 0..7
    const int pl = l >> 3, xo = l & 7;
    int val[2][8];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int d = dy[i], fy = mv[2 * i + 1] & 31;
        QuadTaps t;
        t.set(gld<uint32_t>(d_tab_inter_chroma_filters + (fy ? vf_idx * 32 + fy : 0) * 4), d & 1);
        // tap 0 of output y reads window row y + d: intermediate row y + 2 + d, rounded down to a pair (0 .. 4, reads end at 15)
        const uint32_t *cp = (const uint32_t *)(L.tmpT[2 * i + pl] + xo * kQtP + 2 + d - (d & 1));
        uint32_t c[6];
#pragma unroll
        for (int m = 0; m < 6; m++) c[m] = cp[m];
#pragma unroll
        for (int yp = 0; yp < 4; yp++) {
            int o0, o1;
            t.apply(c[yp], c[yp + 1], c[yp + 2], o0, o1);
            val[i][2 * yp] = (int16_t)(o0 >> 6);                                     // put[..] stores int16
            val[i][2 * yp + 1] = (int16_t)(o1 >> 6);
        }
    }

    // ---- epilogue: the lane's plane has its own weights and destination
    const uint32_t s18 = pl ? b[18] : a[18], s19 = pl ? b[19] : a[19], s20 = pl ? b[20] : a[20], s22 = pl ? b[22] : a[22];
    const bool wf = ((s22 >> 8) & 0xff) != 0;
    const int denom = wf ? lo16s(s18) : 0, w0 = wf ? hi16s(s18) : 1, w1 = wf ? lo16s(s19) : 1;
    const int osum = wf ? hi16s(s19) + lo16s(s20) : 0;
    const int shift = denom + max(3, 15 - BD);
    const int off = ((osum << (BD - 8)) + 1) << (shift - 1);
    uint8_t *dst = (uint8_t *)(pl ? ptr64(b[0], b[1]) : ptr64(a[0], a[1]));
    const int dst_stride = (int)(pl ? b[8] : a[8]);
#pragma unroll
    for (int yy = 0; yy < 8; yy++) {
        const int p = (val[0][yy] * w0 + val[1][yy] * w1 + off) >> shift;
        st_px<BD>(dst + row_off(yy, dst_stride), xo, clip_px<BD>(p));
    }
    return true;
}

} // namespace vvc355
