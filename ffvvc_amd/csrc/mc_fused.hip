// Fused motion-compensated prediction for gfx950: for every block of at most 16x16 samples, interpolate from one or two
// reference pictures (8-tap luma / 4-tap chroma, any of the copy / h / v / hv cases) and blend (avg, w_avg) or round
// (put_uni, put_uni_w) straight to pixels — the 14-bit intermediates never go to HBM.
//
// This is the batched form of what the reference does per prediction block in luma_mc_bi / chroma_mc_bi / *_mc_uni
// (libavcodec/vvc/vvc_inter.c:222-460): put[..] x2 + avg / w_avg, or put_uni / put_uni_w.  Arithmetic follows
// libavcodec/h26x/h2656_inter_template.c:29-577 and libavcodec/vvc/vvc_inter_template.c:25-58 exactly (int16 narrowing of
// the horizontal pass and of the bi-prediction operands included).  Larger prediction blocks are cut into <= 16x16 tiles
// by the job builder; the interpolation is separable per output tile, so the result does not depend on the tiling.
//
// Mapping: one wave per block, four blocks per workgroup, no workgroup barrier.  The job descriptor is wave-uniform.
// Both reference windows are requested before anything waits on them, then go to LDS as uint16.  Each lane produces two
// horizontally adjacent outputs per step from aligned sample pairs with v_dot2c_i32_i16 (9 dot products for two 8-tap
// outputs, 5 for two 4-tap outputs) and writes the intermediate transposed, so that the vertical pass again reads aligned
// pairs.  The kernel is VALU-issue bound (rocprofv3: > 80 % of the per-SIMD VALU slots), hence the 4-tap specialisation.
#include <type_traits>
#include "common.hpp"
#include "pk16.hpp"
#include "wave.hpp"
#include "mc_filters.hpp"
#include "mc_tools.hpp"
#include "mc_chroma_quad.hpp"
#include "runtime.hpp"
#include "../../include/vvc_mi355.h"

namespace vvc355 {

static constexpr int kWinW = 24;      // LDS source window: up to 16 + 8 columns, even pitch
static constexpr int kWinH = 23;
static constexpr int kTmpP = 24;      // transposed intermediate: [column][row], up to 23 rows (+1 read-only slack), even pitch

// Window staging is split in two so that the loads of BOTH references are in flight before anything waits on them.
// Window index (r, c) <-> picture sample (r - LEAD, c - LEAD) when that direction is filtered, else (r, c - LEAD):
// LEAD = 3 (8 taps) or 1 (4 taps).  Lane -> column c = lane & 31, rows (lane >> 5) + 2 * it.  Lanes / rows the reference
// would not read load the block's own origin sample instead (always valid) and are zeroed by the select.
template <int BD, int NTAP>
__device__ __forceinline__ void fetch_window(const uint8_t *src, int src_stride, int lw, int h, bool hfrac, bool vfrac,
                                             int lane, uint16_t (&v)[(16 + NTAP) / 2])
{
    using px_t = typename Px<BD>::type;
    constexpr int LEAD = NTAP == 8 ? 3 : 1, NIT = (16 + NTAP) / 2;
    const int w = 1 << lw;
    const int c = lane & 31, col = c - LEAD;
    const bool col_ok = hfrac ? (c < w + NTAP - 1) : (col >= 0 && col < w);
    const int r_hi = vfrac ? h + NTAP - 1 : h;                       // window rows the filter reads
    const px_t *base = (const px_t *)src;
    const px_t *p = (const px_t *)(src + (ptrdiff_t)((lane >> 5) - (vfrac ? LEAD : 0)) * src_stride) + col;
    const ptrdiff_t step = (ptrdiff_t)src_stride * 2 / (ptrdiff_t)sizeof(px_t);
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        const int r = (lane >> 5) + 2 * it;
        const bool ok = col_ok && r < r_hi;
        const px_t *pp = ok ? p : base;
        const uint16_t s = (uint16_t)gld<px_t>(pp);
        v[it] = ok ? s : (uint16_t)0;
        p += step;
    }
}

template <int NTAP>
__device__ __forceinline__ void store_window(uint16_t *win, int lane, const uint16_t (&v)[(16 + NTAP) / 2])
{
    constexpr int NIT = (16 + NTAP) / 2;
    const int c = lane & 31;
    if (c < kWinW) {
        uint16_t *q = win + (lane >> 5) * kWinW + c;
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            if ((lane >> 5) + 2 * it < kWinH)
                q[it * 2 * kWinW] = v[it];
        }
    }
}

// One reference of one block, from its LDS window -> up to 4 intermediate values per lane (two row pairs of one column),
// 14-bit scaled ints.  Result layout: column x = lane & 15, row pair yp = (lane >> 4) + 4 * i (i = 0, 1), rows 2yp, 2yp + 1.
// SPLIT: the block is two 8-wide blocks of two planes side by side (outputs 0..7 | 8..15); the second plane's window starts
// at window column 12 instead of 8, i.e. its outputs read 4 columns further right.
template <int BD, int NTAP, bool SPLIT = false>
__device__ __forceinline__ void interp_block(int lw, int h, bool hfrac, bool vfrac, uint32_t hf_lo, uint32_t hf_hi,
                                             uint32_t vf_lo, uint32_t vf_hi, const uint16_t *win, int16_t *tmpT, int lane, int (&val)[4])
{
    constexpr int LEAD = NTAP == 8 ? 3 : 1, NO = NTAP / 2 + 1;
    const int w = 1 << lw;
    const int sh = vfrac ? h + NTAP - 1 : h;

    // ---- horizontal pass -> tmpT[x][r] (int16), r over the sh window rows
    if (hfrac) {
        Taps<NTAP> t;
        t.set(hf_lo, hf_hi);
        const int lhw = lw - 1;                         // log2 of the number of output pairs per row
        const int n = sh << lhw;
        for (int i = lane; i < n; i += 64) {
            const int r = i >> lhw, xp = i & ((1 << lhw) - 1);                  // outputs x = 2*xp, 2*xp + 1
            const uint32_t *d = (const uint32_t *)(win + r * kWinW + 2 * xp + (SPLIT && xp >= 4 ? 4 : 0));   // tap 0 of output x sits at window index x: aligned
            uint32_t dd[NO];
#pragma unroll
            for (int m = 0; m < NO; m++) dd[m] = d[m];
            int o0, o1;
            t.apply(dd, o0, o1);
            tmpT[(2 * xp) * kTmpP + r] = (int16_t)(o0 >> (BD - 8));
            tmpT[(2 * xp + 1) * kTmpP + r] = (int16_t)(o1 >> (BD - 8));
        }
    } else {
        const int n = sh << lw;
        for (int i = lane; i < n; i += 64) {
            const int r = i >> lw, x = i & (w - 1);
            tmpT[x * kTmpP + r] = (int16_t)win[r * kWinW + x + LEAD + (SPLIT && x >= 8 ? 4 : 0)];           // raw samples
        }
    }
    wave_sync();

    // ---- vertical pass: lane -> column x, two row pairs
    const int x = lane & 15;
    Taps<NTAP> t;
    t.set(vf_lo, vf_hi);
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int yp = (lane >> 4) + 4 * i;
        int o0 = 0, o1 = 0;
        if (x < w && 2 * yp < h) {
            if (vfrac) {
                const uint32_t *d = (const uint32_t *)(tmpT + x * kTmpP + 2 * yp);   // tap 0 of output y sits at window row y: aligned
                uint32_t dd[NO];
#pragma unroll
                for (int m = 0; m < NO; m++) dd[m] = d[m];
                t.apply(dd, o0, o1);
                // hv: second stage >> 6 on the int16 intermediates; v only: first stage on raw samples >> (bd - 8)
                const int sh2 = hfrac ? 6 : BD - 8;
                o0 >>= sh2; o1 >>= sh2;
            } else {
                const uint32_t d = *(const uint32_t *)(tmpT + x * kTmpP + 2 * yp);
                o0 = (int16_t)(d & 0xffff);
                o1 = (int16_t)(d >> 16);
                if (!hfrac) { o0 <<= 14 - BD; o1 <<= 14 - BD; }                      // integer position: sample << (14 - bd)
            }
        }
        val[2 * i] = o0;
        val[2 * i + 1] = o1;
    }
    wave_sync();
}

// both references of one block: windows requested together, then interpolated one after the other
template <int BD, int NTAP>
__device__ __forceinline__ void predict_refs(const vvc355_pred_job *job, int lw, int h, int mode, int frac,
                                             uint16_t (*win)[kWinH * kWinW], int16_t *tmpT, int lane, int (&v0)[4], int (&v1)[4])
{
    const uint32_t *taps = (const uint32_t *)job->hf0;  // hf0, vf0, hf1, vf1: 8 dwords (4-tap filters use the low dword)
    {
        uint16_t r0[(16 + NTAP) / 2], r1[(16 + NTAP) / 2];
        fetch_window<BD, NTAP>((const uint8_t *)job->src0, job->src0_stride, lw, h, frac & 1, frac & 2, lane, r0);
        if (mode < 2)
            fetch_window<BD, NTAP>((const uint8_t *)job->src1, job->src1_stride, lw, h, frac & 4, frac & 8, lane, r1);
        store_window<NTAP>(win[0], lane, r0);
        if (mode < 2)
            store_window<NTAP>(win[1], lane, r1);
        wave_sync();
    }
    interp_block<BD, NTAP>(lw, h, frac & 1, frac & 2, taps[0], taps[1], taps[2], taps[3], win[0], tmpT, lane, v0);
    if (mode < 2)
        interp_block<BD, NTAP>(lw, h, frac & 4, frac & 8, taps[4], taps[5], taps[6], taps[7], win[1], tmpT, lane, v1);
}

template <int BD>
__global__ __launch_bounds__(256) void pred_fused_kernel(const vvc355_pred_job *__restrict__ jobs, int n_jobs)
{
    __shared__ __attribute__((aligned(16))) uint16_t win_all[4][2][kWinH * kWinW];
    __shared__ __attribute__((aligned(16))) int16_t tmp_all[4][16 * kTmpP];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int ji = blockIdx.x * 4 + wave;
    if (ji >= n_jobs)
        return;
    const vvc355_pred_job job_copy = load_uniform(jobs + ji);           // wave-uniform address: scalar dword loads, fields unpacked on the SALU
    const vvc355_pred_job *job = &job_copy;
    const int w = job->w, h = job->h, mode = job->mode, frac = job->frac;
    const int lw = 31 - __builtin_clz(w);
    int v0[4], v1[4] = { 0, 0, 0, 0 };
    if (job->chroma)
        predict_refs<BD, 4>(job, lw, h, mode, frac, win_all[wave], tmp_all[wave], lane, v0, v1);
    else
        predict_refs<BD, 8>(job, lw, h, mode, frac, win_all[wave], tmp_all[wave], lane, v0, v1);
    if (mode < 2) {
        // the reference carries bi-prediction operands in int16 planes (put[..] narrows on store)
#pragma unroll
        for (int i = 0; i < 4; i++) { v0[i] = (int16_t)v0[i]; v1[i] = (int16_t)v1[i]; }
    }

    const int denom = job->denom, w0 = job->w0, w1 = job->w1, o0 = job->o0, o1 = job->o1;
    int shift, off;
    if (mode == 0)      { shift = max(3, 15 - BD); off = 1 << (shift - 1); }                                        // avg
    else if (mode == 1) { shift = denom + max(3, 15 - BD); off = (((o0 + o1) << (BD - 8)) + 1) << (shift - 1); }    // w_avg
    else if (mode == 2) { shift = 14 - BD; off = 1 << (shift - 1); }                                                // put_uni
    else                { shift = denom + 14 - BD; off = 1 << (shift - 1); }                                        // put_uni_w
    const int x = lane & 15;
    uint8_t *dst = (uint8_t *)job->dst;
    const int dst_stride = job->dst_stride;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int y = 2 * ((lane >> 4) + 4 * (i >> 1)) + (i & 1);
        if (x >= w || y >= h)
            continue;
        int p;
        if (mode == 0)      p = (v0[i] + v1[i] + off) >> shift;
        else if (mode == 1) p = (v0[i] * w0 + v1[i] * w1 + off) >> shift;
        else if (mode == 2) p = (frac & 3) ? (v0[i] + off) >> shift : v0[i] >> (14 - BD);      // integer position = plain copy
        else                p = ((v0[i] * w0 + off) >> shift) + o0 * (1 << (BD - 8));
        gst_at<typename Px<BD>::type>(dst, (uint32_t)(__mul24(y, dst_stride) + x * (int)sizeof(typename Px<BD>::type)), (typename Px<BD>::type)clip_px<BD>(p));
    }
}

// ------------------------------------------------------------------------------------------------ regular bi-prediction
//
// One wave per sub-block of at most 16x16: what pred_regular_blk (vvc_inter.c:772-822) does around the slots, on device.
// Every read of a reference plane goes through clamped coordinates (edge emulation, vvc_inter.c:33-110).  Bi-predicted luma
// sub-blocks with DMVR and / or BDOF (8 or 16 on a side) take the tools path of mc_tools.hpp; every other job (uni- and plain
// bi-prediction, GPM, chroma) takes bipred_plain below.

struct ClampRect { int x0, y0, x1, y1; };               // inclusive, in samples of the component

// NIT row pairs of a window whose index (0, 0) is plane sample (wx0, wy0): lane -> column lane & 31, rows (lane >> 5) + 2 it
template <int BD, int NIT>
__device__ __forceinline__ void fetch_clamped(const uint8_t *plane, int stride, const ClampRect &rc, int wx0, int wy0, int lane,
                                              uint16_t (&v)[NIT])
{
    using px_t = typename Px<BD>::type;
    const int xa = clip3(wx0 + (lane & 31), rc.x0, rc.x1) * (int)sizeof(px_t);
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        const int ya = clip3(wy0 + (lane >> 5) + 2 * it, rc.y0, rc.y1);
        v[it] = (uint16_t)gld_at<px_t>(plane, (uint32_t)(__mul24(ya, stride) + xa));      // clamped: never negative
    }
}

template <int NIT>
__device__ __forceinline__ void store_rows(uint16_t *win, int lane, const uint16_t (&v)[NIT])
{
    const int c = lane & 31;
    if (c < kWinW) {
        uint16_t *q = win + (lane >> 5) * kWinW + c;
#pragma unroll
        for (int it = 0; it < NIT; it++)
            if ((lane >> 5) + 2 * it < kWinH)
                q[it * 2 * kWinW] = v[it];
    }
}

// Unclamped form for windows that lie inside their readable rectangle (the common case): a lane moves 4 consecutive samples
// per step (one 8-byte load, one ds_write_b64), kWinW / 4 = 6 vectors per row: 3 steps cover a 23-row window, instead of 12
// one-sample steps.  fetch_vec4 only issues the loads (both references' loads go out before anything waits), put_vec4 stores.
template <int BD, int NV>
__device__ __forceinline__ void fetch_vec4(const uint8_t *plane, int stride, int wx0, int wy0, int nrows, int lane, uint2 (&v)[NV])
{
    using px_t = typename Px<BD>::type;
    const uint8_t *org = plane + row_off(wy0, stride) + wx0 * (int)sizeof(px_t);
#pragma unroll
    for (int it = 0; it < NV; it++) {
        const int id = lane + 64 * it, r = min(id / 6, nrows - 1), k = id - (id / 6) * 6;    // rows past the window re-read its last row
        const uint32_t p = (uint32_t)(__mul24(r, stride) + k * 4 * (int)sizeof(px_t));       // org is wave-uniform
        if (BD > 8) {
            v[it] = gld_at<uint2>(org, p);
        } else {
            const uint32_t q = gld_at<uint32_t>(org, p);
            v[it] = make_uint2(widen_lo(q), widen_hi(q));
        }
    }
}
template <int NV>
__device__ __forceinline__ void put_vec4(uint16_t *win, int nrows, int lane, const uint2 (&v)[NV])
{
#pragma unroll
    for (int it = 0; it < NV; it++) {
        const int id = lane + 64 * it, r = id / 6, k = id - r * 6;
        if (r < nrows)
            *(uint2 *)(win + r * kWinW + 4 * k) = v[it];
    }
}
__device__ __forceinline__ bool rect_holds(const ClampRect &rc, int wx0, int wy0, int nrows)
{
    return wx0 >= rc.x0 && wx0 + kWinW - 1 <= rc.x1 && wy0 >= rc.y0 && wy0 + nrows - 1 <= rc.y1;
}

// Per-wave LDS of the plain path (both reference windows, the transposed intermediate of interp_block): 2.9 KB per wave
struct BipredLds {
    uint16_t win[2][kWinH * kWinW];
    int16_t tmpT[16 * kTmpP];
};

// integer positions, fractions, readable rectangles of both references at motion mv (luma_mc_bi :262-283 / chroma_mc_bi
// :344-362, emulated_edge* :33-88); dmvr: the rectangle is the window of the unrefined block (emulated_edge_dmvr :61-88)
struct RefGeom {
    int ox[2], oy[2], fx[2], fy[2];
    ClampRect rc[2];
};
__device__ __forceinline__ RefGeom ref_geometry(const vvc355_bipred_job *job, const int (&mv)[4], bool chroma, bool dmvr)
{
    const int w = job->w, h = job->h;
    const int before = chroma ? 1 : 3, after = chroma ? 2 : 4;
    const int shx = 4 + (chroma ? job->hs : 0), shy = 4 + (chroma ? job->vs : 0);
    RefGeom g;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int mvx = mv[2 * i], mvy = mv[2 * i + 1];
        g.fx[i] = chroma ? (mvx & ((1 << shx) - 1)) << (1 - job->hs) : mvx & 15;
        g.fy[i] = chroma ? (mvy & ((1 << shy) - 1)) << (1 - job->vs) : mvy & 15;
        g.ox[i] = job->x + (mvx >> shx);
        g.oy[i] = job->y + (mvy >> shy);
        ClampRect &rc = g.rc[i];
        rc = ClampRect{ 0, 0, job->pic_w - 1, job->pic_h - 1 };
        if (dmvr) {
            const int x_sb = job->x + (job->mv[2 * i] >> shx), y_sb = job->y + (job->mv[2 * i + 1] >> shy);
            rc.x0 = min(max(x_sb - before, 0), job->pic_w - 1);
            rc.y0 = min(max(y_sb - before, 0), job->pic_h - 1);
            rc.x1 = rc.x0 + max(min((int)job->pic_w, x_sb + w + after) - rc.x0, 1) - 1;
            rc.y1 = rc.y0 + max(min((int)job->pic_h, y_sb + h + after) - rc.y0, 1) - 1;
        }
    }
    return g;
}

// both references at the positions of g: windows through clamped coordinates, then the separable interpolation of interp_block
// both = false: uni-prediction — only the first reference (the caller put the list in use at index 0 of g and in pa / sa)
template <int BD, int NTAP>
__device__ __forceinline__ void predict_clamped(const vvc355_bipred_job *job, BipredLds &L, int lane, int lw, int h, const RefGeom &g,
                                                int (&v0)[4], int (&v1)[4], const uint8_t *pa, int sa, const uint8_t *pb, int sb, bool both)
{
    constexpr int LEAD = NTAP == 8 ? 3 : 1, NIT = (16 + NTAP) / 2;
    {
        const int ax = g.ox[0] - LEAD, ay = g.oy[0] - (g.fy[0] ? LEAD : 0), an = g.fy[0] ? h + NTAP - 1 : h;
        const int bx = g.ox[1] - LEAD, by = g.oy[1] - (g.fy[1] ? LEAD : 0), bn = g.fy[1] ? h + NTAP - 1 : h;
        if (rect_holds(g.rc[0], ax, ay, an) && (!both || rect_holds(g.rc[1], bx, by, bn))) {
            constexpr int NV = NTAP == 8 ? 3 : 2;            // 23 x 6 = 138 <= 192 (luma), 19 x 6 = 114 <= 128 (chroma, h <= 16)
            uint2 q0[NV], q1[NV];
            fetch_vec4<BD, NV>(pa, sa, ax, ay, an, lane, q0);
            if (both)
                fetch_vec4<BD, NV>(pb, sb, bx, by, bn, lane, q1);
            put_vec4<NV>(L.win[0], an, lane, q0);
            if (both)
                put_vec4<NV>(L.win[1], bn, lane, q1);
        } else {
            uint16_t r0[NIT], r1[NIT];
            fetch_clamped<BD, NIT>(pa, sa, g.rc[0], ax, ay, lane, r0);
            if (both)
                fetch_clamped<BD, NIT>(pb, sb, g.rc[1], bx, by, lane, r1);
            store_rows<NIT>(L.win[0], lane, r0);
            if (both)
                store_rows<NIT>(L.win[1], lane, r1);
        }
        wave_sync();
    }
    uint32_t t[2][4];       // hf lo/hi, vf lo/hi per reference
#pragma unroll
    for (int i = 0; i < 2; i++) {
        if (NTAP == 8) {
            const uint2 hf = gld<uint2>(d_tab_inter_luma_filters + (job->hf_idx * 16 + g.fx[i]) * 8);
            const uint2 vf = gld<uint2>(d_tab_inter_luma_filters + (job->vf_idx * 16 + g.fy[i]) * 8);
            t[i][0] = hf.x; t[i][1] = hf.y; t[i][2] = vf.x; t[i][3] = vf.y;
        } else {
            t[i][0] = gld<uint32_t>(d_tab_inter_chroma_filters + (job->hf_idx * 32 + g.fx[i]) * 4); t[i][1] = 0;
            t[i][2] = gld<uint32_t>(d_tab_inter_chroma_filters + (job->vf_idx * 32 + g.fy[i]) * 4); t[i][3] = 0;
        }
    }
    interp_block<BD, NTAP>(lw, h, g.fx[0] != 0, g.fy[0] != 0, t[0][0], t[0][1], t[0][2], t[0][3], L.win[0], L.tmpT, lane, v0);
    if (both)
        interp_block<BD, NTAP>(lw, h, g.fx[1] != 0, g.fy[1] != 0, t[1][0], t[1][1], t[1][2], t[1][3], L.win[1], L.tmpT, lane, v1);
    else {
#pragma unroll
        for (int i = 0; i < 4; i++) v1[i] = 0;
    }
}

// what one wave of a luma launch needs: the plain path's planes or the tools path's (5.6 KB: 28 waves per CU)
union BipredLdsAll {
    BipredLds plain;
    ToolsLds<16, 16> tools;
};

// Every job but the ones of the tools path (bipred_kernel): uni-prediction, bi-prediction with avg / w_avg, and with gpm != nullptr
// the two parts of a geometric-partition coding unit (pred_gpm_blk, vvc_inter.c:466-527: luma_mc / chroma_mc per part, then
// inter.put_gpm with the per-sample weights of the partition's mask).  Luma ignores dmvr / bdof (vvc355_bipred_job) and records
// the unrefined motion; chroma is predicted at the motion in *rec, and its dmvr selects the clamp window.
template <int BD>
__device__ __forceinline__ void bipred_plain(const vvc355_bipred_job *job, BipredLds &L, int lane, const vvc355_gpm_job *gpm = nullptr)
{
    const int uni = job->pred_flag == 1 || job->pred_flag == 2;        // luma_mc_uni / chroma_mc_uni: one list
    const int w = job->w, h = job->h, chroma = job->chroma;
    const int lw = 31 - __builtin_clz(w);
    vvc355_bipred_result *rec = (vvc355_bipred_result *)job->rec;
    int mv[4] = { job->mv[0], job->mv[1], job->mv[2], job->mv[3] };
    if (rec && chroma) {
#pragma unroll
        for (int k = 0; k < 4; k++) mv[k] = gld<int>(&rec->mv[k]);
    } else if (rec && lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) gst<int>(&rec->mv[k], mv[k]);
        gst<int>(&rec->bdof, 0);
        gst<int>(&rec->min_sad, 0);
        gst<int>(&rec->searched, 0);
    }
    RefGeom g = ref_geometry(job, mv, chroma, chroma && job->dmvr && !uni);
    const uint8_t *lut = chroma ? nullptr : (const uint8_t *)job->lmcs_lut;      // luma of an LMCS slice is stored through the forward map
    int v0[4], v1[4];
    const uint8_t *pa = (const uint8_t *)job->ref0, *pb = (const uint8_t *)job->ref1;
    int sa = job->ref0_stride, sb = job->ref1_stride;
    if (uni && job->pred_flag == 2) {                     // list 1 only: it takes the first slot
        pa = pb; sa = sb;
        g.ox[0] = g.ox[1]; g.oy[0] = g.oy[1]; g.fx[0] = g.fx[1]; g.fy[0] = g.fy[1]; g.rc[0] = g.rc[1];
    }
    if (chroma)
        predict_clamped<BD, 4>(job, L, lane, lw, h, g, v0, v1, pa, sa, pb, sb, !uni);
    else
        predict_clamped<BD, 8>(job, L, lane, lw, h, g, v0, v1, pa, sa, pb, sb, !uni);
    if (uni) {
        // put_uni / put_uni_w (h2656_inter_template.c:44-81): rounding to pixels, weights from derive_weight_uni in (denom, w0, o0)
        const int wfu = job->weight_flag, sh = (wfu ? job->denom : 0) + 14 - BD, rnd = 1 << (sh - 1);
        const int xu = lane & 15;
        uint8_t *dstu = (uint8_t *)job->dst;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int y = 2 * ((lane >> 4) + 4 * (i >> 1)) + (i & 1);
            if (xu >= w || y >= h)
                continue;
            const int p = wfu ? ((v0[i] * job->w0 + rnd) >> sh) + job->o0 * (1 << (BD - 8)) : (v0[i] + rnd) >> sh;
            gst_at<typename Px<BD>::type>(dstu, (uint32_t)(__mul24(y, job->dst_stride) + xu * (int)sizeof(typename Px<BD>::type)), (typename Px<BD>::type)lmcs_fwd<BD>(lut, clip_px<BD>(p)));
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) { v0[i] = (int16_t)v0[i]; v1[i] = (int16_t)v1[i]; }     // put[..] stores int16
    if (gpm) {
        // put_gpm (vvc_inter_template.c:78): (s0 w + s1 (8 - w) + offset) >> max(5, 17 - bd), w = weights[y step_y + x step_x]
        constexpr int gsh = BD <= 12 ? 17 - BD : 5, goff = 1 << (gsh - 1);
        const uint8_t *wt = (const uint8_t *)gpm->weights;
        const int xg = lane & 15;
        uint8_t *dstg = (uint8_t *)job->dst;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int y = 2 * ((lane >> 4) + 4 * (i >> 1)) + (i & 1);
            if (xg >= w || y >= h)
                continue;
            const int wg = gld<uint8_t>(wt + y * gpm->step_y + xg * gpm->step_x);
            const int p = (v0[i] * wg + v1[i] * (8 - wg) + goff) >> gsh;
            gst_at<typename Px<BD>::type>(dstg, (uint32_t)(__mul24(y, job->dst_stride) + xg * (int)sizeof(typename Px<BD>::type)), (typename Px<BD>::type)lmcs_fwd<BD>(lut, clip_px<BD>(p)));
        }
        return;
    }
    int shift, off;
    const int wf = job->weight_flag, w0 = job->w0, w1 = job->w1;
    if (!wf) { shift = max(3, 15 - BD); off = 1 << (shift - 1); }                                                   // avg
    else     { shift = job->denom + max(3, 15 - BD); off = (((job->o0 + job->o1) << (BD - 8)) + 1) << (shift - 1); } // w_avg
    const int x = lane & 15;
    uint8_t *dst = (uint8_t *)job->dst;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int y = 2 * ((lane >> 4) + 4 * (i >> 1)) + (i & 1);
        if (x >= w || y >= h)
            continue;
        const int p = wf ? (v0[i] * w0 + v1[i] * w1 + off) >> shift : (v0[i] + v1[i] + off) >> shift;
        gst_at<typename Px<BD>::type>(dst, (uint32_t)(__mul24(y, job->dst_stride) + x * (int)sizeof(typename Px<BD>::type)), (typename Px<BD>::type)lmcs_fwd<BD>(lut, clip_px<BD>(p)));
    }
}

template <int BD, bool TOOLS>
__global__ __launch_bounds__(256) void bipred_kernel(const vvc355_bipred_job *__restrict__ jobs, int n_jobs)
{
    __shared__ __attribute__((aligned(16))) BipredLdsAll lds_all[4];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int ji = xcd_chunked(blockIdx.x, gridDim.x) * 4 + wave;
    if (ji >= n_jobs)
        return;
    // The descriptor is copied dword-wise at a wave-uniform address (scalar loads, issued once); reading its byte / short
    // fields through the pointer would be a vector load with a full memory round trip at every point of use.
    const vvc355_bipred_job job_copy = load_uniform(jobs + ji);
    const vvc355_bipred_job *job = &job_copy;
    BipredLdsAll &L = lds_all[wave];
    const int w = job->w, h = job->h, uni = job->pred_flag == 1 || job->pred_flag == 2;
    // bi-predicted luma sub-blocks with DMVR and / or BDOF (8 or 16 on a side, the only shapes those tools run on): mc_tools.hpp
    if (TOOLS && !job->chroma && !uni && (job->dmvr || job->bdof) && (w == 8 || w == 16) && (h == 8 || h == 16)) {
        if (w == 16 && h == 16)     bipred_tools<BD, 16, 16>(job, L.tools, lane);
        else if (w == 16)           bipred_tools<BD, 16, 8>(job, *(ToolsLds<16, 8> *)&L.tools, lane);
        else if (h == 16)           bipred_tools<BD, 8, 16>(job, *(ToolsLds<8, 16> *)&L.tools, lane);
        else                        bipred_tools<BD, 8, 8>(job, *(ToolsLds<8, 8> *)&L.tools, lane);
        return;
    }
    bipred_plain<BD>(job, L.plain, lane);
}

// Geometric-partition blocks: one wave per (<= 16x16 tile of a) part pair.  The job's base is a bi-prediction job without tools
// whose two references are the two parts' reference pictures.
template <int BD>
__global__ __launch_bounds__(256) void gpm_kernel(const vvc355_gpm_job *__restrict__ jobs, int n_jobs)
{
    __shared__ __attribute__((aligned(16))) BipredLds lds_all[4];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int ji = xcd_chunked(blockIdx.x, gridDim.x) * 4 + wave;
    if (ji >= n_jobs)
        return;
    const vvc355_gpm_job job = load_uniform(jobs + ji);
    vvc355_bipred_job base = job.base;
    base.pred_flag = 3; base.dmvr = 0; base.bdof = 0; base.weight_flag = 0; base.rec = 0;
    bipred_plain<BD>(&base, lds_all[wave], lane, &job);
}

// One PAIR of consecutive jobs, ia and ia + 1, by one wave.  When the two are the Cb and Cr blocks of one sub-block (same
// geometry and motion, width <= 8) they are predicted together as one 16-wide block whose halves come from two planes —
// an 8x8 block alone leaves half of the lanes of the vertical pass and of the window fetch idle.  Any other pair is done one
// job after the other; jobs that are not chroma are skipped.  ia is wave-uniform.
template <int BD>
__device__ __forceinline__ void chroma_pair(const vvc355_bipred_job *__restrict__ jobs, int ia, int n_jobs, BipredLds &L, int lane)
{
    using px_t = typename Px<BD>::type;
    const bool has_b = ia + 1 < n_jobs;
    const vvc355_bipred_job ja = load_uniform(jobs + ia), jb = load_uniform(jobs + (has_b ? ia + 1 : ia));
    const bool bi_a = !(ja.pred_flag == 1 || ja.pred_flag == 2), bi_b = !(jb.pred_flag == 1 || jb.pred_flag == 2);
    bool pair = has_b && bi_a && bi_b && ja.chroma && jb.chroma && ja.w <= 8 && ja.w == jb.w && ja.h == jb.h && ja.x == jb.x && ja.y == jb.y &&
                ja.rec == jb.rec && ja.hs == jb.hs && ja.vs == jb.vs && ja.dmvr == jb.dmvr && ja.hf_idx == jb.hf_idx &&
                ja.vf_idx == jb.vf_idx && ja.pic_w == jb.pic_w && ja.pic_h == jb.pic_h;
#pragma unroll
    for (int k = 0; k < 4; k++) pair = pair && ja.mv[k] == jb.mv[k];
    if (!pair) {
        if (ja.chroma)
            bipred_plain<BD>(&ja, L, lane);
        if (has_b && jb.chroma) {
            wave_sync();
            bipred_plain<BD>(&jb, L, lane);
        }
        return;
    }
    const vvc355_bipred_job *job = &ja;
    const int w = job->w, h = job->h;
    const vvc355_bipred_result *rec = (const vvc355_bipred_result *)job->rec;
    int mv[4] = { job->mv[0], job->mv[1], job->mv[2], job->mv[3] };
    if (rec) {
#pragma unroll
        for (int k = 0; k < 4; k++) mv[k] = rec->mv[k];                  // written by the luma launch: plain (scalar) loads
    }
    const RefGeom g = ref_geometry(job, mv, true, job->dmvr);
    // windows: columns 0..11 from the first plane, 12..23 from the second, both starting one sample left of the block
    {
        const int c = lane & 31, second = c >= 12, cc = c - (second ? 12 : 0);
        uint16_t r[2][10];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const uint8_t *pa = (const uint8_t *)(i ? ja.ref1 : ja.ref0), *pb = (const uint8_t *)(i ? jb.ref1 : jb.ref0);
            const int sa = i ? ja.ref1_stride : ja.ref0_stride, sb = i ? jb.ref1_stride : jb.ref0_stride;
            const uint8_t *plane = second ? pb : pa;
            const int stride = second ? sb : sa;
            const int xa = clip3(g.ox[i] - 1 + cc, g.rc[i].x0, g.rc[i].x1);
            const uint8_t *col = plane + xa * (int)sizeof(px_t);
            const int wy0 = g.oy[i] - (g.fy[i] ? 1 : 0);
#pragma unroll
            for (int it = 0; it < 10; it++) {
                const int ya = clip3(wy0 + (lane >> 5) + 2 * it, g.rc[i].y0, g.rc[i].y1);
                r[i][it] = (uint16_t)gld<px_t>(col + row_off(ya, stride));
            }
        }
        store_rows<10>(L.win[0], lane, r[0]);
        store_rows<10>(L.win[1], lane, r[1]);
        wave_sync();
    }
    uint32_t t[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        t[i][0] = gld<uint32_t>(d_tab_inter_chroma_filters + (job->hf_idx * 32 + g.fx[i]) * 4);
        t[i][1] = gld<uint32_t>(d_tab_inter_chroma_filters + (job->vf_idx * 32 + g.fy[i]) * 4);
    }
    int v0[4], v1[4];
    interp_block<BD, 4, true>(4, h, g.fx[0] != 0, g.fy[0] != 0, t[0][0], 0, t[0][1], 0, L.win[0], L.tmpT, lane, v0);
    interp_block<BD, 4, true>(4, h, g.fx[1] != 0, g.fy[1] != 0, t[1][0], 0, t[1][1], 0, L.win[1], L.tmpT, lane, v1);
#pragma unroll
    for (int i = 0; i < 4; i++) { v0[i] = (int16_t)v0[i]; v1[i] = (int16_t)v1[i]; }     // put[..] stores int16
    // lanes 0..7 of a row write the first plane, 8..15 the second, each with its own weights
    const int x = lane & 15, second = x >= 8, xo = x - (second ? 8 : 0);
    const int wf = second ? jb.weight_flag : ja.weight_flag, w0 = second ? jb.w0 : ja.w0, w1 = second ? jb.w1 : ja.w1;
    const int denom = second ? jb.denom : ja.denom, osum = second ? jb.o0 + jb.o1 : ja.o0 + ja.o1;
    const int shift = wf ? denom + max(3, 15 - BD) : max(3, 15 - BD);
    const int off = wf ? ((osum << (BD - 8)) + 1) << (shift - 1) : 1 << (shift - 1);
    uint8_t *dst = (uint8_t *)(second ? jb.dst : ja.dst);
    const int dst_stride = second ? jb.dst_stride : ja.dst_stride;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int y = 2 * ((lane >> 4) + 4 * (i >> 1)) + (i & 1);
        if (xo >= w || y >= h)
            continue;
        const int p = wf ? (v0[i] * w0 + v1[i] * w1 + off) >> shift : (v0[i] + v1[i] + off) >> shift;
        st_px<BD>(dst + row_off(y, dst_stride), xo, clip_px<BD>(p));
    }
}

// Chroma launch: one wave per EIGHT consecutive jobs, two waves per workgroup.  Four Cb/Cr pairs of 4:2:0 8x8 blocks whose windows
// lie inside their planes are predicted together by chroma_quad (mc_chroma_quad.hpp); any other wave — the tail of the launch
// included — does its pairs one after the other with chroma_pair.  The choice is wave-uniform.
union ChromaLds {
    BipredLds plain;
    QuadLds quad;
};

template <int BD>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(5, 5))) void bipred_chroma_pair_kernel(const vvc355_bipred_job *__restrict__ jobs, int n_jobs)
{
    __shared__ __attribute__((aligned(16))) ChromaLds lds_all[2];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int ia = 8 * (xcd_chunked(blockIdx.x, gridDim.x) * 2 + wave);
    if (ia >= n_jobs)
        return;
    ChromaLds &L = lds_all[wave];
    if (ia + 8 <= n_jobs) {
        // scalar look at the first descriptor: a wave of jobs of another shape declines before chroma_quad's 48 vector loads
        const vvc355_bipred_job j0 = load_uniform(jobs + ia);
        if (j0.w == 8 && j0.h == 8 && j0.hs == 1 && j0.vs == 1 && j0.chroma && j0.pred_flag != 1 && j0.pred_flag != 2 &&
            chroma_quad<BD>(jobs, ia, L.quad, lane))
            return;
    }
    const int end = min(ia + 8, n_jobs);
#pragma unroll 1
    for (int i = ia; i < end; i += 2) {
        chroma_pair<BD>(jobs, i, n_jobs, L.plain, lane);
        wave_sync();
    }
}

// The launch for job arrays that cannot take the quad path, e.g. the 4x4 chroma blocks of affine coding units: one wave per pair,
// four per workgroup, the one-pair path's 2.9 KB of LDS per wave and its registers only, so its occupancy is not the quad path's.
template <int BD>
__global__ __launch_bounds__(256) void bipred_chroma_one_pair_kernel(const vvc355_bipred_job *__restrict__ jobs, int n_jobs)
{
    __shared__ __attribute__((aligned(16))) BipredLds lds_all[4];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int ia = 2 * (xcd_chunked(blockIdx.x, gridDim.x) * 4 + wave);
    if (ia >= n_jobs)
        return;
    chroma_pair<BD>(jobs, ia, n_jobs, lds_all[wave], lane);
}

// The inter half of combined inter / intra coding units (vvc355_ciip_frame_pass): one wave per job, luma and chroma tiles of a
// picture in one launch.  CIIP has neither DMVR nor BDOF, so every job takes bipred_plain and a wave needs only the plain path's
// LDS.  A job with w == 0 or h == 0 does nothing: the builder leaves such jobs in the slots of the records it rejects.
template <int BD>
__global__ __launch_bounds__(256) void ciip_pred_kernel(const vvc355_bipred_job *__restrict__ jobs, int n_jobs)
{
    __shared__ __attribute__((aligned(16))) BipredLds lds_all[4];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int ji = xcd_chunked(blockIdx.x, gridDim.x) * 4 + wave;
    if (ji >= n_jobs)
        return;
    const vvc355_bipred_job job = load_uniform(jobs + ji);
    if (job.w <= 0 || job.h <= 0)                     // wave-uniform
        return;
    bipred_plain<BD>(&job, lds_all[wave], lane);
}

} // namespace vvc355

extern "C" void vvc355_pred_fused_batch(void *stream, int bd, const vvc355_pred_job *jobs_dev, int n_jobs)
{
    using namespace vvc355;
    if (n_jobs <= 0) return;
    VVC355_BD_DISPATCH(bd, hipLaunchKernelGGL((pred_fused_kernel<BD>), dim3((n_jobs + 3) / 4), dim3(256), 0, (hipStream_t)stream, jobs_dev, n_jobs));
    HIP_CHECK(hipGetLastError());
}

extern "C" void vvc355_bipred_batch(void *stream, int bd, const vvc355_bipred_job *jobs_dev, int n_jobs)
{
    using namespace vvc355;
    if (n_jobs <= 0) return;
    VVC355_BD_DISPATCH(bd, hipLaunchKernelGGL((bipred_kernel<BD, true>), dim3((n_jobs + 3) / 4), dim3(256), 0, (hipStream_t)stream, jobs_dev, n_jobs));
    HIP_CHECK(hipGetLastError());
}

extern "C" void vvc355_gpm_batch(void *stream, int bd, const vvc355_gpm_job *jobs_dev, int n_jobs)
{
    using namespace vvc355;
    if (n_jobs <= 0) return;
    VVC355_BD_DISPATCH(bd, hipLaunchKernelGGL((gpm_kernel<BD>), dim3((n_jobs + 3) / 4), dim3(256), 0, (hipStream_t)stream, jobs_dev, n_jobs));
    HIP_CHECK(hipGetLastError());
}

extern "C" void vvc355_bipred_chroma_batch(void *stream, int bd, const vvc355_bipred_job *jobs_dev, int n_jobs)
{
    using namespace vvc355;
    if (n_jobs <= 0) return;
    const int n_waves = (n_jobs + 7) / 8;             // eight jobs (four Cb/Cr pairs) per wave
    VVC355_BD_DISPATCH(bd, hipLaunchKernelGGL((bipred_chroma_pair_kernel<BD>), dim3((n_waves + 1) / 2), dim3(128), 0, (hipStream_t)stream, jobs_dev, n_jobs));
    HIP_CHECK(hipGetLastError());
}

// the launch of ciip_pred_kernel for inter_cu.hip's vvc355_ciip_frame_pass (the kernel lives here, next to bipred_plain)
namespace vvc355 {

// chroma jobs that are known not to be 4:2:0 8x8 pairs (inter_cu.hip's affine pass writes 4x4 blocks): bipred_chroma_one_pair_kernel
void chroma_pairs_launch(hipStream_t stream, int bd, const vvc355_bipred_job *jobs_dev, int n_jobs)
{
    if (n_jobs <= 0) return;
    const int n_pairs = (n_jobs + 1) / 2;
    VVC355_BD_DISPATCH(bd, hipLaunchKernelGGL((bipred_chroma_one_pair_kernel<BD>), dim3((n_pairs + 3) / 4), dim3(256), 0, stream, jobs_dev, n_jobs));
    HIP_CHECK(hipGetLastError());
}

void ciip_pred_launch(hipStream_t stream, int bd, const vvc355_bipred_job *jobs_dev, int n_jobs)
{
    if (n_jobs <= 0) return;
    VVC355_BD_DISPATCH(bd, hipLaunchKernelGGL((ciip_pred_kernel<BD>), dim3((n_jobs + 3) / 4), dim3(256), 0, stream, jobs_dev, n_jobs));
    HIP_CHECK(hipGetLastError());
}

} // namespace vvc355
