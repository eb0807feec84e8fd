// Inverse transform (DCT-2 / DST-7 / DCT-8, 1-D and 2-D, up to 64x64), LFNST, residual add and BDPCM kernels for gfx950.
//
// Reference behaviour: libavcodec/vvc/vvcdsp.c:67-195 (scale_clip, scale, itx_2d, itx_1d, the generator),
// libavcodec/vvc/vvc_itx_1d.c:64-721 (nz gating of the DCT-2 butterflies, matrix_mul, ff_vvc_inv_lfnst_1d),
// libavcodec/vvc/vvcdsp_template.c:32-100 (add_residual, joint variants, transform_bdpcm) and :142-159 (which entries exist).
//
// The reference's partial butterflies are wrapping int32 arithmetic, i.e. exactly a dot product with the transform matrix
// over the inputs its nz gating keeps.  One workgroup owns one transform block: coefficients are staged in LDS, the column
// pass spreads (column, output row) pairs over the lanes, then the row pass does the same for (row, output column).
#include <type_traits>
#include "common.hpp"
#include "pk16.hpp"
#include "wave.hpp"
#include "runtime.hpp"
#include "resid_math.hpp"
#include "../../include/vvc_mi355.h"
#include "stage_checks.hpp"

namespace vvc355 {

#define VVC355_TABLE(type, name, count) __device__ static const type d_tab_##name[count]
#include "tables.inc"
#undef VVC355_TABLE
// the reference's inline tables as compile-time constants (tables_small.inc): the arithmetic / packed forms the kernels use are proven
// equal to them here
#define VVC355_TABLE(type, name, count) static constexpr type c_##name[count]
#include "tables_small.inc"
#undef VVC355_TABLE
// levelScale[rect_non_ts][qp % 6] of the scaling process (level_scale, vvc_intra.c:329-336)
__host__ __device__ constexpr int level_scale_of(int rect, int rem)
{
    return rect ? (rem == 0 ? 57 : rem == 1 ? 64 : rem == 2 ? 72 : rem == 3 ? 80 : rem == 4 ? 90 : 102)
                : (rem == 0 ? 40 : rem == 1 ? 45 : rem == 2 ? 51 : rem == 3 ? 57 : rem == 4 ? 64 : 72);
}
// 6.5.2 up-right diagonal scan of a 4x4 block (ff_vvc_diag_scan_x / _y [2][2], vvc_data.c:27,152), one 4-bit field per scan position
static constexpr unsigned long long kDiag4X = 0x3323213210210100ull, kDiag4Y = 0x3231230123012010ull;
constexpr bool itx_small_tables_match()
{
    for (int r = 0; r < 2; r++)
        for (int q = 0; q < 6; q++)
            if (level_scale_of(r, q) != c_level_scale[r * 6 + q]) return false;
    for (int i = 0; i < 16; i++)
        if ((int)((kDiag4X >> (4 * i)) & 15) != c_diag_scan_4x4_x[i] || (int)((kDiag4Y >> (4 * i)) & 15) != c_diag_scan_4x4_y[i]) return false;
    return true;
}
static_assert(itx_small_tables_match(), "level scale / 4x4 diagonal scan differ from vvc_intra.c:329-336 / vvc_data.c:27,152");

enum { TX_DCT2 = 0, TX_DST7 = 1, TX_DCT8 = 2 };

__device__ __forceinline__ const int8_t *dxt_matrix(int type, int n)
{
    if (type == TX_DST7)
        return n == 4 ? d_tab_dst7_4 : n == 8 ? d_tab_dst7_8 : n == 16 ? d_tab_dst7_16 : d_tab_dst7_32;
    return n == 4 ? d_tab_dct8_4 : n == 8 ? d_tab_dct8_8 : n == 16 ? d_tab_dct8_16 : d_tab_dct8_32;
}

// Number of leading inputs a 1-D transform of size n reads for a given nz (vvc_itx_1d.c:64-67,:498,:659):
// DCT-2 gates inputs in groups {0,1},{2,3},{4..7},{8..15},{16..31} and never reads inputs >= 32 of the 64-point transform;
// DST-7 / DCT-8 read exactly nz (<= 16) inputs.
__device__ __forceinline__ int inputs_used(int type, int n, int nz)
{
    if (type != TX_DCT2)
        return nz;
    int used = 2;
    while (used < nz)
        used <<= 1;                  // k takes part iff k < 2 or nz > 2^floor(log2 k)  <=>  k < used
    used = min(used, n);
    return n == 64 ? min(used, 32) : used;
}

// output i of an n-point inverse transform of `cnt` inputs in[0], in[step], ...
__device__ __forceinline__ int inv_tx_out(int type, int n, int i, const int *in, int step, int cnt, const int8_t *cos_lds)
{
    unsigned acc = 0;
    if (type == TX_DCT2) {
        const int ang = (2 * i + 1) * (64 / n);
        for (int k = 0; k < cnt; k++)
            acc += (unsigned)in[k * step] * (unsigned)(int)cos_lds[(ang * k) & 255];
    } else {
        const int8_t *m = dxt_matrix(type, n) + i;
        for (int k = 0; k < cnt; k++)
            acc += (unsigned)in[k * step] * (unsigned)(int)m[k * n];
    }
    return (int)acc;
}

// Scaling process for transform coefficients (vvc_intra.c:277-417) as a per-coefficient function: derive_qp's shift and
// rectangular correction (:297-309), derive_scale (:311-338), derive_scale_m's up-sampling and DC override (:373-381),
// scale_coeff (:391-397).  Shared by dequant_kernel and by the itx kernels' fused load stage.
// derive_transform_type (vvc_intra.c:130-164): implicit / explicit MTS -> trh | trv << 4; flags = VVC355_TU_*
__host__ __device__ inline int derive_tr_type(int flags, int mts_idx, int lfnst_idx, int c_idx, int w, int h)
{
    const bool isp = flags & VVC355_TU_ISP, sbt = flags & VVC355_TU_SBT;
    if (c_idx || (isp && lfnst_idx))
        return 0;
    bool implicit = false;
    if (flags & VVC355_TU_MTS_ENABLED)
        implicit = isp || (sbt && (w > h ? w : h) <= 32) ||
                   (!(flags & VVC355_TU_EXPLICIT_MTS_INTRA) && (flags & VVC355_TU_INTRA) && !lfnst_idx && !(flags & VVC355_TU_MIP));
    if (implicit) {
        int trh, trv;
        if (sbt) {
            const bool hor = flags & VVC355_TU_SBT_HORIZONTAL, pos = flags & VVC355_TU_SBT_POS;
            trh = (hor || pos) ? 1 : 2;
            trv = (!hor || pos) ? 1 : 2;
        } else {
            trh = (w >= 4 && w <= 16) ? 1 : 0;
            trv = (h >= 4 && h <= 16) ? 1 : 0;
        }
        return trh | (trv << 4);
    }
    // mts_idx -> (trh, trv): { DCT2, DST7, DCT8, DST7, DCT8 } / { DCT2, DST7, DST7, DCT8, DCT8 }
    const int trh = mts_idx == 0 ? 0 : (mts_idx & 1) ? 1 : 2, trv = mts_idx == 0 ? 0 : mts_idx <= 2 ? 1 : 2;
    return trh | (trv << 4);
}
// a job that asks for it gets its transform types from the rule above instead of from its trh / trv fields
__device__ __forceinline__ void resolve_type(vvc355_itx_job &job)
{
    if (job.mts_flags & VVC355_ITX_DERIVE_TYPE) {
        const int t = derive_tr_type(job.tu_flags, job.mts_idx, job.lfnst_idx, job.c_idx, 1 << job.log2_w, 1 << job.log2_h);
        job.trh = (uint8_t)(t & 15);
        job.trv = (uint8_t)(t >> 4);
    }
}

struct Dequant {
    int on, scale, bd_shift, bd_offset, range, lw, lh, lm, dc;
    const uint8_t *sm;
    __device__ __forceinline__ void setup(int enable, int lw_, int lh_, int qp_in, int ts, int dep_quant, int bit_depth, int range_,
                                          const uint8_t *sm_, int lm_, int dc_)
    {
        on = enable; lw = lw_; lh = lh_; range = range_; sm = sm_; lm = lm_; dc = dc_;
        const int log_sum = lw + lh, rect = ts ? 0 : (log_sum & 1);
        bd_shift = ts ? 10 : bit_depth + rect + (log_sum / 2) + 10 - range + dep_quant;
        bd_offset = (1 << bd_shift) >> 1;
        const int qp = qp_in + (dep_quant && !ts ? 1 : 0), rem = qp % 6;
        scale = level_scale_of(rect, rem) << (qp / 6);
    }
    __device__ __forceinline__ int apply(int c, int x, int y) const
    {
        if (!on || !c)
            return c;
        int m = 16;
        if (sm) {
            m = gld<uint8_t>(sm + (((y << lm) >> lh) << lm) + ((x << lm) >> lw));
            if (dc >= 0 && x == 0 && y == 0)
                m = dc;
        }
        return clip_intp2((int)((unsigned)c * (unsigned)scale * (unsigned)m + (unsigned)bd_offset) >> bd_shift, range);
    }
    // the same for |c| < 2^15 (every level a conforming stream codes): c * m and (c * m) * scale are 24-bit multiplies, full
    // rate instead of two quarter-rate 32-bit multiplies; products wrap to 32 bits exactly like the expression above
    __device__ __forceinline__ int apply_small(int c, int x, int y) const
    {
        if (!on || !c)
            return c;
        int m = 16;
        if (sm) {
            m = gld<uint8_t>(sm + (((y << lm) >> lh) << lm) + ((x << lm) >> lw));
            if (dc >= 0 && x == 0 && y == 0)
                m = dc;
        }
        return clip_intp2((int)((unsigned)__mul24(__mul24(c, m), scale) + (unsigned)bd_offset) >> bd_shift, range);
    }
};

__device__ __forceinline__ Dequant itx_job_dequant(const vvc355_itx_job &job, int bd)
{
    Dequant dq;
    dq.setup(job.dq_flags & 1, job.log2_w, job.log2_h, job.dq_qp, 0, (job.dq_flags >> 1) & 1, bd, job.range,
             (const uint8_t *)job.scale_matrix, job.log2_matrix_size, job.dc);
    return dq;
}

// Level source of the _lv entries (vvc355_tb_levels): side records paired with the jobs, and the picture's int16 group stream.
struct LvSrc {
    const vvc355_tb_levels *lv;
    const int16_t *levels;
};
// The kernels take it as an optional trailing argument (a pack of zero or one LvSrc), so that their int32 instantiations keep the
// argument list and the code they had before packed levels existed.
__device__ __forceinline__ LvSrc lv_src() { return LvSrc{ nullptr, nullptr }; }
__device__ __forceinline__ LvSrc lv_src(LvSrc s) { return s; }
// the group of a packed block that holds sample (x, y): first + the number of coded tiles before it in bit order; nullptr when the tile is
// not coded (or lies beyond the 32 x 32 grid, where nothing is)
__device__ __forceinline__ const int16_t *lv_group(const vvc355_tb_levels &r, const int16_t *levels, int log2_w, int x, int y)
{
    if (x >= 32 || y >= 32)
        return nullptr;
    const int b = (y >> 2) * (((1 << min(log2_w, 5)) + 3) >> 2) + (x >> 2);
    if (!((r.groups >> b) & 1))
        return nullptr;
    return levels + ((size_t)r.first + __popcll(r.groups & ((1ull << b) - 1))) * 16;
}
__device__ __forceinline__ int lv_level(const vvc355_tb_levels &r, const int16_t *levels, int log2_w, int x, int y)
{
    const int16_t *g = lv_group(r, levels, log2_w, x, y);
    return g ? (int)gld<int16_t>(g + (y & 3) * 4 + (x & 3)) : 0;
}
__device__ __forceinline__ int4 unpack_i16x4(uint2 u)
{
    return make_int4((int)(int16_t)(u.x & 0xffff), (int)u.x >> 16, (int)(int16_t)(u.y & 0xffff), (int)u.y >> 16);
}
// levels e .. e + 3 of a row-major block: 8 bytes of one group when the block is at least 4 wide, single levels otherwise
__device__ __forceinline__ int4 lv_load4(const vvc355_tb_levels &r, const int16_t *levels, int log2_w, int e)
{
    const int w = 1 << log2_w;
    if (w >= 4) {
        const int x = e & (w - 1), y = e >> log2_w;
        const int16_t *g = lv_group(r, levels, log2_w, x, y);
        return g ? unpack_i16x4(gld<uint2>(g + (y & 3) * 4)) : make_int4(0, 0, 0, 0);
    }
    int v[4];
#pragma unroll
    for (int q = 0; q < 4; q++)
        v[q] = lv_level(r, levels, log2_w, (e + q) & (w - 1), (e + q) >> log2_w);
    return make_int4(v[0], v[1], v[2], v[3]);
}

// One transform block of any shape with w * h <= CAP, worked on by the NT lanes `tid` = 0..NT-1 of a group (NT <= 64: the
// group sits inside one wave and synchronises at wave level; NT = 256: the whole workgroup).  buf / tmp: CAP ints of LDS each.
// PACKED: the levels come from the side record `lvr` (groups in `levels`, or int32 at job.coeffs for VVC355_LEVELS_INT32).
// LFNST: with lf_idx = 1 / 2 the staged block goes through ilfnst_transform (vvc_intra.c:65-127) between the scaling process and the column
// pass (the intra record path; lf_idx, lf_mode are uniform over the group, w and h are at least 4).
// EPI: with an epilogue type the residual goes sample by sample to epi->sample(x, y, element, residual) instead of to job.coeffs / job.dst
// (the inter record path's blocks that cannot take the shape-specialised code; such a job has dst = 0 and store_coeffs = 0).
template <int BD, int NT, int CAP, bool PACKED = false, bool LFNST = false, class EPI = void>
__device__ __forceinline__ void itx_generic_block(const vvc355_itx_job &job, int *buf, int *tmp, const int8_t *cos_lds, int tid,
                                                  const vvc355_tb_levels *lvr = nullptr, const int16_t *levels = nullptr,
                                                  int lf_idx = 0, int lf_mode = 0, EPI *epi = nullptr)
{
    constexpr bool WAVE = NT <= 64;                  // the group lives inside one wave
    const int w = 1 << job.log2_w, h = 1 << job.log2_h, n = w * h;
    int nzw = job.nzw, nzh = job.nzh;
    const int range = job.range, bd = job.bd ? job.bd : BD;
    int *coeffs = (int *)job.coeffs;

    // I/O mapping: lane `tid` owns the PER consecutive elements starting at tid * PER (row-major), so coefficients move as
    // 16-byte vectors and pixels as 8/16-byte row segments.  The prediction samples the residual is added to are requested
    // together with the coefficients, long before they are needed (one memory round trip on the critical path, not two).
    constexpr int PER = CAP >= NT ? CAP / NT : 1;    // 1, 4, 4, 16
    using px_t = typename Px<BD>::type;
    uint8_t *dst = (uint8_t *)job.dst;
    const int e0 = tid * PER;
    const bool row_io = PER > 1 && w >= PER;         // the lane's elements sit in one row: vector pixel access
    px_t pred[PER];
    if (dst && e0 < n) {
        if (row_io) {
            const VVC355_GLOBAL px_t *prow = (const VVC355_GLOBAL px_t *)(dst + (ptrdiff_t)(e0 >> job.log2_w) * job.dst_stride) + (e0 & (w - 1));
#pragma unroll
            for (int q = 0; q < PER; q++)
                pred[q] = prow[q];                   // contiguous, aligned to PER samples: merged into wide loads
        } else {
#pragma unroll
            for (int q = 0; q < PER; q++) {
                const int o = e0 + q;
                pred[q] = o < n ? (px_t)ld_px<BD>(dst + (ptrdiff_t)(o >> job.log2_w) * job.dst_stride, o & (w - 1)) : (px_t)0;
            }
        }
    }
    const Dequant dq = itx_job_dequant(job, bd);
    const bool packed = PACKED && !(lvr->flags & VVC355_LEVELS_INT32);
    if (PER < 4) {
#pragma unroll
        for (int q = 0; q < PER; q++)
            if (e0 + q < n) {
                const int x = (e0 + q) & (w - 1), y = (e0 + q) >> job.log2_w;
                buf[e0 + q] = dq.apply(packed ? lv_level(*lvr, levels, job.log2_w, x, y) : gld<int>(coeffs + e0 + q), x, y);
            }
    } else {
#pragma unroll
        for (int c4 = 0; c4 < PER / 4; c4++) {
            const int e = e0 + c4 * 4;
            if (e < n) {                             // n is a multiple of 4 for every block of >= 4 coefficients
                int4 v = packed ? lv_load4(*lvr, levels, job.log2_w, e) : gld<int4>(coeffs + e);
                if (dq.on) {
                    const int y = e >> job.log2_w, x = e & (w - 1);      // w >= 4 here: the four share a row
                    v.x = dq.apply(v.x, x, y); v.y = dq.apply(v.y, x + 1, y); v.z = dq.apply(v.z, x + 2, y); v.w = dq.apply(v.w, x + 3, y);
                }
                *(int4 *)&buf[e] = v;
            }
        }
    }
    group_sync<NT>();

    if constexpr (LFNST) {
        if (lf_idx) {
            // The first 8 / 16 scaled levels in 4x4 diagonal scan order times the 16x16 / 16x48 matrix of (set, lf_idx), rounded and clipped
            // (ff_vvc_inv_lfnst_1d, vvc_itx_1d.c:708), into the top-left 4x4 or the 8x8 L-shape, transposed for modes above 34: the
            // arithmetic of lfnst_batch_kernel, with the outputs spread over the group's lanes.  The L-shape overlaps the scan positions,
            // so nothing is written before every lane has finished reading.
            constexpr int MAXO = NT >= 64 ? 1 : NT == 16 ? 3 : 4;        // outputs per lane: ceil(48 / NT); 4 lanes only ever hold a 4x4
            const bool big = w >= 8 && h >= 8;
            const int n_out = big ? 48 : 16;
            const int nz = ((w == 8 && h == 8) || (w == 4 && h == 4)) ? 8 : 16;
            const int set = lf_mode < 0 ? 1 : d_tab_lfnst_tr_set_index[lf_mode];
            const int8_t *m = big ? d_tab_lfnst_8x8 + (set * 2 + lf_idx - 1) * 16 * 48 : d_tab_lfnst_4x4 + (set * 2 + lf_idx - 1) * 16 * 16;
            unsigned t[MAXO];
#pragma unroll
            for (int q = 0; q < MAXO; q++)
                t[q] = 0;
            for (int i = 0; i < nz; i++) {
                const unsigned u = (unsigned)buf[w * (int)((kDiag4Y >> (4 * i)) & 15) + (int)((kDiag4X >> (4 * i)) & 15)];
#pragma unroll
                for (int q = 0; q < MAXO; q++) {
                    const int j = tid + q * NT;
                    if (j < n_out)
                        t[q] += u * (unsigned)(int)m[i * n_out + j];
                }
            }
            group_sync<NT>();
#pragma unroll
            for (int q = 0; q < MAXO; q++) {
                const int j = tid + q * NT;
                if (j < n_out) {
                    int x, y;
                    if (lf_mode > 34) {         // transposed placement (:86-110)
                        if (!big)        { y = j & 3; x = j >> 2; }
                        else if (j < 32) { y = j & 7; x = j >> 3; }
                        else             { y = (j - 32) & 3; x = 4 + ((j - 32) >> 2); }
                    } else {                    // row by row: 8 (4) values in rows 0..3, 4 in rows 4..7 (:111-120)
                        if (!big)        { y = j >> 2; x = j & 3; }
                        else if (j < 32) { y = j >> 3; x = j & 7; }
                        else             { y = 4 + ((j - 32) >> 2); x = (j - 32) & 3; }
                    }
                    buf[y * w + x] = clip_intp2(((int)t[q] + 64) >> 7, range);
                }
            }
            nzw = nzh = big ? 8 : 4;
            group_sync<NT>();
        }
    }

    const bool dc_only = job.trh == TX_DCT2 && job.trv == TX_DCT2 && nzw == 1 && nzh == 1;
    int sh_final;
    if (w > 1 && h > 1) {
        const int sh1 = 7;
        sh_final = 5 + range - bd;
        if (w == h && dc_only) {
            const int t = (buf[0] * 64 + (1 << (sh1 - 1))) >> sh1;
            const int dc = (t * 64 + (1 << (sh_final - 1))) >> sh_final;
            group_sync<NT>();
            for (int i = tid; i < n; i += NT)
                buf[i] = dc;
            sh_final = -1;
        } else if (w >= 4 && h >= 4) {
            // Register-tiled passes: every lane accumulates FOUR outputs that share the matrix entry, reading the four
            // inputs as one 16-byte LDS vector, i.e. one LDS vector + one table byte + four multiply-adds per four products.
            // Column pass: lane -> (row y, columns x0..x0+3); result stored transposed (tmp[x][y]) so that the row pass can
            // do the same with lane -> (column x, rows y0..y0+3).
            const int cnt = inputs_used(job.trv, h, nzh);
            const int cnt2 = inputs_used(job.trh, w, nzw);          // the row pass reads columns < cnt2 (zero beyond nzw)
            // 24-bit multiplies are exact when every input magnitude is below 2^23: always true for the clipped intermediates
            // of the row pass (range <= 20), checked here for the coefficients (the decoder's dequantiser clips them to range)
            bool small = true;
            for (int i = tid; i < n; i += NT)
                small &= (unsigned)(buf[i] + (1 << 23)) < (1u << 24);
            bool fast1;
            if (WAVE) {
                // group vote inside the wave: the NT lanes of this block occupy an aligned bit field of the ballot
                const unsigned long long gm = (NT == 64 ? ~0ull : ((1ull << (NT & 63)) - 1)) << ((threadIdx.x & 63) & ~(NT - 1));
                fast1 = (__ballot(small) & gm) == gm;
            } else {
                fast1 = (bool)__syncthreads_and(small);
            }
            const int gx = (cnt2 + 3) >> 2, lgh = job.log2_h;
            const int8_t *mv = job.trv == TX_DCT2 ? nullptr : dxt_matrix(job.trv, h);
            for (int g = tid; g < (gx << lgh); g += NT) {
                const int y = g & (h - 1), x0 = (g >> lgh) << 2;
                int acc[4] = { 0, 0, 0, 0 };
                if (x0 < nzw) {
                    const int ang = (2 * y + 1) * (64 >> lgh);
                    int a = 0;
                    for (int k = 0; k < cnt; k++) {
                        const int m = mv ? (int)mv[k * h + y] : (int)cos_lds[a];
                        a = (a + ang) & 255;
                        const int4 v = *(const int4 *)&buf[k * w + x0];
                        if (fast1) {
                            acc[0] += __mul24(m, v.x); acc[1] += __mul24(m, v.y); acc[2] += __mul24(m, v.z); acc[3] += __mul24(m, v.w);
                        } else {
                            acc[0] += m * v.x; acc[1] += m * v.y; acc[2] += m * v.z; acc[3] += m * v.w;
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int x = x0 + q;
                    if (x < w)
                        tmp[x * h + y] = x < nzw ? clip_intp2((acc[q] + (1 << (sh1 - 1))) >> sh1, range) : 0;
                }
            }
            group_sync<NT>();
            const int8_t *mh = job.trh == TX_DCT2 ? nullptr : dxt_matrix(job.trh, w);
            for (int g = tid; g < (n >> 2); g += NT) {
                const int x = g & (w - 1), y0 = (g >> job.log2_w) << 2;
                const int ang = (2 * x + 1) * (64 >> job.log2_w);
                int acc[4] = { 0, 0, 0, 0 }, a = 0;
                for (int k = 0; k < cnt2; k++) {
                    const int m = mh ? (int)mh[k * w + x] : (int)cos_lds[a];
                    a = (a + ang) & 255;
                    const int4 v = *(const int4 *)&tmp[k * h + y0];
                    acc[0] += __mul24(m, v.x); acc[1] += __mul24(m, v.y); acc[2] += __mul24(m, v.z); acc[3] += __mul24(m, v.w);
                }
                // the old contents of buf (the coefficients) are dead once every lane has left the column pass
#pragma unroll
                for (int q = 0; q < 4; q++)
                    buf[(y0 + q) * w + x] = acc[q];
            }
        } else {
            // column pass on columns < nzw (vertical type, size h), then scale_clip; other columns become zero
            const int cnt = inputs_used(job.trv, h, nzh);
            for (int o = tid; o < n; o += NT) {
                const int y = o >> job.log2_w, x = o & (w - 1);
                int v = 0;
                if (x < nzw) {
                    v = inv_tx_out(job.trv, h, y, buf + x, w, cnt, cos_lds);
                    v = clip_intp2((v + (1 << (sh1 - 1))) >> sh1, range);
                }
                tmp[o] = v;
            }
            group_sync<NT>();
            // row pass (horizontal type, size w) with nz = nzw
            const int cnt2 = inputs_used(job.trh, w, nzw);
            for (int o = tid; o < n; o += NT) {
                const int y = o >> job.log2_w, x = o & (w - 1);
                buf[o] = inv_tx_out(job.trh, w, x, tmp + y * w, 1, cnt2, cos_lds);
            }
        }
    } else {
        sh_final = 6 + range - bd;
        if (dc_only) {
            const int dc = (buf[0] * 64 + (1 << (sh_final - 1))) >> sh_final;
            group_sync<NT>();
            for (int i = tid; i < n; i += NT)
                buf[i] = dc;
            sh_final = -1;
        } else {
            const int type = w > 1 ? job.trh : job.trv, nz = w > 1 ? nzw : nzh;
            const int cnt = inputs_used(type, n, nz);
            for (int o = tid; o < n; o += NT)
                tmp[o] = inv_tx_out(type, n, o, buf, 1, cnt, cos_lds);
            group_sync<NT>();
            for (int o = tid; o < n; o += NT)
                buf[o] = tmp[o];
        }
    }
    group_sync<NT>();
    // final scale, then store residuals in place (slot semantics) and/or add them to the prediction
    if (e0 < n) {
        int r[PER];
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const int o = e0 + q;
            r[q] = o < n ? (sh_final < 0 ? buf[o] : (buf[o] + (1 << (sh_final - 1))) >> sh_final) : 0;
        }
        if constexpr (!std::is_void<EPI>::value) {
#pragma unroll
            for (int q = 0; q < PER; q++)
                if (e0 + q < n)
                    epi->sample((e0 + q) & (w - 1), (e0 + q) >> job.log2_w, e0 + q, r[q]);
            return;
        }
        if (job.store_coeffs) {
            if (PER < 4) {
#pragma unroll
                for (int q = 0; q < PER; q++)
                    if (e0 + q < n)
                        gst<int>(coeffs + e0 + q, r[q]);
            } else {
#pragma unroll
                for (int c4 = 0; c4 < PER / 4; c4++)
                    if (e0 + c4 * 4 < n)
                        gst<int4>(coeffs + e0 + c4 * 4, make_int4(r[c4 * 4], r[c4 * 4 + 1], r[c4 * 4 + 2], r[c4 * 4 + 3]));
            }
        }
        if (dst) {
            if (row_io) {
                VVC355_GLOBAL px_t *prow = (VVC355_GLOBAL px_t *)(dst + (ptrdiff_t)(e0 >> job.log2_w) * job.dst_stride) + (e0 & (w - 1));
                px_t outv[PER];
#pragma unroll
                for (int q = 0; q < PER; q++)
                    outv[q] = (px_t)clip_px<BD>((int)pred[q] + r[q]);
#pragma unroll
                for (int q = 0; q < PER; q++)
                    prow[q] = outv[q];
            } else {
#pragma unroll
                for (int q = 0; q < PER; q++) {
                    const int o = e0 + q;
                    if (o < n)
                        st_px<BD>(dst + (ptrdiff_t)(o >> job.log2_w) * job.dst_stride, o & (w - 1), clip_px<BD>((int)pred[q] + r[q]));
                }
            }
        }
    }
}

// NT lanes share one block of at most CAP coefficients (CAP / NT = 4 elements per lane, 16 for 64x64):
//   NT 4 / CAP 16 (4x4), NT 16 / CAP 64 (8x8), NT 64 / CAP 256 (16x16): sub-wave groups, wave-level synchronisation only;
//   NT 256 / CAP 1024 (32x32) and NT 256 / CAP 4096 (64x64): one workgroup per block.
template <int BD, int NT, int CAP, typename... Lv>
__global__ __launch_bounds__(256) void itx_kernel(const vvc355_itx_job *__restrict__ jobs, int n_jobs, Lv... lv)
{
    constexpr bool PACKED = sizeof...(Lv) > 0;       // levels from an LvSrc instead of int32 at job.coeffs
    constexpr int TBS = 256 / NT;                    // blocks per workgroup
    __shared__ __attribute__((aligned(16))) int buf_all[TBS][CAP];
    __shared__ __attribute__((aligned(16))) int tmp_all[TBS][CAP];
    __shared__ int8_t cos_lds[256];
    cos_lds[threadIdx.x] = d_tab_dct2_cos[threadIdx.x];
    __syncthreads();
    const int sub = threadIdx.x / NT, tid = threadIdx.x % NT;
    const int ji = blockIdx.x * TBS + sub;
    if (ji >= n_jobs)
        return;                                      // whole groups leave together
    vvc355_itx_job job = jobs[ji];
    resolve_type(job);
    if (job.log2_w + job.log2_h > __builtin_ctz(CAP))
        return;                                      // larger than this launch's size class: contract violation, skipped
    if constexpr (PACKED) {
        const LvSrc ls = lv_src(lv...);
        const vvc355_tb_levels r = ls.lv[ji];
        itx_generic_block<BD, NT, CAP, true>(job, buf_all[sub], tmp_all[sub], cos_lds, tid, &r, ls.levels);
    } else {
        itx_generic_block<BD, NT, CAP>(job, buf_all[sub], tmp_all[sub], cos_lds, tid);
    }
}

// ------------------------------------------------------------------------------------------------ shape-specialised path
//
// All jobs of a launch share one shape W x H (both 4..64).  With log2_transform_range <= 15 the coefficients the reference
// reads and its clipped first-stage results are 16-bit, so both passes are packed 16-bit dot products (v_dot2_i32_i16, two
// multiply-adds per lane per instruction; the true sums stay far below 2^31, so the reference's wrapping int32 sums are
// reproduced exactly).  A block is cut into 4x4 tiles, one lane per tile in each pass; per 8 inputs a lane reads 4 matrix
// rows and 4 data rows as 16-byte LDS vectors and issues 64 dot products.  LDS images (int16, input index contiguous):
//   cT [x][k]  the coefficients the column pass reads, transposed; rows / columns the nz gating excludes are zero
//   tmp[y][k]  the clipped column-pass output, only the columns the row pass reads
//   tab[type][out][k]  the transform matrices of this shape (generated: itx16_<N> in tables.inc)
// Only the coefficients inside the nz window are fetched from HBM.  A workgroup in which any block is not eligible
// (other shape, range > 15, a coefficient beyond 16 bits) redoes all of its blocks with the generic code above.

template <int N> struct TxDim {
    static constexpr int KV = N < 32 ? N : 32;               // inputs an N-point inverse transform can read
    static constexpr int P = KV + (KV >= 16 ? 8 : 0);        // LDS row pitch (int16): 16-byte aligned rows, staggered banks
    static constexpr int KS = KV < 8 ? 4 : 8;                // inputs per LDS vector
    static constexpr int NTYPE = N <= 32 ? 3 : 1;            // DST-7 / DCT-8 exist up to 32 points
    __device__ static __forceinline__ const int16_t *table()
    {
        return N == 4 ? d_tab_itx16_4 : N == 8 ? d_tab_itx16_8 : N == 16 ? d_tab_itx16_16 : N == 32 ? d_tab_itx16_32 : d_tab_itx16_64;
    }
    // global -> LDS, re-pitched
    __device__ static __forceinline__ void stage(int16_t *lds)
    {
        const int16_t *src = table();
        constexpr int ND = NTYPE * N * KV / 2;
        for (int i = threadIdx.x; i < ND; i += 256) {
            const int row = i / (KV / 2), c2 = i % (KV / 2);
            *(uint32_t *)&lds[row * P + 2 * c2] = gld<uint32_t>(src + 2 * i);
        }
    }
};

template <int KS> __device__ __forceinline__ void lds_row(const int16_t *p, uint32_t (&d)[KS / 2])
{
    if constexpr (KS == 8) {
        const uint4 v = *(const uint4 *)p;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else {
        const uint2 v = *(const uint2 *)p;
        d[0] = v.x; d[1] = v.y;
    }
}

// Four samples of a row of a plane, as loaded (two per dword above 8 bits, four in one dword at 8 bits), and the add that ends the transform
template <int BD> __device__ __forceinline__ uint2 px4_load(const uint8_t *p)
{
    uint2 v = make_uint2(0, 0);
    if (BD > 8) v = gld<uint2>(p);
    else v.x = gld<uint32_t>(p);
    return v;
}
template <int BD> __device__ __forceinline__ void px4_add_store(uint8_t *p, uint2 praw, const int (&res)[4])
{
    if (BD > 8) {
        const int o0 = clip_px<BD>((int)(praw.x & 0xffff) + res[0]), o1 = clip_px<BD>((int)(praw.x >> 16) + res[1]);
        const int o2 = clip_px<BD>((int)(praw.y & 0xffff) + res[2]), o3 = clip_px<BD>((int)(praw.y >> 16) + res[3]);
        gst<uint2>(p, make_uint2((uint32_t)o0 | ((uint32_t)o1 << 16), (uint32_t)o2 | ((uint32_t)o3 << 16)));
    } else {
        const uint32_t pr = praw.x;
        const int o0 = clip_px<BD>((int)(pr & 0xff) + res[0]), o1 = clip_px<BD>((int)((pr >> 8) & 0xff) + res[1]);
        const int o2 = clip_px<BD>((int)((pr >> 16) & 0xff) + res[2]), o3 = clip_px<BD>((int)(pr >> 24) + res[3]);
        gst<uint32_t>(p, (uint32_t)o0 | ((uint32_t)o1 << 8) | ((uint32_t)o2 << 16) | ((uint32_t)o3 << 24));
    }
}

// PACKED: a lane whose tile is coded loads its group (32 bytes, two 16-byte loads; its position is a popcount of the lower mask bits),
// any other lane loads nothing; jobs with VVC355_LEVELS_INT32 read int32 levels as the plain kernel does.
template <int BD, int LW, int LH, typename... Lv>
__global__ __launch_bounds__(256) void itx_shape_kernel(const vvc355_itx_job *__restrict__ jobs, int n_jobs, Lv... lv)
{
    constexpr bool PACKED = sizeof...(Lv) > 0;
#include "itx_shape_body.inc"
}

// vvc355_levels_expand: one wave per job, lanes over the 4-sample row segments of the job's nzw x nzh window.  A segment is 8 bytes of one
// group (slots outside a block narrower than 4 are zero in the stream, and no store reaches past nzw <= w).
__global__ __launch_bounds__(256) void levels_expand_kernel(const vvc355_itx_job *__restrict__ jobs, LvSrc ls, int n_jobs)
{
    const int ji = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (ji >= n_jobs)
        return;
    const vvc355_tb_levels r = ls.lv[ji];
    if (r.flags & VVC355_LEVELS_INT32)
        return;
    const vvc355_itx_job job = jobs[ji];
    int *coeffs = (int *)job.coeffs;
    const int lw = job.log2_w, w = 1 << lw;
    const int nzw = min((int)job.nzw, w), nzh = min((int)job.nzh, 1 << job.log2_h);
    const int sw = (nzw + 3) >> 2;                            // row segments per window row
    for (int u = lane; u < sw * nzh; u += 64) {
        const int y = u / sw, x0 = (u - y * sw) * 4;
        const int16_t *g = lv_group(r, ls.levels, lw, x0, y);
        const int4 v = g ? unpack_i16x4(gld<uint2>(g + (y & 3) * 4)) : make_int4(0, 0, 0, 0);
        int *row = coeffs + y * w + x0;
        gst<int>(row, v.x);
        if (x0 + 1 < nzw) gst<int>(row + 1, v.y);
        if (x0 + 2 < nzw) gst<int>(row + 2, v.z);
        if (x0 + 3 < nzw) gst<int>(row + 3, v.w);
    }
}

// Scaling process for transform coefficients (vvc_intra.c:277-417): 16 lanes per transform block (most blocks are small and
// their non-zero windows smaller still), lanes over the scan rectangle.  levelScale / qp arithmetic per derive_qp (:277) and
// derive_scale (:311).
__global__ __launch_bounds__(256) void dequant_kernel(const vvc355_dequant_job *__restrict__ jobs, int n_jobs)
{
    const int ji = blockIdx.x * 16 + (threadIdx.x >> 4), tid = threadIdx.x & 15;
    if (ji >= n_jobs)
        return;
    const vvc355_dequant_job job = jobs[ji];
    const int lw = job.log2_w;
    Dequant dq;
    dq.setup(1, lw, job.log2_h, job.qp, job.ts, job.dep_quant, job.bit_depth, job.range, (const uint8_t *)job.scale_matrix,
             job.log2_matrix_size, job.dc);
    const int rw = job.max_x - job.min_x + 1, rh = job.max_y - job.min_y + 1;
    int *coeffs = (int *)job.coeffs;
    // lane -> column (tid mod rw') with rw' = rw rounded up to a power of two <= 16, so that no division is needed per element
    const int cw = rw >= 16 ? 16 : rw > 8 ? 16 : rw > 4 ? 8 : rw > 2 ? 4 : rw > 1 ? 2 : 1;    // columns per pass
    const int rows_per_pass = 16 / cw;
    for (int xb = 0; xb < rw; xb += 16) {
        const int xo = xb + (tid & (cw - 1));
        if (xo >= rw)
            continue;
        for (int yo = tid / cw; yo < rh; yo += rows_per_pass) {
            const int y = job.min_y + yo, x = job.min_x + xo;
            const int c = gld<int>(coeffs + (y << lw) + x);
            if (c)
                gst<int>(coeffs + (y << lw) + x, dq.apply(c, x, y));
        }
    }
}

// add_residual / add_residual_joint / pred_residual_joint (vvcdsp_template.c:32,48,65); job.src0 = int residuals,
// mode 0 add, 1 joint add (w0 = c_sign, denom = shift), 2 joint in place on the int buffer (dst unused)
template <int BD>
__global__ __launch_bounds__(256) void residual_kernel(const vvc355_blend_job *__restrict__ jobs)
{
    const vvc355_blend_job job = load_uniform(jobs + (blockIdx.y));
    int *res = (int *)job.src0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < job.w * job.h; i += gridDim.x * blockDim.x) {
        int r = res[i];
        if (job.mode)
            r = (r * job.w0) >> job.denom;
        if (job.mode == 2) {
            res[i] = r;
            continue;
        }
        const int y = i / job.w, x = i - y * job.w;
        uint8_t *row = (uint8_t *)job.dst + (ptrdiff_t)y * job.dst_stride;
        st_px<BD>(row, x, clip_px<BD>(ld_px<BD>(row, x) + r));
    }
}

// transform_bdpcm (:76): one lane per column (vertical) or row; job.dst = int coeffs, mode = vertical, denom = range
__global__ __launch_bounds__(128) void bdpcm_kernel(const vvc355_blend_job *__restrict__ jobs)
{
    const vvc355_blend_job job = load_uniform(jobs + (blockIdx.x));
    int *c = (int *)job.dst;
    const int w = job.w, h = job.h, range = job.denom, t = threadIdx.x;
    if (job.mode) {
        if (t < w)
            for (int y = 1; y < h; y++)
                c[y * w + t] = clip_intp2(c[y * w + t] + c[(y - 1) * w + t], range);
    } else {
        if (t < h)
            for (int x = 1; x < w; x++)
                c[t * w + x] = clip_intp2(c[t * w + x] + c[t * w + x - 1], range);
    }
}

// ff_vvc_inv_lfnst_1d (vvc_itx_1d.c:708): v[j] = clip((sum_i u[i] * M[i][j] + 64) >> 7); one lane per output
__global__ __launch_bounds__(64) void lfnst_kernel(int *v, const int *u, int nz, int n_tr_s, int set, int idx, int range)
{
    const int j = threadIdx.x;
    if (j >= n_tr_s)
        return;
    const int8_t *m = n_tr_s > 16 ? d_tab_lfnst_8x8 + (set * 2 + idx - 1) * 16 * 48 : d_tab_lfnst_4x4 + (set * 2 + idx - 1) * 16 * 16;
    unsigned t = 0;
    for (int i = 0; i < nz; i++)
        t += (unsigned)u[i] * (unsigned)(int)m[i * n_tr_s + j];
    v[j] = clip_intp2(((int)t + 64) >> 7, range);
}

// dequant (when asked) + ilfnst_transform (vvc_intra.c:65-127) of one transform block per wave, in place: the scaling process over
// the whole scan window first (what the reference's dequant leaves, :400-417), then the first 8 / 16 levels in 4x4 diagonal scan
// order through ff_vvc_inv_lfnst_1d, scattered into the top-left 4x4 or the 8x8 L-shape (48 outputs), transposed for modes > 34
__global__ __launch_bounds__(256) void lfnst_batch_kernel(const vvc355_lfnst_job *__restrict__ jobs, int n_jobs)
{
    __shared__ int u_all[4][16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ji = blockIdx.x * 4 + wave;
    if (ji >= n_jobs)
        return;
    const vvc355_lfnst_job job = jobs[ji];
    int *coeffs = (int *)job.coeffs;
    const int lw = job.log2_w, w = 1 << lw, h = 1 << job.log2_h;
    if (job.dequant) {
        Dequant dq;
        dq.setup(1, lw, job.log2_h, job.qp, 0, job.dep_quant, job.bit_depth, job.range, (const uint8_t *)job.scale_matrix, job.log2_matrix_size, job.dc);
        const int rw = job.max_x + 1, n = rw * (job.max_y + 1);
        for (int i = lane; i < n; i += 64) {
            const int y = i / rw, x = i - y * rw;
            const int c = gld<int>(coeffs + (y << lw) + x);
            if (c)
                gst<int>(coeffs + (y << lw) + x, dq.apply(c, x, y));
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the gather below reads what other lanes of this wave stored
        wave_sync();
    }
    const bool big = w >= 8 && h >= 8;
    const int n_out = big ? 48 : 16;
    const int nz = ((w == 8 && h == 8) || (w == 4 && h == 4)) ? 8 : 16;
    // 6.5.2 up-right diagonal scan of a 4x4 block (ff_vvc_diag_scan_x / _y [2][2]), packed one nibble per position
    const unsigned long long sx = kDiag4X, sy = kDiag4Y;
    if (lane < 16)
        u_all[wave][lane] = lane < nz ? gld<int>(coeffs + w * (int)((sy >> (4 * lane)) & 15) + (int)((sx >> (4 * lane)) & 15)) : 0;
    wave_sync();
    if (lane < n_out) {
        const int mode = job.pred_mode_intra;
        const int set = mode < 0 ? 1 : d_tab_lfnst_tr_set_index[mode];
        const int8_t *m = big ? d_tab_lfnst_8x8 + (set * 2 + job.lfnst_idx - 1) * 16 * 48 : d_tab_lfnst_4x4 + (set * 2 + job.lfnst_idx - 1) * 16 * 16;
        unsigned t = 0;
        for (int i = 0; i < nz; i++)
            t += (unsigned)u_all[wave][i] * (unsigned)(int)m[i * n_out + lane];
        const int v = clip_intp2(((int)t + 64) >> 7, job.range);
        int x, y;
        const int j = lane;
        if (mode > 34) {            // transposed placement (:86-110)
            if (!big)        { y = j & 3; x = j >> 2; }
            else if (j < 32) { y = j & 7; x = j >> 3; }
            else             { y = (j - 32) & 3; x = 4 + ((j - 32) >> 2); }
        } else {                    // row by row: 8 (4) values in rows 0..3, 4 in rows 4..7 (:111-120)
            if (!big)        { y = j >> 2; x = j & 3; }
            else if (j < 32) { y = j >> 3; x = j & 7; }
            else             { y = 4 + ((j - 32) >> 2); x = (j - 32) & 3; }
        }
        gst<int>(coeffs + y * w + x, v);
    }
}

static bool itx_entry_exists(int trh, int trv, int lw, int lh)
{
    if (lw < 0 || lh < 0 || lw > 6 || lh > 6 || trh < 0 || trh > 2 || trv < 0 || trv > 2 || (lw == 0 && lh == 0))
        return false;
    if (lh == 0) return trv == TX_DCT2 && (lw == 4 || lw == 5 || (lw == 6 && trh == TX_DCT2));
    if (lw == 0) return trh == TX_DCT2 && (lh == 4 || lh == 5 || (lh == 6 && trv == TX_DCT2));
    if (trh != TX_DCT2 && (lw < 2 || lw > 5)) return false;
    if (trv != TX_DCT2 && (lh < 2 || lh > 5)) return false;
    return true;
}

template <int BD, int LW, bool PACKED = false>
static void launch_itx_shape(hipStream_t st, const vvc355_itx_job *jobs_dev, int n_jobs, int log2_h, LvSrc ls = {})
{
#define VVC355_ITX_SHAPE(LH)                                                                                          \
    case LH: {                                                                                                        \
        constexpr int TBS = 256 / ((1 << (LW + LH)) / 16);                                                            \
        if constexpr (PACKED)                                                                                         \
            hipLaunchKernelGGL((itx_shape_kernel<BD, LW, LH, LvSrc>), dim3((n_jobs + TBS - 1) / TBS), dim3(256), 0, st, jobs_dev, n_jobs, ls); \
        else                                                                                                          \
            hipLaunchKernelGGL((itx_shape_kernel<BD, LW, LH>), dim3((n_jobs + TBS - 1) / TBS), dim3(256), 0, st, jobs_dev, n_jobs); \
    } break;
    switch (log2_h) {
    VVC355_ITX_SHAPE(2) VVC355_ITX_SHAPE(3) VVC355_ITX_SHAPE(4) VVC355_ITX_SHAPE(5) VVC355_ITX_SHAPE(6)
    }
#undef VVC355_ITX_SHAPE
}


template <int BD, bool PACKED = false>
static void launch_itx_shape_any(hipStream_t st, const vvc355_itx_job *jobs_dev, int n_jobs, int log2_w, int log2_h, LvSrc ls = {})
{
    switch (log2_w) {
    case 2: launch_itx_shape<BD, 2, PACKED>(st, jobs_dev, n_jobs, log2_h, ls); break;
    case 3: launch_itx_shape<BD, 3, PACKED>(st, jobs_dev, n_jobs, log2_h, ls); break;
    case 4: launch_itx_shape<BD, 4, PACKED>(st, jobs_dev, n_jobs, log2_h, ls); break;
    case 5: launch_itx_shape<BD, 5, PACKED>(st, jobs_dev, n_jobs, log2_h, ls); break;
    case 6: launch_itx_shape<BD, 6, PACKED>(st, jobs_dev, n_jobs, log2_h, ls); break;
    }
}

// one lane per transform block record: the 48-byte job the transform kernels consume (vvc355_itx_frame_build), and the chroma residual job
// where the frame asks for them.  The lane leaves both as rows in LDS; the workgroup's 256 jobs, contiguous in either array, go out through
// lds_rows_to_global.
__global__ __launch_bounds__(256) void itx_build_kernel(const vvc355_itx_frame *__restrict__ fp)
{
    constexpr int WG = 256, JOB_DW = sizeof(vvc355_itx_job) / 4, RES_DW = sizeof(vvc355_lmcs_resid_job) / 4;
    __shared__ uint32_t s_jobs[WG * (JOB_DW + 1)], s_resid[WG * (RES_DW + 1)];
    const vvc355_itx_frame f = load_uniform(fp);
    const int tid = threadIdx.x, first = blockIdx.x * WG, n = min(WG, f.n_tus - first);
    if (tid < n) {
        uint32_t tw[sizeof(vvc355_itx_tu) / 4];
#pragma unroll
        for (int k = 0; k < 4; k++) tw[k] = gld<uint32_t>((const uint32_t *)f.tus + (size_t)(first + tid) * 4 + k);
        vvc355_itx_tu t;
        __builtin_memcpy(&t, tw, sizeof(t));
        vvc355_itx_job j = {};
        j.coeffs = f.coeffs + (uint64_t)t.coeff_off * 4;
        const int c = t.c_idx;
        const uint64_t plane = c == 0 ? f.plane[0] : c == 1 ? f.plane[1] : f.plane[2];
        const int stride = c == 0 ? f.stride[0] : c == 1 ? f.stride[1] : f.stride[2];
        const bool keep = (t.flags & 4) != 0;
        j.dst = keep ? 0 : plane + (uint64_t)t.y0 * stride + ((uint64_t)t.x0 << f.pixel_shift);
        j.dst_stride = stride;
        j.trh = t.tr & 15; j.trv = t.tr >> 4;
        j.log2_w = t.log2_w; j.log2_h = t.log2_h; j.nzw = t.nzw; j.nzh = t.nzh;
        j.range = f.range; j.bd = f.bd;
        j.store_coeffs = keep;
        j.dq_flags = (uint8_t)((t.flags & 1) | (t.flags & 2)); j.dq_qp = t.qp;
        j.log2_matrix_size = 1; j.dc = -1;
        j.mts_flags = (t.flags & 8) ? VVC355_ITX_DERIVE_TYPE : 0; j.tu_flags = f.tu_flags; j.c_idx = t.c_idx;
        lds_row_put<JOB_DW + 1>(s_jobs, tid, j);
        if (f.resid_jobs) {
            vvc355_lmcs_resid_job r = {};
            if (t.flags & 64) {
                r.dst = plane + (uint64_t)t.y0 * stride + ((uint64_t)t.x0 << f.pixel_shift);
                r.resid = j.coeffs; r.luma = f.plane[0];
                r.dst_stride = stride; r.luma_stride = f.stride[0];
                r.w = (int16_t)(1 << t.log2_w); r.h = (int16_t)(1 << t.log2_h);
                r.x_vpdu = (int16_t)((t.x0 << (c ? f.hs : 0)) & ~(f.size_y - 1)); r.y_vpdu = (int16_t)((t.y0 << (c ? f.vs : 0)) & ~(f.size_y - 1));
                r.pic_w = (int16_t)f.width; r.pic_h = (int16_t)f.height; r.size_y = f.size_y;
                r.avail_l = (t.flags >> 4) & 1; r.avail_t = (t.flags >> 5) & 1;
                r.joint = 8;
                if (f.scale_table) {          // the unit's entry of vvc355_lmcs_vpdu_scale_pass's table instead of a derivation per block
                    const int ux = (f.width + f.size_y - 1) / f.size_y;
                    r.luma = f.scale_table + (uint64_t)((r.y_vpdu / f.size_y) * ux + r.x_vpdu / f.size_y) * 2;
                    r.joint = 8 | 16;
                }
            }
            lds_row_put<RES_DW + 1>(s_resid, tid, r);
        }
    }
    __syncthreads();
    lds_rows_to_global<JOB_DW, JOB_DW + 1>(s_jobs, (vvc355_itx_job *)f.jobs + first, n);
    if (f.resid_jobs)
        lds_rows_to_global<RES_DW, RES_DW + 1>(s_resid, (vvc355_lmcs_resid_job *)f.resid_jobs + first, n);
}

// ------------------------------------------------------------------------------------------------ intra transform stage from records
//
// vvc355_intra_tb_pass: a group of NT lanes turns one 16-byte vvc355_intra_tu into the job itx_generic_block consumes, in registers (what
// itx_build_kernel writes to memory for the inter path), and runs scaling + LFNST + transform on it.  The residual stays in the arena
// (dst = 0), so the pixel type of the add path plays no part and the kernels are not specialised by bit depth: the block template is
// entered with BD = 10 and job.bd = the frame's.
// Records [first, end) of one area class, `wg` = workgroup index inside the class; buf / tmp: 256 / NT blocks of CAP ints each.
template <int NT, int CAP, bool PACKED>
__device__ __forceinline__ void intra_tb_group(const vvc355_intra_tb_frame &f, int first, int end, int wg, int *buf, int *tmp,
                                               const int8_t *cos_lds)
{
    constexpr int TBS = 256 / NT;                    // blocks per workgroup
    const int sub = threadIdx.x / NT, tid = threadIdx.x % NT;
    const int i = first + wg * TBS + sub;
    if (i >= end)
        return;                                      // whole groups leave together
    const vvc355_intra_tu t = ((const vvc355_intra_tu *)f.tus)[i];
    const int lw = t.log2_w, lh = t.log2_h;
    const bool lfnst = t.flags & VVC355_INTRA_TU_LFNST;
    // contract violations are skipped, never executed: the area bounds the LDS tile and the arena slot, 4 coefficients are the unit of the
    // vector loads, 64 the largest transform, and LFNST reads a 4x4 corner and a table row picked by lfnst_idx / pred_mode_intra
    if (lw + lh > __builtin_ctz(CAP) || lw + lh < 2 || lw > 6 || lh > 6 || (t.flags & ~(VVC355_INTRA_TU_DEP_QUANT | VVC355_INTRA_TU_LFNST)))
        return;
    if (lfnst && (lw < 2 || lh < 2 || t.lfnst_idx < 1 || t.lfnst_idx > 2 || t.pred_mode_intra > 94))
        return;
    vvc355_itx_job job = {};
    job.coeffs = f.coeffs + (uint64_t)t.coeff_off * 4;
    job.log2_w = t.log2_w; job.log2_h = t.log2_h;
    job.nzw = (uint8_t)min((int)t.nzw, 1 << lw); job.nzh = (uint8_t)min((int)t.nzh, 1 << lh);
    job.range = f.range; job.bd = f.bd;
    job.store_coeffs = 1;
    job.dq_flags = (uint8_t)(1 | ((t.flags & VVC355_INTRA_TU_DEP_QUANT) << 1)); job.dq_qp = t.qp;
    job.log2_matrix_size = 1; job.dc = -1;
    job.mts_flags = VVC355_ITX_DERIVE_TYPE; job.tu_flags = t.tu_flags; job.mts_idx = t.mts_idx; job.lfnst_idx = t.lfnst_idx; job.c_idx = t.c_idx;
    resolve_type(job);
    if constexpr (PACKED) {
        const vvc355_tb_levels r = ((const vvc355_tb_levels *)f.lv)[i];
        itx_generic_block<10, NT, CAP, true, true>(job, buf + sub * CAP, tmp + sub * CAP, cos_lds, tid, &r, (const int16_t *)f.levels,
                                                   lfnst ? t.lfnst_idx : 0, t.pred_mode_intra);
    } else {
        itx_generic_block<10, NT, CAP, false, true>(job, buf + sub * CAP, tmp + sub * CAP, cos_lds, tid, nullptr, nullptr,
                                                    lfnst ? t.lfnst_idx : 0, t.pred_mode_intra);
    }
}

// one area class per launch (launch_mode 1, and the 64x64 class of either mode)
template <int NT, int CAP, bool PACKED>
__global__ __launch_bounds__(256) void intra_tb_kernel(const vvc355_intra_tb_frame *__restrict__ fp, int first, int end)
{
    constexpr int TBS = 256 / NT;
    __shared__ __attribute__((aligned(16))) int buf_all[TBS * CAP];
    __shared__ __attribute__((aligned(16))) int tmp_all[TBS * CAP];
    __shared__ int8_t cos_lds[256];
    cos_lds[threadIdx.x] = d_tab_dct2_cos[threadIdx.x];
    __syncthreads();
    const vvc355_intra_tb_frame f = load_uniform(fp);
    intra_tb_group<NT, CAP, PACKED>(f, first, end, blockIdx.x, buf_all, tmp_all, cos_lds);
}

// classes 0..3 in one grid (launch_mode 2): class 0 owns the workgroups below wg_first[0], class k those in [wg_first[k - 1], wg_first[k]);
// the host computes the four offsets from the class counts.  Every class fills the same 2 x 1024 ints of LDS, with 64 / 16 / 4 / 1 blocks
struct IntraTbGrid {
    int wg_first[4];                                 // first workgroup of classes 1, 2, 3 and the end of class 3 (= the grid)
};
template <bool PACKED>
__global__ __launch_bounds__(256) void intra_tb_merged_kernel(const vvc355_intra_tb_frame *__restrict__ fp, IntraTbGrid g)
{
    __shared__ __attribute__((aligned(16))) int buf_all[1024];
    __shared__ __attribute__((aligned(16))) int tmp_all[1024];
    __shared__ int8_t cos_lds[256];
    cos_lds[threadIdx.x] = d_tab_dct2_cos[threadIdx.x];
    __syncthreads();
    const vvc355_intra_tb_frame f = load_uniform(fp);
    const int b = blockIdx.x;
    if (b < g.wg_first[0])
        intra_tb_group<4, 16, PACKED>(f, f.class_first[0], f.class_first[1], b, buf_all, tmp_all, cos_lds);
    else if (b < g.wg_first[1])
        intra_tb_group<16, 64, PACKED>(f, f.class_first[1], f.class_first[2], b - g.wg_first[0], buf_all, tmp_all, cos_lds);
    else if (b < g.wg_first[2])
        intra_tb_group<64, 256, PACKED>(f, f.class_first[2], f.class_first[3], b - g.wg_first[1], buf_all, tmp_all, cos_lds);
    else if (b < g.wg_first[3])
        intra_tb_group<256, 1024, PACKED>(f, f.class_first[3], f.class_first[4], b - g.wg_first[2], buf_all, tmp_all, cos_lds);
}

// which launch shape launch_mode 0 takes: the faster one on the bench's 8K picture (tools/intra_tb_time.py measures both)
static constexpr int kIntraTbDefaultMode = 2;

template <bool PACKED>
static void launch_intra_tb(hipStream_t st, const vvc355_intra_tb_frame *fd, const vvc355_intra_tb_frame &fh, int mode)
{
    const int32_t *cf = fh.class_first;
    int wgs[5];
    for (int k = 0; k < 5; k++) {
        const int cnt = cf[k + 1] - cf[k], tbs = k == 0 ? 64 : k == 1 ? 16 : k == 2 ? 4 : 1;
        wgs[k] = (cnt + tbs - 1) / tbs;
    }
    if (mode == 2) {
        IntraTbGrid g;
        int total = 0;
        for (int k = 0; k < 4; k++)
            g.wg_first[k] = total += wgs[k];
        if (total)
            hipLaunchKernelGGL((intra_tb_merged_kernel<PACKED>), dim3(total), dim3(256), 0, st, fd, g);
    } else {
        if (wgs[0]) hipLaunchKernelGGL((intra_tb_kernel<4, 16, PACKED>), dim3(wgs[0]), dim3(256), 0, st, fd, cf[0], cf[1]);
        if (wgs[1]) hipLaunchKernelGGL((intra_tb_kernel<16, 64, PACKED>), dim3(wgs[1]), dim3(256), 0, st, fd, cf[1], cf[2]);
        if (wgs[2]) hipLaunchKernelGGL((intra_tb_kernel<64, 256, PACKED>), dim3(wgs[2]), dim3(256), 0, st, fd, cf[2], cf[3]);
        if (wgs[3]) hipLaunchKernelGGL((intra_tb_kernel<256, 1024, PACKED>), dim3(wgs[3]), dim3(256), 0, st, fd, cf[3], cf[4]);
    }
    if (wgs[4]) hipLaunchKernelGGL((intra_tb_kernel<256, 4096, PACKED>), dim3(wgs[4]), dim3(256), 0, st, fd, cf[4], cf[5]);
}

// ------------------------------------------------------------------------------------------------ inter transform stage from records
//
// vvc355_inter_tb_pass: the records of one shape bin go through the shape-specialised body (itx_shape_body.inc), the job made in registers
// from the 16-byte vvc355_inter_tu (what itx_build_kernel writes to memory), the residual added from the registers the row pass leaves
// it in: plain, through the 64x64 unit's chroma scale, to both chroma planes of a joint transform unit, or stored to the arena (KEEP).
template <int BD> struct InterEpi {
    uint8_t *dst0, *dst1;                            // the block in its own plane; in plane 3 - c_idx for a joint record, else null
    int stride0, stride1;
    int *keep;                                       // the arena slot of a KEEP record, else null
    int joint, scale;
    uint2 p0[4], p1[4];
    static constexpr int PXS = (int)sizeof(typename Px<BD>::type);
    __device__ __forceinline__ void prefetch(bool act, int x0, int y0)
    {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            p0[r] = p1[r] = make_uint2(0, 0);
            if (act && !keep) {
                p0[r] = px4_load<BD>(dst0 + row_off(y0 + r, stride0) + x0 * PXS);
                if (dst1)
                    p1[r] = px4_load<BD>(dst1 + row_off(y0 + r, stride1) + x0 * PXS);
            }
        }
    }
    template <int W> __device__ __forceinline__ void row(int r, int x0, int y, const int (&res)[4])
    {
        if (keep) {
            gst<int4>(keep + y * W + x0, make_int4(res[0], res[1], res[2], res[3]));
            return;
        }
        int own[4], other[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            own[q] = resid_sample<BD>(res[q], joint & 8, scale);
            other[q] = resid_sample<BD>(res[q], joint, scale);
        }
        px4_add_store<BD>(dst0 + row_off(y, stride0) + x0 * PXS, p0[r], own);
        if (dst1)
            px4_add_store<BD>(dst1 + row_off(y, stride1) + x0 * PXS, p1[r], other);
    }
    // itx_generic_block's hook: thin blocks, and the workgroups that fall back to the generic arithmetic
    __device__ __forceinline__ void sample(int x, int y, int o, int r)
    {
        if (keep) {
            gst<int>(keep + o, r);
            return;
        }
        uint8_t *row0 = dst0 + row_off(y, stride0);
        st_px<BD>(row0, x, clip_px<BD>(ld_px<BD>(row0, x) + resid_sample<BD>(r, joint & 8, scale)));
        if (dst1) {
            uint8_t *row1 = dst1 + row_off(y, stride1);
            st_px<BD>(row1, x, clip_px<BD>(ld_px<BD>(row1, x) + resid_sample<BD>(r, joint, scale)));
        }
    }
};

// what the kernels read of vvc355_inter_tb_frame: everything in front of bin_first (the launches are the host's)
struct InterTbHead {
    uint64_t tus, coeffs, lv, levels, plane[3], scale_table;
    int32_t  stride[3], width, height, n_tus;
    uint8_t  hs, vs, size_y, range, bd, pad_[3];
};
static_assert(sizeof(InterTbHead) == offsetof(vvc355_inter_tb_frame, bin_first) && offsetof(InterTbHead, hs) == offsetof(vvc355_inter_tb_frame, hs) &&
              offsetof(InterTbHead, stride) == offsetof(vvc355_inter_tb_frame, stride), "InterTbHead is the frame without bin_first");

// Records [first, ...) of bin `bin` of channel type `ch`; (lw0, lh0) the bin's shape (what a skipped record's stand-in job gets).
//   get(i, job, epi)        record i as a job (types resolved) and its epilogue; false = the record is skipped (the job is then a harmless one
//                           of the bin's shape: nothing is read or written for it)
//   levels_of(i), stream()  the block's side record (an int32 one when the picture has no packed levels) and the level stream
template <int BD> struct InterTbSrc {
    using Epi = InterEpi<BD>;
    InterTbHead f;
    int first, ch, bin, lw0, lh0;
    __device__ __forceinline__ vvc355_tb_levels levels_of(int i) const
    {
        if (!f.lv)
            return vvc355_tb_levels{ 0, 0, VVC355_LEVELS_INT32 };
        const uint4 v = gld<uint4>((const vvc355_tb_levels *)f.lv + first + i);
        return vvc355_tb_levels{ (uint64_t)v.x | ((uint64_t)v.y << 32), v.z, v.w };
    }
    __device__ __forceinline__ const int16_t *stream() const { return (const int16_t *)f.levels; }
    __device__ __forceinline__ bool get(int i, vvc355_itx_job &job, Epi &epi) const
    {
        vvc355_inter_tu t;
        const uint4 raw = gld<uint4>((const vvc355_inter_tu *)f.tus + first + i);
        __builtin_memcpy(&t, &raw, sizeof(t));
        const int lw = t.log2_w, lh = t.log2_h, c = t.flags & 3, joint = t.joint_mts & 15, mts = (t.joint_mts >> 4) & 7;
        const bool keep = t.flags & VVC355_INTER_TU_KEEP;
        // contract violations are skipped, never executed: the shape bounds the LDS tiles and the arena slot, the rectangle the pixel
        // accesses, 4 elements are the unit of the vector loads, the unit indexes the scale table
        bool ok = lw <= 6 && lh <= 6 && lw + lh >= 2 && ((lw >= 2 && lh >= 2) ? (lw - 2) * 5 + (lh - 2) : 25) == bin;
        ok &= !(t.flags & 0xc0) && !(t.joint_mts & 0x80) && mts <= 4 && c != 3 && (c != 0) == (ch != 0) && !(c == 0 && joint);
        ok &= !((joint & 8) && !f.scale_table);
        const int hs = c ? f.hs : 0, vs = c ? f.vs : 0;
        ok &= t.x0 >= 0 && t.y0 >= 0 && t.x0 + (1 << (lw & 7)) <= (f.width >> hs) && t.y0 + (1 << (lh & 7)) <= (f.height >> vs);
        if (keep || (levels_of(i).flags & VVC355_LEVELS_INT32))
            ok &= !(t.coeff_off & 3);
        int scale = 0;
        if (ok && (joint & 8)) {
            // the unit of (cu->x0, cu->y0): the block's own unit minus the record's two bits
            const int ls = f.size_y == 64 ? 6 : 5;
            const int ux = ((t.x0 << hs) >> ls) - ((t.flags >> 4) & 1), uy = ((t.y0 << vs) >> ls) - ((t.flags >> 5) & 1);
            ok = ux >= 0 && uy >= 0;
            if (ok)
                scale = (int)gld<int16_t>((const int16_t *)f.scale_table + uy * ((f.width + (1 << ls) - 1) >> ls) + ux);
        }
        job = {};
        job.log2_w = (uint8_t)(ok ? lw : lw0); job.log2_h = (uint8_t)(ok ? lh : lh0);
        job.nzw = job.nzh = 1;
        job.range = f.range; job.bd = f.bd;
        job.log2_matrix_size = 1; job.dc = -1;
        epi.dst0 = epi.dst1 = nullptr;
        epi.keep = nullptr;
        epi.stride0 = epi.stride1 = 0;
        epi.joint = epi.scale = 0;
        if (!ok)
            return false;
        job.coeffs = f.coeffs + (uint64_t)t.coeff_off * 4;
        job.nzw = (uint8_t)min((int)t.nzw, 1 << lw); job.nzh = (uint8_t)min((int)t.nzh, 1 << lh);
        job.dq_flags = (uint8_t)(1 | ((t.flags & VVC355_INTER_TU_DEP_QUANT) ? 2 : 0)); job.dq_qp = t.qp;
        job.mts_flags = VVC355_ITX_DERIVE_TYPE; job.tu_flags = t.tu_flags; job.mts_idx = (uint8_t)mts; job.c_idx = (uint8_t)c;
        resolve_type(job);
        if (((lw < 2 || lw > 5) && job.trh) || ((lh < 2 || lh > 5) && job.trv)) {       // DST-7 / DCT-8 exist for 4..32 points only
            job.trh = job.trv = 0;
            return false;
        }
        // (picked between values, not between members: a conditional of lvalues is a conditional of addresses)
        const uint64_t p0 = f.plane[0], p1 = f.plane[1], p2 = f.plane[2];
        const int s0 = f.stride[0], s1 = f.stride[1], s2 = f.stride[2];
        const uint64_t plane = c == 0 ? p0 : c == 1 ? p1 : p2, other = c == 1 ? p2 : p1;
        const int stride = c == 0 ? s0 : c == 1 ? s1 : s2, ostride = c == 1 ? s2 : s1;
        if (keep) {
            epi.keep = (int *)job.coeffs;
            return true;
        }
        epi.dst0 = (uint8_t *)plane + row_off(t.y0, stride) + t.x0 * Epi::PXS;
        epi.stride0 = stride;
        if (joint & 1) {
            epi.dst1 = (uint8_t *)other + row_off(t.y0, ostride) + t.x0 * Epi::PXS;
            epi.stride1 = ostride;
        }
        epi.joint = joint;
        epi.scale = scale;
        return true;
    }
};

template <int BD, int LW, int LH>
__global__ __launch_bounds__(256) void inter_tb_shape_kernel(const vvc355_inter_tb_frame *__restrict__ fp, int first, int end, int ch)
{
    constexpr bool PACKED = true;                    // a picture without packed levels has int32 side records made up by the source
    const InterTbSrc<BD> src{ load_uniform((const InterTbHead *)fp), first, ch, (LW - 2) * 5 + (LH - 2), LW, LH };
    const int n_jobs = end - first;
#define ITX_SHAPE_RECORDS
#include "itx_shape_body.inc"
#undef ITX_SHAPE_RECORDS
}

// bin 25, blocks with a side of 1 or 2 (at most 128 coefficients): a wave per block through the generic code
template <int BD>
__global__ __launch_bounds__(256) void inter_tb_thin_kernel(const vvc355_inter_tb_frame *__restrict__ fp, int first, int end, int ch)
{
    __shared__ __attribute__((aligned(16))) int buf_all[4 * 256];
    __shared__ __attribute__((aligned(16))) int tmp_all[4 * 256];
    __shared__ int8_t cos_lds[256];
    cos_lds[threadIdx.x] = d_tab_dct2_cos[threadIdx.x];
    __syncthreads();
    const int sub = threadIdx.x >> 6, tid = threadIdx.x & 63;
    const int i = xcd_chunked(blockIdx.x, gridDim.x) * 4 + sub;
    if (i >= end - first)
        return;                                      // whole waves leave together
    const InterTbSrc<BD> src{ load_uniform((const InterTbHead *)fp), first, ch, 25, 1, 1 };
    vvc355_itx_job job;
    InterEpi<BD> epi;
    if (!src.get(i, job, epi))
        return;
    const vvc355_tb_levels r = src.levels_of(i);
    itx_generic_block<BD, 64, 256, true, false, InterEpi<BD>>(job, buf_all + sub * 256, tmp_all + sub * 256, cos_lds, tid, &r, src.stream(), 0, 0, &epi);
}

template <int BD, int LW>
static void launch_inter_tb_shape(hipStream_t st, const vvc355_inter_tb_frame *fd, int first, int end, int ch, int log2_h)
{
#define VVC355_INTER_TB_SHAPE(LH)                                                                                     \
    case LH: {                                                                                                        \
        constexpr int TBS = 256 / ((1 << (LW + LH)) / 16);                                                            \
        hipLaunchKernelGGL((inter_tb_shape_kernel<BD, LW, LH>), dim3((end - first + TBS - 1) / TBS), dim3(256), 0, st, fd, first, end, ch); \
    } break;
    switch (log2_h) {
    VVC355_INTER_TB_SHAPE(2) VVC355_INTER_TB_SHAPE(3) VVC355_INTER_TB_SHAPE(4) VVC355_INTER_TB_SHAPE(5) VVC355_INTER_TB_SHAPE(6)
    }
#undef VVC355_INTER_TB_SHAPE
}

// one launch per non-empty bin of the requested channel types
template <int BD>
static void launch_inter_tb(hipStream_t st, const vvc355_inter_tb_frame *fd, const vvc355_inter_tb_frame &fh, int channels)
{
    for (int ch = 0; ch < 2; ch++) {
        if (!(channels & (1 << ch)))
            continue;
        for (int bin = 0; bin < VVC355_INTER_TB_BINS; bin++) {
            const int first = fh.bin_first[ch][bin], end = fh.bin_first[ch][bin + 1];
            if (end <= first)
                continue;
            if (bin == 25) {
                hipLaunchKernelGGL((inter_tb_thin_kernel<BD>), dim3((end - first + 3) / 4), dim3(256), 0, st, fd, first, end, ch);
                continue;
            }
            switch (bin / 5 + 2) {
            case 2: launch_inter_tb_shape<BD, 2>(st, fd, first, end, ch, bin % 5 + 2); break;
            case 3: launch_inter_tb_shape<BD, 3>(st, fd, first, end, ch, bin % 5 + 2); break;
            case 4: launch_inter_tb_shape<BD, 4>(st, fd, first, end, ch, bin % 5 + 2); break;
            case 5: launch_inter_tb_shape<BD, 5>(st, fd, first, end, ch, bin % 5 + 2); break;
            case 6: launch_inter_tb_shape<BD, 6>(st, fd, first, end, ch, bin % 5 + 2); break;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ transform-skip blocks from records
//
// vvc355_ts_tb_pass: what itransform does for a block with tb->ts (vvc_intra.c:455-475) — transform_bdpcm on the levels, the scaling
// process with ts = 1, no transform, the tail — from one 16-byte vvc355_ts_tu.  A lane owns one 4x4 tile of its block (the unit of the
// packed level stream, bit `tile` of the side record's mask) in 16 registers; NT lanes, one per tile of the largest block of the area
// class, form a group inside one wave.  Nothing is staged in LDS and no job array exists.

// what the kernel reads of vvc355_ts_tb_frame: everything in front of class_first (the grid is the host's)
struct TsTbHead {
    uint64_t tus, coeffs, lv, levels, plane[3], scale_table;
    int32_t  stride[3], width, height, n_tus;
    uint8_t  hs, vs, size_y, range, bd, pad_[3];
};
static_assert(sizeof(TsTbHead) == offsetof(vvc355_ts_tb_frame, class_first) && offsetof(TsTbHead, hs) == offsetof(vvc355_ts_tb_frame, hs) &&
              offsetof(TsTbHead, stride) == offsetof(vvc355_ts_tb_frame, stride), "TsTbHead is the frame without class_first");

// one channel type's four area classes in one grid: class k owns the workgroups [wg_first[k - 1], wg_first[k]) (class 0 those below
// wg_first[0]) and the records [first[k], first[k + 1])
struct TsTbGrid {
    int wg_first[4];
    int first[5];
};

// transform_bdpcm (vvcdsp_template.c:76) along the second index of v: line l of the tile holds a[0..3], the tile is number `pos` of its
// line of tiles, the tile before it belongs to lane - stride.  Every step is x -> clip(x + a), and steps compose into
// x -> clamp(x + s, lo, hi), so a tile is one such triple and the carry walks the at most MAXP tiles of a line exactly, saturation
// included.  The first sample of a line is taken as it is (the reference starts at the second).
template <int MAXP>
__device__ __forceinline__ void ts_bdpcm_lines(int (&v)[4][4], int pos, int stride, int range)
{
    const int lane = threadIdx.x & 63;
    int s[4], lo[4], hi[4], out[4], cin[4];
#pragma unroll
    for (int l = 0; l < 4; l++) {
        s[l] = out[l] = v[l][0];
        lo[l] = -(1 << range); hi[l] = (1 << range) - 1;
        cin[l] = 0;
#pragma unroll
        for (int k = 1; k < 4; k++) {
            s[l] += v[l][k];
            lo[l] = clip_intp2(lo[l] + v[l][k], range); hi[l] = clip_intp2(hi[l] + v[l][k], range);
            out[l] = clip_intp2(out[l] + v[l][k], range);       // the line's last sample when the tile is its first
        }
    }
#pragma unroll
    for (int p = 1; p < MAXP; p++) {
#pragma unroll
        for (int l = 0; l < 4; l++) {
            const int prev = __shfl(out[l], lane - stride);
            if (pos == p) {
                cin[l] = prev;
                out[l] = clip3(prev + s[l], lo[l], hi[l]);
            }
        }
    }
#pragma unroll
    for (int l = 0; l < 4; l++) {
        int x = pos ? clip_intp2(cin[l] + v[l][0], range) : v[l][0];
        v[l][0] = x;
#pragma unroll
        for (int k = 1; k < 4; k++)
            v[l][k] = x = clip_intp2(x + v[l][k], range);
    }
}

__device__ __forceinline__ void ts_transpose(int (&v)[4][4])
{
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int q = r + 1; q < 4; q++) {
            const int a = v[r][q];
            v[r][q] = v[q][r];
            v[q][r] = a;
        }
}

// Record wg * (256 / NT) + threadIdx.x / NT of [first, end), an area class of at most 1 << CAPLOG2 samples, of channel type ch.
template <int BD, int NT, int CAPLOG2>
__device__ __forceinline__ void ts_tb_group(const TsTbHead &f, int first, int end, int wg, int ch)
{
    constexpr int PXS = (int)sizeof(typename Px<BD>::type);
    constexpr int MAXP = NT < 8 ? NT : 8;            // tiles along a side: a side is at most 32
    const int tile = threadIdx.x % NT;
    const int i = first + wg * (256 / NT) + threadIdx.x / NT;
    if (i >= end)
        return;                                      // whole groups leave together
    vvc355_ts_tu t;
    const uint4 raw = gld<uint4>((const vvc355_ts_tu *)f.tus + i);
    __builtin_memcpy(&t, &raw, sizeof(t));
    vvc355_tb_levels r = { 0, 0, VVC355_LEVELS_INT32 };
    if (f.lv) {
        const uint4 q = gld<uint4>((const vvc355_tb_levels *)f.lv + i);
        r = vvc355_tb_levels{ (uint64_t)q.x | ((uint64_t)q.y << 32), q.z, q.w };
    }
    const bool packed = !(r.flags & VVC355_LEVELS_INT32);
    const int lw = t.log2_w, lh = t.log2_h, c = t.flags & 3, joint = t.joint & 15;
    const bool keep = t.flags & VVC355_TS_TU_KEEP;
    // contract violations are skipped, never executed: the area bounds the group's tiles and the arena slot, the rectangle the pixel
    // accesses, 4 elements are the unit of the vector accesses, the unit indexes the scale table
    bool ok = lw >= 1 && lw <= 5 && lh >= 1 && lh <= 5 && lw + lh >= 3 && lw + lh <= CAPLOG2;
    ok &= !(t.flags & 0x80) && !(t.joint & 0xf0) && !t.pad_ && c != 3 && (c != 0) == (ch != 0) && !(c == 0 && joint);
    ok &= !((joint & 8) && !f.scale_table);
    const int hs = c ? f.hs : 0, vs = c ? f.vs : 0;
    ok &= t.x0 >= 0 && t.y0 >= 0 && t.x0 + (1 << (lw & 7)) <= (f.width >> hs) && t.y0 + (1 << (lh & 7)) <= (f.height >> vs);
    if (keep || !packed)
        ok &= !(t.coeff_off & 3);
    int scale = 0;
    if (ok && (joint & 8)) {
        // the unit of (cu->x0, cu->y0): the block's own unit minus the record's two bits
        const int ls = f.size_y == 64 ? 6 : 5;
        const int ux = ((t.x0 << hs) >> ls) - ((t.flags >> 4) & 1), uy = ((t.y0 << vs) >> ls) - ((t.flags >> 5) & 1);
        ok = ux >= 0 && uy >= 0;
        if (ok)
            scale = (int)gld<int16_t>((const int16_t *)f.scale_table + uy * ((f.width + (1 << ls) - 1) >> ls) + ux);
    }
    if (!ok)
        return;

    const int w = 1 << lw, h = 1 << lh, ltw = max(lw - 2, 0), tw = 1 << ltw, th = 1 << max(lh - 2, 0);
    const int gx = tile & (tw - 1), gy = tile >> ltw, x0 = gx * 4, y0 = gy * 4;
    const bool act = tile < tw * th;                 // idle lanes stay for the shuffles of the scan
    const int rows = act ? min(4, h - y0) : 0;       // of the tile inside the block; its columns: 4, or 2 when w is 2

    // (picked between values, not between members: a conditional of lvalues is a conditional of addresses)
    const uint64_t pl0 = f.plane[0], pl1 = f.plane[1], pl2 = f.plane[2];
    const int s0 = f.stride[0], s1 = f.stride[1], s2 = f.stride[2];
    const int stride = c == 0 ? s0 : c == 1 ? s1 : s2, ostride = c == 1 ? s2 : s1;
    uint8_t *dst0 = (uint8_t *)(c == 0 ? pl0 : c == 1 ? pl1 : pl2) + row_off(t.y0 + y0, stride) + (t.x0 + x0) * PXS;
    uint8_t *dst1 = (joint & 1) ? (uint8_t *)(c == 1 ? pl2 : pl1) + row_off(t.y0 + y0, ostride) + (t.x0 + x0) * PXS : nullptr;
    int *slot = (int *)f.coeffs + t.coeff_off;
    // the samples the residual is added to are requested in front of the levels: one memory round trip on the critical path
    uint2 p0[4], p1[4];
#pragma unroll
    for (int y = 0; y < 4; y++) {
        p0[y] = p1[y] = make_uint2(0, 0);
        if (!keep && y < rows && w >= 4) {
            p0[y] = px4_load<BD>(dst0 + row_off(y, stride));
            if (dst1)
                p1[y] = px4_load<BD>(dst1 + row_off(y, ostride));
        }
    }

    // levels: the lane's group of the packed stream (two 16-byte loads; a tile whose bit is clear loads nothing), or the int32 rows of its
    // tile; nothing outside the nzw x nzh window is read
    const int nzw = min((int)t.nzw, w), nzh = min((int)t.nzh, h);
    int v[4][4];
#pragma unroll
    for (int y = 0; y < 4; y++)
#pragma unroll
        for (int x = 0; x < 4; x++)
            v[y][x] = 0;
    if (act && x0 < nzw && y0 < nzh) {
        if (packed) {
            if ((r.groups >> tile) & 1) {
                const int16_t *g = (const int16_t *)f.levels + ((size_t)r.first + __popcll(r.groups & ((1ull << tile) - 1))) * 16;
                const uint4 a = gld<uint4>(g), b = gld<uint4>(g + 8);
                const int4 r0 = unpack_i16x4(make_uint2(a.x, a.y)), r1 = unpack_i16x4(make_uint2(a.z, a.w));
                const int4 r2 = unpack_i16x4(make_uint2(b.x, b.y)), r3 = unpack_i16x4(make_uint2(b.z, b.w));
                v[0][0] = r0.x; v[0][1] = r0.y; v[0][2] = r0.z; v[0][3] = r0.w;
                v[1][0] = r1.x; v[1][1] = r1.y; v[1][2] = r1.z; v[1][3] = r1.w;
                v[2][0] = r2.x; v[2][1] = r2.y; v[2][2] = r2.z; v[2][3] = r2.w;
                v[3][0] = r3.x; v[3][1] = r3.y; v[3][2] = r3.z; v[3][3] = r3.w;
            }
        } else {
#pragma unroll
            for (int y = 0; y < 4; y++)
                if (y < rows && y0 + y < nzh) {
                    if (w >= 4) {
                        const int4 q = gld<int4>(slot + ((y0 + y) << lw) + x0);
                        v[y][0] = q.x; v[y][1] = q.y; v[y][2] = q.z; v[y][3] = q.w;
                    } else {
                        const int2 q = gld<int2>(slot + (y0 + y) * 2);
                        v[y][0] = q.x; v[y][1] = q.y;
                    }
                }
        }
#pragma unroll
        for (int y = 0; y < 4; y++)
#pragma unroll
            for (int x = 0; x < 4; x++)
                if (x0 + x >= nzw || y0 + y >= nzh)
                    v[y][x] = 0;
    }

    if (t.flags & VVC355_TS_TU_BDPCM) {
        const bool vert = t.flags & VVC355_TS_TU_VERTICAL;
        if (vert)
            ts_transpose(v);
        ts_bdpcm_lines<MAXP>(v, vert ? gy : gx, vert ? tw : 1, f.range);
        if (vert)
            ts_transpose(v);
    }

    // the scaling process with ts = 1 (bd_shift 10, flat matrix): Dequant::apply's arithmetic, wrap included — after BDPCM a value can be
    // -2^(range - 1) with range 20, outside the domain of apply_small
    Dequant dq;
    dq.setup(1, lw, lh, t.qp, 1, 0, BD, f.range, nullptr, 1, -1);
#pragma unroll
    for (int y = 0; y < 4; y++)
#pragma unroll
        for (int x = 0; x < 4; x++)
            v[y][x] = dq.apply(v[y][x], 0, 0);

#pragma unroll
    for (int y = 0; y < 4; y++) {
        if (y >= rows)
            continue;
        if (keep) {                                  // the whole w x h residual: BDPCM fills the block beyond the level window
            if (w >= 4)
                gst<int4>(slot + ((y0 + y) << lw) + x0, make_int4(v[y][0], v[y][1], v[y][2], v[y][3]));
            else
                gst<int2>(slot + (y0 + y) * 2, make_int2(v[y][0], v[y][1]));
            continue;
        }
        int own[4], other[4];
#pragma unroll
        for (int x = 0; x < 4; x++) {
            own[x] = resid_sample<BD>(v[y][x], joint & 8, scale);
            other[x] = resid_sample<BD>(v[y][x], joint, scale);
        }
        uint8_t *row0 = dst0 + row_off(y, stride), *row1 = dst1 + row_off(y, ostride);
        if (w >= 4) {
            px4_add_store<BD>(row0, p0[y], own);
            if (dst1)
                px4_add_store<BD>(row1, p1[y], other);
        } else {
#pragma unroll
            for (int x = 0; x < 2; x++) {
                st_px<BD>(row0, x, clip_px<BD>(ld_px<BD>(row0, x) + own[x]));
                if (dst1)
                    st_px<BD>(row1, x, clip_px<BD>(ld_px<BD>(row1, x) + other[x]));
            }
        }
    }
}

template <int BD>
__global__ __launch_bounds__(256) void ts_tb_kernel(const vvc355_ts_tb_frame *__restrict__ fp, TsTbGrid g, int ch)
{
    const TsTbHead f = load_uniform((const TsTbHead *)fp);
    const int b = blockIdx.x;
    if (b < g.wg_first[0])
        ts_tb_group<BD, 2, 4>(f, g.first[0], g.first[1], b, ch);
    else if (b < g.wg_first[1])
        ts_tb_group<BD, 8, 6>(f, g.first[1], g.first[2], b - g.wg_first[0], ch);
    else if (b < g.wg_first[2])
        ts_tb_group<BD, 16, 8>(f, g.first[2], g.first[3], b - g.wg_first[1], ch);
    else if (b < g.wg_first[3])
        ts_tb_group<BD, 64, 10>(f, g.first[3], g.first[4], b - g.wg_first[2], ch);
}

// one launch per requested channel type, its four classes in one grid
template <int BD>
static void launch_ts_tb(hipStream_t st, const vvc355_ts_tb_frame *fd, const vvc355_ts_tb_frame &fh, int channels)
{
    static const int kLanes[4] = { 2, 8, 16, 64 };
    for (int ch = 0; ch < 2; ch++) {
        if (!(channels & (1 << ch)))
            continue;
        TsTbGrid g;
        int total = 0;
        for (int k = 0; k < 4; k++) {
            const int cnt = fh.class_first[ch][k + 1] - fh.class_first[ch][k], tbs = 256 / kLanes[k];
            g.wg_first[k] = total += (cnt + tbs - 1) / tbs;
        }
        for (int k = 0; k < 5; k++)
            g.first[k] = fh.class_first[ch][k];
        if (total)
            hipLaunchKernelGGL((ts_tb_kernel<BD>), dim3(total), dim3(256), 0, st, fd, g, ch);
    }
}

} // namespace vvc355

// The host checks of the three TB record passes, as the header states them (also run by vvc355_picture_pass for the whole picture)
int vvc355::intra_tb_check(const vvc355_intra_tb_frame *frame_host)
{
    if (!frame_host || frame_host->n_tus < 0 || frame_host->class_first[0] != 0 || frame_host->class_first[5] != frame_host->n_tus)
        return VVC355_INTRA_TB_E_CLASS;
    for (int k = 0; k < 5; k++)
        if (frame_host->class_first[k] > frame_host->class_first[k + 1])
            return VVC355_INTRA_TB_E_CLASS;
    if (frame_host->bd != 8 && frame_host->bd != 10 && frame_host->bd != 12)
        return VVC355_INTRA_TB_E_BD;
    if (frame_host->range < 15 || frame_host->range > 20)
        return VVC355_INTRA_TB_E_RANGE;
    if (!frame_host->lv != !frame_host->levels)
        return VVC355_INTRA_TB_E_LEVELS;
    if (frame_host->launch_mode > 2)
        return VVC355_INTRA_TB_E_MODE;
    return 0;
}

int vvc355::inter_tb_check(const vvc355_inter_tb_frame *f, int channels)
{
    if (!f || f->n_tus < 0 || f->bin_first[0][0] != 0 || f->bin_first[0][VVC355_INTER_TB_BINS] != f->bin_first[1][0] ||
        f->bin_first[1][VVC355_INTER_TB_BINS] != f->n_tus)
        return VVC355_INTER_TB_E_BINS;
    for (int ch = 0; ch < 2; ch++)
        for (int k = 0; k < VVC355_INTER_TB_BINS; k++)
            if (f->bin_first[ch][k] > f->bin_first[ch][k + 1])
                return VVC355_INTER_TB_E_BINS;
    if (f->bd != 8 && f->bd != 10 && f->bd != 12)
        return VVC355_INTER_TB_E_BD;
    if (f->range < 15 || f->range > 20)
        return VVC355_INTER_TB_E_RANGE;
    if (!f->lv != !f->levels)
        return VVC355_INTER_TB_E_LEVELS;
    if (f->scale_table && f->size_y != 32 && f->size_y != 64)
        return VVC355_INTER_TB_E_SIZE_Y;
    if (f->hs > 1 || f->vs > 1)
        return VVC355_INTER_TB_E_SHIFT;
    if (channels < 1 || channels > 3)
        return VVC355_INTER_TB_E_CHANNELS;
    if (channels == 3 && f->scale_table)
        return VVC355_INTER_TB_E_ORDER;
    return 0;
}

int vvc355::ts_tb_check(const vvc355_ts_tb_frame *f, int channels)
{
    if (!f || f->n_tus < 0 || f->class_first[0][0] != 0 || f->class_first[0][4] != f->class_first[1][0] || f->class_first[1][4] != f->n_tus)
        return VVC355_TS_TB_E_CLASS;
    for (int ch = 0; ch < 2; ch++)
        for (int k = 0; k < 4; k++)
            if (f->class_first[ch][k] > f->class_first[ch][k + 1])
                return VVC355_TS_TB_E_CLASS;
    if (f->bd != 8 && f->bd != 10 && f->bd != 12)
        return VVC355_TS_TB_E_BD;
    if (f->range < 15 || f->range > 20)
        return VVC355_TS_TB_E_RANGE;
    if (!f->lv != !f->levels)
        return VVC355_TS_TB_E_LEVELS;
    if (f->scale_table && f->size_y != 32 && f->size_y != 64)
        return VVC355_TS_TB_E_SIZE_Y;
    if (f->hs > 1 || f->vs > 1)
        return VVC355_TS_TB_E_SHIFT;
    if (channels < 1 || channels > 3)
        return VVC355_TS_TB_E_CHANNELS;
    if (channels == 3 && f->scale_table)
        return VVC355_TS_TB_E_ORDER;
    return 0;
}

using namespace vvc355;

extern "C" {
extern const uint8_t vvc355_tab_lfnst_tr_set_index[95];

void vvc355_itx_batch(void *stream, int bd, const vvc355_itx_job *jobs_dev, int n_jobs, int max_log2_area)
{
    if (n_jobs <= 0) return;
    hipStream_t st = (hipStream_t)stream;
    VVC355_BD_DISPATCH(bd, {
        if (max_log2_area <= 4)       hipLaunchKernelGGL((itx_kernel<BD, 4, 16>), dim3((n_jobs + 63) / 64), dim3(256), 0, st, jobs_dev, n_jobs);
        else if (max_log2_area <= 6)  hipLaunchKernelGGL((itx_kernel<BD, 16, 64>), dim3((n_jobs + 15) / 16), dim3(256), 0, st, jobs_dev, n_jobs);
        else if (max_log2_area <= 8)  hipLaunchKernelGGL((itx_kernel<BD, 64, 256>), dim3((n_jobs + 3) / 4), dim3(256), 0, st, jobs_dev, n_jobs);
        else if (max_log2_area <= 10) hipLaunchKernelGGL((itx_kernel<BD, 256, 1024>), dim3(n_jobs), dim3(256), 0, st, jobs_dev, n_jobs);
        else                          hipLaunchKernelGGL((itx_kernel<BD, 256, 4096>), dim3(n_jobs), dim3(256), 0, st, jobs_dev, n_jobs);
    });
    HIP_CHECK(hipGetLastError());
}

void vvc355_itx_frame_build(void *stream, const vvc355_itx_frame *frame_dev, const vvc355_itx_frame *frame_host)
{
    if (frame_host->n_tus <= 0) return;
    hipLaunchKernelGGL(vvc355::itx_build_kernel, dim3((frame_host->n_tus + 255) / 256), dim3(256), 0, (hipStream_t)stream, frame_dev);
    HIP_CHECK(hipGetLastError());
}

int vvc355_intra_tb_pass(void *stream, const vvc355_intra_tb_frame *frame_dev, const vvc355_intra_tb_frame *frame_host)
{
    // the host copy is checked before any HIP call: a refused frame launches nothing
    const int err = intra_tb_check(frame_host);
    if (err)
        return err;
    if (frame_host->n_tus == 0)
        return 0;
    const int mode = frame_host->launch_mode ? frame_host->launch_mode : kIntraTbDefaultMode;
    if (frame_host->lv)
        launch_intra_tb<true>((hipStream_t)stream, frame_dev, *frame_host, mode);
    else
        launch_intra_tb<false>((hipStream_t)stream, frame_dev, *frame_host, mode);
    HIP_CHECK(hipGetLastError());
    return 0;
}

int vvc355_inter_tb_pass(void *stream, const vvc355_inter_tb_frame *frame_dev, const vvc355_inter_tb_frame *frame_host, int channels)
{
    // the host copy is checked before any HIP call: a refused frame launches nothing
    const vvc355_inter_tb_frame *f = frame_host;
    const int err = inter_tb_check(f, channels);
    if (err)
        return err;
    if (f->n_tus == 0)
        return 0;
    VVC355_BD_DISPATCH(f->bd, launch_inter_tb<BD>((hipStream_t)stream, frame_dev, *f, channels));
    HIP_CHECK(hipGetLastError());
    return 0;
}

int vvc355_ts_tb_pass(void *stream, const vvc355_ts_tb_frame *frame_dev, const vvc355_ts_tb_frame *frame_host, int channels)
{
    // the host copy is checked before any HIP call: a refused frame launches nothing
    const vvc355_ts_tb_frame *f = frame_host;
    const int err = ts_tb_check(f, channels);
    if (err)
        return err;
    if (f->n_tus == 0)
        return 0;
    VVC355_BD_DISPATCH(f->bd, launch_ts_tb<BD>((hipStream_t)stream, frame_dev, *f, channels));
    HIP_CHECK(hipGetLastError());
    return 0;
}

void vvc355_itx_shape_batch(void *stream, int bd, const vvc355_itx_job *jobs_dev, int n_jobs, int log2_w, int log2_h)
{
    if (n_jobs <= 0) return;
    if (log2_w < 2 || log2_w > 6 || log2_h < 2 || log2_h > 6) {
        vvc355_itx_batch(stream, bd, jobs_dev, n_jobs, log2_w + log2_h);
        return;
    }
    hipStream_t st = (hipStream_t)stream;
    VVC355_BD_DISPATCH(bd, launch_itx_shape_any<BD>(st, jobs_dev, n_jobs, log2_w, log2_h));
    HIP_CHECK(hipGetLastError());
}

void vvc355_itx_batch_lv(void *stream, int bd, const vvc355_itx_job *jobs_dev, const vvc355_tb_levels *lv_dev, const int16_t *levels_dev,
                         int n_jobs, int max_log2_area)
{
    if (n_jobs <= 0) return;
    hipStream_t st = (hipStream_t)stream;
    const LvSrc ls = { lv_dev, levels_dev };
    VVC355_BD_DISPATCH(bd, {
        if (max_log2_area <= 4)       hipLaunchKernelGGL((itx_kernel<BD, 4, 16, LvSrc>), dim3((n_jobs + 63) / 64), dim3(256), 0, st, jobs_dev, n_jobs, ls);
        else if (max_log2_area <= 6)  hipLaunchKernelGGL((itx_kernel<BD, 16, 64, LvSrc>), dim3((n_jobs + 15) / 16), dim3(256), 0, st, jobs_dev, n_jobs, ls);
        else if (max_log2_area <= 8)  hipLaunchKernelGGL((itx_kernel<BD, 64, 256, LvSrc>), dim3((n_jobs + 3) / 4), dim3(256), 0, st, jobs_dev, n_jobs, ls);
        else if (max_log2_area <= 10) hipLaunchKernelGGL((itx_kernel<BD, 256, 1024, LvSrc>), dim3(n_jobs), dim3(256), 0, st, jobs_dev, n_jobs, ls);
        else                          hipLaunchKernelGGL((itx_kernel<BD, 256, 4096, LvSrc>), dim3(n_jobs), dim3(256), 0, st, jobs_dev, n_jobs, ls);
    });
    HIP_CHECK(hipGetLastError());
}

void vvc355_itx_shape_batch_lv(void *stream, int bd, const vvc355_itx_job *jobs_dev, const vvc355_tb_levels *lv_dev, const int16_t *levels_dev,
                               int n_jobs, int log2_w, int log2_h)
{
    if (n_jobs <= 0) return;
    if (log2_w < 2 || log2_w > 6 || log2_h < 2 || log2_h > 6) {
        vvc355_itx_batch_lv(stream, bd, jobs_dev, lv_dev, levels_dev, n_jobs, log2_w + log2_h);
        return;
    }
    hipStream_t st = (hipStream_t)stream;
    VVC355_BD_DISPATCH(bd, (launch_itx_shape_any<BD, true>(st, jobs_dev, n_jobs, log2_w, log2_h, LvSrc{ lv_dev, levels_dev })));
    HIP_CHECK(hipGetLastError());
}

void vvc355_levels_expand(void *stream, const vvc355_itx_job *jobs_dev, const vvc355_tb_levels *lv_dev, const int16_t *levels_dev, int n_jobs)
{
    if (n_jobs <= 0) return;
    hipLaunchKernelGGL(levels_expand_kernel, dim3((n_jobs + 3) / 4), dim3(256), 0, (hipStream_t)stream, jobs_dev, LvSrc{ lv_dev, levels_dev }, n_jobs);
    HIP_CHECK(hipGetLastError());
}

void vvc355_dequant_batch(void *stream, const vvc355_dequant_job *jobs_dev, int n_jobs)
{
    if (n_jobs <= 0) return;
    hipLaunchKernelGGL(dequant_kernel, dim3((n_jobs + 15) / 16), dim3(256), 0, (hipStream_t)stream, jobs_dev, n_jobs);
    HIP_CHECK(hipGetLastError());
}

void vvc355_dequant(int *coeffs, int log2_w, int log2_h, int min_x, int min_y, int max_x, int max_y, int qp, int ts,
                    int dep_quant, int bit_depth, int log2_transform_range, const uint8_t *scale_matrix, int log2_matrix_size, int dc)
{
    SlotCall call;
    vvc355_dequant_job job = {};
    job.coeffs = (uint64_t)call.linear(coeffs, (sizeof(int) << (log2_w + log2_h)), true, true);
    if (scale_matrix)
        job.scale_matrix = (uint64_t)call.linear(scale_matrix, (size_t)1 << (2 * log2_matrix_size), true, false);
    job.log2_w = (uint8_t)log2_w; job.log2_h = (uint8_t)log2_h;
    job.min_x = (uint8_t)min_x; job.min_y = (uint8_t)min_y; job.max_x = (uint8_t)max_x; job.max_y = (uint8_t)max_y;
    job.qp = (uint8_t)qp; job.ts = (uint8_t)ts; job.dep_quant = (uint8_t)dep_quant; job.bit_depth = (uint8_t)bit_depth;
    job.range = (uint8_t)log2_transform_range; job.log2_matrix_size = (uint8_t)log2_matrix_size; job.dc = (int16_t)dc;
    vvc355_dequant_batch(call.stream(), call.upload(&job, 1), 1);
}

int vvc355_itx(int trh, int trv, int log2_w, int log2_h, int *coeffs, size_t nzw, size_t nzh,
               intptr_t log2_transform_range, intptr_t bit_depth)
{
    if (!itx_entry_exists(trh, trv, log2_w, log2_h))
        return -1;
    const int n = 1 << (log2_w + log2_h);
    SlotCall call;
    vvc355_itx_job job = {};
    job.coeffs = (uint64_t)call.linear(coeffs, (size_t)n * sizeof(int), true, true);
    job.trh = (uint8_t)trh; job.trv = (uint8_t)trv; job.log2_w = (uint8_t)log2_w; job.log2_h = (uint8_t)log2_h;
    job.nzw = (uint8_t)nzw; job.nzh = (uint8_t)nzh; job.range = (uint8_t)log2_transform_range; job.bd = (uint8_t)bit_depth;
    job.store_coeffs = 1;
    const int kbd = (int)bit_depth == 8 || (int)bit_depth == 10 || (int)bit_depth == 12 ? (int)bit_depth : 10;
    if (log2_w >= 2 && log2_h >= 2)
        vvc355_itx_shape_batch(call.stream(), kbd, call.upload(&job, 1), 1, log2_w, log2_h);
    else
        vvc355_itx_batch(call.stream(), kbd, call.upload(&job, 1), 1, log2_w + log2_h);
    return 0;
}

void vvc355_inv_lfnst_1d(int *v, const int *u, int no_zero_size, int n_tr_s, int pred_mode_intra, int lfnst_idx,
                         int log2_transform_range)
{
    const int set = pred_mode_intra < 0 ? 1 : vvc355_tab_lfnst_tr_set_index[pred_mode_intra];
    SlotCall call;
    int *dv = (int *)call.linear(v, (size_t)n_tr_s * sizeof(int), false, true);
    const int *du = (const int *)call.linear(u, (size_t)no_zero_size * sizeof(int), true, false);
    hipLaunchKernelGGL(lfnst_kernel, dim3(1), dim3(64), 0, call.stream(), dv, du, no_zero_size, n_tr_s, set, lfnst_idx, log2_transform_range);
    HIP_CHECK(hipGetLastError());
}

void vvc355_lfnst_batch(void *stream, const vvc355_lfnst_job *jobs_dev, int n_jobs)
{
    if (n_jobs <= 0) return;
    hipLaunchKernelGGL(lfnst_batch_kernel, dim3((n_jobs + 3) / 4), dim3(256), 0, (hipStream_t)stream, jobs_dev, n_jobs);
    HIP_CHECK(hipGetLastError());
}

int vvc355_ilfnst_transform(int *coeffs, int w, int h, int pred_mode_intra, int lfnst_idx, int log2_transform_range)
{
    SlotCall call;
    vvc355_lfnst_job job = {};
    job.coeffs = (uint64_t)call.linear(coeffs, (size_t)w * h * sizeof(int), true, true);
    int lw = 0, lh = 0;
    while ((1 << lw) < w) lw++;
    while ((1 << lh) < h) lh++;
    job.log2_w = (uint8_t)lw; job.log2_h = (uint8_t)lh; job.range = (uint8_t)log2_transform_range;
    job.pred_mode_intra = (int8_t)pred_mode_intra; job.lfnst_idx = (uint8_t)lfnst_idx;
    vvc355_lfnst_batch(call.stream(), call.upload(&job, 1), 1);
    return (w >= 8 && h >= 8) ? 8 : 4;
}

int vvc355_derive_transform_type(int tu_flags, int mts_idx, int lfnst_idx, int c_idx, int w, int h)
{
    return derive_tr_type(tu_flags, mts_idx, lfnst_idx, c_idx, w, h);
}

static void slot_residual(int bd, int mode, uint8_t *dst, int *res, int width, int height, ptrdiff_t stride, int c_sign, int shift)
{
    if (width <= 0 || height <= 0) return;
    const int px = bd > 8 ? 2 : 1;
    SlotCall call;
    vvc355_blend_job job = {};
    if (mode != 2) {
        const Staged d = call.rect(dst, stride, 0, width * px, 0, height, true, true);
        job.dst = (uint64_t)d.dev; job.dst_stride = (int32_t)d.pitch;
    }
    job.src0 = (uint64_t)call.linear(res, (size_t)width * height * sizeof(int), true, mode == 2);
    job.w = (int16_t)width; job.h = (int16_t)height; job.mode = (int16_t)mode; job.w0 = (int16_t)c_sign; job.denom = (int16_t)shift;
    const vvc355_blend_job *jd = call.upload(&job, 1);
    const int gx = (width * height + 1023) / 1024;
    VVC355_BD_DISPATCH(bd, hipLaunchKernelGGL((residual_kernel<BD>), dim3(gx, 1), dim3(256), 0, call.stream(), jd));
    HIP_CHECK(hipGetLastError());
}

void vvc355_add_residual(int bd, uint8_t *dst, const int *res, int width, int height, ptrdiff_t stride)
{
    slot_residual(bd, 0, dst, const_cast<int *>(res), width, height, stride, 0, 0);
}

void vvc355_add_residual_joint(int bd, uint8_t *dst, const int *res, int width, int height, ptrdiff_t stride, int c_sign, int shift)
{
    slot_residual(bd, 1, dst, const_cast<int *>(res), width, height, stride, c_sign, shift);
}

void vvc355_pred_residual_joint(int *buf, int width, int height, int c_sign, int shift)
{
    slot_residual(10, 2, nullptr, buf, width, height, 0, c_sign, shift);
}

void vvc355_transform_bdpcm(int *coeffs, int width, int height, int vertical, int log2_transform_range)
{
    if (width <= 0 || height <= 0 || width > 128 || height > 128) return;
    SlotCall call;
    vvc355_blend_job job = {};
    job.dst = (uint64_t)call.linear(coeffs, (size_t)width * height * sizeof(int), true, true);
    job.w = (int16_t)width; job.h = (int16_t)height; job.mode = (int16_t)!!vertical; job.denom = (int16_t)log2_transform_range;
    hipLaunchKernelGGL(bdpcm_kernel, dim3(1), dim3(128), 0, call.stream(), call.upload(&job, 1));
    HIP_CHECK(hipGetLastError());
}

} // extern "C"
