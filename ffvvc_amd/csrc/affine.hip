// Affine motion compensation with PROF for gfx950: the luma work of pred_affine_blk (libavcodec/vvc/vvc_inter.c:864-897) for
// one 4x4 sub-block per job — luma_prof_uni (:369-406) / luma_prof_bi (:408-447): interpolation with the affine filter set
// (ff_vvc_inter_luma_filters[2], h2656_inter_template.c:29-340), edge emulation to the picture (:33-59, by clamped reads),
// and where cb_prof_flag is set fetch_samples (vvc_inter_template.c:130) + apply_prof / apply_prof_uni / apply_prof_uni_w
// (:160-235), then put_uni / put_uni_w rounding or avg / w_avg (:25-58) straight to pixels.
//
// Mapping: 16 lanes per sub-block, four sub-blocks per wave, wave-level synchronisation only; the lists in use are "slots" (slot 0 is
// list 1 for pred_flag 2) and a bi-predicted sub-block gives eight lanes to each slot, so both lists go through every stage together:
//  * descriptor: one dword per lane (and eight lanes a second one) to LDS, read back from there by every lane;
//  * window: 11 rows of 12 samples per slot as three 8-byte loads per row (4-byte at 8 bit) when rows -3 .. 7 and columns -3 .. 8
//    around the block lie inside the picture, all of a lane's loads in flight before the first LDS store; otherwise sample by sample
//    at clamped coordinates (emulated_edge, vvc_inter.c:33-59);
//  * h pass: two adjacent outputs per item from five aligned sample pairs with v_dot2 (nine dot products), 11 rows x 2 items per slot,
//    stored transposed; v pass: two vertically adjacent outputs per lane the same way, eight lanes per slot.  A zero fraction takes the
//    taps {0, 0, 0, 64, 0, 0, 0, 0}, which makes copy / h / v / hv one formula: 64 s >> (bd - 8) = s << (14 - bd), (64 t) >> 6 = t, and
//    for v only ((sum f s) << (14 - bd)) >> 6 = (sum f s) >> (bd - 8), all exact;
//  * the 14-bit predictions of both slots meet in 6x6 LDS planes, with the integer-sample ring where the list has PROF; then one lane
//    per sample: gradients, refinement, rounding or blending, the forward map, the store.
// Three group synchronisations after the descriptor's, whatever the number of lists.
#include "common.hpp"
#include "pk16.hpp"
#include "wave.hpp"
#include "runtime.hpp"
#include "../../include/vvc_mi355.h"

namespace vvc355 {

#define VVC355_TABLE(type, name, count) __device__ static const type a_tab_##name[count]
#include "tables.inc"
#undef VVC355_TABLE

static constexpr int kAwP = 12;          // window pitch: 11 columns, and the 12th the vector fetch brings along (zero tap)
static constexpr int kAtP = 12;          // transposed h output: 11 rows, and a 12th that only a zero tap reads

struct AffineLds {
    uint32_t job[24];                    // the descriptor
    uint16_t win[2][11 * kAwP];          // per slot: samples (-3 .. 8) x (-3 .. 7) around the block
    int16_t thT[2][4 * kAtP];            // per slot: horizontal pass output, [column][row]
    int16_t pp[2][6 * 6];                // per slot: prediction (14-bit) with its ring, (1, 1) = block origin
};
static_assert(sizeof(AffineLds) % 16 == 0 && offsetof(AffineLds, win) % 8 == 0 && sizeof(uint16_t[11 * kAwP]) % 8 == 0, "8-byte window rows");

// Two adjacent outputs of an 8-tap filter from five aligned sample pairs d[m] = (p[2m], p[2m + 1]): out0 = sum f[k] p[k],
// out1 = sum f[k] p[k + 1]; p[9] meets a zero.
struct AffineTaps {
    uint32_t e[4], o[5];
    __device__ __forceinline__ void set(int frac)
    {
        uint2 raw = make_uint2(64u << 24, 0u);                                   // whole sample: {0, 0, 0, 64, 0, 0, 0, 0}
        if (frac)
            raw = gld<uint2>(a_tab_inter_luma_filters + (2 * 16 + frac) * 8);
        int f[8];
#pragma unroll
        for (int k = 0; k < 8; k++) f[k] = (int)(int8_t)((k < 4 ? raw.x : raw.y) >> ((k & 3) * 8));
#pragma unroll
        for (int m = 0; m < 4; m++) e[m] = pack16(f[2 * m], f[2 * m + 1]);
        o[0] = pack16(0, f[0]);
#pragma unroll
        for (int m = 1; m < 4; m++) o[m] = pack16(f[2 * m - 1], f[2 * m]);
        o[4] = pack16(f[7], 0);
    }
    __device__ __forceinline__ void apply(const uint32_t *d, int &out0, int &out1) const
    {
        uint32_t dd[5];
#pragma unroll
        for (int m = 0; m < 5; m++) dd[m] = d[m];
        int a = 0, b = 0;
#pragma unroll
        for (int m = 0; m < 4; m++) a = dot2(dd[m], e[m], a);
#pragma unroll
        for (int m = 0; m < 5; m++) b = dot2(dd[m], o[m], b);
        out0 = a; out1 = b;
    }
};

template <int BD>
__global__ __launch_bounds__(256) void affine_kernel(const vvc355_affine_job *__restrict__ jobs, int n_jobs)
{
    using px_t = typename Px<BD>::type;
    static_assert(sizeof(vvc355_affine_job) == 96, "descriptor: 24 dwords");
    __shared__ __attribute__((aligned(16))) AffineLds lds_all[16];
    const int ji = blockIdx.x * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
    if (ji >= n_jobs)
        return;                                          // whole 16-lane groups leave together
    AffineLds &L = lds_all[threadIdx.x >> 4];
    {
        const uint32_t *q = (const uint32_t *)(jobs + ji);
        L.job[l] = gld<uint32_t>(q + l);
        if (l < 8)
            L.job[16 + l] = gld<uint32_t>(q + 16 + l);
        wave_sync();
    }
    vvc355_affine_job job;
    __builtin_memcpy(&job, L.job, sizeof(job));
    const int nl = (job.pred_flag & 1) + ((job.pred_flag >> 1) & 1);
    if (!nl)
        return;
    const bool bi = nl == 2;
    const int first_list = job.pred_flag == 2 ? 1 : 0;   // the list of slot 0; slot 1 is list 1
    // the lane's slot for the fetch and the two passes, its number among the slot's lanes, and their count
    const int sl = bi ? l >> 3 : 0, li = bi ? l & 7 : l, nlan = bi ? 8 : 16;
    {
        const int lst = sl ? 1 : first_list;
        const int mvx = lst ? job.mv[2] : job.mv[0], mvy = lst ? job.mv[3] : job.mv[1];
        const int ox = job.x + (mvx >> 4), oy = job.y + (mvy >> 4);
        const uint8_t *plane = (const uint8_t *)(lst ? job.ref1 : job.ref0);
        const int stride = lst ? job.ref1_stride : job.ref0_stride;
        uint16_t *win = L.win[sl];
        // ---- 11 x 11 (12) window
        if (ox >= 3 && ox + 8 < job.pic_w && oy >= 3 && oy + 7 < job.pic_h) {
            const uint8_t *org = plane + row_off(oy - 3, stride) + (ox - 3) * (int)sizeof(px_t);
            uint2 v[5];
#pragma unroll
            for (int it = 0; it < 5; it++) {
                const int e = li + nlan * it, r = e / 3, k = e - 3 * r;
                if (e < 33) {
                    const uint8_t *p = org + row_off(r, stride) + k * 4 * (int)sizeof(px_t);
                    if (BD > 8) {
                        v[it] = gld<uint2>(p);
                    } else {
                        const uint32_t q = gld<uint32_t>(p);
                        v[it] = make_uint2(widen_lo(q), widen_hi(q));
                    }
                }
            }
#pragma unroll
            for (int it = 0; it < 5; it++) {
                const int e = li + nlan * it, r = e / 3, k = e - 3 * r;
                if (e < 33)
                    *(uint2 *)(win + r * kAwP + 4 * k) = v[it];
            }
        } else {
            // clamped coordinates (emulated_edge, vvc_inter.c:33-59)
            for (int e = li; e < 121; e += nlan) {
                const int r = e / 11, c = e - r * 11;
                const int xa = clip3(ox - 3 + c, 0, job.pic_w - 1), ya = clip3(oy - 3 + r, 0, job.pic_h - 1);
                win[r * kAwP + c] = (uint16_t)gld<px_t>(plane + (ptrdiff_t)ya * stride + xa * (int)sizeof(px_t));
            }
        }
        wave_sync();
        // ---- put[LUMA][..] (h2656_inter_template.c:29, :97, :112, :127), horizontal: rows 0 .. 10, outputs 2 xp and 2 xp + 1
        AffineTaps t;
        t.set(mvx & 15);
        int16_t *thT = L.thT[sl];
        for (int e = li; e < 22; e += nlan) {
            const int r = e >> 1, xp = e & 1;
            int o0, o1;
            t.apply((const uint32_t *)(win + r * kAwP + 2 * xp), o0, o1);
            thT[(2 * xp) * kAtP + r] = (int16_t)(o0 >> (BD - 8));
            thT[(2 * xp + 1) * kAtP + r] = (int16_t)(o1 >> (BD - 8));
        }
        wave_sync();
        // ---- vertical: column x, rows 2 yp and 2 yp + 1; put stores int16
        if ((l >> 3) < nl) {
            const int x = l & 3, yp = (l >> 2) & 1;
            t.set(mvy & 15);
            int o0, o1;
            t.apply((const uint32_t *)(thT + x * kAtP + 2 * yp), o0, o1);
            L.pp[sl][(2 * yp + 1) * 6 + x + 1] = (int16_t)(o0 >> 6);
            L.pp[sl][(2 * yp + 2) * 6 + x + 1] = (int16_t)(o1 >> 6);
        }
    }
    const int16_t *dmv = (const int16_t *)job.diff_mv;
    // ---- fetch_samples (vvc_inter_template.c:130): ring position (rx, ry) in -1 .. 4 reads the integer sample at
    // (rx + (mx >> 3), ry + (my >> 3)) of the block
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const int lst = s ? 1 : first_list;
        if (s >= nl || !(lst ? job.prof1 : job.prof0))
            continue;
        const int mx = (lst ? job.mv[2] : job.mv[0]) & 15, my = (lst ? job.mv[3] : job.mv[1]) & 15;
        for (int e = l; e < 20; e += 16) {
            int rx, ry;
            if (e < 6)       { ry = -1; rx = e - 1; }
            else if (e < 12) { ry = 4;  rx = e - 7; }
            else             { const int k = e - 12; ry = k >> 1; rx = (k & 1) ? 4 : -1; }
            const int v = L.win[s][(ry + (my >> 3) + 3) * kAwP + rx + (mx >> 3) + 3];
            L.pp[s][(ry + 1) * 6 + rx + 1] = (int16_t)(v << (14 - BD));
        }
    }
    wave_sync();
    // ---- one lane per sample: the PROF gradients and refinement (:135, :160-235), then the output
    const int x = l & 3, y = l >> 2, o = (y + 1) * 6 + x + 1;
    int val[2] = { 0, 0 };
    bool prof_last = false;
#pragma unroll
    for (int s = 0; s < 2; s++) {
        if (s >= nl)
            continue;
        const int lst = s ? 1 : first_list;
        const int16_t *pp = L.pp[s];
        int p = pp[o];
        prof_last = lst ? job.prof1 : job.prof0;
        if (prof_last) {
            const int g_h = (int16_t)((pp[o + 1] >> 6) - (pp[o - 1] >> 6));
            const int g_v = (int16_t)((pp[o + 6] >> 6) - (pp[o - 6] >> 6));
            const int limit = 1 << max(13, BD + 1);
            const int di = g_h * (int)gld<int16_t>(dmv + lst * 32 + l) + g_v * (int)gld<int16_t>(dmv + lst * 32 + 16 + l);
            p = p + clip3(di, -limit, limit - 1);
        }
        val[s] = p;
    }
    uint8_t *drow = (uint8_t *)job.dst + (ptrdiff_t)y * job.dst_stride;
    int out;
    if (!bi) {
        // uni-prediction: put_uni / put_uni_w (h2656_inter_template.c:44, :60) or apply_prof_uni(_w)
        const int p = val[0];
        if (!job.weight_flag) {
            const int sh = 14 - BD;
            out = (p + (1 << (sh - 1))) >> sh;
        } else {
            const int sh = job.denom + (prof_last ? max(2, 14 - BD) : 14 - BD);
            out = ((p * job.w0 + (1 << (sh - 1))) >> sh) + job.o0 * (1 << (BD - 8));
        }
    } else {
        // apply_prof / put leave int16 operands; avg / w_avg (vvc_inter_template.c:25, :42)
        const int a = (int16_t)val[0], b = (int16_t)val[1];
        if (!job.weight_flag) {
            const int sh = max(3, 15 - BD);
            out = (a + b + (1 << (sh - 1))) >> sh;
        } else {
            const int sh = job.denom + max(3, 15 - BD);
            out = (a * job.w0 + b * job.w1 + ((((job.o0 + job.o1) << (BD - 8)) + 1) << (sh - 1))) >> sh;
        }
    }
    st_px<BD>(drow, x, lmcs_fwd<BD>((const uint8_t *)job.lmcs_lut, clip_px<BD>(out)));
}

} // namespace vvc355

extern "C" void vvc355_affine_batch(void *stream, int bd, const vvc355_affine_job *jobs_dev, int n_jobs)
{
    using namespace vvc355;
    if (n_jobs <= 0) return;
    VVC355_BD_DISPATCH(bd, hipLaunchKernelGGL((affine_kernel<BD>), dim3((n_jobs + 15) / 16), dim3(256), 0, (hipStream_t)stream, jobs_dev, n_jobs));
    HIP_CHECK(hipGetLastError());
}
