// Affine, geometric-partition and combined inter / intra (CIIP) stage drivers for gfx950: the job arrays of a whole picture's affine,
// GPM and CIIP coding units, written on the device from the decoder's MvField table, reference-picture lists and prediction weight
// tables plus one record per coding unit, then the prediction kernels of affine.hip and mc_fused.hip.  Reference behaviour:
// predict_inter (libavcodec/vvc/vvc_inter.c:875-891) -> pred_affine_blk (:828-873, derive_affine_mvc :813-826) and pred_gpm_blk
// (:466-527); the inter part of ff_vvc_predict_ciip (:915; pred_regular_luma :545-581, pred_regular_chroma :583-640,
// ciip_derive_intra_weight :523-543); weights derive_weight_uni / derive_weight (:129-177, inter_weight.hpp).
//
// The GPM weight masks are not the reference's tables but the closed form of the standard's weighted sample prediction for the
// geometric partitioning mode, evaluated at compile time: one 112x112 mask per angle that a partition uses, indexed at
// (yL + offsetY + 56, xL + offsetX + 56).  Every block size (8 .. 64 per side) addresses it with steps 1 << hs and 112 << vs.
#include <utility>

#include "common.hpp"
#include "inter_weight.hpp"
#include "runtime.hpp"
#include "../../include/vvc_mi355.h"
#include "stage_checks.hpp"

namespace vvc355 {

static_assert(sizeof(vvc355_affine_cu) == 144 && offsetof(vvc355_affine_cu, diff_mv) == 16 && offsetof(vvc355_affine_cu, first_job) == 12,
              "vvc355_affine_cu layout");
static_assert(sizeof(vvc355_gpm_cu) == 64 && offsetof(vvc355_gpm_cu, gpm_mv) == 16 && offsetof(vvc355_gpm_cu, first_job) == 12,
              "vvc355_gpm_cu layout");
static_assert(sizeof(vvc355_inter_frame) == 136, "vvc355_inter_frame layout");
static_assert(sizeof(vvc355_affine_frame) == 168 && offsetof(vvc355_affine_frame, cus) == 136 && offsetof(vvc355_affine_frame, n_cus) == 160,
              "vvc355_affine_frame layout");
static_assert(sizeof(vvc355_gpm_frame) == 160 && offsetof(vvc355_gpm_frame, cus) == 136 && offsetof(vvc355_gpm_frame, n_cus) == 152,
              "vvc355_gpm_frame layout");
static_assert(sizeof(vvc355_affine_job) == 96 && sizeof(vvc355_bipred_job) == 104 && sizeof(vvc355_gpm_job) == 120, "job layouts");
static_assert(sizeof(vvc355_ciip_cu) == 32 && offsetof(vvc355_ciip_cu, first_job) == 12 && offsetof(vvc355_ciip_cu, cmd) == 20, "vvc355_ciip_cu layout");
static_assert(sizeof(vvc355_ciip_frame) == 224 && offsetof(vvc355_ciip_frame, cus) == 136 && offsetof(vvc355_ciip_frame, n_cus) == 192 &&
              offsetof(vvc355_ciip_frame, ctb_log2) == 220, "vvc355_ciip_frame layout");
static_assert(sizeof(vvc355_recon_cmd) == 40 && offsetof(vvc355_recon_cmd, joint) == 33, "vvc355_recon_cmd layout");

// mc_fused.hip: ciip_pred_kernel<bd> over jobs[0 .. n_jobs), one wave per job
void ciip_pred_launch(hipStream_t stream, int bd, const vvc355_bipred_job *jobs_dev, int n_jobs);
// mc_fused.hip: bipred_chroma_one_pair_kernel<bd>, one wave per pair of chroma jobs: what vvc355_bipred_chroma_batch does for arrays
// that cannot take its four-pairs-per-wave path, without that path's LDS and registers
void chroma_pairs_launch(hipStream_t stream, int bd, const vvc355_bipred_job *jobs_dev, int n_jobs);

// partition -> angleIdx / distanceIdx and disLut (tables_small.inc; tables.cpp exports the same text as vvc355_tab_gpm_*)
#define VVC355_TABLE(type, name, count) static constexpr type c_##name[count]
#include "tables_small.inc"
#undef VVC355_TABLE
#define VVC355_TABLE(type, name, count) __device__ static const type t_##name[count]
#include "tables_small.inc"
#undef VVC355_TABLE

// ------------------------------------------------------------------ GPM weight masks

constexpr int kGpmMaskSize = 112;            // VVC_GPM_WEIGHT_SIZE: |xL + offsetX| <= 56 for every allowed block size
struct GpmMask { uint8_t w[kGpmMaskSize * kGpmMaskSize]; };

// the angles the 64 partitions use, one mask each, in increasing angle order
constexpr uint32_t gpm_used_angles()
{
    uint32_t m = 0;
    for (int p = 0; p < 64; p++) m |= 1u << c_gpm_angle_idx[p];
    return m;
}
constexpr uint32_t kGpmAngles = gpm_used_angles();
constexpr int kGpmMasks = __builtin_popcount(kGpmAngles);
static_assert(kGpmMasks == 20, "GPM uses 20 of the 32 angles");
__host__ __device__ constexpr int gpm_mask_slot(int angle) { return __builtin_popcount(kGpmAngles & ((1u << angle) - 1)); }
constexpr int gpm_slot_angle(int slot)
{
    for (int a = 0; a < 32; a++)
        if (((kGpmAngles >> a) & 1) && gpm_mask_slot(a) == slot) return a;
    return -1;
}

// The weight of luma-grid position (u - 56, v - 56) relative to the block's partition origin (xL + offsetX, yL + offsetY):
// weightIdx = ((xL + offsetX) * 2 + 1) * disLut[angleIdx] + ((yL + offsetY) * 2 + 1) * disLut[displacementY], displacementY =
// (angleIdx + 8) % 32, partFlip = !(13 <= angleIdx <= 27), w = Clip3(0, 8, ((partFlip ? 32 + weightIdx : 32 - weightIdx) + 4) >> 3)
constexpr GpmMask make_gpm_mask(int angle)
{
    GpmMask m = {};
    const int dx = c_gpm_distance_lut[angle], dy = c_gpm_distance_lut[(angle + 8) % 32];
    const bool flip = !(angle >= 13 && angle <= 27);
    for (int v = 0; v < kGpmMaskSize; v++) {
        const int ry = (2 * (v - 56) + 1) * dy;
        for (int u = 0; u < kGpmMaskSize; u++) {
            const int idx = (2 * (u - 56) + 1) * dx + ry;
            const int s = ((flip ? 32 + idx : 32 - idx) + 4) >> 3;
            m.w[v * kGpmMaskSize + u] = (uint8_t)(s < 0 ? 0 : s > 8 ? 8 : s);
        }
    }
    return m;
}
// one constant evaluation per mask (each stays below clang's constexpr step limit)
template <int A> constexpr GpmMask kGpmMaskOf = make_gpm_mask(A);

template <typename Seq> struct GpmMaskSet;
template <size_t... S> struct GpmMaskSet<std::index_sequence<S...>> { GpmMask m[sizeof...(S)]; };
using GpmMaskTable = GpmMaskSet<std::make_index_sequence<kGpmMasks>>;
template <size_t... S> constexpr GpmMaskSet<std::index_sequence<S...>> make_gpm_masks(std::index_sequence<S...>)
{
    return { { kGpmMaskOf<gpm_slot_angle(S)>... } };
}
// the same data twice: the device copy the jobs address, the host copy vvc355_gpm_weights reads
__device__ const GpmMaskTable d_gpm_masks = make_gpm_masks(std::make_index_sequence<kGpmMasks>{});
static const GpmMaskTable h_gpm_masks = make_gpm_masks(std::make_index_sequence<kGpmMasks>{});

// Where a component of a cb_width x cb_height unit of partition (angle, distance) starts in its mask: offsetX = (-nW) >> 1 and offsetY =
// (-nH) >> 1, one of them moved by (distanceIdx * n) >> 3 along the axis shiftHor selects (+ for angleIdx < 16).  Sample (x, y) of the
// component is element first + y * step_y + x * step_x of mask `slot`.  A unit outside 8 .. 64 per side gets steps 0 (no read
// outside the masks).
struct GpmAddr { int slot, first, step_x, step_y; };
__host__ __device__ inline GpmAddr gpm_address(int angle, int distance, int cb_width, int cb_height, int hs, int vs)
{
    GpmAddr a;
    a.slot = gpm_mask_slot(angle);
    const bool shift_hor = !(angle % 16 == 8 || (angle % 16 != 0 && cb_height >= cb_width));
    int off_x = (-cb_width) >> 1, off_y = (-cb_height) >> 1;
    if (shift_hor)
        off_x += angle < 16 ? (distance * cb_width) >> 3 : -((distance * cb_width) >> 3);
    else
        off_y += angle < 16 ? (distance * cb_height) >> 3 : -((distance * cb_height) >> 3);
    const bool ok = cb_width >= 8 && cb_width <= 64 && cb_height >= 8 && cb_height <= 64 && ((kGpmAngles >> angle) & 1);
    a.first = ok ? (off_y + 56) * kGpmMaskSize + off_x + 56 : 0;
    a.step_x = ok ? 1 << hs : 0;
    a.step_y = ok ? kGpmMaskSize << vs : 0;
    return a;
}

// ------------------------------------------------------------------ builders

// the record whose [first_job, next first_job) holds job i: the last one with first_job <= i
template <typename Cu> __device__ __forceinline__ int find_cu(const Cu *cus, int n_cus, uint32_t i)
{
    int lo = 0, hi = n_cus - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cus[mid].first_job <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ uint64_t plane_at(const vvc355_inter_frame &f, int c, int x, int y)
{
    return f.dst[c] + (uint64_t)y * f.dst_stride[c] + ((uint64_t)x << f.pixel_shift);
}

// ff_vvc_round_mv(mv, 0, 1) (vvc_mvs.c:1739)
__device__ __forceinline__ int32_t round_mv_half(int32_t v) { return (v + 1 - (v >= 0)) >> 1; }

// pred_affine_blk: one lane per 4x4 luma sub-block (job), sub-blocks in raster order inside their unit.  The lane of a sub-block at a
// chroma position also writes that position's Cb and Cr jobs.
__global__ __launch_bounds__(256) void affine_build_kernel(const vvc355_affine_frame *__restrict__ fp)
{
    const vvc355_affine_frame F = load_uniform(fp);
    const vvc355_inter_frame &f = F.pic;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)F.n_jobs)
        return;
    const vvc355_affine_cu *cus = (const vvc355_affine_cu *)F.cus;
    const int u = find_cu(cus, F.n_cus, i);
    const vvc355_affine_cu *cu = cus + u;
    const int x0 = cu->x0, y0 = cu->y0, cbw = cu->cb_width, cbh = cu->cb_height, nsx = cu->num_sb_x, nsy = cu->num_sb_y;
    const uint32_t first = cu->first_job;
    const uint32_t n_local = (u + 1 < F.n_cus ? cus[u + 1].first_job : (uint32_t)F.n_jobs) - first;
    const uint32_t k = i - first;
    const int hs = f.hs, vs = f.vs, csh = hs + vs;
    vvc355_affine_job *jl = (vvc355_affine_job *)F.jobs_luma;
    vvc355_bipred_job *jc = (vvc355_bipred_job *)F.jobs_chroma;
    const uint32_t cfirst = first >> csh;

    // affine sub-blocks are 4x4 (vvc_mvs.c:1272); a record that says otherwise gets jobs that predict nothing (pred_flag 0, chroma 0)
    if (nsx != cbw >> 2 || nsy != cbh >> 2 || cbw < 8 || cbh < 8 || n_local != (uint32_t)(nsx * nsy)) {
        jl[i] = vvc355_affine_job{};
        if (f.chroma_format_idc && k < (n_local >> csh)) {
            jc[2 * (cfirst + k)] = vvc355_bipred_job{};
            jc[2 * (cfirst + k) + 1] = vvc355_bipred_job{};
        }
        return;
    }
    const vvc355_inter_slice *sl = (const vvc355_inter_slice *)f.slices + cu->slice;
    const vvc355_ref_pic *refs = (const vvc355_ref_pic *)f.refs;
    const MvFieldDev *mvf_tab = (const MvFieldDev *)f.mvf;
    const int sbx = k % nsx, sby = k / nsx;
    const int x = x0 + 4 * sbx, y = y0 + 4 * sby;
    const MvFieldDev mv = mvf_tab[(y >> 2) * f.mvf_stride + (x >> 2)];                           // ff_vvc_get_mvf

    // luma: luma_prof_uni / luma_prof_bi (:369-447)
    vvc355_affine_job j = {};
    j.dst = plane_at(f, 0, x, y);
    j.dst_stride = f.dst_stride[0];
    for (int l = 0; l < 2; l++) {
        if (!(mv.pred_flag & (1 << l)))
            continue;
        const vvc355_ref_pic rp = refs[l * 16 + mv.ref_idx[l]];                                   // pred_get_refs
        (l ? j.ref1 : j.ref0) = rp.plane[0];
        (l ? j.ref1_stride : j.ref0_stride) = rp.stride[0];
        j.mv[2 * l] = mv.mv[l][0];
        j.mv[2 * l + 1] = mv.mv[l][1];
    }
    j.diff_mv = F.cus + (uint64_t)u * sizeof(vvc355_affine_cu) + offsetof(vvc355_affine_cu, diff_mv);
    j.x = (int16_t)x; j.y = (int16_t)y; j.pic_w = (int16_t)f.width; j.pic_h = (int16_t)f.height;
    set_pred_weight(j, derive_pred_weight(sl, mv, 0, false, false));                              // derive_weight(.., dmvr_flag 0)
    j.pred_flag = mv.pred_flag;
    j.prof0 = cu->prof_flags & 1;
    j.prof1 = (cu->prof_flags >> 1) & 1;
    j.lmcs_lut = sl->lmcs_used ? f.lmcs_fwd_lut : 0;                                             // predict_inter's lmcs.filter (:888-891)
    jl[i] = j;

    // chroma: pred_regular_chroma (:583-640) of a 4x4 chroma block at derive_affine_mvc's motion (:813-826), filter set 0, no DMVR
    if (!f.chroma_format_idc || (sbx & ((1 << hs) - 1)) || (sby & ((1 << vs) - 1)))
        return;
    const MvFieldDev mv2 = mvf_tab[((y + vs * 4) >> 2) * f.mvf_stride + ((x + hs * 4) >> 2)];
    MvFieldDev mvc = mv;
    for (int l = 0; l < 2; l++)
        for (int d = 0; d < 2; d++)
            mvc.mv[l][d] = round_mv_half(mv.mv[l][d] + mv2.mv[l][d]);
    const uint32_t ck = cfirst + (sby >> vs) * (nsx >> hs) + (sbx >> hs);
    for (int c = 1; c < 3; c++) {
        vvc355_bipred_job b = {};
        const int xc = x >> hs, yc = y >> vs;
        b.dst = plane_at(f, c, xc, yc);
        b.dst_stride = f.dst_stride[c];
        for (int l = 0; l < 2; l++) {
            if (!(mvc.pred_flag & (1 << l)))
                continue;
            const vvc355_ref_pic rp = refs[l * 16 + mvc.ref_idx[l]];
            (l ? b.ref1 : b.ref0) = rp.plane[c];
            (l ? b.ref1_stride : b.ref0_stride) = rp.stride[c];
            b.mv[2 * l] = mvc.mv[l][0];
            b.mv[2 * l + 1] = mvc.mv[l][1];
        }
        b.x = (int16_t)xc; b.y = (int16_t)yc; b.w = 4; b.h = 4;
        b.pic_w = (int16_t)(f.width >> hs); b.pic_h = (int16_t)(f.height >> vs);
        b.chroma = 1; b.hs = (uint8_t)hs; b.vs = (uint8_t)vs;
        set_pred_weight(b, derive_pred_weight(sl, mvc, c, false, false));
        b.pred_flag = mvc.pred_flag;
        jc[2 * ck + c - 1] = b;
    }
}

// pred_gpm_blk: one lane per <= 16x16 tile; a unit's jobs are its luma tiles, then its Cb tiles, then its Cr tiles, each in raster order
__global__ __launch_bounds__(256) void gpm_build_kernel(const vvc355_gpm_frame *__restrict__ fp)
{
    const vvc355_gpm_frame F = load_uniform(fp);
    const vvc355_inter_frame &f = F.pic;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)F.n_jobs)
        return;
    const vvc355_gpm_cu *cus = (const vvc355_gpm_cu *)F.cus;
    const int u = find_cu(cus, F.n_cus, i);
    const vvc355_gpm_cu cu = cus[u];
    const vvc355_inter_slice *sl = (const vvc355_inter_slice *)f.slices + cu.slice;
    const vvc355_ref_pic *refs = (const vvc355_ref_pic *)f.refs;
    const int cbw = cu.cb_width, cbh = cu.cb_height;
    int k = (int)(i - cu.first_job), c = 0;
    for (; c < (f.chroma_format_idc ? 2 : 0); c++) {                   // which component's tiles k falls in
        const int sx = c ? f.hs : 0, sy = c ? f.vs : 0;
        const int nt = (((cbw >> sx) + 15) >> 4) * (((cbh >> sy) + 15) >> 4);
        if (k < nt)
            break;
        k -= nt;
    }
    const int hs = c ? f.hs : 0, vs = c ? f.vs : 0;
    const int w = cbw >> hs, h = cbh >> vs, tw = min(w, 16), th = min(h, 16);
    const int ntx = (w + 15) >> 4;
    const int tx = (k % ntx) * tw, ty = (k / ntx) * th;
    const int x = (cu.x0 >> hs) + tx, y = (cu.y0 >> vs) + ty;
    const int part = cu.partition_idx & 63;
    const GpmAddr a = gpm_address(t_gpm_angle_idx[part], t_gpm_distance_idx[part], cbw, cbh, hs, vs);

    vvc355_gpm_job g = {};
    vvc355_bipred_job &j = g.base;
    j.dst = plane_at(f, c, x, y);
    j.dst_stride = f.dst_stride[c];
    const MvFieldDev *gmv = (const MvFieldDev *)cu.gpm_mv;
    for (int p = 0; p < 2; p++) {
        const MvFieldDev &m = gmv[p];
        const int lx = m.pred_flag - 1;                                   // each part is uni-predicted
        const vvc355_ref_pic rp = refs[lx * 16 + m.ref_idx[lx]];
        (p ? j.ref1 : j.ref0) = rp.plane[c];
        (p ? j.ref1_stride : j.ref0_stride) = rp.stride[c];
        j.mv[2 * p] = m.mv[lx][0];
        j.mv[2 * p + 1] = m.mv[lx][1];
    }
    j.x = (int16_t)x; j.y = (int16_t)y; j.w = (int16_t)tw; j.h = (int16_t)th;
    j.pic_w = (int16_t)(f.width >> hs); j.pic_h = (int16_t)(f.height >> vs);
    j.chroma = c > 0; j.hs = f.hs; j.vs = f.vs;
    j.pred_flag = 3;
    j.lmcs_lut = (!c && sl->lmcs_used) ? f.lmcs_fwd_lut : 0;              // predict_inter's lmcs.filter (:888-891)
    g.weights = (uint64_t)&d_gpm_masks.m[a.slot].w[a.first + ty * a.step_y + tx * a.step_x];
    g.step_x = a.step_x;
    g.step_y = a.step_y;
    ((vvc355_gpm_job *)F.jobs)[i] = g;
}

// The inter part of ff_vvc_predict_ciip: one lane per job slot.  A unit's slots are its luma tiles, then its Cb tiles, then its Cr tiles,
// each in raster order; the lane of a component's first tile also completes that component's VVC355_RECON_CIIP command.  Every slot
// below n_jobs is written by its own lane and by no other: the job, or zeros (w = h = 0: ciip_pred_kernel skips it) where the slot
// belongs to a rejected record or to none.  Nothing a record says reaches an address before it is checked against the frame.
__global__ __launch_bounds__(256) void ciip_build_kernel(const vvc355_ciip_frame *__restrict__ fp)
{
    const vvc355_ciip_frame F = load_uniform(fp);
    const vvc355_inter_frame &f = F.pic;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)F.n_jobs)
        return;
    vvc355_bipred_job *slot = (vvc355_bipred_job *)F.jobs + i;
    vvc355_bipred_job j = {};
    const vvc355_ciip_cu *cus = (const vvc355_ciip_cu *)F.cus;
    const int u = find_cu(cus, F.n_cus, i);
    const vvc355_ciip_cu cu = cus[u];
    const int x0 = cu.x0, y0 = cu.y0, cbw = cu.cb_width, cbh = cu.cb_height, ctb_log2 = F.ctb_log2;
    const bool side_ok = cbw >= 4 && cbw <= 64 && !(cbw & (cbw - 1)) && cbh >= 4 && cbh <= 64 && !(cbh & (cbh - 1)) && cbw * cbh >= 64;
    const bool inside = x0 >= 0 && y0 >= 0 && !((x0 | y0) & 3) && x0 + cbw <= f.width && y0 + cbh <= f.height &&
                        (x0 >> ctb_log2) == ((x0 + cbw - 1) >> ctb_log2) && (y0 >> ctb_log2) == ((y0 + cbh - 1) >> ctb_log2);
    // the unit's tiles and its region
    const bool has_c = f.chroma_format_idc != 0;
    const int wc = cbw >> f.hs, hc = cbh >> f.vs;
    const bool blend_c = has_c && wc > 2;                                  // do_ciip (:590)
    const uint32_t ntl = ((cbw + 15) >> 4) * ((cbh + 15) >> 4), ntc = has_c ? ((wc + 15) >> 4) * ((hc + 15) >> 4) : 0;
    const uint32_t region = cbw * cbh + (blend_c ? 2 * wc * hc : 0);
    uint32_t k = i - cu.first_job;
    if (!side_ok || !inside || i < cu.first_job || cu.slice >= F.n_slices || (uint64_t)cu.first_job + ntl + 2 * ntc > (uint64_t)(uint32_t)F.n_jobs ||
        (uint64_t)cu.scratch_off + region > (uint64_t)(uint32_t)F.scratch_len || k >= ntl + 2 * ntc) {
        *slot = j;
        return;
    }
    const MvFieldDev *mvf_tab = (const MvFieldDev *)f.mvf;
    const MvFieldDev mv = mvf_tab[(y0 >> 2) * f.mvf_stride + (x0 >> 2)];                             // ff_vvc_get_mvf
    bool mv_ok = mv.pred_flag >= 1 && mv.pred_flag <= 3;
    for (int l = 0; l < 2; l++)
        mv_ok = mv_ok && (!(mv.pred_flag & (1 << l)) || (mv.ref_idx[l] >= 0 && mv.ref_idx[l] <= 15));
    if (!mv_ok) {
        *slot = j;
        return;
    }
    const vvc355_inter_slice *sl = (const vvc355_inter_slice *)f.slices + cu.slice;
    const vvc355_ref_pic *refs = (const vvc355_ref_pic *)f.refs;
    int c = 0;
    if (k >= ntl) {                                                        // which component's tiles k falls in
        k -= ntl;
        c = 1;
        if (k >= ntc) { k -= ntc; c = 2; }
    }
    const int hs = c ? f.hs : 0, vs = c ? f.vs : 0;
    const int w = cbw >> hs, h = cbh >> vs, tw = min(w, 16), th = min(h, 16);
    const int ntx = (w + 15) >> 4;
    const int tx = (k % ntx) * tw, ty = (k / ntx) * th;
    const int x = (x0 >> hs) + tx, y = (y0 >> vs) + ty;
    const bool to_plane = c && !blend_c;
    // component c's part of the unit's region: luma, then Cb, then Cr, rows packed
    const uint64_t part = F.scratch + (((uint64_t)cu.scratch_off + (c ? cbw * cbh + (c - 1) * wc * hc : 0)) << f.pixel_shift);

    if (to_plane) {                                                       // c is 1 or 2 here; no indexing of the descriptor copy by a variable
        j.dst_stride = c == 1 ? f.dst_stride[1] : f.dst_stride[2];
        j.dst = (c == 1 ? f.dst[1] : f.dst[2]) + (uint64_t)y * j.dst_stride + ((uint64_t)x << f.pixel_shift);
    } else {
        j.dst = part + ((uint64_t)(ty * w + tx) << f.pixel_shift);
        j.dst_stride = w << f.pixel_shift;
    }
    for (int l = 0; l < 2; l++) {
        if (!(mv.pred_flag & (1 << l)))
            continue;
        const vvc355_ref_pic *rp = refs + l * 16 + mv.ref_idx[l];                                    // pred_get_refs
        (l ? j.ref1 : j.ref0) = rp->plane[c];
        (l ? j.ref1_stride : j.ref0_stride) = rp->stride[c];
        j.mv[2 * l] = mv.mv[l][0];
        j.mv[2 * l + 1] = mv.mv[l][1];
    }
    j.x = (int16_t)x; j.y = (int16_t)y; j.w = (int16_t)tw; j.h = (int16_t)th;
    j.pic_w = (int16_t)(f.width >> hs); j.pic_h = (int16_t)(f.height >> vs);
    j.chroma = c > 0; j.hs = f.hs; j.vs = f.vs;
    j.hf_idx = j.vf_idx = c ? 0 : cu.hpel_if_idx & 1;
    j.pred_flag = mv.pred_flag;
    j.lmcs_lut = (!c && sl->lmcs_used) ? f.lmcs_fwd_lut : 0;              // the inter part is mapped before the blend (:573-574)
    set_pred_weight(j, derive_pred_weight(sl, mv, c, false, true));       // derive_weight(.., dmvr_flag 0) with ciip_flag: no bcw weights (:158)
    *slot = j;

    if (!F.cmds || k || to_plane)
        return;
    // the component's VVC355_RECON_CIIP command: where its inter prediction lies, and ciip_derive_intra_weight (:523-543)
    const uint32_t ci = cus[u].cmd[c];
    if (ci >= (uint32_t)F.n_cmds)
        return;
    vvc355_recon_cmd *cmd = (vvc355_recon_cmd *)F.cmds + ci;
    if (cmd->kind != VVC355_RECON_CIIP || cmd->c_idx != c || cmd->x0 != x0 || cmd->y0 != y0 || cmd->w != cbw || cmd->h != cbh)
        return;
    // ctb_left / ctb_up: ff_vvc_decode_neighbour (vvc_ctu.c:2468-2495), as the RECON pass derives them
    const int16_t *slice_idx = (const int16_t *)F.slice_idx, *col_bd = (const int16_t *)F.ctb_to_col_bd, *row_bd = (const int16_t *)F.ctb_to_row_bd;
    const int rx = x0 >> ctb_log2, ry = y0 >> ctb_log2, ncx = F.ctb_width, rs = ry * ncx + rx, ctb_mask = (1 << ctb_log2) - 1;
    const bool left_tile = rx > 0 && col_bd[rx] != col_bd[rx - 1];
    const bool upper_tile = ry > 0 && row_bd[ry] != row_bd[ry - 1];
    const bool upper_slice = ry > 0 && slice_idx[rs] != slice_idx[rs - ncx];
    const bool ctb_left = rx > 0 && !left_tile, ctb_up = ry > 0 && !upper_tile && !upper_slice;
    const bool available_l = ctb_left || (x0 & ctb_mask), available_u = ctb_up || (y0 & ctb_mask);
    int weight = 1;
    if (available_u && mvf_tab[((y0 - 1) >> 2) * f.mvf_stride + ((x0 - 1 + cbw) >> 2)].pred_flag == 0)
        weight++;
    if (available_l && mvf_tab[((y0 - 1 + cbh) >> 2) * f.mvf_stride + ((x0 - 1) >> 2)].pred_flag == 0)
        weight++;
    cmd->resid = part;
    cmd->joint = (uint8_t)weight;
}

// the host copy of a CIIP frame, before any HIP call; bd < 0: no bit depth to check (vvc355_ciip_frame_build)
int ciip_frame_check(const vvc355_ciip_frame *F, int bd)
{
    if (!F)
        return VVC355_CIIP_E_FRAME;
    const vvc355_inter_frame &f = F->pic;
    if (f.width <= 0 || f.height <= 0 || (f.width & 3) || (f.height & 3))
        return VVC355_CIIP_E_SIZE;
    if (F->ctb_log2 < 5 || F->ctb_log2 > 7)
        return VVC355_CIIP_E_CTB;
    const int ctb = 1 << F->ctb_log2;
    if (F->ctb_width != (f.width + ctb - 1) >> F->ctb_log2 || F->ctb_height != (f.height + ctb - 1) >> F->ctb_log2)
        return VVC355_CIIP_E_GRID;
    if (F->n_cus < 0 || F->n_jobs < 0 || F->scratch_len < 0 || F->n_slices < 0 || F->n_cmds < 0)
        return VVC355_CIIP_E_COUNT;
    if (bd >= 0 && ((bd != 8 && bd != 10 && bd != 12) || f.pixel_shift != (bd > 8)))
        return VVC355_CIIP_E_DEPTH;
    if (bd < 0 && f.pixel_shift > 1)
        return VVC355_CIIP_E_DEPTH;
    const int fmt_hs[4] = { 0, 1, 1, 0 }, fmt_vs[4] = { 0, 1, 0, 0 };
    if (f.chroma_format_idc > 3 || f.hs != fmt_hs[f.chroma_format_idc] || f.vs != fmt_vs[f.chroma_format_idc])
        return VVC355_CIIP_E_FORMAT;
    if (F->n_cus > 0 && !F->cus)
        return VVC355_CIIP_E_RECORDS;
    if (F->n_jobs > 0 && !F->jobs)
        return VVC355_CIIP_E_JOBS;
    if (!F->scratch || !f.mvf || !f.refs || !f.slices || !f.dst[0] || (f.chroma_format_idc && (!f.dst[1] || !f.dst[2])) || f.mvf_stride < f.width / 4)
        return VVC355_CIIP_E_TABLES;
    if (F->cmds && (!F->slice_idx || !F->ctb_to_col_bd || !F->ctb_to_row_bd))
        return VVC355_CIIP_E_CMDS;
    return 0;
}

} // namespace vvc355

extern "C" {

void vvc355_affine_frame_build(void *stream, const vvc355_affine_frame *frame_dev, const vvc355_affine_frame *frame_host)
{
    if (frame_host->n_cus <= 0 || frame_host->n_jobs <= 0) return;
    hipLaunchKernelGGL(vvc355::affine_build_kernel, dim3((frame_host->n_jobs + 255) / 256), dim3(256), 0, (hipStream_t)stream, frame_dev);
    HIP_CHECK(hipGetLastError());
}

void vvc355_affine_frame_pass(void *stream, int bd, const vvc355_affine_frame *frame_dev, const vvc355_affine_frame *frame_host)
{
    if (frame_host->n_cus <= 0 || frame_host->n_jobs <= 0) return;
    vvc355_affine_frame_build(stream, frame_dev, frame_host);
    vvc355_affine_frame_predict(stream, bd, frame_dev, frame_host);
}

void vvc355_affine_frame_predict(void *stream, int bd, const vvc355_affine_frame *, const vvc355_affine_frame *frame_host)
{
    if (frame_host->n_cus <= 0 || frame_host->n_jobs <= 0) return;
    vvc355_affine_batch(stream, bd, (const vvc355_affine_job *)frame_host->jobs_luma, frame_host->n_jobs);
    if (frame_host->pic.chroma_format_idc)
        vvc355::chroma_pairs_launch((hipStream_t)stream, bd, (const vvc355_bipred_job *)frame_host->jobs_chroma,      // 4x4 blocks: never the quad path
                                    2 * (frame_host->n_jobs >> (frame_host->pic.hs + frame_host->pic.vs)));
}

void vvc355_gpm_frame_build(void *stream, const vvc355_gpm_frame *frame_dev, const vvc355_gpm_frame *frame_host)
{
    if (frame_host->n_cus <= 0 || frame_host->n_jobs <= 0) return;
    hipLaunchKernelGGL(vvc355::gpm_build_kernel, dim3((frame_host->n_jobs + 255) / 256), dim3(256), 0, (hipStream_t)stream, frame_dev);
    HIP_CHECK(hipGetLastError());
}

void vvc355_gpm_frame_pass(void *stream, int bd, const vvc355_gpm_frame *frame_dev, const vvc355_gpm_frame *frame_host)
{
    if (frame_host->n_cus <= 0 || frame_host->n_jobs <= 0) return;
    vvc355_gpm_frame_build(stream, frame_dev, frame_host);
    vvc355_gpm_frame_predict(stream, bd, frame_dev, frame_host);
}

void vvc355_gpm_frame_predict(void *stream, int bd, const vvc355_gpm_frame *, const vvc355_gpm_frame *frame_host)
{
    if (frame_host->n_cus <= 0 || frame_host->n_jobs <= 0) return;
    vvc355_gpm_batch(stream, bd, (const vvc355_gpm_job *)frame_host->jobs, frame_host->n_jobs);
}

int vvc355_ciip_frame_build(void *stream, const vvc355_ciip_frame *frame_dev, const vvc355_ciip_frame *frame_host)
{
    const int err = frame_dev ? vvc355::ciip_frame_check(frame_host, -1) : VVC355_CIIP_E_FRAME;
    if (err)
        return err;
    if (frame_host->n_cus == 0 || frame_host->n_jobs == 0) return 0;
    hipLaunchKernelGGL(vvc355::ciip_build_kernel, dim3((frame_host->n_jobs + 255) / 256), dim3(256), 0, (hipStream_t)stream, frame_dev);
    HIP_CHECK(hipGetLastError());
    return 0;
}

int vvc355_ciip_frame_pass(void *stream, int bd, const vvc355_ciip_frame *frame_dev, const vvc355_ciip_frame *frame_host)
{
    const int err = frame_dev ? vvc355::ciip_frame_check(frame_host, bd) : VVC355_CIIP_E_FRAME;
    if (err)
        return err;
    if (frame_host->n_cus == 0 || frame_host->n_jobs == 0) return 0;
    vvc355_ciip_frame_build(stream, frame_dev, frame_host);
    return vvc355_ciip_frame_predict(stream, bd, frame_dev, frame_host);
}

int vvc355_ciip_frame_predict(void *stream, int bd, const vvc355_ciip_frame *frame_dev, const vvc355_ciip_frame *frame_host)
{
    const int err = frame_dev ? vvc355::ciip_frame_check(frame_host, bd) : VVC355_CIIP_E_FRAME;
    if (err)
        return err;
    if (frame_host->n_cus == 0 || frame_host->n_jobs == 0) return 0;
    vvc355::ciip_pred_launch((hipStream_t)stream, bd, (const vvc355_bipred_job *)frame_host->jobs, frame_host->n_jobs);
    return 0;
}

void vvc355_gpm_weights(int partition_idx, int cb_width, int cb_height, int hs, int vs, uint8_t *out)
{
    using namespace vvc355;
    const int part = partition_idx & 63;
    const GpmAddr a = gpm_address(c_gpm_angle_idx[part], c_gpm_distance_idx[part], cb_width, cb_height, hs, vs);
    const uint8_t *m = h_gpm_masks.m[a.slot].w;
    const int w = cb_width >> hs, h = cb_height >> vs;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            out[y * w + x] = m[a.first + y * a.step_y + x * a.step_x];
}

} // extern "C"
