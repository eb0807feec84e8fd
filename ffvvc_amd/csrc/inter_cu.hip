// Affine and geometric-partition stage drivers for gfx950: the job arrays of a whole picture's affine and GPM coding units, written
// on the device from the decoder's MvField table, reference-picture lists and prediction weight tables plus one record per coding
// unit, then the prediction kernels of affine.hip and mc_fused.hip.  Reference behaviour: predict_inter (libavcodec/vvc/vvc_inter.c:
// 875-891) -> pred_affine_blk (:828-873, derive_affine_mvc :813-826) and pred_gpm_blk (:466-527); weights derive_weight_uni /
// derive_weight (:129-177, inter_weight.hpp).
//
// The GPM weight masks are not the reference's tables but the closed form of the standard's weighted sample prediction for the
// geometric partitioning mode, evaluated at compile time: one 112x112 mask per angle that a partition uses, indexed at
// (yL + offsetY + 56, xL + offsetX + 56).  Every block size (8 .. 64 per side) addresses it with steps 1 << hs and 112 << vs.
#include <utility>

#include "common.hpp"
#include "inter_weight.hpp"
#include "runtime.hpp"
#include "../../include/vvc_mi355.h"

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
    vvc355_affine_batch(stream, bd, (const vvc355_affine_job *)frame_host->jobs_luma, frame_host->n_jobs);
    if (frame_host->pic.chroma_format_idc)
        vvc355_bipred_chroma_batch(stream, bd, (const vvc355_bipred_job *)frame_host->jobs_chroma,
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
    vvc355_gpm_batch(stream, bd, (const vvc355_gpm_job *)frame_host->jobs, frame_host->n_jobs);
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
