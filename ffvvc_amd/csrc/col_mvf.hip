// The hand-back of collocated motion for gfx950 (vvc355_col_mvf_pass): of the MvField table that later pictures read as collocated motion
// (fc->ref->tab_dmvr_mvf: temporal_luma_motion_vector vvc_mvs.c:220-245, sb_temproal_luma_motion :1016-1022) the one entry in four that is
// read — those at (x & ~7, y & ~7) — and of it the fields that are read, packed into 16 bytes, the vector through mv_compression
// (vvc_mvs.c:57-69, H.266 clause 8.5.2.15) where asked.  A strided gather: only the address pattern can be done well or badly.
//
// First launch, one lane per entry, a wave per 64 neighbouring entries of a row of `col`: a lane reads its 24-byte MvField, which is 8-byte
// aligned, with three 8-byte loads at a 48-byte stride (the compiler joins the first two into one 16-byte load; the wave touches every
// 128-byte line of its 3 KiB of the table row once and uses half of it; the odd table rows are never touched), and writes ONE 16-byte
// store, so that a wave writes one contiguous kilobyte.  A cooperative row load through LDS would fetch the same lines from HBM and add a
// round trip; nothing is reused, so there is no LDS.
//
// Second launch (n_jobs > 0), one lane per luma job: set_dmvr_info (vvc_inter.c:750-762) restricted to the entries anyone reads.  A DMVR
// job puts its record's refined vector into the one to four entries whose grid point lies in its rectangle.  Sub-blocks are disjoint: no
// atomics.  Vector stores only.
#include "common.hpp"
#include "../../include/vvc_mi355.h"

namespace vvc355 {

static_assert(sizeof(vvc355_col_mv) == 16 && sizeof(vvc355_col_mvf_frame) == 56 && sizeof(vvc355_mvfield) == 24, "layout of the hand-back");

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// mv_compression on one component (vvc_mvs.c:59-65)
__device__ __forceinline__ int col_mv_compress(int v)
{
    const int s = v >> 17;
    const int f = ilog2((unsigned)((v ^ s) | 31)) - 4;
    return (v + ((1 << f) >> 2)) & ((-(1 << f)) >> 1);
}

__device__ __forceinline__ uint32_t col_mv_field(int v, bool compress) { return (uint32_t)(compress ? col_mv_compress(v) : v) & 0x7FFFF; }

__global__ __launch_bounds__(256) void col_mvf_kernel(const vvc355_col_mvf_frame *__restrict__ fp)
{
    const vvc355_col_mvf_frame f = load_uniform(fp);
    const int gw = (f.width + 7) >> 3, gh = (f.height + 7) >> 3, per_row = (gw + 63) >> 6;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (wave >= (uint32_t)gh * per_row)
        return;
    const int gy = (int)(wave / per_row), gx = (int)(wave - (uint32_t)gy * per_row) * 64 + (threadIdx.x & 63);
    if (gx >= gw)
        return;
    const bool compress = f.flags & VVC355_COL_MVF_COMPRESS;
    // table position (2 * gy, 2 * gx); spans are below 2 GiB (checked on the host)
    const uint8_t *src = (const uint8_t *)f.mvf + (uint64_t)(2 * gy) * f.mvf_stride * sizeof(vvc355_mvfield);
    const uint32_t at = (uint32_t)gx * 2 * sizeof(vvc355_mvfield);
    const u32x2 m0 = gld_at<u32x2>(src, at), m1 = gld_at<u32x2>(src, at + 8), t = gld_at<u32x2>(src, at + 16);
    const uint32_t pf = t.y & 3;                                  // ref_idx[0], ref_idx[1], hpel_if_idx, bcw_idx | pred_flag, ciip_flag, pad
    u32x4 e = { 0, pf << 19, 0, 0 };
    if (pf & 1) {
        e.x = col_mv_field((int)m0.x, compress) | (t.x & 0x1F) << 19;
        e.y |= col_mv_field((int)m0.y, compress);
    }
    if (pf & 2) {
        e.z = col_mv_field((int)m1.x, compress) | ((t.x >> 8) & 0x1F) << 19;
        e.w = col_mv_field((int)m1.y, compress);
    }
    gst_at<u32x4>((uint8_t *)f.col + (uint64_t)gy * f.col_stride * sizeof(vvc355_col_mv), (uint32_t)gx * sizeof(vvc355_col_mv), e);
}

__global__ __launch_bounds__(256) void col_mvf_overlay_kernel(const vvc355_col_mvf_frame *__restrict__ fp)
{
    const vvc355_col_mvf_frame f = load_uniform(fp);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= f.n_jobs)
        return;
    const VVC355_GLOBAL vvc355_bipred_job *j = (const VVC355_GLOBAL vvc355_bipred_job *)f.jobs_luma + i;
    if (!j->dmvr)
        return;
    const int x = j->x, y = j->y, w = j->w, h = j->h;
    // a rectangle set_dmvr_info could not have: nothing is written for it
    if (((x | y) & 3) || x < 0 || y < 0 || (w != 8 && w != 16) || (h != 8 && h != 16) || x + w > f.width || y + h > f.height)
        return;
    const u32x4 r = gld<u32x4>((const vvc355_bipred_result *)f.records + i);             // mv[4]: L0 x, y, L1 x, y
    const bool compress = f.flags & VVC355_COL_MVF_COMPRESS;
    const uint32_t keep = ~0x7FFFFu;                              // ref_idx and pred_flag stay what the first launch wrote
    // grid points 8 * g in [x, x + w): inside the picture, so inside the rows of `col`
    for (int gy = (y + 7) >> 3; 8 * gy < y + h; gy++)
        for (int gx = (x + 7) >> 3; 8 * gx < x + w; gx++) {
            uint8_t *p = (uint8_t *)f.col + ((uint64_t)gy * f.col_stride + gx) * sizeof(vvc355_col_mv);
            u32x4 e = gld<u32x4>(p);
            const uint32_t pf = (e.y >> 19) & 3;
            if (pf & 1) {
                e.x = (e.x & keep) | col_mv_field((int)r.x, compress);
                e.y = (e.y & keep) | col_mv_field((int)r.y, compress);
            }
            if (pf & 2) {
                e.z = (e.z & keep) | col_mv_field((int)r.z, compress);
                e.w = (e.w & keep) | col_mv_field((int)r.w, compress);
            }
            gst<u32x4>(p, e);
        }
}

// [a, a + an) and [b, b + bn) share a byte
static bool col_spans_meet(uint64_t a, uint64_t an, uint64_t b, uint64_t bn) { return a < b + bn && b < a + an; }

// the frame as the header states it, every refusal before any HIP call
static int col_mvf_check(const vvc355_col_mvf_frame *f)
{
    if (!f)
        return VVC355_COL_MVF_E_FRAME;
    if (f->width <= 0 || f->height <= 0 || (f->width & 3) || (f->height & 3) || f->width > 32764 || f->height > 32764)
        return VVC355_COL_MVF_E_SIZE;
    const int tw = f->width >> 2, th = f->height >> 2, gw = (f->width + 7) >> 3, gh = (f->height + 7) >> 3;
    if (f->mvf_stride < tw || f->col_stride < gw || (int64_t)f->mvf_stride * th * (int64_t)sizeof(vvc355_mvfield) >= ((int64_t)1 << 31) ||
        (int64_t)f->col_stride * gh * (int64_t)sizeof(vvc355_col_mv) >= ((int64_t)1 << 31))
        return VVC355_COL_MVF_E_STRIDE;
    if (!f->mvf || (f->mvf & 7) || !f->col || (f->col & 15))
        return VVC355_COL_MVF_E_TABLES;
    if (f->n_jobs < 0 || (f->n_jobs > 0 && (!f->jobs_luma || (f->jobs_luma & 7) || !f->records || (f->records & 15))))
        return VVC355_COL_MVF_E_JOBS;
    if ((f->flags & ~VVC355_COL_MVF_COMPRESS) || f->pad_[0] || f->pad_[1] || f->pad_[2])
        return VVC355_COL_MVF_E_FLAGS;
    if (col_spans_meet(f->col, ((uint64_t)f->col_stride * (gh - 1) + gw) * sizeof(vvc355_col_mv),
                       f->mvf, ((uint64_t)f->mvf_stride * (th - 1) + tw) * sizeof(vvc355_mvfield)))
        return VVC355_COL_MVF_E_OVERLAP;
    return 0;
}

} // namespace vvc355

using namespace vvc355;

extern "C" {

int vvc355_col_mvf_pass(void *stream, const vvc355_col_mvf_frame *frame_dev, const vvc355_col_mvf_frame *frame_host)
{
    const int err = frame_dev ? col_mvf_check(frame_host) : VVC355_COL_MVF_E_FRAME;
    if (err)
        return err;
    const int gw = (frame_host->width + 7) >> 3, gh = (frame_host->height + 7) >> 3;
    const uint32_t waves = (uint32_t)gh * ((gw + 63) >> 6);                             // <= 4096 * 64
    hipLaunchKernelGGL(col_mvf_kernel, dim3((waves + 3) / 4), dim3(256), 0, (hipStream_t)stream, frame_dev);
    HIP_CHECK(hipGetLastError());
    if (frame_host->n_jobs > 0) {
        hipLaunchKernelGGL(col_mvf_overlay_kernel, dim3((frame_host->n_jobs + 255) / 256), dim3(256), 0, (hipStream_t)stream, frame_dev);
        HIP_CHECK(hipGetLastError());
    }
    return 0;
}

} // extern "C"
