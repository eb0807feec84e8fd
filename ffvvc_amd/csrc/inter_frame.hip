// Inter prediction stage driver for gfx950: the sub-block job arrays of a whole picture, written on the device from the decoder's
// MvField table, reference-picture lists, prediction weight tables and a list of coding units, then the fused sub-block kernels of
// mc_fused.hip.  Reference behaviour: pred_regular_blk and its helpers, libavcodec/vvc/vvc_inter.c:129-177 (derive_weight_uni,
// derive_weight), :764-813 (derive_sb_mv, the sub-block walk), pred_regular_luma / _chroma (:549-640: filter set, uni / bi split).
#include "common.hpp"
#include "inter_weight.hpp"
#include "runtime.hpp"
#include "../../include/vvc_mi355.h"

namespace vvc355 {

// The reference pictures of one motion, from a table of vvc355_ref_pic[2][16] in LDS (RefLds) or in memory (RefMem).
struct RefMem {
    const vvc355_ref_pic *t;
    __device__ __forceinline__ uint64_t plane(int i, int c) const { return t[i].plane[c]; }
    __device__ __forceinline__ int stride(int i, int c) const { return t[i].stride[c]; }
};
struct RefLds {
    static constexpr int DW = sizeof(vvc355_ref_pic) / 4;
    const uint32_t *t;
    __device__ __forceinline__ uint64_t plane(int i, int c) const { return t[i * DW + 2 * c] | (uint64_t)t[i * DW + 2 * c + 1] << 32; }
    __device__ __forceinline__ int stride(int i, int c) const { return (int)t[i * DW + 6 + c]; }
};

// the job of component c for the tile at luma (px, py), tw x th luma samples, of a sub-block with motion mv in coding unit pu
template <typename Refs>
__device__ __forceinline__ vvc355_bipred_job inter_tile_job(const vvc355_inter_frame &f, const vvc355_inter_pu &pu, const vvc355_inter_slice *sl,
                                                            const MvFieldDev &mv, const Refs &refs, int c, uint32_t job, int px, int py, int tw, int th)
{
    const int hs = c ? f.hs : 0, vs = c ? f.vs : 0;
    const bool bi = mv.pred_flag == 3;
    vvc355_bipred_job j = {};
    const int x = px >> hs, y = py >> vs;
    j.dst = f.dst[c] + (uint64_t)y * f.dst_stride[c] + ((uint64_t)x << f.pixel_shift);
    j.dst_stride = f.dst_stride[c];
    for (int l = 0; l < 2; l++) {
        if (!(mv.pred_flag & (1 << l)))
            continue;
        const int r = l * 16 + (mv.ref_idx[l] & 15);
        (l ? j.ref1 : j.ref0) = refs.plane(r, c);
        (l ? j.ref1_stride : j.ref0_stride) = refs.stride(r, c);
        j.mv[2 * l] = mv.mv[l][0];
        j.mv[2 * l + 1] = mv.mv[l][1];
    }
    j.rec = (uint64_t)((vvc355_bipred_result *)f.records + job);
    j.x = (int16_t)x; j.y = (int16_t)y; j.w = (int16_t)(tw >> hs); j.h = (int16_t)(th >> vs);
    j.pic_w = (int16_t)(f.width >> hs); j.pic_h = (int16_t)(f.height >> vs);
    j.chroma = c > 0; j.hs = f.hs; j.vs = f.vs;
    j.dmvr = bi && pu.dmvr_flag;
    j.bdof = !c && bi && pu.bdof_flag;
    j.hf_idx = j.vf_idx = c ? 0 : pu.hpel_if_idx;
    j.pred_flag = mv.pred_flag;
    // predict_inter's lmcs.filter (:888-891): luma of the coding unit goes through the forward map, CIIP units excepted
    j.lmcs_lut = (!c && sl->lmcs_used && !pu.ciip_flag) ? f.lmcs_fwd_lut : 0;
    set_pred_weight(j, derive_pred_weight(sl, mv, c, pu.dmvr_flag, pu.ciip_flag));
    return j;
}

__device__ __forceinline__ MvFieldDev load_mvf(const vvc355_inter_frame &f, int sx, int sy)                       // ff_vvc_get_mvf
{
    const uint32_t *p = (const uint32_t *)((const MvFieldDev *)f.mvf + ((sy >> 2) * f.mvf_stride + (sx >> 2)));
    uint32_t w[sizeof(MvFieldDev) / 4];
#pragma unroll
    for (int k = 0; k < (int)(sizeof(MvFieldDev) / 4); k++) w[k] = gld<uint32_t>(p + k);
    MvFieldDev mv;
    __builtin_memcpy(&mv, w, sizeof(mv));
    return mv;
}

// One lane writes all jobs of coding unit pu to the places its first_job names: only for a workgroup whose units' first_job values are not
// the running sum of their job counts (a list that was reordered after the sums were taken), where the jobs are no contiguous range.
__device__ void inter_build_unit(const vvc355_inter_frame &f, const vvc355_inter_pu &pu)
{
    const vvc355_inter_slice *sl = (const vvc355_inter_slice *)f.slices + pu.slice;
    const RefMem refs = { (const vvc355_ref_pic *)f.refs };
    vvc355_bipred_job *jl = (vvc355_bipred_job *)f.jobs_luma, *jc = (vvc355_bipred_job *)f.jobs_chroma;
    const int sbw = pu.cb_width / pu.num_sb_x, sbh = pu.cb_height / pu.num_sb_y;
    const int tw = min(sbw, 16), th = min(sbh, 16);
    uint32_t job = pu.first_job;
    for (int sby = 0; sby < pu.num_sb_y; sby++)
        for (int sbx = 0; sbx < pu.num_sb_x; sbx++) {
            const int sx = pu.x0 + sbx * sbw, sy = pu.y0 + sby * sbh;
            const MvFieldDev mv = load_mvf(f, sx, sy);
            for (int ty = 0; ty < sbh; ty += th)
                for (int tx = 0; tx < sbw; tx += tw, job++) {
                    jl[job] = inter_tile_job(f, pu, sl, mv, refs, 0, job, sx + tx, sy + ty, tw, th);
                    if (!f.chroma_format_idc)
                        continue;
                    jc[2 * job] = inter_tile_job(f, pu, sl, mv, refs, 1, job, sx + tx, sy + ty, tw, th);
                    jc[2 * job + 1] = inter_tile_job(f, pu, sl, mv, refs, 2, job, sx + tx, sy + ty, tw, th);
                }
        }
}

// A workgroup of four waves takes kInterBuildUnits coding units.  first_job is the running sum of the units' job counts, so their jobs are one
// contiguous range of jobs_luma and twice that range of jobs_chroma.  The range is walked in chunks of 64 jobs.  Wave c builds component c
// of the chunk: a lane takes one job, finds its unit by a search in the staged first_job values, decodes sub-block and tile from the job's
// index inside the unit (walk order sby, sbx, ty, tx), builds the job in registers and leaves it as a row in LDS, Cb and Cr interleaved as
// jobs_chroma holds them; then all four waves copy the rows out as contiguous ranges (lds_rows_to_global).  A unit with many jobs is spread
// over as many lanes.  64 units and not 256 per workgroup: the picture then has 22 waves per CU instead of 6 to hide the load chain
// (unit -> MvField, slice) behind.
constexpr int kInterBuildUnits = 64;
__global__ __launch_bounds__(256) void inter_build_kernel(const vvc355_inter_frame *__restrict__ fp)
{
    constexpr int WG = 256, U = kInterBuildUnits, CH = 64, JOB_DW = sizeof(vvc355_bipred_job) / 4, PITCH = JOB_DW + 1, PU_DW = sizeof(vvc355_inter_pu) / 4;
    constexpr int REF_DW = 32 * RefLds::DW;
    static_assert(JOB_DW == 26 && PU_DW == 5 && RefLds::DW == 10, "row pitches below are odd");
    __shared__ uint32_t s_luma[CH * PITCH], s_chroma[2 * CH * PITCH];
    __shared__ uint32_t s_pu[(U + 1) * PU_DW];        // the units; dword 4 of a row is first_job, and row nu holds the end of the range
    __shared__ uint32_t s_refs[REF_DW];
    const vvc355_inter_frame f = load_uniform(fp);
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64, u0 = blockIdx.x * U, nu = min(U, f.n_pus - u0);
    for (int k = tid; k < REF_DW; k += WG)
        s_refs[k] = gld<uint32_t>((const uint32_t *)f.refs + k);
    vvc355_inter_pu own = {};
    uint32_t own_end = 0;
    if (tid < nu) {
        uint32_t w[PU_DW];
#pragma unroll
        for (int k = 0; k < PU_DW; k++) s_pu[tid * PU_DW + k] = w[k] = gld<uint32_t>((const uint32_t *)f.pus + (size_t)(u0 + tid) * PU_DW + k);
        __builtin_memcpy(&own, w, sizeof(own));
        const int sbw = own.cb_width / own.num_sb_x, sbh = own.cb_height / own.num_sb_y;
        own_end = own.first_job + own.num_sb_x * own.num_sb_y * ((sbw + 15) / 16) * ((sbh + 15) / 16);
        if (tid == nu - 1)
            s_pu[nu * PU_DW + 4] = own_end;
    }
    __syncthreads();
    if (!__syncthreads_and(tid >= nu || s_pu[(tid + 1) * PU_DW + 4] == own_end)) {
        if (tid < nu)
            inter_build_unit(f, own);
        return;
    }
    const RefLds refs = { s_refs };
    const uint32_t first = s_pu[4], total = s_pu[nu * PU_DW + 4] - first;
    const int ncomp = f.chroma_format_idc ? 3 : 1;
    for (uint32_t c0 = 0; c0 < total; c0 += CH) {
        const int n = (int)min((uint32_t)CH, total - c0);
        if (wave < ncomp && lane < n) {
            const uint32_t job = first + c0 + lane;
            int lo = 0, hi = nu;                      // the unit lo with first_job[lo] <= job < first_job[lo + 1]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_pu[mid * PU_DW + 4] <= job) lo = mid; else hi = mid;
            }
            uint32_t w[PU_DW];
#pragma unroll
            for (int k = 0; k < PU_DW; k++) w[k] = s_pu[lo * PU_DW + k];
            vvc355_inter_pu pu;
            __builtin_memcpy(&pu, w, sizeof(pu));
            const vvc355_inter_slice *sl = (const vvc355_inter_slice *)f.slices + pu.slice;
            const int sbw = pu.cb_width / pu.num_sb_x, sbh = pu.cb_height / pu.num_sb_y;
            const int tw = min(sbw, 16), th = min(sbh, 16);
            const int ntx = (sbw + 15) / 16, nty = (sbh + 15) / 16;
            const int local = (int)(job - pu.first_job), sb = local / (ntx * nty), t = local - sb * (ntx * nty);
            const int sby = sb / pu.num_sb_x, sbx = sb - sby * pu.num_sb_x, ty = t / ntx, tx = t - ty * ntx;
            const int sx = pu.x0 + sbx * sbw, sy = pu.y0 + sby * sbh, px = sx + tx * tw, py = sy + ty * th;
            const MvFieldDev mv = load_mvf(f, sx, sy);
            if (wave == 0)
                lds_row_put<PITCH>(s_luma, lane, inter_tile_job(f, pu, sl, mv, refs, 0, job, px, py, tw, th));
            else if (wave == 1)
                lds_row_put<PITCH>(s_chroma, 2 * lane, inter_tile_job(f, pu, sl, mv, refs, 1, job, px, py, tw, th));
            else
                lds_row_put<PITCH>(s_chroma, 2 * lane + 1, inter_tile_job(f, pu, sl, mv, refs, 2, job, px, py, tw, th));
        }
        __syncthreads();
        lds_rows_to_global<JOB_DW, PITCH>(s_luma, (vvc355_bipred_job *)f.jobs_luma + (first + c0), n);
        if (f.chroma_format_idc)
            lds_rows_to_global<JOB_DW, PITCH>(s_chroma, (vvc355_bipred_job *)f.jobs_chroma + 2 * (size_t)(first + c0), 2 * n);
        __syncthreads();
    }
}

// set_dmvr_info (vvc_inter.c:750-762) after the luma launch: one lane per luma job; a DMVR sub-block's 4x4 units get its MvField with
// the refined motion of its record
__global__ __launch_bounds__(256) void inter_dmvr_info_kernel(const vvc355_inter_frame *__restrict__ fp)
{
    const vvc355_inter_frame f = load_uniform(fp);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= f.n_jobs)
        return;
    const vvc355_bipred_job *j = (const vvc355_bipred_job *)f.jobs_luma + i;
    if (!j->dmvr)
        return;
    const vvc355_bipred_result *r = (const vvc355_bipred_result *)f.records + i;
    const MvFieldDev *src = (const MvFieldDev *)f.mvf;
    MvFieldDev *dst = (MvFieldDev *)f.dmvr_mvf;
    MvFieldDev m = src[(j->y >> 2) * f.mvf_stride + (j->x >> 2)];
    m.mv[0][0] = r->mv[0]; m.mv[0][1] = r->mv[1]; m.mv[1][0] = r->mv[2]; m.mv[1][1] = r->mv[3];
    for (int y = j->y; y < j->y + j->h; y += 4)
        for (int x = j->x; x < j->x + j->w; x += 4)
            dst[(y >> 2) * f.mvf_stride + (x >> 2)] = m;
}

} // namespace vvc355

extern "C" {

void vvc355_inter_frame_build(void *stream, const vvc355_inter_frame *frame_dev, const vvc355_inter_frame *frame_host)
{
    if (frame_host->n_pus <= 0) return;
    hipLaunchKernelGGL(vvc355::inter_build_kernel, dim3((frame_host->n_pus + vvc355::kInterBuildUnits - 1) / vvc355::kInterBuildUnits), dim3(256), 0,
                       (hipStream_t)stream, frame_dev);
    HIP_CHECK(hipGetLastError());
}

void vvc355_inter_frame_pass(void *stream, int bd, const vvc355_inter_frame *frame_dev, const vvc355_inter_frame *frame_host)
{
    if (frame_host->n_pus <= 0 || frame_host->n_jobs <= 0) return;
    vvc355_inter_frame_build(stream, frame_dev, frame_host);
    vvc355_inter_frame_predict(stream, bd, frame_dev, frame_host);
}

void vvc355_inter_frame_predict(void *stream, int bd, const vvc355_inter_frame *frame_dev, const vvc355_inter_frame *frame_host)
{
    if (frame_host->n_pus <= 0 || frame_host->n_jobs <= 0) return;
    vvc355_bipred_batch(stream, bd, (const vvc355_bipred_job *)frame_host->jobs_luma, frame_host->n_jobs);
    if (frame_host->dmvr_mvf) {
        hipLaunchKernelGGL(vvc355::inter_dmvr_info_kernel, dim3((frame_host->n_jobs + 255) / 256), dim3(256), 0, (hipStream_t)stream, frame_dev);
        HIP_CHECK(hipGetLastError());
    }
    if (frame_host->chroma_format_idc)
        vvc355_bipred_chroma_batch(stream, bd, (const vvc355_bipred_job *)frame_host->jobs_chroma, 2 * frame_host->n_jobs);
}

} // extern "C"
