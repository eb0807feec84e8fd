// The QP tables of the deblocking stage straight from the unit records (vvc355_deblock_qp_rec_pass).
//
// vvc355_deblock_frame_pass reads fc->tab.qp[LUMA] per coding unit and fc->tab.qp[CB] / [CR] per chroma transform block.  The reference
// paints them from one value per unit (set_qp_y, set_qp_c_tab: vvc_ctu.c:144-185); here those values arrive as sidecars of the records
// vvc355_deblock_bs_rec_pass already takes (one byte per coding-unit record, two per transform-unit record, paired by index) and the
// planes are painted on the device, so that nothing whose size follows the picture's 4x4 grid is uploaded.
//
// One workgroup per CTU, 256 lanes, one launch, no device scratch, no atomics, no halo (nothing here looks across a CTU edge).
//   paint   the CTU's coding-unit and tree-1 transform-unit records -> map[2][32 x 32] (record index relative to the CTU's first record),
//           as bs_rec_kernel does (rec_map.hpp, CHECKED); tree-0 transform units paint nothing.
//   gather  a lane owns four consecutive units of a row: four map entries in one 8-byte LDS read, the sidecar bytes at base + index, one
//           dword store per table (byte stores at the picture's right edge, or where the pitch or the base leaves the row unaligned).
// LDS: 2 x 1024 uint16 + 1024 uint2 heads = 12 KB.
//
// The records are not trusted (see include/vvc_mi355.h): a malformed record paints nothing, the CTU's ranges are clamped to the arrays, and
// a sidecar is read only at the index of a record that painted; a unit no record covers gets 0.
#include "common.hpp"
#include "runtime.hpp"
#include "rec_map.hpp"
#include "../../include/vvc_mi355.h"
#include "stage_checks.hpp"

namespace vvc355 {

// four consecutive units of a table row, unit k in bits 8k..8k+7; n < 4: the picture ends after n of them
__device__ __forceinline__ void store_units(uint8_t *p, uint32_t v, int n)
{
    if (n == 4 && !((uintptr_t)p & 3)) {
        gst<uint32_t>(p, v);
        return;
    }
    for (int k = 0; k < n; k++)
        gst<uint8_t>(p + k, (uint8_t)(v >> (8 * k)));
}

__global__ __launch_bounds__(256) void qp_rec_kernel(const vvc355_qp_rec_frame *__restrict__ fp)
{
    __shared__ __attribute__((aligned(8))) uint16_t map[2][kMaxUnits];              // coding unit, transform unit tree 1
    __shared__ uint2 heads[kMaxUnits];
    const vvc355_qp_rec_frame F = load_uniform(fp);
    const int rs = blockIdx.x, ry = rs / F.ctb_width, rx = rs - ry * F.ctb_width;
    const int ctb_log2 = F.ctb_log2;
    const int lw = ctb_log2 - 2, side = 1 << lw, n_units = side * side;
    const int ox = rx << ctb_log2, oy = ry << ctb_log2;
    const bool chroma = F.n_comp == 3;
    for (int i = threadIdx.x; i < 2 * kMaxUnits / 2; i += 256)
        ((uint32_t *)map)[i] = 0xffffffffu;
    __syncthreads();
    const vvc355_cu_rec *cus = (const vvc355_cu_rec *)F.cu;
    const vvc355_tu_rec *tus = (const vvc355_tu_rec *)F.tu;
    // both ranges are asked for before the first is used: one round trip, not two
    int cu_base = 0, cu_end = 0, tu_base = 0, tu_end = 0;
    ctu_range((const int *)F.ctu_first_cu, rs, F.n_cu, cu_base, cu_end);
    if (chroma)
        ctu_range((const int *)F.ctu_first_tu, rs, F.n_tu, tu_base, tu_end);
    map_records<vvc355_cu_rec, true>(map[0], (uint16_t *)nullptr, heads, cus, cu_base, cu_end, ox, oy, lw);
    map_records<vvc355_tu_rec, true, true>((uint16_t *)nullptr, map[1], heads, tus, tu_base, tu_end, ox, oy, lw);
    __syncthreads();

    const uint8_t *cu_qp = (const uint8_t *)F.cu_qp, *tu_qp_c = (const uint8_t *)F.tu_qp_c;
    const int pw = F.width >> 2, ph = F.height >> 2;                                    // picture size in units
    for (int g = threadIdx.x; g < n_units >> 2; g += 256) {
        const int i = g << 2, dy = i >> lw, dx = i & (side - 1);
        const int ux = (ox >> 2) + dx, uy = (oy >> 2) + dy;
        if (ux >= pw || uy >= ph)
            continue;
        const int n = min(4, pw - ux);
        const size_t off = (size_t)uy * F.unit_pitch + ux;
        const uint2 m_cu = *(const uint2 *)&map[0][i];
        const uint16_t i_cu[4] = { (uint16_t)m_cu.x, (uint16_t)(m_cu.x >> 16), (uint16_t)m_cu.y, (uint16_t)(m_cu.y >> 16) };
        uint32_t y = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int q = abs_rec(i_cu[k], cu_base);
            if (q >= 0)
                y |= (uint32_t)gld<uint8_t>(cu_qp + q) << (8 * k);
        }
        store_units((uint8_t *)F.qp_y + off, y, n);
        if (!chroma)
            continue;
        const uint2 m_tu = *(const uint2 *)&map[1][i];
        const uint16_t i_tu[4] = { (uint16_t)m_tu.x, (uint16_t)(m_tu.x >> 16), (uint16_t)m_tu.y, (uint16_t)(m_tu.y >> 16) };
        uint32_t cb = 0, cr = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int q = abs_rec(i_tu[k], tu_base);
            if (q >= 0) {
                cb |= (uint32_t)gld<uint8_t>(tu_qp_c + 2 * (size_t)q) << (8 * k);
                cr |= (uint32_t)gld<uint8_t>(tu_qp_c + 2 * (size_t)q + 1) << (8 * k);
            }
        }
        store_units((uint8_t *)F.qp_c[0] + off, cb, n);
        store_units((uint8_t *)F.qp_c[1] + off, cr, n);
    }
}

} // namespace vvc355

// the frame as the header states it: every refusal before any HIP call
int vvc355::qp_rec_check(const vvc355_qp_rec_frame *f)
{
    if (!f)
        return VVC355_QP_REC_E_FRAME;
    if (f->width <= 0 || f->height <= 0 || (f->width & 3) || (f->height & 3))
        return VVC355_QP_REC_E_SIZE;
    if (f->ctb_log2 < 5 || f->ctb_log2 > 7)
        return VVC355_QP_REC_E_CTB;
    const int ctb = 1 << f->ctb_log2;
    if (f->ctb_width != (f->width + ctb - 1) >> f->ctb_log2 || f->ctb_height != (f->height + ctb - 1) >> f->ctb_log2)
        return VVC355_QP_REC_E_GRID;
    if (f->unit_pitch < f->width / 4)
        return VVC355_QP_REC_E_PITCH;
    if (f->n_comp != 1 && f->n_comp != 3)
        return VVC355_QP_REC_E_COMP;
    if (f->n_cu < 0 || f->n_tu < 0)
        return VVC355_QP_REC_E_COUNT;
    const bool chroma = f->n_comp == 3;
    if ((f->n_cu > 0 && (!f->cu || !f->ctu_first_cu)) || (chroma && f->n_tu > 0 && (!f->tu || !f->ctu_first_tu)))
        return VVC355_QP_REC_E_RECORDS;
    if ((f->n_cu > 0 && !f->cu_qp) || (chroma && f->n_tu > 0 && !f->tu_qp_c))
        return VVC355_QP_REC_E_SIDECAR;
    if (!f->qp_y || (chroma && (!f->qp_c[0] || !f->qp_c[1])))
        return VVC355_QP_REC_E_OUTPUT;
    return 0;
}

extern "C" int vvc355_deblock_qp_rec_pass(void *stream, const vvc355_qp_rec_frame *frame_dev, const vvc355_qp_rec_frame *frame_host)
{
    const int err = frame_dev ? vvc355::qp_rec_check(frame_host) : VVC355_QP_REC_E_FRAME;
    if (err)
        return err;
    hipLaunchKernelGGL(vvc355::qp_rec_kernel, dim3(frame_host->ctb_width * frame_host->ctb_height), dim3(256), 0, (hipStream_t)stream, frame_dev);
    HIP_CHECK(hipGetLastError());
    return 0;
}
