// The MvField table from one 64-byte record per prediction unit (vvc355_mvf_unit_pass): the reference's three motion-storage rules on the
// device.  A regular unit stores one MvField over its rectangle (ff_vvc_store_mvf / ff_vvc_store_mv); an affine unit derives one per 4x4
// sub-block from its control points (ff_vvc_store_sb_mvs, vvc_mvs.c:402-446, H.266 clause 8.5.5.9) and with it the PROF switches and
// offsets of the affine stage driver; a GPM unit chooses per 4x4 block between its two candidates and their combination
// (ff_vvc_store_gpm_mvf, :448-491).  vvc355_tab_fill_pass takes the RESULT of those derivations, cut into rectangles of equal motion; this
// pass takes their inputs.
//
// One workgroup per CTU, 256 lanes, one launch, no device scratch, no atomics.  Per chunk of 1024 of the CTU's records (a CTU whose
// records are all well-formed has at most 1024, so one chunk):
//   check   one lane per record reads its 16-byte head (and, for GPM, the two parts' pred_flag), runs the record predicate — the one
//           vvc355_mvf_unit_check exports — and leaves position, size, kind and aux in LDS; a record that fails leaves a size of 0.
//           Nothing below indexes LDS or HBM from a record that did not pass.
//   paint   sixteen lanes per record write its index into the LDS map of the CTU's 4x4 units.
//   prof    eight lanes per AFFINE record with a link: 16 bytes of diff_mv each (one contiguous 128-byte run per record), and the flag
//           byte.  All records of the chunk at once: their loads are in flight together.
//   units   one lane per unit, in raster order, computes its own entry from the record that painted it (PLAIN: a copy; GPM: motion_idx
//           and a select; AFFINE: a handful of multiply-adds per list) and stores it with three 8-byte stores: a row of the CTU goes out
//           as one contiguous run.  The record's head comes from LDS, its body through the cache (neighbouring lanes share it).
// LDS: 1024 uint16 + 1024 uint2 = 10 KB.
#include <string.h>
#include "common.hpp"
#include "runtime.hpp"
#include "rec_map.hpp"
#include "../../include/vvc_mi355.h"

namespace vvc355 {

static_assert(sizeof(vvc355_mvf_unit) == 64 && sizeof(vvc355_mvf_unit_frame) == 64 && sizeof(vvc355_mvfield) == 24, "layout of the records");
static_assert(sizeof(vvc355_affine_cu) == 144 && offsetof(vvc355_affine_cu, prof_flags) == 10 && offsetof(vvc355_affine_cu, diff_mv) == 16,
              "layout of the affine records");

#define VVC355_TABLE(type, name, count) __device__ static const type mu_##name[count]
#include "tables_small.inc"
#undef VVC355_TABLE

// The record predicate, for the kernel and for vvc355_mvf_unit_check: 0, or the first rule the record breaks.  The head travels as its
// four dwords (x0 y0 | w h kind aux | link | pf ref_idx pad_); gpm_pf0 / gpm_pf1 are looked at for GPM records only.
__host__ __device__ inline int mvf_unit_rule(uint32_t h0, uint32_t h1, uint32_t link, uint32_t h3, int gpm_pf0, int gpm_pf1,
                                             int width, int height, int ox, int oy, int ctb, int n_affine_cus)
{
    const int x0 = (int16_t)(h0 & 0xffff), y0 = (int16_t)(h0 >> 16);
    const int w = h1 & 0xff, h = (h1 >> 8) & 0xff, kind = (h1 >> 16) & 0xff, aux = h1 >> 24;
    if (!w || !h || ((w | h) & 3) || w > 128 || h > 128)
        return VVC355_MVF_UNIT_R_SIDE;
    if (x0 < 0 || y0 < 0 || ((x0 | y0) & 3) || x0 + w > width || y0 + h > height)
        return VVC355_MVF_UNIT_R_PLACE;
    if (x0 < ox || y0 < oy || x0 + w > ox + ctb || y0 + h > oy + ctb)
        return VVC355_MVF_UNIT_R_CTU;
    if (h3 >> 24)
        return VVC355_MVF_UNIT_R_PAD;
    if (kind > VVC355_MVF_GPM)
        return VVC355_MVF_UNIT_R_KIND;
    if (kind == VVC355_MVF_AFFINE) {
        if (w < 8 || h < 8 || (w & (w - 1)) || (h & (h - 1)))
            return VVC355_MVF_UNIT_R_AFF_SHAPE;
        if (aux != 1 && aux != 2)
            return VVC355_MVF_UNIT_R_AFF_MODEL;
        if (!(h3 & 3))
            return VVC355_MVF_UNIT_R_AFF_PRED;
        if (link != VVC355_MVF_LINK_NONE && (n_affine_cus <= 0 || link >= (uint32_t)n_affine_cus))
            return VVC355_MVF_UNIT_R_AFF_LINK;
    } else if (kind == VVC355_MVF_GPM) {
        if (w < 8 || h < 8 || w > 64 || h > 64)
            return VVC355_MVF_UNIT_R_GPM_SHAPE;
        if (w >= 8 * h || h >= 8 * w)
            return VVC355_MVF_UNIT_R_GPM_RATIO;
        if (aux > 63)
            return VVC355_MVF_UNIT_R_GPM_PART;
        if ((gpm_pf0 != 1 && gpm_pf0 != 2) || (gpm_pf1 != 1 && gpm_pf1 != 2))
            return VVC355_MVF_UNIT_R_GPM_PRED;
    }
    return 0;
}

// SubblockParams of one list (init_subblock_params, vvc_mvs.c:338-359) from its three control points
struct SbParams { int d_hor_x, d_ver_x, d_hor_y, d_ver_y, scale_hor, scale_ver; };

__device__ __forceinline__ SbParams sb_params(const int *cp, int model, int log2_w, int log2_h)
{
    SbParams p;
    p.d_hor_x = (cp[2] - cp[0]) * (1 << (7 - log2_w));
    p.d_ver_x = (cp[3] - cp[1]) * (1 << (7 - log2_w));
    if (model == 2) {
        p.d_hor_y = (cp[4] - cp[0]) * (1 << (7 - log2_h));
        p.d_ver_y = (cp[5] - cp[1]) * (1 << (7 - log2_h));
    } else {
        p.d_hor_y = -p.d_ver_x;
        p.d_ver_y = p.d_hor_x;
    }
    p.scale_hor = cp[0] * (1 << 7);
    p.scale_ver = cp[1] * (1 << 7);
    return p;
}

// is_fallback_mode (:313-336)
__device__ __forceinline__ bool sb_fallback(const SbParams &p, bool bi)
{
    const int a = 4 * (2048 + p.d_hor_x), b = 4 * p.d_hor_y, c = 4 * (2048 + p.d_ver_y), d = 4 * p.d_ver_x;
    if (bi) {
        const int max_w4 = max(0, max(a, max(b, a + b))), min_w4 = min(0, min(a, min(b, a + b)));
        const int max_h4 = max(0, max(c, max(d, c + d))), min_h4 = min(0, min(c, min(d, c + d)));
        return (((max_w4 - min_w4) >> 11) + 9) * (((max_h4 - min_h4) >> 11) + 9) > 225;
    }
    return !((((abs(a) >> 11) + 9) * ((abs(d) >> 11) + 9) <= 165) && (((abs(b) >> 11) + 9) * ((abs(c) >> 11) + 9) <= 165));
}

// derive_cb_prof_flag_lx (:282-298) for a list that is in pred_flag
__device__ __forceinline__ bool sb_prof(const int *cp, int model, bool fallback, bool prof_disabled)
{
    if (prof_disabled || fallback)
        return false;
    const bool same1 = cp[0] == cp[2] && cp[1] == cp[3], same2 = cp[0] == cp[4] && cp[1] == cp[5];
    return model == 1 ? !same1 : !(same1 && same2);
}

// ff_vvc_round_mv(., 0, s) on one component (:1739-1749)
__device__ __forceinline__ int round_mv(int v, int s) { return (v + (1 << (s - 1)) - (v >= 0)) >> s; }

__device__ __forceinline__ void load_cp(int *cp, const vvc355_mvf_unit *rec, int list)
{
    const uint2 a = gld<uint2>(&rec->body[6 * list]), b = gld<uint2>(&rec->body[6 * list + 2]), c = gld<uint2>(&rec->body[6 * list + 4]);
    cp[0] = (int)a.x; cp[1] = (int)a.y; cp[2] = (int)b.x; cp[3] = (int)b.y; cp[4] = (int)c.x; cp[5] = (int)c.y;
}

// The entry of unit (gx, gy) of the picture from the record that covers it; head = x0 y0 | w h kind aux of that record, which passed the check
__device__ __forceinline__ void unit_entry(const vvc355_mvf_unit_frame &F, const vvc355_mvf_unit *rec, uint2 head, int gx, int gy)
{
    const int x0 = (int16_t)(head.x & 0xffff), y0 = (int16_t)(head.x >> 16), w = head.y & 0xff, h = (head.y >> 8) & 0xff;
    const int kind = (head.y >> 16) & 0xff, aux = head.y >> 24;
    const int bx = 4 * gx - x0, by = 4 * gy - y0;                    // this 4x4 block inside the unit
    uint2 e0, e1, e2;
    if (kind == VVC355_MVF_PLAIN) {
        e0 = gld<uint2>(&rec->body[0]); e1 = gld<uint2>(&rec->body[2]); e2 = gld<uint2>(&rec->body[4]);
    } else if (kind == VVC355_MVF_GPM) {
        const int angle = mu_gpm_angle_idx[aux], distance = mu_gpm_distance_idx[aux];
        const int disp_x = mu_gpm_distance_lut[angle], disp_y = mu_gpm_distance_lut[(angle + 8) & 31];
        const int is_flip = angle >= 13 && angle <= 27;
        const bool shift_hor = !((angle & 15) == 8 || ((angle & 15) && h >= w));
        const int sign = angle < 16 ? 1 : -1;
        int off_x = (-w) >> 1, off_y = (-h) >> 1;
        if (!shift_hor)
            off_y += sign * ((distance * h) >> 3);
        else
            off_x += sign * ((distance * w) >> 3);
        const int motion_idx = ((bx + off_x) * 2 + 5) * disp_x + ((by + off_y) * 2 + 5) * disp_y;
        const int s_type = abs(motion_idx) < 32 ? 2 : (motion_idx <= 0 ? 1 - is_flip : is_flip);
        const uint2 a0 = gld<uint2>(&rec->body[0]), a1 = gld<uint2>(&rec->body[2]), a2 = gld<uint2>(&rec->body[4]);
        const uint2 b0 = gld<uint2>(&rec->body[6]), b1 = gld<uint2>(&rec->body[8]), b2 = gld<uint2>(&rec->body[10]);
        const int pf0 = a2.y & 0xff, pf1 = b2.y & 0xff;
        if (!s_type) {
            e0 = a0; e1 = a1; e2 = a2;
        } else if (s_type == 1 || (pf0 | pf1) != 3) {
            e0 = b0; e1 = b1; e2 = b2;
        } else {
            // gpm_mv[0] with list pf1 - 1 from gpm_mv[1] and pred_flag PF_BI
            const bool l1 = pf1 == 2;
            e0 = l1 ? a0 : b0;
            e1 = l1 ? b1 : a1;
            e2.x = l1 ? ((a2.x & ~0xff00u) | (b2.x & 0xff00u)) : ((a2.x & ~0xffu) | (b2.x & 0xffu));
            e2.y = (a2.y & ~0xffu) | 3u;
        }
    } else {
        const uint32_t pw3 = gld<uint32_t>(&rec->pf);                   // pf ref_idx[0] ref_idx[1] pad_
        const int log2_w = __builtin_ctz(w), log2_h = __builtin_ctz(h), pred = pw3 & 3;
        int mv[4] = { 0, 0, 0, 0 };
        for (int l = 0; l < 2; l++) {
            if (!(pred >> l & 1))
                continue;
            int cp[6];
            load_cp(cp, rec, l);
            const SbParams p = sb_params(cp, aux, log2_w, log2_h);
            const bool fb = sb_fallback(p, pred == 3);
            const int xp = fb ? w >> 1 : 2 + bx, yp = fb ? h >> 1 : 2 + by;
            mv[2 * l] = clip3(round_mv(p.scale_hor + p.d_hor_x * xp + p.d_hor_y * yp, 7), -(1 << 17), (1 << 17) - 1);
            mv[2 * l + 1] = clip3(round_mv(p.scale_ver + p.d_ver_x * xp + p.d_ver_y * yp, 7), -(1 << 17), (1 << 17) - 1);
        }
        e0 = make_uint2((uint32_t)mv[0], (uint32_t)mv[1]);
        e1 = make_uint2((uint32_t)mv[2], (uint32_t)mv[3]);
        // ref_idx[0] ref_idx[1] hpel_if_idx bcw_idx | pred_flag ciip_flag pad
        e2 = make_uint2(((pw3 >> 8) & 0xffff) | ((pw3 >> 2) & 3) << 16 | ((pw3 >> 4) & 15) << 24, (uint32_t)pred);
    }
    uint8_t *e = (uint8_t *)F.mvf + ((size_t)gy * F.mvf_pitch + gx) * sizeof(vvc355_mvfield);
    gst<uint2>(e, e0); gst<uint2>(e + 8, e1); gst<uint2>(e + 16, e2);
}

__global__ __launch_bounds__(256) void mvf_unit_kernel(const vvc355_mvf_unit_frame *__restrict__ fp)
{
    __shared__ uint16_t map[kMaxUnits];
    __shared__ uint2 heads[kMaxUnits];               // x0 y0 | w h kind aux of a record that passed; .y = 0 of one that did not
    const vvc355_mvf_unit_frame F = load_uniform(fp);
    const int rs = blockIdx.x, ry = rs / F.ctb_width, rx = rs - ry * F.ctb_width;
    const int ctb_log2 = F.ctb_log2, lw = ctb_log2 - 2, side = 1 << lw, n_units = side * side;
    const int ox = rx << ctb_log2, oy = ry << ctb_log2;
    for (int i = threadIdx.x; i < kMaxUnits / 2; i += 256)
        ((uint32_t *)map)[i] = 0xffffffffu;
    const vvc355_mvf_unit *units = (const vvc355_mvf_unit *)F.units;
    vvc355_affine_cu *cus = (vvc355_affine_cu *)F.affine_cus;
    int first = 0, last = 0;
    ctu_range((const int *)F.ctu_first, rs, F.n_units, first, last);
    const int sub = threadIdx.x & 15;
    const int pw = F.width >> 2, ph = F.height >> 2;

    for (int c0 = first; c0 < last; c0 += kMaxUnits) {
        const int nc = min(kMaxUnits, last - c0);
        __syncthreads();
        // check: one lane per record
        for (int i = threadIdx.x; i < nc; i += 256) {
            const vvc355_mvf_unit *rec = units + c0 + i;
            const uint4 hd = gld<uint4>(rec);
            int pf0 = 0, pf1 = 0;
            if (((hd.y >> 16) & 0xff) == VVC355_MVF_GPM) {
                pf0 = gld<uint32_t>(&rec->body[5]) & 0xff;
                pf1 = gld<uint32_t>(&rec->body[11]) & 0xff;
            }
            const int rule = mvf_unit_rule(hd.x, hd.y, hd.z, hd.w, pf0, pf1, F.width, F.height, ox, oy, 1 << ctb_log2, F.n_affine_cus);
            heads[i] = rule ? make_uint2(0, 0) : make_uint2(hd.x, hd.y);
        }
        __syncthreads();
        // paint: sixteen lanes per record
        for (int k = threadIdx.x >> 4; k < nc; k += 16) {
            const uint2 head = heads[k];
            if (!head.y)
                continue;
            const int x0 = (int16_t)(head.x & 0xffff), y0 = (int16_t)(head.x >> 16), w = head.y & 0xff, h = (head.y >> 8) & 0xff;
            const int uw = w >> 2, n = uw * (h >> 2), base = (((y0 - oy) >> 2) << lw) + ((x0 - ox) >> 2);
            const uint16_t idx = (uint16_t)(c0 + k - first);
            if ((uw & (uw - 1)) == 0) {
                const int lg = __builtin_ctz(uw);
                for (int i = sub; i < n; i += 16)
                    map[base + ((i >> lg) << lw) + (i & (uw - 1))] = idx;
            } else {
                for (int i = sub; i < n; i += 16) {
                    const int dy = i / uw, dx = i - dy * uw;
                    map[base + (dy << lw) + dx] = idx;
                }
            }
        }
        // prof: eight lanes per record, those of an AFFINE record that names a vvc355_affine_cu write 16 bytes of its diff_mv each (lane s:
        // list s >> 2, axis (s >> 1) & 1, offsets 8 * (s & 1) .. + 7), so that a record's 128 bytes go out as one run; lane 0 the flag byte
        if (cus) {
            for (int t = threadIdx.x; t < 8 * nc; t += 256) {
                const int k = t >> 3, s = t & 7;
                const uint2 head = heads[k];
                if (!head.y || ((head.y >> 16) & 0xff) != VVC355_MVF_AFFINE)
                    continue;
                const vvc355_mvf_unit *rec = units + c0 + k;
                const uint2 lp = gld<uint2>(&rec->link);              // link | pf ref_idx pad_
                if (lp.x == VVC355_MVF_LINK_NONE)                     // (below n_affine_cus otherwise: the record passed)
                    continue;
                const int model = head.y >> 24, log2_w = __builtin_ctz(head.y & 0xff), log2_h = __builtin_ctz((head.y >> 8) & 0xff);
                const int pred = lp.y & 3;
                int flags = 0, dh = 0, dv = 0;
                for (int l = 0; l < 2; l++) {
                    if (!(pred >> l & 1))
                        continue;
                    int cp[6];
                    load_cp(cp, rec, l);
                    const SbParams p = sb_params(cp, model, log2_w, log2_h);
                    if (!sb_prof(cp, model, sb_fallback(p, pred == 3), F.prof_disabled))
                        continue;
                    flags |= 1 << l;
                    if ((s >> 2) == l) {
                        dh = (s & 2) ? p.d_ver_x : p.d_hor_x;
                        dv = (s & 2) ? p.d_ver_y : p.d_hor_y;
                    }
                }
                // offsets 4 * y + x for y = 2 * (s & 1), + 1; all zero where the list's flag is 0 (dh = dv = 0)
                uint32_t v[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int y = 2 * (s & 1) + (j >> 1), x = 2 * (j & 1);
                    const int lo = clip3(round_mv(x * (dh * 4) + y * (dv * 4) - 6 * (dh + dv), 8), -31, 31);
                    const int hi = clip3(round_mv((x + 1) * (dh * 4) + y * (dv * 4) - 6 * (dh + dv), 8), -31, 31);
                    v[j] = ((uint32_t)lo & 0xffff) | (uint32_t)hi << 16;
                }
                uint8_t *cu = (uint8_t *)(cus + lp.x);
                gst<uint4>(cu + offsetof(vvc355_affine_cu, diff_mv) + 16 * s, make_uint4(v[0], v[1], v[2], v[3]));
                if (s == 0)
                    gst<uint8_t>(cu + offsetof(vvc355_affine_cu, prof_flags), (uint8_t)flags);
            }
        }
        __syncthreads();
        // one lane per unit, raster order within the CTU: the units this chunk's records painted
        for (int i = threadIdx.x; i < n_units; i += 256) {
            const int dy = i >> lw, dx = i & (side - 1);
            const int gx = (ox >> 2) + dx, gy = (oy >> 2) + dy;
            const uint16_t im = map[i];
            const int k = (int)im - (c0 - first);
            if (im == kNoRec || k < 0 || k >= nc || gx >= pw || gy >= ph)
                continue;
            unit_entry(F, units + c0 + k, heads[k], gx, gy);
        }
    }
}

// the frame as the header states it: every refusal before any HIP call
static int mvf_unit_frame_check(const vvc355_mvf_unit_frame *f)
{
    if (!f)
        return VVC355_MVF_UNIT_E_FRAME;
    if (f->width <= 0 || f->height <= 0 || (f->width & 3) || (f->height & 3) || f->width > 32764 || f->height > 32764)
        return VVC355_MVF_UNIT_E_SIZE;
    if (f->n_units < 0 || f->n_affine_cus < 0)
        return VVC355_MVF_UNIT_E_COUNT;
    if (f->ctb_log2 < 5 || f->ctb_log2 > 7)
        return VVC355_MVF_UNIT_E_CTB;
    const int ctb = 1 << f->ctb_log2;
    if (f->ctb_width != (f->width + ctb - 1) >> f->ctb_log2 || f->ctb_height != (f->height + ctb - 1) >> f->ctb_log2)
        return VVC355_MVF_UNIT_E_GRID;
    if (f->mvf_pitch < f->width / 4)
        return VVC355_MVF_UNIT_E_PITCH;
    if (f->n_units > 0 && (!f->units || (f->units & 15) || !f->ctu_first || (f->ctu_first & 3) || !f->mvf || (f->mvf & 7)))
        return VVC355_MVF_UNIT_E_RECORDS;
    if (f->n_affine_cus > 0 && (!f->affine_cus || (f->affine_cus & 15)))
        return VVC355_MVF_UNIT_E_AFFINE;
    return 0;
}

} // namespace vvc355

extern "C" {

int vvc355_mvf_unit_pass(void *stream, const vvc355_mvf_unit_frame *frame_dev, const vvc355_mvf_unit_frame *frame_host)
{
    const int err = frame_dev ? vvc355::mvf_unit_frame_check(frame_host) : VVC355_MVF_UNIT_E_FRAME;
    if (err)
        return err;
    if (frame_host->n_units == 0)
        return 0;
    hipLaunchKernelGGL(vvc355::mvf_unit_kernel, dim3(frame_host->ctb_width * frame_host->ctb_height), dim3(256), 0, (hipStream_t)stream, frame_dev);
    HIP_CHECK(hipGetLastError());
    return 0;
}

int vvc355_mvf_unit_check(const vvc355_mvf_unit *rec, const vvc355_mvf_unit_frame *frame, int ctu_rs)
{
    if (!rec || !frame || frame->ctb_log2 < 5 || frame->ctb_log2 > 7 || frame->ctb_width <= 0 || frame->ctb_height <= 0 || ctu_rs < 0 ||
        ctu_rs >= frame->ctb_width * frame->ctb_height)
        return -1;
    uint32_t hd[4];
    memcpy(hd, rec, sizeof(hd));
    const int ry = ctu_rs / frame->ctb_width, rx = ctu_rs - ry * frame->ctb_width;
    return vvc355::mvf_unit_rule(hd[0], hd[1], hd[2], hd[3], rec->body[5] & 0xff, rec->body[11] & 0xff, frame->width, frame->height,
                                 rx << frame->ctb_log2, ry << frame->ctb_log2, 1 << frame->ctb_log2, frame->n_affine_cus);
}

} // extern "C"
