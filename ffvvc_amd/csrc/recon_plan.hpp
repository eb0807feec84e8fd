// RECON stage driver: a command's plan — everything the walk needs from a command that depends on the command, the availability
// pre-pass's answers and the CTU's context alone, and on no sample.  The walk of a CTU is a chain of dependent blocks run by one
// wave, so whatever it derives per block in scalar code is paid once per link of the chain; the plan is derived by one LANE per
// command instead, for the 64 commands of a window at once, when the window is loaded (recon_one_ctu, load_window), and written
// over the command's slot in LDS.  It never leaves LDS: the commands in HBM stay as the host wrote them (pad bytes aside).
//
// Part of intra.hip (included after the mode helpers, IntraSetup, ReconCtx and wide_angle_mode); host + device, so that the same
// text is checked on the CPU (vvc355_recon_plan_host, tests/test_recon_plan_cpu.py).
//
// A plan is ten dwords, like the command.  Every kind keeps dword 6 (mode | kind << 8 | c_idx << 16 | ref_idx << 24; PRED: the mode
// after the wide-angle mapping, ref_idx 0 for chroma) where the walk's dispatch and its look-ahead read the kind.
//
//   PRED   0  offset of the block's sample (0, 0) from the component accessor's origin, in pixels (y * pitch + x)
//          1  x | w << 16 | h << 24                       (component samples)
//          2  angle | inv << 16                            (both int16)
//          3  uleft | utop << 16        4  la | ta << 16   5  refw | refh << 16        7  left_size | top_size << 16
//          8  nscale (int8) | mip_mode << 8 | flags << 16: kPlanPdpc ... kPlanTwin below, variant << 10 (pred_angular_q's case for a
//             directional mode, pred_simple_q's otherwise)
//          9  ref_line (int8)
//   CCLM   the command, with dword 7 = avail_l | avail_t << 8 | ctu_boundary << 16 (the rest of vvc355_cclm_job is dwords 2, 3, 6, 9)
//   RESID, CIIP (one layout)
//          0-1 the resid pointer, 3 and 8-9 as in the command (the walk's prefetch reads 0, 1, 3 of the NEXT command)
//          2  offset of the block's sample (0, 0), as for PRED
//          4  ilog2(w) | c_idx << 8 (the stride selector) | joint << 16 | scaled << 24          (w in component samples)
//          5  n = samples of the block                     7  origin of the coding unit's 64x64 unit (x | y << 16, luma samples)
#pragma once

namespace vvc355 {

struct ReconPlan { uint32_t d[10]; };
static_assert(sizeof(ReconPlan) == sizeof(vvc355_recon_cmd), "a plan takes its command's slot in the walk's window");

// what the planner needs of the picture: chroma shifts, CTU size, the pitches (pixels) of the luma and chroma accessors the walk
// runs on, and whether it runs on LDS tiles (the rows above a CTU are then a strip of their own)
struct ReconPlanFrame { int hs, vs, ctb_log2, pitch[2]; bool tile; };

enum { kPlanPdpc = 1, kPlanSmooth = 2, kPlanFilter = 4, kPlanUpLeft = 8, kPlanStrip = 16, kPlanMip = 32, kPlanMipT = 64, kPlanQuads = 128,
       kPlanDirectional = 256, kPlanTwin = 512, kPlanVariantShift = 10 };

// Cb and Cr of a coding unit are predicted by two consecutive commands that differ in c_idx only (predict_intra, vvc_intra.c:263-264):
// q = a command's dwords, qn = the next command's.  (The pad bytes in dword 8 are the pre-pass's: zero for every PRED.)
__host__ __device__ inline bool recon_plan_twin(const uint32_t *q, const uint32_t *qn)
{
    if (((q[6] >> 8) & 0xff) != VVC355_RECON_PRED || ((q[6] >> 16) & 0xff) != 1)
        return false;
    bool same = qn[6] == ((q[6] & ~0xff0000u) | 0x020000u);
    for (int i = 2; i < 9; i++)
        if (i != 6)
            same = same && qn[i] == q[i];
    return same;
}

// twin: the command and its right-hand neighbour go through one pass, half a wave each (decides `quads`)
template <typename TB>
__host__ __device__ inline ReconPlan recon_plan(const uint32_t *q, bool twin, const ReconPlanFrame &F, const ReconCtx &cx, TB tabs)
{
    ReconPlan P;
    for (int i = 0; i < 10; i++)
        P.d[i] = q[i];
    const int x0 = (int16_t)(q[2] & 0xffff), y0 = (int16_t)(q[2] >> 16), cw = (int16_t)(q[3] & 0xffff), ch = (int16_t)(q[3] >> 16);
    const int cu_x0 = (int16_t)(q[4] & 0xffff), cu_y0 = (int16_t)(q[4] >> 16);
    const int kind = (q[6] >> 8) & 0xff, c_idx = (q[6] >> 16) & 0xff;
    const int hs = c_idx ? F.hs : 0, vs = c_idx ? F.vs : 0, pitch = F.pitch[c_idx ? 1 : 0];
    const int ctb = 1 << F.ctb_log2, ctb_mask = ctb - 1;
    if (kind == VVC355_RECON_PRED) {
        const int x = x0 >> hs, y = y0 >> vs, w = cw >> hs, h = ch >> vs;
        const int isp_split = (q[7] >> 24) & 0xff;
        vvc355_intra_job j = {};
        j.x = (int16_t)x; j.y = (int16_t)y; j.w = (int16_t)w; j.h = (int16_t)h;
        j.cb_width = (int16_t)(q[5] & 0xffff); j.cb_height = (int16_t)(q[5] >> 16);
        j.mode = (int16_t)wide_angle_mode(isp_split, c_idx, w, h, j.cb_width, j.cb_height, (int8_t)(q[6] & 0xff));
        j.left_avail = (int16_t)(q[9] & 0xffff);
        j.top_avail = (int16_t)(q[9] >> 16);
        j.c_idx = (uint8_t)c_idx; j.ref_idx = c_idx ? 0 : (uint8_t)(q[6] >> 24);
        j.is_mip = (uint8_t)(q[7] & 0xff); j.mip_mode = (uint8_t)((q[7] >> 8) & 0xff); j.mip_transposed = (uint8_t)((q[7] >> 16) & 0xff);
        j.isp_split = (uint8_t)isp_split; j.bdpcm_flag = (uint8_t)(q[8] & 0xff);
        {   // ff_vvc_set_neighbour_available (vvc_ctu.c:2497-2510), luma coordinates
            const int x0b = x0 & ctb_mask, y0b = y0 & ctb_mask;
            const bool cand_up = cx.ctb_up || y0b, cand_left = cx.ctb_left || x0b;
            j.cand_up_left = (x0b || y0b) ? (cand_left && cand_up) : (cx.ctb_up_left != 0);
        }
        IntraSetup s = intra_pred_setup<64>(j, pitch, tabs);
        if (twin)
            s.quads = intra_quads(32, w, h, s.directional, s.mode);
        const bool strip = F.tile && (y & ((ctb >> vs) - 1)) == 0;        // the block sits on the CTU's top edge: the rows above it are the strip
        const uint32_t flags = (s.need_pdpc ? kPlanPdpc : 0) | (s.smooth ? kPlanSmooth : 0) | (s.filter_flag ? kPlanFilter : 0) | (s.cand_up_left ? kPlanUpLeft : 0) |
                               (strip ? kPlanStrip : 0) | (s.is_mip ? kPlanMip : 0) | (s.mip_transposed ? kPlanMipT : 0) | (s.quads ? kPlanQuads : 0) |
                               (s.directional ? kPlanDirectional : 0) | (twin ? kPlanTwin : 0) | ((uint32_t)s.variant << kPlanVariantShift);
        P.d[0] = (uint32_t)s.src_off;
        P.d[1] = (uint32_t)(uint16_t)x | (uint32_t)w << 16 | (uint32_t)h << 24;
        P.d[2] = (uint32_t)(uint16_t)s.angle | (uint32_t)(uint16_t)s.inv << 16;
        P.d[3] = (uint32_t)s.uleft | (uint32_t)s.utop << 16;
        P.d[4] = (uint32_t)s.la | (uint32_t)s.ta << 16;
        P.d[5] = (uint32_t)s.refw | (uint32_t)s.refh << 16;
        P.d[6] = (uint32_t)(uint8_t)s.mode | (uint32_t)kind << 8 | (uint32_t)c_idx << 16 | (uint32_t)s.ref_idx << 24;
        P.d[7] = (uint32_t)s.left_size | (uint32_t)s.top_size << 16;
        P.d[8] = (uint32_t)(uint8_t)s.nscale | (uint32_t)s.mip_mode << 8 | flags << 16;
        P.d[9] = (uint32_t)(uint8_t)s.ref_line;
    } else if (kind == VVC355_RECON_CCLM) {
        P.d[7] = ((q[8] >> 16) & 1) | ((q[8] >> 17) & 1) << 8 | (uint32_t)((y0 & ctb_mask) == 0) << 16;
    } else if (kind == VVC355_RECON_RESID || kind == VVC355_RECON_CIIP) {
        // RESID: w, h are the transform block's (component samples); CIIP: the coding unit's (luma samples)
        const int w = kind == VVC355_RECON_CIIP ? cw >> hs : cw, h = kind == VVC355_RECON_CIIP ? ch >> vs : ch;
        const int joint = (q[8] >> 8) & 0xff, size_y = ctb < 64 ? ctb : 64;
        P.d[2] = (uint32_t)((y0 >> vs) * pitch + (x0 >> hs));
        P.d[4] = (uint32_t)ilog2i(w) | (uint32_t)c_idx << 8 | (uint32_t)joint << 16 | (uint32_t)(kind == VVC355_RECON_RESID && (joint & 8)) << 24;
        P.d[5] = (uint32_t)(w * h);
        P.d[7] = (uint32_t)(uint16_t)(cu_x0 & ~(size_y - 1)) | (uint32_t)(uint16_t)(cu_y0 & ~(size_y - 1)) << 16;
    }
    return P;
}

// a PRED plan back into the set-up intra_pred_run takes (the walk: p = the plan's dwords, wave-uniform)
__host__ __device__ inline IntraSetup recon_plan_setup(const uint32_t *p)
{
    IntraSetup s;
    const uint32_t fl = p[8] >> 16;
    s.src_off = (int)p[0];
    s.x = (int16_t)(p[1] & 0xffff); s.w = (int)((p[1] >> 16) & 0xff); s.h = (int)(p[1] >> 24);
    s.angle = (int16_t)(p[2] & 0xffff); s.inv = (int16_t)(p[2] >> 16);
    s.uleft = (int)(p[3] & 0xffff); s.utop = (int)(p[3] >> 16);
    s.la = (int)(p[4] & 0xffff); s.ta = (int)(p[4] >> 16);
    s.refw = (int)(p[5] & 0xffff); s.refh = (int)(p[5] >> 16);
    s.mode = (int8_t)(p[6] & 0xff); s.c_idx = (int)((p[6] >> 16) & 0xff); s.ref_idx = (int)(p[6] >> 24);
    s.left_size = (int)(p[7] & 0xffff); s.top_size = (int)(p[7] >> 16);
    s.nscale = (int8_t)(p[8] & 0xff); s.mip_mode = (int)((p[8] >> 8) & 0xff);
    s.need_pdpc = (fl & kPlanPdpc) != 0; s.smooth = (fl & kPlanSmooth) != 0; s.filter_flag = (fl & kPlanFilter) != 0;
    s.cand_up_left = (fl & kPlanUpLeft) != 0; s.is_mip = (fl & kPlanMip) != 0; s.mip_transposed = (fl & kPlanMipT) != 0;
    s.quads = (fl & kPlanQuads) != 0; s.directional = (fl & kPlanDirectional) != 0;
    s.variant = (int)((fl >> kPlanVariantShift) & 7);
    s.ref_line = (int8_t)(p[9] & 0xff);
    return s;
}

} // namespace vvc355
