// vvc355_picture_pass: the launch sequence of a picture's record-path stages as one host call (see include/vvc_mi355.h).  The reference
// spreads the same order over its per-CTU task stages (libavcodec/vvc/vvc_thread.c:432-565: run_inter .. run_alf) and their progress
// waits; here the stages are whole-picture launches on one stream, the waits on reference pictures are events.
#include "runtime.hpp"
#include "stage_checks.hpp"
#include "../../include/vvc_mi355.h"

namespace {

template <typename T> inline const T *host_of(const vvc355_stage_ref &r) { return (const T *)(uintptr_t)r.host; }
template <typename T> inline const T *dev_of(const vvc355_stage_ref &r) { return (const T *)(uintptr_t)r.dev; }

inline int pic_error(int stage, int code) { return VVC355_PIC_ERROR(stage, code); }

// every code a stage can return must fit the low 8 bits of the picture's return value
static_assert(-VVC355_INTRA_TB_E_MODE < 256 && -VVC355_INTER_TB_E_ORDER < 256 && -VVC355_TS_TB_E_ORDER < 256 && -VVC355_CIIP_E_CMDS < 256 &&
              -VVC355_BS_REC_E_OUTPUT < 256 && -VVC355_QP_REC_E_OUTPUT < 256 && -VVC355_LMCS_FRAME_E_TABLES < 256 &&
              -VVC355_RECON_ORDER_E_DEPENDENCY < 256 && -VVC355_PIC_E_CAPTURE < 256, "stage codes are 8 bits of vvc355_picture_pass's return value");
static_assert(sizeof(vvc355_picture) == 568, "vvc355_picture has no implicit padding");

// The whole picture before the first launch.  `capturing` is asked for (one HIP query, no launch) only when the picture has events.
int picture_check(void *stream, int bd, const vvc355_picture &p)
{
    const bool split = p.lmcs_scale.host != 0;            // chroma residual scaling: the TB passes run per channel type
    // ---- the picture's own rules
    if (p.n_refs < 0 || p.n_refs > 32)
        return pic_error(VVC355_PIC_STAGE_PICTURE, VVC355_PIC_E_REFS);
    for (int i = 0; i < p.n_refs; i++)
        if (!p.refs[i])
            return pic_error(VVC355_PIC_STAGE_PICTURE, VVC355_PIC_E_REFS);
    if (p.ciip.host && host_of<vvc355_ciip_frame>(p.ciip)->cmds &&
        (!p.recon.host || host_of<vvc355_ciip_frame>(p.ciip)->cmds != host_of<vvc355_recon_frame>(p.recon)->cmds))
        return pic_error(VVC355_PIC_STAGE_PICTURE, VVC355_PIC_E_CIIP_CMDS);
    const uint64_t tables[2] = { p.inter_tb.host ? host_of<vvc355_inter_tb_frame>(p.inter_tb)->scale_table : 0,
                                 p.ts_tb.host ? host_of<vvc355_ts_tb_frame>(p.ts_tb)->scale_table : 0 };
    for (const uint64_t t : tables)
        if (t && (!split || t != host_of<vvc355_lmcs_scale_frame>(p.lmcs_scale)->scale))
            return pic_error(VVC355_PIC_STAGE_PICTURE, VVC355_PIC_E_SCALE_TABLE);

    // ---- a stage that is given needs its device descriptor
    const struct { const vvc355_stage_ref *r; int stage; } all[] = {
        { &p.tab_fill, VVC355_PIC_STAGE_TAB_FILL }, { &p.inter, VVC355_PIC_STAGE_INTER }, { &p.affine, VVC355_PIC_STAGE_AFFINE },
        { &p.gpm, VVC355_PIC_STAGE_GPM }, { &p.ciip, VVC355_PIC_STAGE_CIIP }, { &p.intra_tb, VVC355_PIC_STAGE_INTRA_TB },
        { &p.bs_rec, VVC355_PIC_STAGE_BS_REC }, { &p.qp_rec, VVC355_PIC_STAGE_QP_REC }, { &p.alf, VVC355_PIC_STAGE_ALF },
        { &p.inter_tb, VVC355_PIC_STAGE_INTER_TB }, { &p.ts_tb, VVC355_PIC_STAGE_TS_TB }, { &p.lmcs_scale, VVC355_PIC_STAGE_LMCS_SCALE },
        { &p.recon, VVC355_PIC_STAGE_RECON }, { &p.lmcs, VVC355_PIC_STAGE_LMCS }, { &p.deblock_v, VVC355_PIC_STAGE_DEBLOCK_V },
        { &p.deblock_h, VVC355_PIC_STAGE_DEBLOCK_H }, { &p.sao, VVC355_PIC_STAGE_SAO },
    };
    for (const auto &s : all)
        if (s.r->host && !s.r->dev)
            return pic_error(s.stage, VVC355_PIC_E_NO_DEVICE_FRAME);
    if (p.alf.host && !p.alf_work)
        return pic_error(VVC355_PIC_STAGE_ALF, VVC355_PIC_E_NO_DEVICE_FRAME);

    // ---- every stage's own host check, in launch order
    int err;
    if (p.ciip.host && (err = vvc355::ciip_frame_check(host_of<vvc355_ciip_frame>(p.ciip), bd)))
        return pic_error(VVC355_PIC_STAGE_CIIP, err);
    if (p.intra_tb.host && (err = vvc355::intra_tb_check(host_of<vvc355_intra_tb_frame>(p.intra_tb))))
        return pic_error(VVC355_PIC_STAGE_INTRA_TB, err);
    if (p.bs_rec.host && (err = vvc355::bs_rec_check(host_of<vvc355_bs_rec_frame>(p.bs_rec))))
        return pic_error(VVC355_PIC_STAGE_BS_REC, err);
    if (p.qp_rec.host && (err = vvc355::qp_rec_check(host_of<vvc355_qp_rec_frame>(p.qp_rec))))
        return pic_error(VVC355_PIC_STAGE_QP_REC, err);
    for (int pass = 0; pass < (split ? 2 : 1); pass++) {
        const int ch = split ? 1 << pass : 3;
        if (p.inter_tb.host && (err = vvc355::inter_tb_check(host_of<vvc355_inter_tb_frame>(p.inter_tb), ch)))
            return pic_error(VVC355_PIC_STAGE_INTER_TB, err);
        if (p.ts_tb.host && (err = vvc355::ts_tb_check(host_of<vvc355_ts_tb_frame>(p.ts_tb), ch)))
            return pic_error(VVC355_PIC_STAGE_TS_TB, err);
    }
    if (p.recon.host && p.recon_ctus_host && p.recon_order_host) {
        const vvc355_recon_frame *r = host_of<vvc355_recon_frame>(p.recon);
        if ((err = vvc355_recon_order_check((const vvc355_recon_ctu *)(uintptr_t)p.recon_ctus_host, r->ctb_width, r->ctb_height,
                                            (const int32_t *)(uintptr_t)p.recon_order_host, r->n_work)))
            return pic_error(VVC355_PIC_STAGE_RECON_ORDER, err);
    }
    if (p.lmcs.host && (err = vvc355::lmcs_frame_check(host_of<vvc355_lmcs_frame>(p.lmcs), bd)))
        return pic_error(VVC355_PIC_STAGE_LMCS, err);

    // ---- events and graph capture do not mix: a captured wait would tie the graph to one event
    if (p.n_refs > 0 || p.done) {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        HIP_CHECK(hipStreamIsCapturing((hipStream_t)stream, &st));
        if (st != hipStreamCaptureStatusNone)
            return pic_error(VVC355_PIC_STAGE_PICTURE, VVC355_PIC_E_CAPTURE);
    }
    return 0;
}

} // namespace

extern "C" int vvc355_picture_pass(void *stream, int bd, const vvc355_picture *pic)
{
    if (!pic)
        return pic_error(VVC355_PIC_STAGE_PICTURE, VVC355_PIC_E_PICTURE);
    const vvc355_picture &p = *pic;
    const int err = picture_check(stream, bd, p);
    if (err)
        return err;
    const bool split = p.lmcs_scale.host != 0;

    // ---- before the reference waits: everything that reads only uploaded records
    if (p.tab_fill.host)
        vvc355_tab_fill_pass(stream, dev_of<vvc355_tab_fill>(p.tab_fill), host_of<vvc355_tab_fill>(p.tab_fill));
    if (p.inter.host)
        vvc355_inter_frame_build(stream, dev_of<vvc355_inter_frame>(p.inter), host_of<vvc355_inter_frame>(p.inter));
    if (p.affine.host)
        vvc355_affine_frame_build(stream, dev_of<vvc355_affine_frame>(p.affine), host_of<vvc355_affine_frame>(p.affine));
    if (p.gpm.host)
        vvc355_gpm_frame_build(stream, dev_of<vvc355_gpm_frame>(p.gpm), host_of<vvc355_gpm_frame>(p.gpm));
    if (p.ciip.host)
        vvc355_ciip_frame_build(stream, dev_of<vvc355_ciip_frame>(p.ciip), host_of<vvc355_ciip_frame>(p.ciip));
    if (p.intra_tb.host)
        vvc355_intra_tb_pass(stream, dev_of<vvc355_intra_tb_frame>(p.intra_tb), host_of<vvc355_intra_tb_frame>(p.intra_tb));
    if (p.bs_rec.host)
        vvc355_deblock_bs_rec_pass(stream, dev_of<vvc355_bs_rec_frame>(p.bs_rec), host_of<vvc355_bs_rec_frame>(p.bs_rec));
    if (p.qp_rec.host)
        vvc355_deblock_qp_rec_pass(stream, dev_of<vvc355_qp_rec_frame>(p.qp_rec), host_of<vvc355_qp_rec_frame>(p.qp_rec));
    if (p.alf.host)
        vvc355_alf_frame_build(stream, bd, dev_of<vvc355_alf_frame>(p.alf), host_of<vvc355_alf_frame>(p.alf), (void *)(uintptr_t)p.alf_work);

    for (int i = 0; i < p.n_refs; i++)
        vvc355_stream_wait_event(stream, (void *)(uintptr_t)p.refs[i]);

    // ---- after them
    if (p.inter.host)
        vvc355_inter_frame_predict(stream, bd, dev_of<vvc355_inter_frame>(p.inter), host_of<vvc355_inter_frame>(p.inter));
    if (p.affine.host)
        vvc355_affine_frame_predict(stream, bd, dev_of<vvc355_affine_frame>(p.affine), host_of<vvc355_affine_frame>(p.affine));
    if (p.gpm.host)
        vvc355_gpm_frame_predict(stream, bd, dev_of<vvc355_gpm_frame>(p.gpm), host_of<vvc355_gpm_frame>(p.gpm));
    if (p.ciip.host)
        vvc355_ciip_frame_predict(stream, bd, dev_of<vvc355_ciip_frame>(p.ciip), host_of<vvc355_ciip_frame>(p.ciip));
    for (int pass = 0; pass < (split ? 2 : 1); pass++) {
        const int channels = split ? 1 << pass : 3;
        if (pass == 1)          // the scale table is made from the luma the first calls reconstructed
            vvc355_lmcs_vpdu_scale_pass(stream, bd, dev_of<vvc355_lmcs_scale_frame>(p.lmcs_scale), host_of<vvc355_lmcs_scale_frame>(p.lmcs_scale));
        if (p.inter_tb.host)
            vvc355_inter_tb_pass(stream, dev_of<vvc355_inter_tb_frame>(p.inter_tb), host_of<vvc355_inter_tb_frame>(p.inter_tb), channels);
        if (p.ts_tb.host)
            vvc355_ts_tb_pass(stream, dev_of<vvc355_ts_tb_frame>(p.ts_tb), host_of<vvc355_ts_tb_frame>(p.ts_tb), channels);
    }
    if (p.recon.host)
        vvc355_recon_frame_pass(stream, bd, dev_of<vvc355_recon_frame>(p.recon), host_of<vvc355_recon_frame>(p.recon));
    if (p.lmcs.host)
        vvc355_lmcs_frame_pass(stream, bd, dev_of<vvc355_lmcs_frame>(p.lmcs), host_of<vvc355_lmcs_frame>(p.lmcs));
    if (p.deblock_v.host)
        vvc355_deblock_frame_pass(stream, bd, dev_of<vvc355_deblock_frame>(p.deblock_v), host_of<vvc355_deblock_frame>(p.deblock_v));
    if (p.deblock_h.host)
        vvc355_deblock_frame_pass(stream, bd, dev_of<vvc355_deblock_frame>(p.deblock_h), host_of<vvc355_deblock_frame>(p.deblock_h));
    if (p.sao.host)
        vvc355_sao_frame_pass(stream, bd, dev_of<vvc355_sao_frame>(p.sao), host_of<vvc355_sao_frame>(p.sao));
    if (p.alf.host)
        vvc355_alf_frame_filter(stream, bd, host_of<vvc355_alf_frame>(p.alf), (const void *)(uintptr_t)p.alf_work);
    if (p.done)
        vvc355_event_record((void *)(uintptr_t)p.done, stream);
    return 0;
}
