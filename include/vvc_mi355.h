/*
 * vvc_mi355.h — C ABI of libvvc_mi355.so: hand-written HIP (gfx950 / MI355X) kernels behind the
 * VVCDSPContext function-pointer surface of the ffvvc decoder.
 *
 * Two ways in:
 *
 *  (1) Synchronous per-slot entries, `vvc355_<slot>(int bd, ...)`: HOST pointers, same argument order
 *      and meaning as the reference slot they replace (cited per entry, paths relative to the
 *      reference tree), with the bit depth the reference binds at ff_vvc_dsp_init() time
 *      (libavcodec/vvc/vvcdsp.c:228) passed first, and table indices ([luma/chroma][frac][frac], [h/v])
 *      passed as leading ints.  They stage the touched rectangle to the GPU, run the kernel and copy
 *      the result back: drop-in and bit-exact, meant for the function-pointer table
 *      (ffvvc_amd/host/dsp_init_mi355.c) and for checkasm-style parity — not for speed.
 *
 *  (2) Batched entries, `vvc355_<stage>_batch(stream, bd, jobs_dev, n_jobs)`: DEVICE-resident planes
 *      and a device array of POD job descriptors — one launch per stage for many CTUs.  This is the
 *      performance path (SURVEY §7 "batched API").
 *
 * Every entry returns void like the slot it replaces (no error channel, vvcdsp.h:48-158); a HIP
 * failure or an argument outside the slot's domain prints a message and abort()s.
 */
#ifndef VVC_MI355_H
#define VVC_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ runtime helpers (runtime_api.cpp) */
/* Device count / selection and plain device memory, for C hosts that keep frames resident in HBM. */
int   vvc355_device_count(void);
/* Error policy of the batched / frame entries (the void slots have no error channel: vvcdsp.h).  Default 0: a HIP failure prints
 * and aborts.  With 1 the first failure is recorded instead — the entry goes on, later HIP calls fail too — and the host checks
 * vvc355_last_error() (a hipError_t value, 0 = none) after a stage or at its stream synchronisation. */
void  vvc355_set_error_policy(int record_instead_of_abort);
int   vvc355_last_error(void);
const char *vvc355_last_error_string(void);
void  vvc355_clear_error(void);
void  vvc355_set_device(int ordinal);           /* process-wide: also the device of every thread that calls a slot afterwards */
void *vvc355_malloc(size_t bytes);
void  vvc355_free(void *dev);
void  vvc355_upload(void *dev, const void *host, size_t bytes);
void  vvc355_download(void *host, const void *dev, size_t bytes);
void  vvc355_copy_async(void *stream, void *dst_dev, const void *src_dev, size_t bytes);   /* device to device, stream-ordered */
/* Pinned host memory and the stream-ordered download into it: the copy is queued behind the work already on `stream` and the call returns
 * at once; `host` holds the bytes after vvc355_stream_sync(stream) or an event recorded behind the copy.  `host` comes from
 * vvc355_host_alloc (into pageable memory the runtime stages the copy and the call may block). */
void *vvc355_host_alloc(size_t bytes);
void  vvc355_host_free(void *host);
void  vvc355_download_async(void *stream, void *host, const void *dev, size_t bytes);
void *vvc355_stream_create(void);
void  vvc355_stream_destroy(void *stream);
void  vvc355_stream_sync(void *stream);          /* NULL = the default stream */
/* A frame's launch sequence as a hipGraph: every batched / stage-driver entry called on `stream` between begin and end is
 * recorded instead of run (stream = one made by vvc355_stream_create, not the default stream); the returned executable graph
 * replays the whole sequence with one launch.  The descriptors the entries were given must stay alive and unchanged. */
void  vvc355_graph_begin(void *stream);
void *vvc355_graph_end(void *stream);
void  vvc355_graph_launch(void *graph_exec, void *stream);
void  vvc355_graph_destroy(void *graph_exec);
/* Events: how one picture waits for another across streams — what the reference does with ff_vvc_report_progress / ff_vvc_add_progress_listener
 * (libavcodec/vvc/vvc_refs.c:532, :552; vvc_thread.c:252) on the host.  Created with timing disabled.  vvc355_event_query: 1 = everything recorded before the
 * event has finished, 0 = not yet.  All under the error policy above. */
void *vvc355_event_create(void);
void  vvc355_event_destroy(void *event);
void  vvc355_event_record(void *event, void *stream);
void  vvc355_stream_wait_event(void *stream, void *event);
int   vvc355_event_query(void *event);
const char *vvc355_version(void);

/* ------------------------------------------------------------------ constant tables (tables.cpp) */
/* H.266 tables, flat: the same data libavcodec/vvc/vvc_data.c:1735 (luma [3][16][8]) and :1798 (chroma [3][32][4]) hold */
extern const int8_t vvc355_tab_inter_luma_filters[3 * 16 * 8];
extern const int8_t vvc355_tab_inter_chroma_filters[3 * 32 * 4];
extern const int16_t vvc355_tab_alf_fix_filt_coeff[64 * 12];          /* vvc_data.c:1644 */
extern const uint8_t vvc355_tab_alf_class_to_filt_map[16 * 25];       /* vvc_data.c:1712 */
extern const uint8_t vvc355_tab_alf_aps_class_to_filt_map[25];        /* vvc_data.c:1731 */
/* the tables the reference keeps inline in its .c files, as the kernels use them (ffvvc_amd/csrc/tables_small.inc) */
extern const uint16_t vvc355_tab_tc_table[66];                        /* tctable, vvc_filter.c:38 */
extern const uint8_t vvc355_tab_beta_table[64];                       /* betatable, vvc_filter.c:47 */
extern const int16_t vvc355_tab_intra_angles[31];                     /* angles[], vvc_intra.c:667 */
extern const uint8_t vvc355_tab_level_scale[12];                      /* level_scale[2][6], vvc_intra.c:329 */
extern const int8_t  vvc355_tab_ref_filter_modes[12];                 /* modes[], vvc_intra.c:657 */
extern const uint8_t vvc355_tab_intra_filter_thres[5];                /* intra_hor_ver_dist_thres[], vvc_intra_template.c:559 */
extern const uint8_t vvc355_tab_cclm_div_sig[16];                     /* div_sig_table[], vvc_intra_template.c:261 */
extern const uint8_t vvc355_tab_alf_arg_var[16];                      /* arg_var[], vvc_filter_template.c:272 */
extern const uint8_t vvc355_tab_alf_transpose_index[48];              /* index[4][12], vvc_filter_template.c:387 */
extern const uint8_t vvc355_tab_diag_scan_4x4_x[16], vvc355_tab_diag_scan_4x4_y[16];      /* ff_vvc_diag_scan_x / _y [2][2], vvc_data.c:27,152 */
extern const uint8_t vvc355_tab_gpm_angle_idx[64];                    /* ff_vvc_gpm_angle_idx, vvc_data.c:1998 (partition -> angleIdx) */
extern const uint8_t vvc355_tab_gpm_distance_idx[64];                 /* ff_vvc_gpm_distance_idx, vvc_data.c:2005 (partition -> distanceIdx) */
extern const int8_t  vvc355_tab_gpm_distance_lut[32];                 /* ff_vvc_gpm_distance_lut, vvc_data.c:2012 (disLut) */

/* ------------------------------------------------------------------ ALF (alf.hip) */

/*
 * One ALF rectangle (normally one CTB of one component).  Addresses are DEVICE addresses of the
 * rectangle's top-left sample in the destination plane and in the pre-ALF source plane.
 * ext_* = number of samples that may be READ beyond the rectangle on that side of the source
 * (>= 3 luma / 2 chroma means "plain read"; fewer means replicate the last readable sample, which is
 * what the reference's alf_prepare_buffer does at picture / slice / tile edges,
 * libavcodec/vvc/vvc_filter.c:1105-1137).
 */
typedef struct vvc355_alf_job {
    uint64_t dst;
    uint64_t src;            /* luma/chroma: source plane; CC-ALF: the co-located LUMA plane */
    uint64_t coeff;          /* luma slot mode: int16[n4x4][12]; luma fused: int16 coeff_set[][12];
                                chroma: int16[6]; CC: int16[7]; classify-only: int class_idx[n4x4] (output) */
    uint64_t clip;           /* luma slot mode: int16[n4x4][12]; luma fused: uint8 clip_idx_set[25][12];
                                chroma: int16[6]; classify-only: int transpose_idx[n4x4] (output) */
    uint64_t class_to_filt;  /* luma fused: uint8[25] */
    int32_t  dst_stride;     /* bytes */
    int32_t  src_stride;     /* bytes */
    int16_t  w, h;           /* samples; luma/chroma: multiples of 4, <= 128 */
    int16_t  vb_pos;         /* virtual boundary row relative to the rectangle (vvc_filter.c:1305-1314) */
    int8_t   ext_l, ext_r, ext_t, ext_b;
    int8_t   hs, vs;         /* CC-ALF chroma subsampling shifts */
    int8_t   pad_[4];
} vvc355_alf_job;

/* alf.filter[LUMA] over many rectangles; fused != 0 additionally runs alf.classify and
 * alf.recon_coeff_and_clip in the same kernel (what vvc_filter.c:1139-1186 chains per CTB). */
void vvc355_alf_luma_batch(void *stream, int bd, int fused, const vvc355_alf_job *jobs_dev, int n_jobs);
void vvc355_alf_chroma_batch(void *stream, int bd, const vvc355_alf_job *jobs_dev, int n_jobs);
void vvc355_alf_cc_batch(void *stream, int bd, const vvc355_alf_job *jobs_dev, int n_jobs);

/* VVCALFDSPContext.filter[LUMA] — libavcodec/vvc/vvcdsp.h:149, vvc_filter_template.c:43 */
void vvc355_alf_filter_luma(int bd, uint8_t *dst, ptrdiff_t dst_stride, const uint8_t *src, ptrdiff_t src_stride,
    int width, int height, const int16_t *filter, const int16_t *clip, int vb_pos);
/* VVCALFDSPContext.filter[CHROMA] — vvcdsp.h:149, vvc_filter_template.c:137 */
void vvc355_alf_filter_chroma(int bd, uint8_t *dst, ptrdiff_t dst_stride, const uint8_t *src, ptrdiff_t src_stride,
    int width, int height, const int16_t *filter, const int16_t *clip, int vb_pos);
/* VVCALFDSPContext.filter_cc — vvcdsp.h:151, vvc_filter_template.c:223 */
void vvc355_alf_filter_cc(int bd, uint8_t *dst, ptrdiff_t dst_stride, const uint8_t *luma, ptrdiff_t luma_stride,
    int width, int height, int hs, int vs, const int16_t *filter, int vb_pos);
/* VVCALFDSPContext.classify — vvcdsp.h:154, vvc_filter_template.c:299 (gradient_tmp is not touched) */
void vvc355_alf_classify(int bd, int *class_idx, int *transpose_idx, const uint8_t *src, ptrdiff_t src_stride,
    int width, int height, int vb_pos, int *gradient_tmp);
/* VVCALFDSPContext.recon_coeff_and_clip — vvcdsp.h:156, vvc_filter_template.c:383 */
void vvc355_alf_recon_coeff_and_clip(int bd, int16_t *coeff, int16_t *clip, const int *class_idx, const int *transpose_idx,
    int size, const int16_t *coeff_set, const uint8_t *clip_idx_set, const uint8_t *class_to_filt);

/* ------------------------------------------------------------------ inter prediction (inter.hip) */

/* One motion-compensated block: put (kind 0: int16 dst, 14-bit scaled), put_uni (1) or put_uni_w (2).
 * src = DEVICE address of the block's integer-position sample in the reference plane; the kernel reads the
 * 3/4 (luma) or 1/2 (chroma) sample apron the filter needs, so edge emulation (vvc_inter.c:33-110) must already
 * have been applied by whoever built the plane (padded reference planes). */
typedef struct vvc355_mc_job {
    uint64_t dst;
    uint64_t src;
    int32_t  dst_stride;     /* bytes (put slot: 256 = MAX_PB_SIZE int16) */
    int32_t  src_stride;     /* bytes */
    int16_t  w, h;
    int8_t   hf[8], vf[8];   /* filter taps: 8 luma / 4 chroma (dmvr: hf[0] = mx, vf[0] = my) */
    uint8_t  kind, chroma, hfrac, vfrac;
    int16_t  denom, wx, ox;  /* put_uni_w */
    int16_t  pad_;
} vvc355_mc_job;

/* Element-wise work on two operands: mode 0 avg, 1 w_avg, 2 put_ciip (src0 = inter pixels, w0 = intra weight),
 * 3 put_gpm (aux = weight mask, step_x/step_y); also the descriptor of bdof / prof / sad / ring-fetch jobs. */
typedef struct vvc355_blend_job {
    uint64_t dst;
    uint64_t src0;
    uint64_t src1;
    uint64_t aux;
    int32_t  dst_stride, src0_stride, src1_stride;   /* bytes */
    int32_t  step_x, step_y;
    int16_t  w, h, mode, denom, w0, w1, o0, o1;
    int32_t  pad_;
} vvc355_blend_job;

void vvc355_mc_batch(void *stream, int bd, const vvc355_mc_job *jobs_dev, int n_jobs, int max_w, int max_h);
void vvc355_blend_batch(void *stream, int bd, const vvc355_blend_job *jobs_dev, int n_jobs, int max_w, int max_h);
void vvc355_bdof_batch(void *stream, int bd, const vvc355_blend_job *jobs_dev, int n_jobs);

/* VVCInterDSPContext.put[chroma][*][vfrac][hfrac] — vvcdsp.h:49, h2656_inter_template.c:29,97,112,127,342,357,372 */
void vvc355_put(int bd, int chroma, int vfrac, int hfrac, int16_t *dst, const uint8_t *src, ptrdiff_t src_stride,
    int height, const int8_t *hf, const int8_t *vf, int width);
/* .put_uni — vvcdsp.h:53, h2656_inter_template.c:44,154,180,207,401,425,449 */
void vvc355_put_uni(int bd, int chroma, int vfrac, int hfrac, uint8_t *dst, ptrdiff_t dst_stride,
    const uint8_t *src, ptrdiff_t src_stride, int height, const int8_t *hf, const int8_t *vf, int width);
/* .put_uni_w — vvcdsp.h:57, h2656_inter_template.c:60,247,273,299,487,513,540 */
void vvc355_put_uni_w(int bd, int chroma, int vfrac, int hfrac, uint8_t *dst, ptrdiff_t dst_stride,
    const uint8_t *src, ptrdiff_t src_stride, int height, int denom, int wx, int ox,
    const int8_t *hf, const int8_t *vf, int width);
/* .avg / .w_avg — vvcdsp.h:61,64, vvc_inter_template.c:25,42 */
void vvc355_avg(int bd, uint8_t *dst, ptrdiff_t dst_stride, const int16_t *src0, const int16_t *src1, int width, int height);
void vvc355_w_avg(int bd, uint8_t *dst, ptrdiff_t dst_stride, const int16_t *src0, const int16_t *src1, int width, int height,
    int denom, int w0, int w1, int o0, int o1);
/* .put_ciip / .put_gpm — vvcdsp.h:68,71, vvc_inter_template.c:60,78 */
void vvc355_put_ciip(int bd, uint8_t *dst, ptrdiff_t dst_stride, int width, int height,
    const uint8_t *inter, ptrdiff_t inter_stride, int intra_weight);
void vvc355_put_gpm(int bd, uint8_t *dst, ptrdiff_t dst_stride, int width, int height,
    const int16_t *src0, const int16_t *src1, const uint8_t *weights, int step_x, int step_y);
/* .fetch_samples / .bdof_fetch_samples — vvcdsp.h:75,76, vvc_inter_template.c:130,101 */
void vvc355_fetch_samples(int bd, int16_t *dst, const uint8_t *src, ptrdiff_t src_stride, int x_frac, int y_frac);
void vvc355_bdof_fetch_samples(int bd, int16_t *dst, const uint8_t *src, ptrdiff_t src_stride, int x_frac, int y_frac,
    int width, int height);
/* .prof_grad_filter / .apply_prof* — vvcdsp.h:79-87, vvc_inter_template.c:135,160,181,210 */
void vvc355_prof_grad_filter(int bd, int16_t *gradient_h, int16_t *gradient_v, ptrdiff_t gradient_stride,
    const int16_t *src, ptrdiff_t src_stride, int width, int height, int pad);
void vvc355_apply_prof(int bd, int16_t *dst, const int16_t *src, const int16_t *diff_mv_x, const int16_t *diff_mv_y);
void vvc355_apply_prof_uni(int bd, uint8_t *dst, ptrdiff_t dst_stride, const int16_t *src,
    const int16_t *diff_mv_x, const int16_t *diff_mv_y);
void vvc355_apply_prof_uni_w(int bd, uint8_t *dst, ptrdiff_t dst_stride, const int16_t *src,
    const int16_t *diff_mv_x, const int16_t *diff_mv_y, int denom, int wx, int ox);
/* .apply_bdof — vvcdsp.h:89, vvc_inter_template.c:288 (pads src0/src1 in place, like the reference) */
void vvc355_apply_bdof(int bd, uint8_t *dst, ptrdiff_t dst_stride, int16_t *src0, int16_t *src1, int block_w, int block_h);
/* .sad — vvcdsp.h:91, vvcdsp.c:49 (bit-depth independent) */
int  vvc355_sad(const int16_t *src0, const int16_t *src1, int dx, int dy, int block_w, int block_h);
/* .dmvr[vfrac][hfrac] — vvcdsp.h:92, vvc_inter_template.c:324,347,365,384 */
void vvc355_dmvr(int bd, int vfrac, int hfrac, int16_t *dst, const uint8_t *src, ptrdiff_t src_stride, int height,
    intptr_t mx, intptr_t my, int width);

/* ------------------------------------------------------------------ LMCS / SAO / deblock (loopfilter.hip) */

/* One SAO rectangle (a CTB of one component).  type 1 = band (h2656_sao_template.c:24), 2 = edge (:50),
 * 3 = edge + restore fused (what vvc_filter.c:290-293 chains: src = the pre-SAO plane itself, picture-border and
 * slice/tile-edge samples handled per borders[] / *_edge[]), 4 = restore only (:81 / :131). */
typedef struct vvc355_sao_job {
    uint64_t dst;
    uint64_t src;
    int32_t  dst_stride, src_stride;      /* bytes */
    int16_t  w, h;
    int16_t  offset_val[5];               /* SAOParams.offset_val[c_idx] */
    uint8_t  type, eo, band_position, restore;
    uint8_t  borders[4];                  /* left, top, right, bottom picture borders */
    uint8_t  vert_edge[2], horiz_edge[2], diag_edge[4];
    uint8_t  pad_[2];
} vvc355_sao_job;

/* One deblocking call of the reference: 8 samples along an edge (2 luma segments of 4 lines; chroma 2 x 4 or,
 * when subsampled along the edge, 4 x 2).  pix = DEVICE address of q0 of the first line; dir 0 = the [h] slot
 * (horizontal edge), 1 = the [v] slot.  flag = hor_ctu_edge (luma) / shift (chroma). */
typedef struct vvc355_deblock_job {
    uint64_t pix;
    int32_t  stride;                      /* bytes */
    int32_t  beta[4], tc[4];
    uint8_t  no_p[4], no_q[4], max_len_p[4], max_len_q[4];
    uint8_t  dir, chroma, flag, pad_;
} vvc355_deblock_job;

void vvc355_sao_batch(void *stream, int bd, const vvc355_sao_job *jobs_dev, int n_jobs, int max_w, int max_h);
/* fast form of the frame stage: every job type 1 or 3, w <= 128, dst/src addresses and strides multiples of 16 bytes */
void vvc355_sao_ctb_batch(void *stream, int bd, const vvc355_sao_job *jobs_dev, int n_jobs, int max_h);
/* all jobs of one launch must be independent (e.g. every vertical edge of a frame, then every horizontal edge) */
void vvc355_deblock_batch(void *stream, int bd, const vvc355_deblock_job *jobs_dev, int n_jobs);
/* blend_job: dst = luma rectangle (in place), src0 = LUT of 2^bd pixel-typed entries */
void vvc355_lmcs_batch(void *stream, int bd, const vvc355_blend_job *jobs_dev, int n_jobs, int max_w, int max_h);

/*
 * Inverse luma mapping of a whole picture: ff_vvc_lmcs_filter (vvc_filter.c:1322) for every CTB in one launch — lmcs.filter over the CTB's
 * part of the picture with fc->ps.lmcs.inv_lut where the CTB's slice has sh_lmcs_used_flag.  No job array: a workgroup finds its CTB's slice
 * itself.  A CTB whose slice_idx is outside [0, n_slices) is a hole and is left alone, like a CTB of a slice that does not use LMCS.
 * Nothing outside [0, width) x [0, height) is read or written; the pitch padding keeps its bytes.  No implicit padding: 64 bytes.
 */
typedef struct vvc355_lmcs_frame {
    uint64_t plane;          /* DEVICE luma plane, mapped in place */
    uint64_t inv_lut;        /* DEVICE fc->ps.lmcs.inv_lut, 1 << bd pixel-typed entries */
    uint64_t slice_idx;      /* DEVICE int16 per CTB, as in the other frames */
    uint64_t slice_lmcs_used;/* DEVICE uint8 per slice: sh_lmcs_used_flag */
    int32_t  stride, width, height, ctb_width, ctb_height, n_slices;
    uint8_t  ctb_log2, pad_[3];
} vvc355_lmcs_frame;
/* what vvc355_lmcs_frame_pass returns for a frame it refuses: no frame; bd not 8 / 10 / 12; width or height <= 0 or beyond 65535; ctb_log2 outside
 * 5..7; ctb_width / ctb_height not ceil(size >> ctb_log2); a stride smaller than a row, no multiple of the pixel size, 8 MiB or more, or a
 * plane of 2 GiB or more; n_slices < 0; plane, inv_lut, slice_idx or slice_lmcs_used missing */
enum { VVC355_LMCS_FRAME_E_FRAME = -1, VVC355_LMCS_FRAME_E_BD = -2, VVC355_LMCS_FRAME_E_SIZE = -3, VVC355_LMCS_FRAME_E_CTB = -4,
       VVC355_LMCS_FRAME_E_GRID = -5, VVC355_LMCS_FRAME_E_STRIDE = -6, VVC355_LMCS_FRAME_E_COUNT = -7, VVC355_LMCS_FRAME_E_TABLES = -8 };
/* One launch on `stream`.  The host copy of the frame is checked before any HIP call.
 * returns 0, or a negative VVC355_LMCS_FRAME_E_* with NOTHING launched */
int vvc355_lmcs_frame_pass(void *stream, int bd, const vvc355_lmcs_frame *frame_dev, const vvc355_lmcs_frame *frame_host);

/*
 * The checksums of a decoded picture, computed where the picture lies: one streaming read of the planes gives the number the framecrc
 * muxer prints for the picture and two of the three forms of the decoded picture hash SEI, so a host can check what was decoded without
 * downloading it.  A host issues the pass on the picture's stream after vvc355_picture_pass (vvc355_picture itself does not carry it).
 *
 * The BYTES of component c are rows 0..height[c]-1 of its rectangle, each width[c] samples: one byte per sample at bd 8, two bytes, low
 * byte first, at bd 10 and 12 — AS STORED: nothing is masked to the bit depth.  Pitch padding is never read.
 *
 *   adler32, plane_adler32[c]   zlib's Adler-32 (RFC 1950 §8.2) with start value 0 (A = 0, B = 0) instead of 1: what
 *                       libavformat/framecrcenc.c:53 does, av_adler32_update(0, pkt->data, pkt->size).  `adler32` is over the bytes of
 *                       components 0..n_comp-1 one after the other (the rawvideo payload of the picture: the planes without pitch),
 *                       plane_adler32[c] over component c alone.
 *   checksum[c]         dph_sei_picture_checksum[c] (Rec. ITU-T H.274 §8.8.2; HEVC §D.3.19, picture_checksum): sum = 0; for every sample
 *                       s at (x, y) of the rectangle, mask = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8); sum += (s & 0xFF) ^ mask; above
 *                       8 bit also sum += (s >> 8) ^ mask; modulo 2^32.
 *   crc[c]              dph_sei_picture_crc[c] (same clauses): the bit-serial CRC with register 0xFFFF, polynomial 0x1021, most significant
 *                       bit first, over the bytes of the component followed by 16 zero bits.  That is the direct-form CRC-CCITT with
 *                       initial value 0x1D0F over the same bytes.
 * The third form of the SEI, MD5, is not computed: it chains 64-byte blocks serially per component.
 * Fields of the result that `what` does not ask for are written as 0, as are the entries of components beyond n_comp.
 */
enum { VVC355_DIGEST_ADLER32 = 1, VVC355_DIGEST_CHECKSUM = 2, VVC355_DIGEST_CRC = 4 };

typedef struct vvc355_pic_digest_result {   /* 36 bytes, no implicit padding */
    uint32_t adler32;           /* planes 0..n_comp-1 concatenated row by row without pitch, start value 0: framecrc's number */
    uint32_t plane_adler32[3];  /* each plane alone, start value 0 */
    uint32_t checksum[3];       /* decoded picture hash SEI, picture_checksum per component */
    uint16_t crc[3];            /* decoded picture hash SEI, picture_crc per component */
    uint16_t n_comp;
} vvc355_pic_digest_result;

typedef struct vvc355_pic_digest_frame {    /* 80 bytes, no implicit padding */
    uint64_t plane[3];   /* DEVICE: first sample of each component's rectangle (the caller adds a crop offset); read only */
    uint64_t result;     /* DEVICE vvc355_pic_digest_result, written whole */
    uint64_t work;       /* DEVICE scratch of vvc355_pic_digest_work_bytes() bytes, one per call in flight */
    int32_t  stride[3];  /* bytes */
    int32_t  width[3], height[3];   /* samples, per component */
    uint8_t  n_comp;     /* 1 (4:0:0) or 3 */
    uint8_t  what;       /* VVC355_DIGEST_* bits; fields not asked for are written as 0 */
    uint8_t  pad_[2];
} vvc355_pic_digest_frame;
/* what vvc355_pic_digest_pass returns for a frame it refuses, in this order: no frame, or n_comp not 1 or 3; bd not 8 / 10 / 12; `what` 0 or
 * with bits above 7, or non-zero pad bytes; a width or height of a counted component <= 0 or beyond 65535; a stride smaller than a row, no
 * multiple of the pixel size, 8 MiB or more, or a plane span (stride * height) of 2 GiB or more; a plane of a counted component, `result`
 * or `work` missing (or a plane not aligned to the pixel size, `result` or `work` not aligned to 4 bytes) */
enum { VVC355_PIC_DIGEST_E_FRAME = -1, VVC355_PIC_DIGEST_E_BD = -2, VVC355_PIC_DIGEST_E_WHAT = -3, VVC355_PIC_DIGEST_E_SIZE = -4,
       VVC355_PIC_DIGEST_E_STRIDE = -5, VVC355_PIC_DIGEST_E_TABLES = -6 };
/* bytes of frame.work for this frame (they depend on the sizes only, and stay below 128 KiB); 0 for a frame the pass would refuse, so a
 * host that sizes the buffer before it has one puts any non-zero value into `work` for this call */
size_t vvc355_pic_digest_work_bytes(const vvc355_pic_digest_frame *frame_host, int bd);
/* Two launches on `stream`, the second a single workgroup: no host synchronisation, no allocation, no atomics; may be captured in a
 * graph.  The host copy of the frame is checked before any HIP call.
 * returns 0, or a negative VVC355_PIC_DIGEST_E_* with NOTHING launched */
int vvc355_pic_digest_pass(void *stream, int bd, const vvc355_pic_digest_frame *frame_dev, const vvc355_pic_digest_frame *frame_host);

/*
 * The hand-over of a decoded picture: crop, repack and (where asked) change the sample size of the planes where they lie, so that only
 * the bytes a consumer wants leave the device.  The planes of a decoder are planar at a padded pitch, samples above 8 bit in the LOW bits
 * of a uint16; the surfaces consumers take are planar without padding (yuv420p, yuv420p10le, ...) or semi-planar with the value in the
 * HIGH bits (NV12 / NV16 / NV24, P010 / P210 / P410, P012 / P212 / P412: libavutil/pixdesc.c; the repack is what
 * libswscale/swscale_unscaled.c:142-270 does on a host).  A host issues the pass on the picture's stream after vvc355_picture_pass, like the
 * digest (vvc355_picture itself does not carry it), and vvc355_download_async() moves the packed bytes.
 *
 * S is the stored sample of the source: uint8 at bd 8, uint16, low byte first, at bd 10 and 12 — AS STORED: nothing is masked.
 *   out_bits == bd            D = S, the sample size unchanged (yuv4xxp, yuv4xxp10le, yuv4xxp12le; NV12 / NV16 / NV24 at bd 8)
 *   out_bits == 16, any bd    D = (S << (16 - bd)) & 0xFFFF, uint16, low byte first (the P010 / P012 family; swscale_unscaled.c:237-264)
 *   out_bits == 8, bd 10 / 12 D = min((S + (1 << (bd - 9))) >> (bd - 8), 255), uint8 (rounded, not dithered; 1023 at 10 bit rounds to 256: clipped)
 * VVC355_OUT_PLANAR: component c goes to dst[c].  VVC355_OUT_SEMI: n_comp is 3, width[1] == width[2], height[1] == height[2] and dst[2] is 0;
 * luma goes to dst[0]; row y of dst[1] holds Cb(x, y) at sample index 2x and Cr(x, y) at 2x + 1, with VVC355_OUT_SWAP_UV the two exchanged
 * (NV21, NV42); dst_stride[2] is not looked at.  VVC355_OUT_SWAP_UV is refused under VVC355_OUT_PLANAR (exchange dst[1] and dst[2]).
 * In dst only the bytes of the rows are written: pitch padding and everything around the planes keep their bytes.  Nothing outside the
 * source rectangles is read.
 */
enum { VVC355_OUT_PLANAR = 0, VVC355_OUT_SEMI = 1 };
enum { VVC355_OUT_SWAP_UV = 1 };

typedef struct vvc355_pic_output_frame {    /* 104 bytes, no implicit padding */
    uint64_t src[3];         /* DEVICE: first sample of each component's rectangle (the caller adds the conformance window's offset); read only */
    uint64_t dst[3];         /* DEVICE: first byte of each output plane */
    int32_t  src_stride[3];  /* bytes */
    int32_t  dst_stride[3];  /* bytes */
    int32_t  width[3], height[3];   /* samples, per component */
    uint8_t  n_comp;         /* 1 (4:0:0) or 3 */
    uint8_t  layout;         /* VVC355_OUT_PLANAR or VVC355_OUT_SEMI */
    uint8_t  out_bits;       /* bd, 16, or 8 */
    uint8_t  flags;          /* VVC355_OUT_SWAP_UV */
    uint8_t  pad_[4];        /* 0 */
} vvc355_pic_output_frame;
/* what vvc355_pic_output_pass returns for a frame it refuses, in this order: no frame, or n_comp not 1 or 3; bd not 8 / 10 / 12; a layout,
 * out_bits or flags outside the above, non-zero pad bytes, or the conditions of VVC355_OUT_SEMI not met; a width or height of a component
 * <= 0 or beyond 65535; a source or destination stride smaller than a row, no multiple of its sample size or 8 MiB or more, or a plane
 * span (stride * height) of 2 GiB or more; a source or destination plane missing or not aligned to its sample size; a destination plane
 * whose bytes (first row to the end of the last) overlap those of a source plane: the pass does not work in place */
enum { VVC355_PIC_OUTPUT_E_FRAME = -1, VVC355_PIC_OUTPUT_E_BD = -2, VVC355_PIC_OUTPUT_E_FORMAT = -3, VVC355_PIC_OUTPUT_E_SIZE = -4,
       VVC355_PIC_OUTPUT_E_STRIDE = -5, VVC355_PIC_OUTPUT_E_PLANES = -6, VVC355_PIC_OUTPUT_E_OVERLAP = -7 };
/* One launch on `stream`: no host synchronisation, no allocation, no atomics; may be captured in a graph.  The host copy of the frame is
 * checked before any HIP call.
 * returns 0, or a negative VVC355_PIC_OUTPUT_E_* with NOTHING launched */
int vvc355_pic_output_pass(void *stream, int bd, const vvc355_pic_output_frame *frame_dev, const vvc355_pic_output_frame *frame_host);

/*
 * The hand-back of collocated motion: the third thing that leaves the device per picture, after the digest and the packed surface.
 * vvc355_inter_frame_predict refines motion on the device (DMVR) and set_dmvr_info (vvc_inter.c:750-762) stores it in
 * fc->ref->tab_dmvr_mvf, which the motion derivation of LATER pictures reads as collocated motion: temporal_luma_motion_vector
 * (vvc_mvs.c:220-245) and sb_temproal_luma_motion (vvc_mvs.c:1016-1022).  Motion derivation is host work, so a parser bound to this
 * backend needs that motion on the host.  It does not need the table: every read is at (x & ~7, y & ~7) (vvc_mvs.c:231-232, :241-242,
 * :1001-1002), one entry in four; of the entry pred_flag, ref_idx[2] and mv[2] are used; and the vector goes through mv_compression
 * (vvc_mvs.c:57-69, the temporal motion buffer compression of H.266 clause 8.5.2.15) before anything else (check_mvset, :104).  So the pass
 * writes one 16-byte entry per 8x8 luma block: a sixth of the table (24 bytes per 4x4 block), moved by vvc355_download_async.
 *
 * Entry (gx, gy) of `col`, gx < ceil(width / 8), gy < ceil(height / 8), describes the MvField M at table position (row 2 * gy, column
 * 2 * gx); width and height are multiples of 4, so that position exists.  For each list l, with used = (M.pred_flag >> l) & 1:
 *   w[l][0] = used ? (M.mv[l][0] & 0x7FFFF) | (M.ref_idx[l] & 0x1F) << 19 : 0
 *   w[l][1] = (used ? M.mv[l][1] & 0x7FFFF : 0) | (l == 0 ? (M.pred_flag & 3) << 19 : 0)
 * An intra unit is sixteen zero bytes.  The entry is a function of what the reference reads and of nothing else: not of M's pad bytes,
 * hpel_if_idx, bcw_idx, ciip_flag, nor of the stale motion and ref_idx of a list that is not used.
 * With VVC355_COL_MVF_COMPRESS the stored vector is mv_compression(mv), per component (>> arithmetic, log2 = floor):
 *   s = v >> 17; f = log2((v ^ s) | 31) - 4; v' = (v + ((1 << f) >> 2)) & ((-(1 << f)) >> 1)
 * which lies in [-2^17, 2^17] and needs 19 bits signed: hence the field.  mv_compression is idempotent, so check_mvset run on vectors that
 * are compressed already gives the same result bit for bit, and TAB_MVF reads of a table filled by vvc355_col_mvf_scatter work unchanged
 * (tests/test_col_mvf_cpu.py proves the idempotence over the whole range).  Without the flag the vector is stored as it is; a component
 * outside 19 bits signed is outside the contract (the reference clips motion to 18 bits wherever it makes it).
 * Nothing outside the ceil(width / 8) entries of a row of `col` is written: col_stride padding and everything around the array keep
 * their bytes.
 *
 * Where the refined motion comes from:
 *   n_jobs == 0   `mvf` is taken as it is: a host that kept a full dmvr_mvf on the device passes that.
 *   n_jobs > 0    `mvf` is the UNREFINED table (vvc355_inter_frame.mvf, dmvr_mvf = 0 there) and a second launch overlays the refinement:
 *                 for each luma job i with dmvr != 0, every grid point inside its rectangle (x <= 8 * gx < x + w, likewise y) gets the
 *                 vector of records[i].mv in the lists the entry uses, compressed when asked; the flags and ref_idx of the entry stay
 *                 what the first launch wrote.  That is set_dmvr_info restricted to the entries anyone reads.  DMVR sub-blocks are 8 or
 *                 16 wide and high and may start at x = 4 mod 8 (a unit behind a 4-wide neighbour), so a job covers one to four grid
 *                 points; sub-blocks are disjoint, so no atomics.  A job whose rectangle is not 4-aligned, not 8 or 16 on a side, or
 *                 reaches outside the picture is skipped: nothing is written for it.
 * vvc355_picture does not carry the pass: like the digest and the output pass it is issued on the picture's stream, after
 * vvc355_inter_frame_predict (or _pass, or vvc355_picture_pass) when it reads jobs and records.
 */
enum { VVC355_COL_MVF_COMPRESS = 1 };

typedef struct vvc355_col_mv { uint32_t w[2][2]; } vvc355_col_mv;    /* 16 bytes: [list][x, y] */

typedef struct vvc355_col_mvf_frame {     /* 56 bytes, no implicit padding */
    uint64_t mvf;          /* DEVICE MvField[] (vvc355_mvfield, 24 bytes), mvf_stride entries per row: read only */
    uint64_t col;          /* DEVICE vvc355_col_mv[], col_stride entries per row, ceil(height / 8) rows */
    uint64_t jobs_luma, records;   /* 0, or vvc355_inter_frame.jobs_luma / .records as vvc355_inter_frame_predict left them */
    int32_t  width, height;        /* luma samples */
    int32_t  mvf_stride, col_stride, n_jobs;
    uint8_t  flags;        /* VVC355_COL_MVF_COMPRESS = 1 */
    uint8_t  pad_[3];      /* 0 */
} vvc355_col_mvf_frame;
/* what vvc355_col_mvf_pass returns for a frame it refuses, in this order: no frame; a width or height <= 0, no multiple of 4 or beyond
 * 32764 (the jobs carry int16 positions); mvf_stride < width / 4, col_stride < ceil(width / 8), or a table span (stride * rows * entry
 * size) of 2 GiB or more; `mvf` or `col` missing, or not aligned to 8 / 16 bytes; n_jobs < 0, or n_jobs > 0 with jobs_luma or records
 * missing (or not aligned to 8 / 16 bytes); flag bits above 0, or non-zero pad bytes; the bytes of `col` (first entry to the last of the
 * last row) overlapping those of `mvf` */
enum { VVC355_COL_MVF_E_FRAME = -1, VVC355_COL_MVF_E_SIZE = -2, VVC355_COL_MVF_E_STRIDE = -3, VVC355_COL_MVF_E_TABLES = -4,
       VVC355_COL_MVF_E_JOBS = -5, VVC355_COL_MVF_E_FLAGS = -6, VVC355_COL_MVF_E_OVERLAP = -7 };
/* One launch on `stream`, two with n_jobs > 0: no host synchronisation, no allocation, no atomics; may be captured in a graph.  The host
 * copy of the frame is checked before any HIP call.
 * returns 0, or a negative VVC355_COL_MVF_E_* with NOTHING launched */
int vvc355_col_mvf_pass(void *stream, const vvc355_col_mvf_frame *frame_dev, const vvc355_col_mvf_frame *frame_host);
/* Host side (host/col_mvf.c, plain C, no HIP), on the downloaded entries.
 * _unpack: mv sign-extended from 19 bits, ref_idx, pred_flag; a list that is not used gives mv 0 and ref_idx -1.
 * _scatter: for every entry (gx, gy) of a width x height picture, writes mv, ref_idx and pred_flag of the MvField (vvc355_mvfield, 24 bytes)
 * at (row 2 * gy, column 2 * gx) of the host table `tab_mvf` (fc->ref->tab_dmvr_mvf, min_pu_width entries per row) and NOTHING else: not
 * the entry's other fields, not the entries at odd positions, which nobody reads as collocated motion. */
void vvc355_col_mv_unpack(const vvc355_col_mv *e, int32_t mv[2][2], int8_t ref_idx[2], uint8_t *pred_flag);
void vvc355_col_mvf_scatter(const vvc355_col_mv *col, int col_stride, int width, int height, void *tab_mvf, int min_pu_width);

/* VVCLMCSDSPContext.filter — vvcdsp.h:124, vvc_filter_template.c:25 */
void vvc355_lmcs_filter(int bd, uint8_t *dst, ptrdiff_t dst_stride, int width, int height, const uint8_t *lut);
/* VVCSAODSPContext.band_filter[*] — vvcdsp.h:138, h2656_sao_template.c:24 */
void vvc355_sao_band_filter(int bd, uint8_t *dst, const uint8_t *src, ptrdiff_t dst_stride, ptrdiff_t src_stride,
    const int16_t *sao_offset_val, int sao_left_class, int width, int height);
/* .edge_filter[*] — vvcdsp.h:141, h2656_sao_template.c:50 (implicit source stride 2*128+64 bytes) */
void vvc355_sao_edge_filter(int bd, uint8_t *dst, const uint8_t *src, ptrdiff_t dst_stride,
    const int16_t *sao_offset_val, int eo, int width, int height);
/* .edge_restore[variant] — vvcdsp.h:143, h2656_sao_template.c:81,131; SAOParams flattened to
 * offset_val = sao->offset_val[c_idx], eo_class = sao->eo_class[c_idx] (vvc_ctu.h:440) */
void vvc355_sao_edge_restore(int bd, int variant, uint8_t *dst, const uint8_t *src, ptrdiff_t dst_stride, ptrdiff_t src_stride,
    const int16_t *offset_val, int eo_class, const int *borders, int width, int height,
    const uint8_t *vert_edge, const uint8_t *horiz_edge, const uint8_t *diag_edge);
/* VVCLFDSPContext.filter_luma[dir] / filter_chroma[dir] / ladf_level[dir] — vvcdsp.h:128-133, vvc_filter_template.c:546,681,788 */
void vvc355_lf_filter_luma(int bd, int dir, uint8_t *pix, ptrdiff_t stride, const int32_t *beta, const int32_t *tc,
    const uint8_t *no_p, const uint8_t *no_q, const uint8_t *max_len_p, const uint8_t *max_len_q, int hor_ctu_edge);
void vvc355_lf_filter_chroma(int bd, int dir, uint8_t *pix, ptrdiff_t stride, const int32_t *beta, const int32_t *tc,
    const uint8_t *no_p, const uint8_t *no_q, const uint8_t *max_len_p, const uint8_t *max_len_q, int shift);
int  vvc355_lf_ladf_level(int bd, int dir, const uint8_t *pix, ptrdiff_t stride);

/* ------------------------------------------------------------------ inverse transform + residual (itx.hip) */

enum { VVC355_DCT2 = 0, VVC355_DST7 = 1, VVC355_DCT8 = 2 };     /* enum TxType, vvcdsp.h:30 */
enum { VVC355_ITX_DERIVE_TYPE = 1 };

/* One transform block.  coeffs: DEVICE int32[w*h], row-major (stride w), transformed in place when store_coeffs != 0.
 * dst != 0 additionally adds the residual to the w x h pixel rectangle at dst (itx + add_residual fused, what
 * vvc_intra.c:464-472 chains).  bd here is the bit_depth ARGUMENT of the slot (it sets the second-stage shift). */
typedef struct vvc355_itx_job {
    uint64_t coeffs;
    uint64_t dst;
    int32_t  dst_stride;
    uint8_t  trh, trv, log2_w, log2_h, nzw, nzh, range, bd;
    uint8_t  store_coeffs;
    /* optional fused scaling process (dequant, vvc_intra.c:277-417) applied to the levels as they are loaded, for blocks
     * that go straight from dequant to the transform (no LFNST, no transform skip): dq_flags bit 0 = on, bit 1 =
     * sh_dep_quant_used_flag; dq_qp = tb->qp; scale_matrix / log2_matrix_size / dc as in vvc355_dequant_job below.
     * Levels outside [0, nzw) x [0, nzh) must be zero (they are: the window holds every coded level). */
    uint8_t  dq_flags, dq_qp, log2_matrix_size;
    uint64_t scale_matrix;
    int16_t  dc;
    /* derive_transform_type on the device (vvc_intra.c:130-164): with VVC355_ITX_DERIVE_TYPE in mts_flags, trh / trv above are ignored
     * and derived from tu_flags (VVC355_TU_*), mts_idx, lfnst_idx and c_idx */
    uint8_t  mts_flags, tu_flags, mts_idx, lfnst_idx, c_idx;
    uint8_t  pad_;
} vvc355_itx_job;

/* max_log2_area = max over the batch of log2_w + log2_h; it selects the lanes-per-block mapping (<= 6: a wave per block) */
void vvc355_itx_batch(void *stream, int bd, const vvc355_itx_job *jobs_dev, int n_jobs, int max_log2_area);
/* Same work for a batch in which every job has the shape 2^log2_w x 2^log2_h (both 2..6): the packed 16-bit fast path
 * (itx.hip, "shape-specialised path").  Jobs of a smaller area, log2_transform_range > 15 or coefficients beyond 16 bits
 * are still computed exactly (generic arithmetic, slower); jobs of a larger area are skipped.  The decoder's TU loop
 * (vvc_intra.c:464-472 via itx_2d, vvcdsp.c:94) is what a caller bins by tb size to fill these launches. */
void vvc355_itx_shape_batch(void *stream, int bd, const vvc355_itx_job *jobs_dev, int n_jobs, int log2_w, int log2_h);

/*
 * The transform-block job list of a picture written on the device from one 16-byte record per transform block — what the parser leaves
 * in a TransformBlock (vvc_ctu.h:136-160) — instead of 48-byte jobs built and uploaded by the host: the TU loop of itransform
 * (vvc_intra.c:431-472) as a descriptor builder.  The jobs land in `jobs` (DEVICE scratch, n_tus entries, same order as the records) and
 * go to vvc355_itx_shape_batch / vvc355_itx_batch like host-built ones.
 *   coeff_off   first coefficient of the block in the picture's coefficient arena (tb->coeffs - fc->tab.coeffs), int32 elements
 *   x0, y0      position in the component's samples; nzw, nzh = max_scan_x + 1, max_scan_y + 1
 *   flags       bit 0: fused scaling process (flat matrix, m = 16); bit 1: sh_dep_quant_used_flag; bit 2: the residual stays in the arena
 *               (store_coeffs, no add: blocks whose residual another stage adds); bit 3: derive the transform types on the device
 *               (VVC355_ITX_DERIVE_TYPE with tu_flags / mts_idx / lfnst_idx = the frame's defaults); tr = trh | trv << 4 otherwise;
 *               bit 6 (with bit 2, chroma blocks): the residual is scaled and added by vvc355_lmcs_chroma_resid_batch — the job is written to
 *               frame.resid_jobs, its 64x64 unit from the block's position, bits 4 / 5 = that unit's left / upper luma neighbours exist
 *               (ff_vvc_get_left / top_available(lc, x_vpdu, y_vpdu, 1, 0))
 */
typedef struct vvc355_itx_tu {
    uint32_t coeff_off;
    int16_t  x0, y0;
    uint8_t  log2_w, log2_h, nzw, nzh;
    uint8_t  c_idx, qp, flags, tr;
} vvc355_itx_tu;
typedef struct vvc355_itx_frame {
    uint64_t tus, jobs, coeffs;   /* DEVICE: records, job scratch, coefficient arena */
    uint64_t plane[3];
    int32_t  stride[3];           /* bytes */
    int32_t  n_tus;
    uint8_t  range, bd, pixel_shift, tu_flags;
    /* chroma residual scaling outside the in-order pass: with resid_jobs != 0 the builder also writes one vvc355_lmcs_resid_job per record
     * (DEVICE scratch, n_tus entries, same order; w = 0 — a job the batch entry skips — for blocks without flags bit 6) */
    uint64_t resid_jobs;
    int32_t  width, height;       /* luma picture size */
    uint8_t  hs, vs, size_y, pad_;      /* chroma shifts; min(CtbSizeY, 64) */
    uint64_t scale_table;         /* 0, or vvc355_lmcs_scale_frame.scale: the residual jobs then take their scale from it (joint bit 4) */
} vvc355_itx_frame;
void vvc355_itx_frame_build(void *stream, const vvc355_itx_frame *frame_dev, const vvc355_itx_frame *frame_host);

/*
 * Packed coefficient levels: what a parser hands over instead of the int32 arena (4 bytes per sample of every coded block, zeros included).
 *   level stream  one picture's levels as int16 GROUPS of 16 (32 bytes): one 4x4 tile of a transform block, row-major, slot (y & 3) * 4 + (x & 3);
 *                 the stream base is 32-byte aligned.  Without extended precision every level fits int16 (CoeffMinY / CoeffMaxY, range 15).
 *   side record   one vvc355_tb_levels per transform block, indexed like the jobs it goes with: lv[i] belongs to jobs[i] (a caller that launches
 *                 a sub-range offsets both pointers alike; the jobs vvc355_itx_frame_build writes are in record order).
 *                 groups: bit gy * gw + gx set = the tile at (4 gx, 4 gy) is in the stream, gw = ceil(min(w, 32) / 4); the grid covers
 *                 min(w, 32) x min(h, 32) (nothing beyond 32 is coded: zero-out), so at most 8 x 8 bits.  Blocks narrower or lower than 4
 *                 (2xN, Nx2, 1x16, 16x1) use one partial tile per 4 rows / columns; slots outside the block are zero.
 *                 first: stream index of the block's first group; its groups follow in increasing bit order.
 *                 flags bit 0 (VVC355_LEVELS_INT32): not packed, the levels are int32 at job.coeffs as for the plain entries (extended precision).
 * For a packed job, job.coeffs is only the int32 OUTPUT (store_coeffs): residuals still land in the device arena the in-order intra pass and the
 * chroma residual stage read, but no levels are read from it.
 */
typedef struct vvc355_tb_levels {
    uint64_t groups;
    uint32_t first;
    uint32_t flags;
} vvc355_tb_levels;
enum { VVC355_LEVELS_INT32 = 1 };
/* vvc355_itx_shape_batch / vvc355_itx_batch with the levels taken from lv[i] (packed groups in `levels`, DEVICE int16, or int32 at
 * jobs[i].coeffs for VVC355_LEVELS_INT32); one launch may mix both kinds. */
void vvc355_itx_shape_batch_lv(void *stream, int bd, const vvc355_itx_job *jobs_dev, const vvc355_tb_levels *lv_dev, const int16_t *levels_dev,
    int n_jobs, int log2_w, int log2_h);
void vvc355_itx_batch_lv(void *stream, int bd, const vvc355_itx_job *jobs_dev, const vvc355_tb_levels *lv_dev, const int16_t *levels_dev,
    int n_jobs, int max_log2_area);
/* The adapter for consumers that read int32 levels (vvc355_lfnst_batch, vvc355_dequant_batch with transform skip, BDPCM): writes every packed
 * job's [0, nzw) x [0, nzh) window into the int32 arena at job.coeffs (row stride w) — coded groups with their levels, the rest of the window
 * zero — and nothing outside it.  The window must cover what the next consumer reads: w x h for transform-skip and BDPCM blocks, the
 * window of the transform that follows LFNST (4 or 8) for LFNST blocks.  Jobs with VVC355_LEVELS_INT32 are left alone. */
void vvc355_levels_expand(void *stream, const vvc355_itx_job *jobs_dev, const vvc355_tb_levels *lv_dev, const int16_t *levels_dev, int n_jobs);
/* Host C, per transform block right after residual coding (ff_vvc_residual_coding): reads the block's int32 levels (row-major, w x h),
 * appends its coded groups at `out` and fills *lv (first = `first`).  Returns the number of groups written, or VVC355_LEVELS_E_RANGE for a
 * level outside int16 / VVC355_LEVELS_E_ZERO_OUT for a non-zero level at x >= 32 or y >= 32: nothing is written to `out` then, *lv is
 * {0, first, VVC355_LEVELS_INT32} and the block stays on the int32 path. */
enum { VVC355_LEVELS_E_RANGE = -1, VVC355_LEVELS_E_ZERO_OUT = -2 };
int  vvc355_levels_pack(const int32_t *coeffs, int log2_w, int log2_h, int16_t *out, vvc355_tb_levels *lv, uint32_t first);

/*
 * The transform stage of a picture's INTRA coding units from one 16-byte record per transform block: itransform (vvc_intra.c:432-466) as
 * dequant -> ilfnst_transform (:65-127) -> derive_transform_type (:130-164) -> itx, in one kernel per block.  No job array is built or
 * uploaded and no job-build launch precedes it: the kernel makes its vvc355_itx_job in registers (flat scaling matrix, fused scaling
 * process, the transform types derived from the record's own tu_flags / mts_idx / lfnst_idx / c_idx), reads the levels from the packed
 * stream (or int32 in place), does LFNST on the staged block and leaves the residual in the arena slot at coeff_off, where the in-order
 * RECON pass adds it.  Transform skip, BDPCM, joint Cb-Cr and scaling lists are NOT covered: transform-skip and BDPCM blocks go to
 * vvc355_ts_tb_pass, the others stay with vvc355_dequant_batch and the residual entries.
 *
 * Record order: the records are GROUPED BY AREA CLASS (log2_w + log2_h <= 4, 6, 8, 10, 12 -> class 0..4), class_first[k] .. class_first[k + 1]
 * being class k.  Grouping is the host's job, as shape grouping is for vvc355_itx_frame_build: a parser appends to five lists and
 * concatenates them at upload.  The order inside a class is free, and so is the order of the arena slots: RECON addresses residuals by
 * coeff_off.  A block may be filed under a LARGER class than its area needs (slower, still correct).  lv[i] belongs to tus[i].
 * coeff_off must be a multiple of 4 elements: the kernels move coefficients as 16-byte vectors (a block has at least 4, and the slots of
 * an arena that packs blocks back to back are aligned by construction: every block size is a multiple of 4).
 *
 * A record that breaks the contract — an area larger than its class holds, fewer than 4 coefficients, a dimension beyond 64, reserved
 * flag bits, the LFNST bit with log2_w < 2, log2_h < 2, lfnst_idx not 1 or 2 or pred_mode_intra above 94 — is SKIPPED: nothing is read or
 * written for it (the vvc355_itx_batch convention for an oversized job).  nzw / nzh are clamped to the block.
 */
typedef struct vvc355_intra_tu {
    uint32_t coeff_off;        /* the block's w*h int32 slot in the residual arena (elements): OUTPUT; also the levels when not packed */
    uint8_t  log2_w, log2_h, nzw, nzh;     /* nzw/nzh = max_scan_x/y + 1 as residual coding left them (before LFNST resets them) */
    uint8_t  c_idx, qp, flags, tu_flags;   /* flags bit 0 = sh_dep_quant_used_flag, bit 1 = cu->apply_lfnst_flag[c_idx]; other bits reserved, must be 0 */
                                           /* tu_flags = VVC355_TU_* of THIS block's coding unit (and SPS) */
    uint8_t  mts_idx, lfnst_idx;
    int8_t   pred_mode_intra;  /* what derive_ilfnst_pred_mode_intra (:34-62) returns; read only with flags bit 1 */
    uint8_t  pad_;
} vvc355_intra_tu;
enum { VVC355_INTRA_TU_DEP_QUANT = 1, VVC355_INTRA_TU_LFNST = 2 };

typedef struct vvc355_intra_tb_frame {
    uint64_t tus;              /* DEVICE vvc355_intra_tu[n_tus], grouped by area class, see class_first */
    uint64_t coeffs;           /* DEVICE int32 residual arena */
    uint64_t lv, levels;       /* DEVICE vvc355_tb_levels[n_tus] paired by index + the int16 group stream; both 0 = int32 levels in place at coeff_off */
    int32_t  n_tus;
    int32_t  class_first[6];   /* records [class_first[k], class_first[k+1]) have log2_w + log2_h in class k: <=4, <=6, <=8, <=10, <=12 */
    uint8_t  range, bd;
    uint8_t  launch_mode;      /* 0 = the library's choice (the faster one, as measured); 1 = one launch per class; 2 = classes 0-3 in one grid */
    uint8_t  pad_;
} vvc355_intra_tb_frame;

/* what vvc355_intra_tb_pass returns for a frame it refuses: class_first not non-decreasing from 0 to n_tus (or n_tus < 0, or no frame);
 * bd not 8 / 10 / 12; range outside 15..20; only one of lv / levels set; launch_mode above 2 */
enum { VVC355_INTRA_TB_E_CLASS = -1, VVC355_INTRA_TB_E_BD = -2, VVC355_INTRA_TB_E_RANGE = -3, VVC355_INTRA_TB_E_LEVELS = -4,
       VVC355_INTRA_TB_E_MODE = -5 };
/* Runs the stage on `stream`: at most two launches (classes 0-3 share one grid, the 64x64 class has its own), or one per non-empty class
 * with launch_mode 1.  The host copy of the frame is checked before any HIP call.
 * returns 0, or a negative VVC355_INTRA_TB_E_* with NOTHING launched */
int vvc355_intra_tb_pass(void *stream, const vvc355_intra_tb_frame *frame_dev, const vvc355_intra_tb_frame *frame_host);

/*
 * The transform stage of every coding unit the in-order pass does not own (the inter coding units) from one 16-byte record per coded
 * transform block: the TU loop of itransform (vvc_intra.c:441-476) as dequant -> derive_transform_type (:130-164) -> itx -> the tail
 * (lmcs_scale_chroma :468-469, add_residual :472, add_residual_for_joint_coding_chroma :166-186) in one kernel per block.  No job array
 * (vvc355_itx_job, vvc355_lmcs_resid_job) is built and the scaled chroma residual never visits the arena: the kernel makes its job in
 * registers and adds the residual, scaled when asked, from the registers the transform left it in.  Transform skip, BDPCM and scaling
 * lists are NOT covered: transform-skip and BDPCM blocks go to vvc355_ts_tb_pass, blocks with scaling lists stay with
 * vvc355_dequant_batch and the residual entries.
 *
 *   coeff_off   the block's slot in the arena, int32 elements, a multiple of 4: its int32 levels when the block is not packed, and its
 *               residual OUTPUT when KEEP is set; unused (and unchecked) otherwise
 *   x0, y0      position in the component's samples; nzw, nzh = max_scan_x + 1, max_scan_y + 1 (clamped to the block)
 *   qp          tb->qp; tu_flags = VVC355_TU_* of THIS block's coding unit (and SPS): SBT and explicit MTS differ from unit to unit
 *   flags       bits 0-1 c_idx; bit 2 sh_dep_quant_used_flag; bit 3 KEEP: transform only — the residual goes to the arena slot and the
 *               picture is not touched (blocks whose add stays with the in-order pass; vvc355_itx_tu.flags bit 2);
 *               bits 4 / 5: the 64x64 unit (size_y) that holds the block minus the unit that holds its coding unit's origin, per axis
 *               (x / y; 0 or 1: a coding unit of 128 luma samples spans two units, and lmcs_scale_chroma takes the scale of
 *               (cu->x0, cu->y0), vvc_intra.c:469 -> vvc_intra_template.c:397-398); read with joint bit 3 only; bits 6-7 reserved, 0
 *   joint_mts   bits 0-3 with the meaning of vvc355_recon_cmd.joint: bit 0 the transform unit has tu_joint_cbcr_residual_flag, bit 1
 *               negative sign (ph_joint_cbcr_sign_flag), bit 2 shift (coded_flag[1] ^ coded_flag[2]), bit 3 chroma residual scaling
 *               (itransform's chroma_scale, :449; the host decides it as for the RESID command); bits 4-6 cu->mts_idx (0..4); bit 7 reserved
 * A joint transform unit is ONE record, the coded block (c_idx 1 or 2): the residual is added to its own plane and the sign / shift form
 * to plane 3 - c_idx at the same position, both through the scale when bit 3 is set.  One transform, two adds.
 *
 * Record order: luma records first, then chroma, and inside a channel type GROUPED BY SHAPE BIN: bin (log2_w - 2) * 5 + (log2_h - 2) for the
 * 25 shapes with both sides 4..64, bin 25 for blocks with a side of 1 or 2.  Records [bin_first[ch][k], bin_first[ch][k + 1]) are bin k of
 * channel type ch, so bin_first[0][0] = 0, bin_first[0][26] = bin_first[1][0] and bin_first[1][26] = n_tus.  Grouping is the host's job, as
 * it is for vvc355_itx_frame_build.  lv[i] belongs to tus[i].
 *
 * A record that breaks the contract is SKIPPED, nothing is read or written for it: a shape that is not its bin's, a side beyond 64, fewer
 * than 4 coefficients, reserved bits, mts_idx above 4, c_idx 3, c_idx 0 with joint bits, c_idx of the other channel type, joint bit 3 with
 * scale_table == 0 or a unit left of / above the picture, a rectangle not inside its plane (for a joint record: either plane), coeff_off
 * not a multiple of 4 where it is used, a transform other than DCT-2 along a side of 1, 2 or 64 (DST-7 / DCT-8 exist for 4..32 points).
 */
typedef struct vvc355_inter_tu {
    uint32_t coeff_off;
    int16_t  x0, y0;
    uint8_t  log2_w, log2_h, nzw, nzh;
    uint8_t  qp, tu_flags, flags, joint_mts;
} vvc355_inter_tu;
enum { VVC355_INTER_TU_DEP_QUANT = 4, VVC355_INTER_TU_KEEP = 8, VVC355_INTER_TU_UNIT_DX = 16, VVC355_INTER_TU_UNIT_DY = 32 };
enum { VVC355_INTER_TB_BINS = 26 };

typedef struct vvc355_inter_tb_frame {
    uint64_t tus;              /* DEVICE vvc355_inter_tu[n_tus], ordered as bin_first says */
    uint64_t coeffs;           /* DEVICE int32 arena: levels of unpacked blocks, residuals of KEEP blocks */
    uint64_t lv, levels;       /* DEVICE vvc355_tb_levels[n_tus] paired by index + the int16 group stream; both 0 = int32 levels in place at coeff_off */
    uint64_t plane[3];         /* DEVICE: sample (0, 0) of each component */
    uint64_t scale_table;      /* DEVICE int16: vvc355_lmcs_scale_frame.scale as vvc355_lmcs_vpdu_scale_pass left it; 0 = no record may set joint bit 3 */
    int32_t  stride[3];        /* bytes */
    int32_t  width, height;    /* luma picture size */
    int32_t  n_tus;
    uint8_t  hs, vs;           /* chroma shifts, 0 or 1 */
    uint8_t  size_y;           /* min(CtbSizeY, 64): 32 or 64; read with scale_table only */
    uint8_t  range, bd;        /* log2_transform_range 15..20; bit depth 8 / 10 / 12 */
    uint8_t  pad_[3];
    int32_t  bin_first[2][VVC355_INTER_TB_BINS + 1];
} vvc355_inter_tb_frame;

/* what vvc355_inter_tb_pass returns for a frame it refuses: bin_first not non-decreasing from 0 to n_tus through both channel types (or
 * n_tus < 0, or no frame); bd not 8 / 10 / 12; range outside 15..20; only one of lv / levels set; size_y not 32 / 64 with a scale table;
 * hs or vs above 1; channels outside 1..3; channels == 3 with a scale table (the table is made from the luma this stage reconstructs) */
enum { VVC355_INTER_TB_E_BINS = -1, VVC355_INTER_TB_E_BD = -2, VVC355_INTER_TB_E_RANGE = -3, VVC355_INTER_TB_E_LEVELS = -4,
       VVC355_INTER_TB_E_SIZE_Y = -5, VVC355_INTER_TB_E_SHIFT = -6, VVC355_INTER_TB_E_CHANNELS = -7, VVC355_INTER_TB_E_ORDER = -8 };
/* Runs the stage on `stream` for the channel types in `channels` (1 luma, 2 chroma, 3 both): one launch per non-empty bin.  A picture
 * with chroma residual scaling calls it with 1, then vvc355_lmcs_vpdu_scale_pass (it reads the luma this call reconstructed), then with 2.
 * The host copy of the frame is checked before any HIP call.
 * returns 0, or a negative VVC355_INTER_TB_E_* with NOTHING launched */
int vvc355_inter_tb_pass(void *stream, const vvc355_inter_tb_frame *frame_dev, const vvc355_inter_tb_frame *frame_host, int channels);

/*
 * The transform-skip blocks of a picture, BDPCM included, of intra and inter coding units alike, from one 16-byte record per coded block:
 * what itransform does when tb->ts is set (vvc_intra.c:455-475), in its order — transform_bdpcm on the LEVELS (the clipped running sum
 * along rows or columns, vvcdsp_template.c:76, :455-457), the scaling process with ts = 1 (bd_shift 10, no rectangular correction, no
 * dep-quant add-in, flat matrix), no transform, the tail (add_residual :472, lmcs_scale_chroma :468-469,
 * add_residual_for_joint_coding_chroma :166-186, or KEEP) — in one kernel, a lane per 4x4 tile, with no job array and no build launch.
 * Blocks have sides 2..32 and at least 8 coefficients (transform skip is not coded above 32, and neither ISP nor SBT blocks use it).
 *
 *   coeff_off   the block's slot in the arena, int32 elements, a multiple of 4: its int32 levels when the block is not packed, and its
 *               residual OUTPUT when KEEP is set; unused (and unchecked) otherwise
 *   x0, y0      position in the component's samples
 *   nzw, nzh    the window of the levels as residual coding left them (max_scan_x + 1, max_scan_y + 1, clamped to the block): levels
 *               outside it are not read and count as 0
 *   qp          tb->qp as derive_qp leaves it for a transform-skip block (the clip to qp_prime_ts_min is the host's job)
 *   flags       bits 0-1 c_idx; bit 2 BDPCM; bit 3 KEEP: the WHOLE w x h residual goes to the arena slot (after BDPCM it reaches beyond
 *               the level window) and the picture is not touched; bits 4 / 5 as in vvc355_inter_tu (the block's 64x64 unit minus the unit
 *               of its coding unit's origin, per axis; read with joint bit 3 only); bit 6 BDPCM direction, 1 = vertical (read with bit 2
 *               only); bit 7 reserved, 0
 *   joint       bits 0-3 with the meaning of vvc355_recon_cmd.joint (joint flag, negative sign, shift, chroma residual scaling); bits 4-7
 *               reserved, 0.  A joint transform unit is ONE record, as in vvc355_inter_tu: the second add goes to plane 3 - c_idx.
 * Levels are int32 and accumulate in int32 as in the reference; a conforming level lies within the transform range.
 *
 * Record order: luma records first, then chroma, and inside a channel type GROUPED BY AREA CLASS (log2_w + log2_h <= 4, 6, 8, 10 -> class
 * 0..3): records [class_first[ch][k], class_first[ch][k + 1]) are class k of channel type ch, so class_first[0][0] = 0, class_first[0][4] =
 * class_first[1][0] and class_first[1][4] = n_tus.  Grouping is the host's job.  A block may be filed under a LARGER class than its area
 * needs (slower, still correct).  lv[i] belongs to tus[i]; a packed picture may hold blocks with VVC355_LEVELS_INT32.
 *
 * A record that breaks the contract is SKIPPED, nothing is read or written for it: a side outside 2..32, fewer than 8 coefficients, an
 * area larger than its class holds, reserved bits (the pad byte included), c_idx 3, c_idx 0 with joint bits, c_idx of the other channel
 * type, joint bit 3 with scale_table == 0 or a unit left of / above the picture, a rectangle not inside its plane (for a joint record:
 * either plane), coeff_off not a multiple of 4 where it is used.
 */
typedef struct vvc355_ts_tu {
    uint32_t coeff_off;
    int16_t  x0, y0;
    uint8_t  log2_w, log2_h, nzw, nzh;
    uint8_t  qp, pad_, flags, joint;       /* qp, flags and joint sit where vvc355_inter_tu has qp, flags and joint_mts */
} vvc355_ts_tu;
enum { VVC355_TS_TU_BDPCM = 4, VVC355_TS_TU_KEEP = 8, VVC355_TS_TU_UNIT_DX = 16, VVC355_TS_TU_UNIT_DY = 32, VVC355_TS_TU_VERTICAL = 64 };
enum { VVC355_TS_TB_CLASSES = 4 };

typedef struct vvc355_ts_tb_frame {
    uint64_t tus;              /* DEVICE vvc355_ts_tu[n_tus], ordered as class_first says */
    uint64_t coeffs;           /* DEVICE int32 arena: levels of unpacked blocks, residuals of KEEP blocks */
    uint64_t lv, levels;       /* DEVICE vvc355_tb_levels[n_tus] paired by index + the int16 group stream; both 0 = int32 levels in place at coeff_off */
    uint64_t plane[3];         /* DEVICE: sample (0, 0) of each component */
    uint64_t scale_table;      /* DEVICE int16: vvc355_lmcs_scale_frame.scale as vvc355_lmcs_vpdu_scale_pass left it; 0 = no record may set joint bit 3 */
    int32_t  stride[3];        /* bytes */
    int32_t  width, height;    /* luma picture size */
    int32_t  n_tus;
    uint8_t  hs, vs;           /* chroma shifts, 0 or 1 */
    uint8_t  size_y;           /* min(CtbSizeY, 64): 32 or 64; read with scale_table only */
    uint8_t  range, bd;        /* log2_transform_range 15..20; bit depth 8 / 10 / 12 */
    uint8_t  pad_[3];
    int32_t  class_first[2][VVC355_TS_TB_CLASSES + 1];
} vvc355_ts_tb_frame;

/* what vvc355_ts_tb_pass returns for a frame it refuses: class_first not non-decreasing from 0 to n_tus through both channel types (or
 * n_tus < 0, or no frame); bd not 8 / 10 / 12; range outside 15..20; only one of lv / levels set; size_y not 32 / 64 with a scale table;
 * hs or vs above 1; channels outside 1..3; channels == 3 with a scale table (the table is made from the luma this stage reconstructs) */
enum { VVC355_TS_TB_E_CLASS = -1, VVC355_TS_TB_E_BD = -2, VVC355_TS_TB_E_RANGE = -3, VVC355_TS_TB_E_LEVELS = -4,
       VVC355_TS_TB_E_SIZE_Y = -5, VVC355_TS_TB_E_SHIFT = -6, VVC355_TS_TB_E_CHANNELS = -7, VVC355_TS_TB_E_ORDER = -8 };
/* Runs the stage on `stream` for the channel types in `channels` (1 luma, 2 chroma, 3 both): one launch per channel type, its four
 * classes in one grid.  A picture with chroma residual scaling calls it (and vvc355_inter_tb_pass, in either order: the two own disjoint
 * blocks) with 1, then vvc355_lmcs_vpdu_scale_pass, then with 2.  The host copy of the frame is checked before any HIP call.
 * returns 0, or a negative VVC355_TS_TB_E_* with NOTHING launched */
int vvc355_ts_tb_pass(void *stream, const vvc355_ts_tb_frame *frame_dev, const vvc355_ts_tb_frame *frame_host, int channels);

/*
 * Scaling process for transform coefficients (dequant) — NOT a table slot in the reference: host C in
 * vvc_intra.c:277-417 (derive_qp :277, derive_scale :311, derive_scale_m :341, scale_coeff :391, dequant :400),
 * called per transform block right before LFNST / itx (vvc_intra.c:455-462).  Flattened: everything read through
 * VVCLocalContext arrives as plain numbers.
 *   qp            = tb->qp as derive_qp leaves it (CU qp + offsets, clipped; :291-303)
 *   ts            = tb->ts (transform skip: bd_shift 10, no rectangular correction, no dep-quant add-in)
 *   dep_quant     = sh_dep_quant_used_flag
 *   scale_matrix  = 0 for the flat default (every factor 16, ff_vvc_default_scale_m), else ScalingMatrixRec[id]
 *                   (uint8, (1 << log2_matrix_size)^2 entries) of the matrix derive_scale_m selects (:343-371)
 *   dc            = ScalingMatrixDcRec value replacing the factor of coefficient (0,0) when id >= 14 and the scan
 *                   rectangle starts at the origin (:380-381); negative = none
 *   min/max_x/y   = tb->min_scan_x .. max_scan_y, the rectangle holding non-zero levels
 * In place on int32 coeffs[h][w]: c = clip_intp2((c * scale * m + bd_offset) >> bd_shift, range) for c != 0.
 */
typedef struct vvc355_dequant_job {
    uint64_t coeffs;
    uint64_t scale_matrix;
    uint8_t  log2_w, log2_h, min_x, min_y, max_x, max_y;
    uint8_t  qp, ts, dep_quant, bit_depth, range, log2_matrix_size;
    int16_t  dc;
    uint8_t  pad_[2];
} vvc355_dequant_job;

void vvc355_dequant_batch(void *stream, const vvc355_dequant_job *jobs_dev, int n_jobs);
void vvc355_dequant(int *coeffs, int log2_w, int log2_h, int min_x, int min_y, int max_x, int max_y, int qp, int ts,
    int dep_quant, int bit_depth, int log2_transform_range, const uint8_t *scale_matrix, int log2_matrix_size, int dc);

/* VVCItxDSPContext.itx[trh][trv][log2 w][log2 h] — vvcdsp.h:118, vvcdsp.c:94-195.  Returns -1 (nothing done) for a
 * combination the reference table leaves NULL (vvcdsp_template.c:142-159), else 0. */
int  vvc355_itx(int trh, int trv, int log2_w, int log2_h, int *coeffs, size_t nzw, size_t nzh,
    intptr_t log2_transform_range, intptr_t bit_depth);
/* ff_vvc_inv_lfnst_1d — vvc_itx_1d.h, vvc_itx_1d.c:708 (called by vvc_intra.c:65-127, not a table slot) */
void vvc355_inv_lfnst_1d(int *v, const int *u, int no_zero_size, int n_tr_s, int pred_mode_intra, int lfnst_idx,
    int log2_transform_range);
/* .add_residual / .add_residual_joint / .pred_residual_joint / .transform_bdpcm — vvcdsp.h:114-120, vvcdsp_template.c:32-100 */
void vvc355_add_residual(int bd, uint8_t *dst, const int *res, int width, int height, ptrdiff_t stride);
void vvc355_add_residual_joint(int bd, uint8_t *dst, const int *res, int width, int height, ptrdiff_t stride, int c_sign, int shift);
void vvc355_pred_residual_joint(int *buf, int width, int height, int c_sign, int shift);
void vvc355_transform_bdpcm(int *coeffs, int width, int height, int vertical, int log2_transform_range);

/* ------------------------------------------------------------------ intra prediction (intra.hip) */

/*
 * VVCIntraDSPContext.intra_pred (vvcdsp.h:100, vvc_intra_template.c:595) with everything it reads through
 * VVCLocalContext flattened (SURVEY 8b "fat slots"):
 *   mode        = intra mode AFTER ff_vvc_wide_angle_mode_mapping (vvc_intra.c:693), -14..80
 *   left_avail  = ff_vvc_get_left_available(lc, x, y, <unbounded>, c_idx)   (vvc_intra.c:622)
 *   top_avail   = ff_vvc_get_top_available (lc, x, y, <unbounded>, c_idx)   (vvc_intra.c:591)
 *   cand_up_left= lc->na.cand_up_left; isp_split = cu->isp_split_type != ISP_NO_SPLIT; cb_* = cu->cb_width/height
 *   is_mip / mip_mode / mip_transposed = fc->tab.imf / imm / imtf at the block (and mip_chroma_direct_flag for chroma)
 * plane = address of sample (0,0) of the component plane; x, y, w, h in component samples.
 */
typedef struct vvc355_intra_job {
    uint64_t plane;
    int32_t  stride;              /* bytes */
    int16_t  x, y, w, h;
    int16_t  mode;
    int16_t  cb_width, cb_height;
    int16_t  left_avail, top_avail;
    int16_t  plane_w, plane_h;    /* component picture size (bounds what the synchronous entry stages) */
    uint8_t  c_idx, ref_idx, is_mip, mip_mode, mip_transposed, isp_split, bdpcm_flag, cand_up_left;
    uint8_t  pad_[6];
} vvc355_intra_job;

/* jobs of one launch must not depend on each other's output (e.g. one anti-diagonal of the RECON wavefront) */
/* max_log2_area = max over the batch of log2(w * h): <= 8 maps one wave per block, larger one workgroup per block */
void vvc355_intra_pred_batch(void *stream, int bd, const vvc355_intra_job *jobs_dev, int n_jobs, int max_log2_area);
/* synchronous form: job->plane is a HOST address */
void vvc355_intra_pred_flat(int bd, const vvc355_intra_job *job);

/* Leaf predictors — vvcdsp.h:101-110.  As in the reference (POS(), vvc_intra_template.c:27) `stride` counts PIXELS.
 * top/left are the prepared reference arrays (negative indices are read by the angular modes). */
void vvc355_pred_planar(int bd, uint8_t *src, const uint8_t *top, const uint8_t *left, int w, int h, ptrdiff_t stride);   /* :686 */
void vvc355_pred_dc(int bd, uint8_t *src, const uint8_t *top, const uint8_t *left, int w, int h, ptrdiff_t stride);       /* :847 */
void vvc355_pred_v(int bd, uint8_t *src, const uint8_t *top, int w, int h, ptrdiff_t stride);                             /* :866 */
void vvc355_pred_h(int bd, uint8_t *src, const uint8_t *left, int w, int h, ptrdiff_t stride);                            /* :877 */
void vvc355_pred_angular_v(int bd, uint8_t *src, const uint8_t *top, const uint8_t *left, int w, int h, ptrdiff_t stride,
    int c_idx, int mode, int ref_idx, int filter_flag, int need_pdpc);                                                    /* :894 */
void vvc355_pred_angular_h(int bd, uint8_t *src, const uint8_t *top, const uint8_t *left, int w, int h, ptrdiff_t stride,
    int c_idx, int mode, int ref_idx, int filter_flag, int need_pdpc);                                                    /* :950 */
void vvc355_pred_mip(int bd, uint8_t *src, const uint8_t *top, const uint8_t *left, int w, int h, ptrdiff_t stride,
    int mode_id, int is_transpose);                                                                                       /* :773 */

/*
 * VVCIntraDSPContext.intra_cclm_pred (vvcdsp.h:98, vvc_intra_template.c:352) flattened.  x0,y0,width,height in LUMA
 * samples like the slot; mode = cu->intra_pred_mode_c (81 LT_CCLM, 82 L_CCLM, 83 T_CCLM); avail_t/avail_l =
 * ff_vvc_get_{top,left}_available(lc, x0, y0, 1, 0) != 0; top_avail_c/left_avail_c = the same functions on the chroma
 * block for an unbounded request (c_idx 1); collocated = sps_chroma_vertical_collocated_flag;
 * ctu_boundary = (y0 % ctb_size == 0).  luma/cb/cr = address of sample (0,0) of each plane.
 */
typedef struct vvc355_cclm_job {
    uint64_t luma, cb, cr;
    int32_t  luma_stride, cb_stride, cr_stride;     /* bytes */
    int16_t  x0, y0, width, height;
    int16_t  top_avail_c, left_avail_c;
    uint8_t  mode, hs, vs, avail_t, avail_l, collocated, ctu_boundary, pad_;
} vvc355_cclm_job;

/* VVCIntraDSPContext.lmcs_scale_chroma (vvcdsp.h:99, vvc_intra_template.c:431 + :390) flattened: the 64x64 VPDU origin
 * (x_vpdu, y_vpdu) of the CU, neighbour availability there, picture size, min(ctb_size, 64) and the LMCS model
 * (fc->ps.lmcs.{min_bin_idx,max_bin_idx,pivot[17],chroma_scale_coeff[16]}, vvc_ps.h:193-202). */
typedef struct vvc355_lmcs_scale_job {
    uint64_t luma;
    int32_t  luma_stride;
    int16_t  x_vpdu, y_vpdu, pic_w, pic_h, size_y;
    uint8_t  avail_t, avail_l, min_bin_idx, max_bin_idx;
    uint16_t pivot[17];
    uint16_t chroma_scale_coeff[16];
    uint16_t pad_[6];
} vvc355_lmcs_scale_job;

void vvc355_cclm_batch(void *stream, int bd, const vvc355_cclm_job *jobs_dev, int n_jobs);

/* fc->ps.lmcs as lmcs_derive_chroma_scale reads it (VVCLMCS, vvc_ps.h:193-202) */
typedef struct vvc355_lmcs_model {
    uint16_t pivot[17];
    uint16_t chroma_scale_coeff[16];
    uint8_t  min_bin_idx, max_bin_idx;
    uint8_t  pad_[4];
} vvc355_lmcs_model;

/*
 * Chroma residual scaling outside the in-order pass: one chroma transform block whose residual (already inverse-transformed, e.g. by
 * vvc355_itx_batch with store_coeffs) is scaled and added to the picture — the tail of itransform (vvc_intra.c:449-472) and
 * add_residual_for_joint_coding_chroma (:166-186) with chroma_scale set.  The scale is the one lmcs_derive_chroma_scale
 * (vvc_intra_template.c:390-429) gives for the 64x64 unit of the coding unit, derived per job from the reconstructed luma plane.
 * Valid wherever the luma left of and above that unit is final when the launch runs — e.g. the inter coding units of CTUs whose left,
 * upper and upper-left neighbour CTUs are not reconstructed by the in-order pass; every other block takes the RESID command of
 * vvc355_recon_frame_pass (joint bit 3), which orders it.
 *   x_vpdu, y_vpdu   (cu->x0, cu->y0) & ~(size_y - 1), luma samples; size_y = min(CtbSizeY, 64); pic_w, pic_h luma picture size
 *   avail_l/_t       ff_vvc_get_left_available / _top_available(lc, x_vpdu, y_vpdu, 1, 0) != 0 (picture, slice, tile borders)
 *   joint            as vvc355_recon_cmd.joint (bit 0 joint residual, bit 1 negative sign, bit 2 shift; bit 3 = scale, 0 = plain add);
 *                    bit 4 (with bit 3): the scale is read from vvc355_lmcs_vpdu_scale_pass's table — `luma` is the address of the unit's entry
 */
typedef struct vvc355_lmcs_resid_job {
    uint64_t dst;                 /* DEVICE: the block in its chroma plane */
    uint64_t resid;               /* DEVICE int32[w * h] */
    uint64_t luma;                /* DEVICE: sample (0, 0) of the luma plane */
    int32_t  dst_stride, luma_stride;      /* bytes */
    int16_t  w, h;                /* chroma samples */
    int16_t  x_vpdu, y_vpdu, pic_w, pic_h, size_y;
    uint8_t  avail_l, avail_t, joint;
    uint8_t  pad_[7];
} vvc355_lmcs_resid_job;
void vvc355_lmcs_chroma_resid_batch(void *stream, int bd, const vvc355_lmcs_resid_job *jobs_dev, int n_jobs, const vvc355_lmcs_model *model_dev);

/*
 * The chroma residual scale of every 64x64 unit of a picture in one launch (lmcs_derive_chroma_scale, vvc_intra_template.c:390-429, for all
 * units at once): int16 scale[unit row][unit column] from the reconstructed luma plane, neighbour availability from the slice / tile maps
 * the way ff_vvc_decode_neighbour sets ctb_left_flag / ctb_up_flag (vvc_ctu.c:2468-2495).  Jobs of vvc355_lmcs_chroma_resid_batch with
 * joint bit 4 take their scale from this table (job.luma = DEVICE address of the unit's entry) instead of deriving it per block — valid for
 * the same blocks as the batch entry itself (units whose neighbours are final when this pass runs).
 */
typedef struct vvc355_lmcs_scale_frame {
    uint64_t luma;                /* DEVICE: sample (0, 0) of the luma plane */
    uint64_t scale;               /* DEVICE int16[units_y][units_x] (output), units_x = ceil(width / size_y) */
    uint64_t model;               /* DEVICE vvc355_lmcs_model */
    uint64_t slice_idx, ctb_to_col_bd, ctb_to_row_bd;      /* int16 per CTB / per CTB column (+1) / per CTB row (+1) */
    int32_t  luma_stride;         /* bytes */
    int32_t  width, height, ctb_width;
    uint8_t  ctb_log2, size_y, pad_[6];
} vvc355_lmcs_scale_frame;
void vvc355_lmcs_vpdu_scale_pass(void *stream, int bd, const vvc355_lmcs_scale_frame *frame_dev, const vvc355_lmcs_scale_frame *frame_host);
/* synchronous forms: plane addresses are HOST addresses; pic_w/pic_h (luma samples) bound what is staged */
void vvc355_intra_cclm_pred_flat(int bd, const vvc355_cclm_job *job, int pic_w, int pic_h);
void vvc355_lmcs_scale_chroma_flat(int bd, const vvc355_lmcs_scale_job *job, int *dst, const int *coeff, int width, int height);

/* ------------------------------------------------------------------ fused prediction stage (mc_fused.hip) */

/*
 * One prediction block of at most 16x16 samples (width 2, 4, 8 or 16; height even), predicted straight to pixels:
 *   mode 0  bi-prediction, avg      = put[..] x2 + inter.avg      (vvc_inter.c:253-296, vvc_inter_template.c:25)
 *   mode 1  bi-prediction, weighted = put[..] x2 + inter.w_avg    (vvc_inter_template.c:42; denom, w0, w1, o0, o1)
 *   mode 2  uni-prediction          = put_uni[..]                 (h2656_inter_template.c:44-245)
 *   mode 3  uni-prediction weighted = put_uni_w[..]               (w0 = wx, o0 = ox, denom)
 * src0/src1 = DEVICE address of the integer-position sample of the block in each (edge-padded) reference plane.
 * frac bits: 1 = horizontal fraction of ref 0, 2 = vertical of ref 0, 4 / 8 = the same for ref 1; hf/vf hold 8 luma
 * taps or 4 chroma taps (chroma != 0).  Larger prediction blocks are split into such tiles by the job builder.
 */
typedef struct vvc355_pred_job {
    uint64_t dst, src0, src1;
    int32_t  dst_stride, src0_stride, src1_stride;      /* bytes */
    int8_t   hf0[8], vf0[8], hf1[8], vf1[8];
    uint8_t  w, h, chroma, frac, mode, pad0_;
    int16_t  denom, w0, w1, o0, o1;
    int16_t  pad1_[2];
} vvc355_pred_job;

void vvc355_pred_fused_batch(void *stream, int bd, const vvc355_pred_job *jobs_dev, int n_jobs);

/* ------------------------------------------------------------------ regular bi-prediction incl. its callers (mc_fused.hip) */

/*
 * One regular bi-predicted sub-block (<= 16x16 in its own component) together with the caller work the reference does
 * around the slots, vvc_inter.c:772-822 (pred_regular_blk):
 *   luma   (chroma = 0): derive_sb_mv -> dmvr_mv_refine (:685-748: inter.dmvr[..] x2, 25 x inter.sad, parametric_mv_refine
 *          :642-681, ff_vvc_clip_mv), then luma_mc_bi (:253-296): put[..] x2 at the refined motion, bdof_fetch_samples +
 *          apply_bdof, or w_avg / avg.  The refined motion and the sub-block BDOF decision go to *rec.
 *   chroma (chroma = 1): chroma_mc_bi (:330-369) at the motion found in *rec (rec = 0: at mv), avg / w_avg.
 * Edge emulation (:33-110) is done by reading the reference planes at clamped coordinates: to the picture, or with
 * dmvr != 0 to the window of the unrefined block (emulated_edge_dmvr :61-88).  Planes need no padding.
 *   ref0 / ref1  DEVICE address of sample (0, 0) of this component in the two reference pictures
 *   mv           mvf->mv[L0].x, .y, mvf->mv[L1].x, .y in 1/16 luma samples, as parsed (the "orig_mv" of the reference)
 *   x, y, w, h   position and size in this component's samples; pic_w, pic_h likewise
 *   hf_idx/vf_idx  filter set (vvc_inter.c:382-383: 0 regular, 1 half-sample alternative)
 *   weight_flag, denom, w0, w1, o0, o1   what derive_weight (:137-167) returns for this component
 *   pred_flag    uni-predicted blocks (luma_mc_uni :222-251 / chroma_mc_uni :298-328: put_uni / put_uni_w, no DMVR / BDOF) go through
 *                the same entry with pred_flag 1 or 2; their weights are derive_weight_uni's (denom, w0 = wx, o0 = ox)
 *   dmvr, bdof   on luma they act only on bi-predicted sub-blocks of 8 or 16 samples per side (the only ones VVC applies them to:
 *                coding units of at least 8x8 and 128 samples, sub-blocks of min(cb, 16) per side).  On any other luma job they are
 *                ignored: plain bi-prediction, and *rec gets the unrefined motion with bdof 0.  On chroma, dmvr selects the
 *                clamp window (above) and bdof is ignored.
 * Launch the luma jobs of a frame first, then the chroma jobs that point at their records.
 */
typedef struct vvc355_bipred_job {
    uint64_t dst, ref0, ref1, rec;
    int32_t  dst_stride, ref0_stride, ref1_stride;      /* bytes */
    int32_t  mv[4];
    int16_t  x, y, w, h, pic_w, pic_h;
    int16_t  denom, w0, w1, o0, o1;
    uint8_t  chroma, hs, vs, dmvr, bdof, hf_idx, vf_idx, weight_flag;
    uint8_t  pred_flag;          /* 0 or 3: bi-prediction; 1: list 0 only; 2: list 1 only (mvf->pred_flag) */
    uint8_t  pad_[5];
    uint64_t lmcs_lut;           /* 0, or DEVICE fc->ps.lmcs.fwd_lut (1 << bd pixel-typed entries): luma blocks only — the prediction is stored
                                  * through the forward map, which is what lmcs.filter does to an inter coding unit after predict_inter
                                  * (vvc_inter.c:888-891, sh_lmcs_used_flag && !ciip_flag) and to the inter part of a combined inter / intra
                                  * block before put_ciip (:573-574) */
} vvc355_bipred_job;

typedef struct vvc355_bipred_result {
    int32_t mv[4];            /* motion after refinement (what set_dmvr_info stores, vvc_inter.c:750-762) */
    int32_t bdof;             /* sb_bdof_flag after the DMVR early termination rule (:744-746) */
    int32_t min_sad;          /* minimum SAD of the search (centre: after the 3/4 scaling), dmvr jobs only */
    int32_t searched;         /* 0 when the centre SAD ended the search early (:712) */
    int32_t pad_;
} vvc355_bipred_result;

void vvc355_bipred_batch(void *stream, int bd, const vvc355_bipred_job *jobs_dev, int n_jobs);
/* the same for a launch in which EVERY job has chroma != 0 (jobs that do not are skipped): smaller LDS footprint */
void vvc355_bipred_chroma_batch(void *stream, int bd, const vvc355_bipred_job *jobs_dev, int n_jobs);

/*
 * One (<= 16x16 tile of a) geometric-partition coding unit, what pred_gpm_blk (vvc_inter.c:466-527) does per component: the two
 * parts' uni-directional predictions (luma_mc / chroma_mc: put[..] at each part's motion, edge emulation to the picture) blended
 * by inter.put_gpm with the partition's per-sample weights.
 *   base      as vvc355_bipred_job: ref0 / mv[0..1] = part 0's reference picture and motion, ref1 / mv[2..3] = part 1's; dst, geometry,
 *             chroma / hs / vs, hf_idx / vf_idx; dmvr, bdof, weights and rec are ignored
 *   weights   DEVICE address of the weight of the tile's sample (0, 0) inside the mask the reference selects
 *             (&ff_vvc_gpm_weights[weights_idx][...] with the mirror handling of :488-497, advanced to the tile), values 0..8
 *   step_x, step_y   address steps per sample / per row in that mask (+-1 << hs, +-(112 << vs))
 */
typedef struct vvc355_gpm_job {
    vvc355_bipred_job base;
    uint64_t weights;
    int32_t  step_x, step_y;
} vvc355_gpm_job;

void vvc355_gpm_batch(void *stream, int bd, const vvc355_gpm_job *jobs_dev, int n_jobs);

/* ------------------------------------------------------------------ inter prediction stage driver (inter_frame.hip) */

/*
 * Regular inter prediction of a whole picture straight from what the decoder holds after parsing, the device half of
 * ff_vvc_predict_inter -> pred_regular_blk (vvc_inter.c:783-813): for every coding unit the sub-block walk (sbw = cb_width /
 * num_sb_x, ...), the sub-block's motion from the MvField table (ff_vvc_get_mvf), the reference pictures of its ref_idx, the
 * interpolation filter set of hpel_if_idx, the weights of derive_weight / derive_weight_uni (:129-177) from the slice's prediction
 * weight table and bcw_idx, and then the fused sub-block kernels above (luma with DMVR + BDOF, chroma at the refined motion).  The
 * job arrays are written by a kernel; the host only lists the coding units.
 *   mvf            DEVICE MvField[] as the decoder keeps it (fc->tab.mvf: one entry per 4x4 luma block, `mvf_stride` entries per row):
 *                  int32 mv[2][2] (x, y per list), int8 ref_idx[2], uint8 hpel_if_idx, bcw_idx, pred_flag, ciip_flag, 2 pad bytes = 24 bytes
 *   refs           DEVICE vvc355_ref_pic[2][16]: the slice's RefPicList[list][ref_idx] planes (sample (0, 0), strides in bytes)
 *   pus            DEVICE vvc355_inter_pu[n_pus]; first_job = running sum of the units' job counts
 *                  num_sb_x * num_sb_y * ceil(sbw / 16) * ceil(sbh / 16): sub-blocks wider or taller than 16 (no DMVR / BDOF there,
 *                  the reference caps those at 16) are predicted in 16x16 tiles, which is exact for plain interpolation + averaging
 *   slices         DEVICE vvc355_inter_slice[]: per slice the weighted-prediction switches and the PredWeightTable
 *   jobs_luma      DEVICE scratch, n_jobs entries; jobs_chroma 2 * n_jobs (Cb, Cr interleaved; unused for 4:0:0); records n_jobs
 */
typedef struct vvc355_ref_pic { uint64_t plane[3]; int32_t stride[3]; int32_t pad_; } vvc355_ref_pic;
typedef struct vvc355_inter_pu {
    int16_t  x0, y0, cb_width, cb_height;     /* luma samples */
    uint8_t  num_sb_x, num_sb_y;              /* pu->mi.num_sb_x / _y */
    uint8_t  dmvr_flag, bdof_flag;            /* pu->dmvr_flag, pu->bdof_flag */
    uint8_t  ciip_flag;                       /* cu->ciip_flag: bcw weights are ignored (derive_weight :158) */
    uint8_t  hpel_if_idx;                     /* pu->mi.hpel_if_idx */
    uint8_t  slice;                           /* index into slices[] */
    uint8_t  pad_;
    uint32_t first_job;
} vvc355_inter_pu;
typedef struct vvc355_inter_slice {
    uint8_t  weighted_pred, weighted_bipred;  /* IS_P && pps_weighted_pred_flag; IS_B && pps_weighted_bipred_flag */
    uint8_t  log2_denom[2];                   /* luma, chroma */
    uint8_t  lmcs_used;                       /* sh_lmcs_used_flag: luma of the slice's inter coding units (not CIIP) goes through frame.lmcs_fwd_lut */
    uint8_t  pad_;
    int16_t  weight[2][3][16], offset[2][3][16];      /* PredWeightTable: [list][component][ref_idx] */
} vvc355_inter_slice;
typedef struct vvc355_inter_frame {
    uint64_t dst[3];              /* the current picture's planes */
    uint64_t mvf, refs, pus, slices;
    uint64_t jobs_luma, jobs_chroma, records;
    uint64_t dmvr_mvf;            /* 0, or DEVICE MvField[] with mvf's geometry: fc->ref->tab_dmvr_mvf.  The pass then does set_dmvr_info
                                   * (vvc_inter.c:750-762): every 4x4 unit of a DMVR sub-block gets the sub-block's MvField with the
                                   * refined motion.  (Units of other blocks are filled by the parser, vvc_ctu.c:1699.) */
    int32_t  dst_stride[3];       /* bytes */
    int32_t  mvf_stride;          /* MvField entries per row (min_pu_width) */
    int32_t  n_pus, n_jobs;
    int32_t  width, height;       /* luma samples */
    uint8_t  hs, vs, chroma_format_idc;
    uint8_t  pixel_shift;         /* 0: 8-bit samples, 1: 16-bit samples (sps->pixel_shift) */
    uint8_t  pad_[4];
    uint64_t lmcs_fwd_lut;        /* 0, or DEVICE fc->ps.lmcs.fwd_lut (pixel-typed, 1 << bd entries) for the slices with lmcs_used */
} vvc355_inter_frame;
/* job arrays only (then vvc355_bipred_batch on jobs_luma, vvc355_bipred_chroma_batch on jobs_chroma) */
void vvc355_inter_frame_build(void *stream, const vvc355_inter_frame *frame_dev, const vvc355_inter_frame *frame_host);
/* what _pass launches after its build: luma (DMVR + BDOF), set_dmvr_info (vvc_inter.c:750-762) when dmvr_mvf is set, chroma — the half that
 * reads the reference pictures (the build reads only the uploaded tables) */
void vvc355_inter_frame_predict(void *stream, int bd, const vvc355_inter_frame *frame_dev, const vvc355_inter_frame *frame_host);
/* build + predict */
void vvc355_inter_frame_pass(void *stream, int bd, const vvc355_inter_frame *frame_dev, const vvc355_inter_frame *frame_host);

/* ------------------------------------------------------------------ affine and geometric-partition stage drivers (inter_cu.hip) */

/*
 * The other two branches of predict_inter (vvc_inter.c:875-891) for a whole picture, from the same decoder tables as
 * vvc355_inter_frame_pass plus one small record per coding unit:
 *   affine (pu->inter_affine_flag)  pred_affine_blk (:828-873): one vvc355_affine_job per 4x4 luma sub-block, motion / ref_idx /
 *          bcw_idx / pred_flag from the MvField table, PROF switches and offsets from the record, weights of derive_weight_uni /
 *          derive_weight (dmvr_flag 0); chroma per (1 << hs) x (1 << vs) sub-blocks, 4x4 chroma samples at the averaged motion of
 *          derive_affine_mvc (:813-826) as vvc355_bipred_job pairs (Cb, Cr) with filter set 0 and rec = 0.  Then vvc355_affine_batch
 *          and vvc355_bipred_chroma_batch.
 *   GPM (pu->merge_gpm_flag)  pred_gpm_blk (:466-527): per present component the coding unit in <= 16x16 tiles, one vvc355_gpm_job
 *          each, part 0 / part 1 from the record's gpm_mv, weights addressed in the library's own masks (computed from the standard's
 *          closed form; vvc355_gpm_weights shows them).  Then vvc355_gpm_batch.
 * The picture is described by an embedded vvc355_inter_frame: the one descriptor a decoder fills for the regular pass serves all three
 * drivers by copy, and the host copy that _pass reads (chroma_format_idc, the counts) is self-contained, which a pointer to a device
 * descriptor would not be.  Of it only dst, dst_stride, mvf, mvf_stride, refs, slices, width, height, hs, vs, chroma_format_idc,
 * pixel_shift and lmcs_fwd_lut are read; pus, jobs_luma, jobs_chroma, records, dmvr_mvf, n_pus and n_jobs are ignored.
 * Affine and GPM coding units are never CIIP; LMCS applies to their luma where the slice has lmcs_used.
 */
typedef struct vvc355_affine_cu {
    int16_t  x0, y0, cb_width, cb_height;     /* luma samples */
    uint8_t  num_sb_x, num_sb_y;              /* cb_width >> 2, cb_height >> 2 (affine sub-blocks are 4x4, vvc_mvs.c:1272); other values are
                                               * rejected: the coding unit's jobs then predict nothing (pred_flag 0) */
    uint8_t  prof_flags;                      /* bit l = pu->cb_prof_flag[l] */
    uint8_t  slice;                           /* index into frame.slices[] */
    uint32_t first_job;                       /* running sum of num_sb_x * num_sb_y */
    int16_t  diff_mv[2][2][16];               /* [list][x | y][16]: pu->diff_mv_x / _y (vvc_mvs.c:361-376); the jobs point here */
} vvc355_affine_cu;
typedef struct vvc355_affine_frame {
    vvc355_inter_frame pic;       /* the picture (see above) */
    uint64_t cus;                 /* DEVICE vvc355_affine_cu[n_cus] */
    uint64_t jobs_luma;           /* DEVICE scratch, vvc355_affine_job[n_jobs] */
    uint64_t jobs_chroma;         /* DEVICE scratch, vvc355_bipred_job[2 * (n_jobs >> (hs + vs))], Cb and Cr interleaved; unused for 4:0:0 */
    int32_t  n_cus, n_jobs;       /* n_jobs = the sub-blocks of all records */
} vvc355_affine_frame;
/* job arrays only */
void vvc355_affine_frame_build(void *stream, const vvc355_affine_frame *frame_dev, const vvc355_affine_frame *frame_host);
/* vvc355_affine_batch on jobs_luma and vvc355_bipred_chroma_batch on jobs_chroma: pred_affine_blk (vvc_inter.c:828-873) once the jobs exist */
void vvc355_affine_frame_predict(void *stream, int bd, const vvc355_affine_frame *frame_dev, const vvc355_affine_frame *frame_host);
/* build, then predict */
void vvc355_affine_frame_pass(void *stream, int bd, const vvc355_affine_frame *frame_dev, const vvc355_affine_frame *frame_host);

typedef struct vvc355_gpm_cu {
    int16_t  x0, y0, cb_width, cb_height;     /* luma samples; 8 .. 64 per side, neither side 8 or more times the other */
    uint8_t  partition_idx;                   /* pu->gpm_partition_idx, 0 .. 63 */
    uint8_t  slice;                           /* index into frame.slices[] */
    uint8_t  pad_[2];
    uint32_t first_job;                       /* running sum of the units' tiles: ceil(w / 16) * ceil(h / 16) per present component */
    int32_t  gpm_mv[2][6];                    /* pu->gpm_mv[0..1]: two vvc355_mvfield (24 bytes each; declared below) */
} vvc355_gpm_cu;
typedef struct vvc355_gpm_frame {
    vvc355_inter_frame pic;       /* the picture (see above) */
    uint64_t cus;                 /* DEVICE vvc355_gpm_cu[n_cus] */
    uint64_t jobs;                /* DEVICE scratch, vvc355_gpm_job[n_jobs]: per unit its luma tiles, then its Cb tiles, then its Cr tiles */
    int32_t  n_cus, n_jobs;
} vvc355_gpm_frame;
/* job arrays only */
void vvc355_gpm_frame_build(void *stream, const vvc355_gpm_frame *frame_dev, const vvc355_gpm_frame *frame_host);
/* vvc355_gpm_batch on jobs: pred_gpm_blk (vvc_inter.c:466-527) once the jobs exist */
void vvc355_gpm_frame_predict(void *stream, int bd, const vvc355_gpm_frame *frame_dev, const vvc355_gpm_frame *frame_host);
/* build, then predict */
void vvc355_gpm_frame_pass(void *stream, int bd, const vvc355_gpm_frame *frame_dev, const vvc355_gpm_frame *frame_host);
/* HOST only (no HIP call): the (cb_width >> hs) x (cb_height >> vs) weights, 0 .. 8, row-major into out, that the jobs the GPM
 * builder writes read for a component of a coding unit of this partition and size: the same masks and the same addressing */
void vvc355_gpm_weights(int partition_idx, int cb_width, int cb_height, int hs, int vs, uint8_t *out);

/*
 * The inter half of the combined inter / intra (CIIP) coding units of a whole picture (cu->ciip_flag; ff_vvc_predict_ciip,
 * vvc_inter.c:915), the fourth kind of inter coding unit: a regular merge unit with num_sb_x = num_sb_y = 1 and neither DMVR nor BDOF,
 * whose inter prediction is not the picture's but one operand of inter.put_ciip.  From the decoder's tables and one 32-byte record per
 * unit the builder writes, per unit, the vvc355_bipred_job of its luma tiles, then of its Cb tiles, then of its Cr tiles (<= 16x16 in the
 * component's own samples, row-major): motion, ref_idx, bcw_idx and pred_flag from the MvField entry at (x0, y0), filter set
 * hpel_if_idx on luma and 0 on chroma, rec = 0, dmvr = bdof = 0, weights of derive_weight_uni / derive_weight with ciip_flag set (bcw
 * weights are ignored, :158; explicit weighted prediction applies).
 *   luma             dst = the unit's region of `scratch` (cb_width x cb_height pixels, packed rows), stored through pic.lmcs_fwd_lut where
 *                    the slice has lmcs_used: the inter part of a CIIP block is mapped before the blend (:573-574)
 *   chroma, wc > 2   (wc = cb_width >> hs, hc = cb_height >> vs) likewise: Cb at scratch_off + cb_width * cb_height, Cr wc * hc further
 *   chroma, wc <= 2  the reference does not blend (do_ciip, :590): the inter prediction IS the chroma, dst = the picture plane; the
 *                    unit's region is luma only and cmd[1], cmd[2] are ignored
 * With cmds != 0 the builder also completes the unit's VVC355_RECON_CIIP commands (declared with the RECON stage driver below), which a
 * decoder can then upload with resid = 0 and joint = 0: cmds[cmd[c]].resid = the DEVICE address of component c's region and .joint = the
 * intra weight of ciip_derive_intra_weight (:523-543), 1 + (upper neighbour available and intra) + (left neighbour available and intra)
 * from the MvField entries at ((x0 + cb_width - 1) >> 2, (y0 - 1) >> 2) and ((x0 - 1) >> 2, (y0 + cb_height - 1) >> 2), available = not on
 * the CTU's edge, or ctb_up / ctb_left of ff_vvc_decode_neighbour (vvc_ctu.c:2468: the upper CTU exists in the same tile and slice; the
 * left CTU exists in the same tile).  A command is patched only when cmd[c] < n_cmds, its kind is VVC355_RECON_CIIP and its c_idx, x0, y0,
 * w, h are the record's; no other byte of the command array changes.
 *
 * pic is used as the affine / GPM drivers use it: dst, dst_stride, mvf, mvf_stride, refs, slices, width, height, hs, vs,
 * chroma_format_idc, pixel_shift and lmcs_fwd_lut are read; pus, jobs_luma, jobs_chroma, records, dmvr_mvf, n_pus and n_jobs are ignored.
 * CIIP units must not also be listed in pus[] of vvc355_inter_frame_pass (that pass would predict them onto the picture).
 *
 * Records are NOT trusted with anything that decides an address.  A unit is rejected when x0 or y0 is no multiple of 4; a side is not one
 * of 4, 8, 16, 32, 64 or the area is below 64; the rectangle is not inside the picture and one CTU; slice >= n_slices; first_job + the
 * unit's tiles > n_jobs; its region is not inside [0, scratch_len); the MvField entry's pred_flag is 0 or above 3; a used list's ref_idx
 * is outside 0..15.  A rejected unit's job slots get w = h = 0 (the prediction kernel skips those), nothing of it is written to scratch
 * or planes and none of its commands is patched.  Every one of the n_jobs slots is written by the builder: slots no record claims are
 * zeroed.  first_job must not decrease along cus[]; regions of different units that overlap are the caller's contract, not checked.
 * No implicit padding: vvc355_ciip_cu 32 bytes, vvc355_ciip_frame 224 bytes.
 */
typedef struct vvc355_ciip_cu {
    int16_t  x0, y0, cb_width, cb_height;     /* luma samples; 4 .. 64 per side, cb_width * cb_height >= 64 */
    uint8_t  hpel_if_idx;                     /* pu->mi.hpel_if_idx (bit 0 is read) */
    uint8_t  slice;                           /* index into pic.slices[] */
    uint8_t  pad_[2];
    uint32_t first_job;                       /* running sum of the units' tiles: ceil(w / 16) * ceil(h / 16) per present component */
    uint32_t scratch_off;                     /* PIXEL offset of the unit's region in frame.scratch: luma, then (wc > 2) Cb, then Cr */
    uint32_t cmd[3];                          /* indices of the unit's Y / Cb / Cr VVC355_RECON_CIIP commands in frame.cmds; 0xFFFFFFFF = none */
} vvc355_ciip_cu;
typedef struct vvc355_ciip_frame {
    vvc355_inter_frame pic;       /* the picture (see above) */
    uint64_t cus;                 /* DEVICE vvc355_ciip_cu[n_cus] */
    uint64_t jobs;                /* DEVICE scratch, vvc355_bipred_job[n_jobs] */
    uint64_t scratch;             /* DEVICE pixels (pic.pixel_shift), scratch_len of them: the units' inter predictions */
    uint64_t cmds;                /* DEVICE vvc355_recon_cmd[n_cmds], read-write; 0 = prediction only, no command is read or patched */
    uint64_t slice_idx, ctb_to_col_bd, ctb_to_row_bd;    /* as in vvc355_recon_frame; read only with cmds != 0 */
    int32_t  n_cus, n_jobs;
    int32_t  scratch_len;         /* pixels */
    int32_t  n_slices, n_cmds;
    int32_t  ctb_width, ctb_height;
    uint8_t  ctb_log2;
    uint8_t  pad_[3];
} vvc355_ciip_frame;

/* what the two entries return for a frame they refuse: no frame; width or height <= 0 or no multiple of 4; ctb_log2 outside 5..7;
 * ctb_width / ctb_height not ceil(size >> ctb_log2); a negative count (n_cus, n_jobs, scratch_len, n_slices, n_cmds); (_pass) bd not 8, 10
 * or 12, or pixel_shift != (bd > 8); chroma_format_idc above 3, hs or vs above 1 or not the format's (0: 0 0, 1: 1 1, 2: 1 0, 3: 0 0);
 * cus missing while n_cus > 0; jobs missing while n_jobs > 0; scratch, mvf, refs, slices or a dst plane of a present component missing,
 * or mvf_stride < width / 4; slice_idx or a tile map missing while cmds is set */
enum { VVC355_CIIP_E_FRAME = -1, VVC355_CIIP_E_SIZE = -2, VVC355_CIIP_E_CTB = -3, VVC355_CIIP_E_GRID = -4, VVC355_CIIP_E_COUNT = -5,
       VVC355_CIIP_E_DEPTH = -6, VVC355_CIIP_E_FORMAT = -7, VVC355_CIIP_E_RECORDS = -8, VVC355_CIIP_E_JOBS = -9, VVC355_CIIP_E_TABLES = -10,
       VVC355_CIIP_E_CMDS = -11 };
/* The host copy of the frame is checked before any HIP call: both return 0, or a negative VVC355_CIIP_E_* with NOTHING launched.
 * n_cus == 0 returns 0 and launches nothing.  Both kernels read their descriptors through device addresses: the sequence can be
 * captured with vvc355_graph_begin / _end. */
/* job array + command patch only */
int vvc355_ciip_frame_build(void *stream, const vvc355_ciip_frame *frame_dev, const vvc355_ciip_frame *frame_host);
/* ONE prediction launch over jobs[0 .. n_jobs), luma and chroma tiles together (the inter operand of ff_vvc_predict_ciip, vvc_inter.c:915);
 * the frame is checked as _pass checks it */
int vvc355_ciip_frame_predict(void *stream, int bd, const vvc355_ciip_frame *frame_dev, const vvc355_ciip_frame *frame_host);
/* build, then predict */
int vvc355_ciip_frame_pass(void *stream, int bd, const vvc355_ciip_frame *frame_dev, const vvc355_ciip_frame *frame_host);

/* ------------------------------------------------------------------ affine sub-blocks with PROF (affine.hip) */

/*
 * One 4x4 luma sub-block of an affine coding unit, what pred_affine_blk (vvc_inter.c:864-897) does per sub-block through
 * luma_prof_uni (:369-406) / luma_prof_bi (:408-447): interpolation with the affine filter set
 * (ff_vvc_inter_luma_filters[2]), edge emulation to the picture by clamped reads, and for the lists whose cb_prof_flag is
 * set fetch_samples + apply_prof / apply_prof_uni / apply_prof_uni_w; otherwise put_uni / put_uni_w, or avg / w_avg for
 * bi-prediction.  Chroma of affine blocks is ordinary 4-tap prediction at the averaged motion (vvc_inter.c:884-895): use
 * vvc355_pred_fused_batch / vvc355_bipred_chroma_batch for it.
 *   pred_flag   1 = list 0 only, 2 = list 1 only, 3 = both (mvf->pred_flag)
 *   mv          sub-block motion mv[L0].x, .y, mv[L1].x, .y in 1/16 sample
 *   prof0/1     pu->cb_prof_flag[L0 / L1]
 *   diff_mv     DEVICE address of int16 [2 lists][x | y][16]: pu->diff_mv_x[l], pu->diff_mv_y[l] (may be 0 when no list uses PROF)
 *   weights     uni-prediction: derive_weight_uni -> (denom, w0, o0); bi-prediction: derive_weight -> (denom, w0, w1, o0, o1)
 */
typedef struct vvc355_affine_job {
    uint64_t dst, ref0, ref1, diff_mv;
    int32_t  dst_stride, ref0_stride, ref1_stride;      /* bytes */
    int32_t  mv[4];
    int16_t  x, y, pic_w, pic_h;
    int16_t  denom, w0, w1, o0, o1;
    uint8_t  pred_flag, prof0, prof1, weight_flag;
    uint8_t  pad_[6];
    uint64_t lmcs_lut;           /* as in vvc355_bipred_job: 0, or the forward luma map the sub-block is stored through */
} vvc355_affine_job;

void vvc355_affine_batch(void *stream, int bd, const vvc355_affine_job *jobs_dev, int n_jobs);

/* ------------------------------------------------------------------ deblocking stage driver (loopfilter.hip) */

/*
 * One deblocking pass (all vertical or all horizontal edges) of a whole picture straight from the decoder's side tables:
 * what ff_vvc_deblock_vertical / ff_vvc_deblock_horizontal (vvc_filter.c:864-1003) do per CTU after vvc_deblock_bs has
 * filled the boundary-strength tables — edge and 8-sample unit enumeration on the luma 4 / chroma 8 grids, QpY / QpC
 * averaging incl. the luma-adaptive offset (get_qp_y :830-848, lf.ladf_level), beta / tc from Table 43 with the CTU's
 * offsets (TC_CALC :823-826), maximum filter lengths (max_filter_length :783-821) and the filter_luma / filter_chroma calls.
 * No job array: the kernel derives each unit's parameters itself.  The boundary strengths themselves (vvc_deblock_bs,
 * :308-781: motion, reference and cbf comparisons) are still the caller's.
 */
typedef struct vvc355_deblock_frame {
    uint64_t plane[3];            /* component planes, filtered in place */
    uint64_t bs[3];               /* this pass's boundary strengths: fc->tab.vertical_bs[c] or horizontal_bs[c], uint8 per 4x4 luma unit */
    uint64_t max_len_p, max_len_q;/* luma: fc->tab.vertical_p / _q or horizontal_p / _q, uint8 per 4x4 luma unit */
    uint64_t tb_size_c;           /* chroma: fc->tab.tb_width[CHROMA] (vertical pass) or tb_height[CHROMA], uint8 per 4x4 luma unit */
    uint64_t qp_y;                /* fc->tab.qp[LUMA], int8 per minimum coding block */
    uint64_t qp_c[2];             /* fc->tab.qp[CB], [CR], int8 per 4x4 luma unit */
    uint64_t db_params;           /* fc->tab.deblock: int8 [ctb][6] = beta_offset[3], tc_offset[3] (DBParams, vvc_ps.h:89-92) */
    int32_t  stride[3];           /* bytes */
    int32_t  width, height;       /* luma picture size */
    int32_t  min_tu_width, min_cb_width, ctb_width;
    int32_t  ladf_lower_bound[5]; /* sps->ladf_interval_lower_bound */
    uint8_t  min_cb_log2, ctb_log2, hs, vs, n_comp, vertical, qp_bd_offset, ladf_enabled;
    uint8_t  num_ladf_intervals;
    int8_t   ladf_lowest_qp_offset, ladf_qp_offset[4];
    uint8_t  pad_[6];
} vvc355_deblock_frame;

/* frame_dev: DEVICE address of one descriptor; the launch covers every edge unit of the pass */
void vvc355_deblock_frame_pass(void *stream, int bd, const vvc355_deblock_frame *frame_dev, const vvc355_deblock_frame *frame_host);

/*
 * Boundary strengths and luma maximum filter lengths of a whole picture, both edge directions in one launch: what
 * vvc_deblock_bs (vvc_filter.c:756-783) derives per transform unit at the start of ff_vvc_deblock_vertical / _horizontal —
 * vvc_deblock_bs_luma_vertical / _horizontal (:477-640: transform-block edges, pcm / intra / ciip / cbf rules, the motion rule
 * boundary_strength :308-372, slice / tile edges that must not be filtered), the sub-block edges of affine / sub-block-merge
 * coding blocks (:399-475), derive_max_filter_length_luma (:374-397) and the chroma rules (:642-754).  One lane per 4x4 luma
 * unit GATHERS its entries (the reference scatters per transform unit); every entry of the output tables is written.
 * The outputs are the bs / max_len inputs of vvc355_deblock_frame_pass.
 */
typedef struct vvc355_mvfield {             /* MvField, vvc_ctu.h:195-202 (same layout: 24 bytes) */
    int32_t mv[2][2];             /* [list][x, y] */
    int8_t  ref_idx[2];
    uint8_t hpel_if_idx, bcw_idx;
    uint8_t pred_flag;            /* PF_INTRA 0, PF_L0 1, PF_L1 2, PF_BI 3 (vvc_ctu.h:216-219) */
    uint8_t ciip_flag;
    uint8_t pad_[2];
} vvc355_mvfield;

/* ------------------------------------------------------------------ side tables from compact records (tabfill.hip) */

/*
 * The per-unit tables above, written on the device from what the parser knows per unit, instead of being filled on the host and uploaded
 * (24 bytes of MvField + ~60 bytes of positions, sizes and flags per 4x4 luma unit).  One record per call site of the reference's table
 * setters; coordinates in luma samples, sizes multiples of 4 up to 128:
 *   vvc355_cu_rec   a coding unit of the luma (or single) tree: set_cb_pos + set_cb_tab of msf / iaf (vvc_ctu.c:1144-1160, :1230-1238)
 *                   flags bit 0 = MergeSubblockFlag, bit 1 = InterAffineFlag
 *   vvc355_tu_rec   a transform unit of one tree: set_tb_pos + set_tb_tab (:41-75, :395-400, :511, :1247).  flags bit 7 = tree (0: luma / single
 *                   tree -> tb_*[0], tu_coded_flag[0], pcmf[0]; 1: chroma tree -> tb_*[1] in chroma samples, tu_coded_flag[1..2], joint, pcmf[1]),
 *                   bits 0..2 = tu_coded_flag of Y / Cb / Cr, bit 3 = tu_joint_cbcr_residual_flag, bit 4 = pcm flag
 *   vvc355_mv_rec   a rectangle of equal motion (a prediction unit, or one sub-block of a sub-block unit): ff_vvc_set_mvf (vvc_mvs.c)
 * Records are grouped per CTU, CTUs in raster order, the way a parser produces them: ctu_first_*[rs] .. ctu_first_*[rs + 1] is CTU rs's
 * range in the record array of that kind (int32, ctb_width * ctb_height + 1 entries; 0 = no records of that kind at all).  Within a CTU
 * any order, rectangles of one kind (and tree) do not overlap and lie inside the CTU.  A CTU holds at most 65535 records of a kind.
 * unit_pitch = 4x4 units per table row (min_tu_width = min_pu_width = min_cb_width for MinCbLog2SizeY = 2), mvf_pitch likewise for mvf.
 */
typedef struct vvc355_cu_rec { int16_t x0, y0; uint8_t w, h, flags, pad_; } vvc355_cu_rec;
typedef struct vvc355_tu_rec { int16_t x0, y0; uint8_t w, h, flags, pad_; } vvc355_tu_rec;
typedef struct vvc355_mv_rec {
    int16_t x0, y0; uint8_t w, h, pad_[2];
    int32_t mvf[6];               /* a vvc355_mvfield (24 bytes; declared below) */
} vvc355_mv_rec;
typedef struct vvc355_tab_fill {
    uint64_t cu, tu, mv;          /* DEVICE record arrays */
    int32_t  n_cu, n_tu, n_mv;
    int32_t  unit_pitch, mvf_pitch;
    uint8_t  hs, vs, ctb_log2, pad_;
    uint64_t ctu_first_cu, ctu_first_tu, ctu_first_mv;     /* DEVICE int32[ctb_width * ctb_height + 1] each, or 0 */
    int32_t  width, height, ctb_width, ctb_height;         /* luma picture size; CTUs per row / column */
    /* DEVICE tables to write (any of them may be shared with vvc355_bs_frame / vvc355_inter_frame / vvc355_deblock_frame) */
    uint64_t mvf;
    uint64_t tu_coded_flag[3], tu_joint_cbcr, pcmf[2];
    uint64_t tb_pos_x0[2], tb_pos_y0[2], tb_width[2], tb_height[2];
    uint64_t cb_pos_x, cb_pos_y, cb_width, cb_height, msf, iaf;
} vvc355_tab_fill;
void vvc355_tab_fill_pass(void *stream, const vvc355_tab_fill *frame_dev, const vvc355_tab_fill *frame_host);

typedef struct vvc355_bs_frame {
    /* inputs: the decoder's side tables (VVCFrameContext.tab, vvcdec.h:122-187), uploaded as they are or written by vvc355_tab_fill_pass */
    uint64_t mvf;                 /* vvc355_mvfield per 4x4 luma unit, row pitch min_pu_width */
    uint64_t ref_poc;             /* int32 [slice][2][32]: RefPicList.list[] (POCs) of the slice's two lists */
    uint64_t slice_idx;           /* int16 per CTB */
    uint64_t ctb_to_col_bd, ctb_to_row_bd;   /* int16 per CTB column (+1) / row (+1) */
    uint64_t tu_coded_flag[3];    /* uint8 per 4x4 luma unit */
    uint64_t tu_joint_cbcr;       /* tu_joint_cbcr_residual_flag, uint8 per 4x4 luma unit */
    uint64_t pcmf[2];             /* uint8 per 4x4 luma unit, [0] luma tree, [1] chroma tree */
    uint64_t tb_pos_x0[2], tb_pos_y0[2];     /* int32 per 4x4 luma unit, luma coordinates, per tree */
    uint64_t tb_width[2], tb_height[2];      /* uint8 per 4x4 luma unit, in samples of the component */
    uint64_t cb_pos_x, cb_pos_y;  /* int32 per minimum coding block (luma tree) */
    uint64_t cb_width, cb_height; /* uint8 per minimum coding block */
    uint64_t msf, iaf;            /* MergeSubblockFlag, InterAffineFlag: uint8 per minimum coding block */
    /* outputs, uint8 per 4x4 luma unit: [0] horizontal edges, [1] vertical edges */
    uint64_t bs[2][3];            /* fc->tab.horizontal_bs[c] / vertical_bs[c] */
    uint64_t max_len_p[2], max_len_q[2];     /* fc->tab.horizontal_p / _q, vertical_p / _q */
    int32_t  width, height;       /* luma picture size */
    int32_t  min_tu_width, min_pu_width, min_cb_width, ctb_width;
    uint8_t  ctb_log2, min_cb_log2, hs, vs, n_comp;
    uint8_t  lfase, lfate;        /* pps_loop_filter_across_slices / _tiles_enabled_flag */
    uint8_t  pad_;
} vvc355_bs_frame;

void vvc355_deblock_bs_pass(void *stream, const vvc355_bs_frame *frame_dev, const vvc355_bs_frame *frame_host);

/*
 * The same outputs straight from the unit records (bs_rec.hip): the coding-unit and transform-unit side tables above exist only to carry
 * the 8-byte records of vvc355_tab_fill from one kernel to the next, and with this entry they never reach HBM.  The records are exactly
 * those vvc355_tab_fill_pass takes (same grouping per CTU, same flag bits, tree bit 7); this pass requires both ctu_first_* arrays.  The
 * MvField table stays an input and must be filled first (vvc355_tab_fill_pass with n_cu = n_tu = 0 and the motion records does that).
 * Minimum coding block = 4.  No implicit padding: 208 bytes.
 *
 * For a picture whose records cover it every output entry equals what vvc355_tab_fill_pass + vvc355_deblock_bs_pass write, the zeros
 * included.  Records are NOT trusted: a malformed record (w or h zero or no multiple of 4, x0 or y0 no multiple of 4, a rectangle not inside
 * its CTU) is skipped.  A unit is complete when it has a coding-unit record, a tree-0 transform-unit record with a coding-unit record at
 * its origin and, with n_comp == 3, a tree-1 record; if a unit, or its P-side neighbour in a direction (where one exists inside the
 * picture), is incomplete, the five entries of (unit, direction) are written as 0.  tb_*_c of a unit without a tree-1 record is 0.
 */
typedef struct vvc355_bs_rec_frame {
    uint64_t cu, tu;                          /* DEVICE vvc355_cu_rec[n_cu] / vvc355_tu_rec[n_tu] */
    uint64_t ctu_first_cu, ctu_first_tu;      /* DEVICE int32[ctb_width * ctb_height + 1] each */
    uint64_t mvf;                             /* vvc355_mvfield per 4x4 luma unit, row pitch mvf_pitch */
    uint64_t ref_poc, slice_idx, ctb_to_col_bd, ctb_to_row_bd;      /* as in vvc355_bs_frame */
    /* outputs, uint8 per 4x4 luma unit, row pitch unit_pitch: same meaning and indexing as in vvc355_bs_frame */
    uint64_t bs[2][3];
    uint64_t max_len_p[2], max_len_q[2];
    uint64_t tb_width_c, tb_height_c;         /* fc->tab.tb_width[CHROMA] / tb_height[CHROMA] in chroma samples (tb_size_c of vvc355_deblock_frame); 0 = not wanted */
    int32_t  n_cu, n_tu;
    int32_t  unit_pitch, mvf_pitch;
    int32_t  width, height, ctb_width, ctb_height;          /* luma picture size; CTUs per row / column */
    uint8_t  ctb_log2, hs, vs, n_comp;        /* n_comp 1: only the luma outputs are written (and mandatory) */
    uint8_t  lfase, lfate;
    uint8_t  pad_[2];
} vvc355_bs_rec_frame;

/* what vvc355_deblock_bs_rec_pass returns for a frame it refuses: no frame; width or height <= 0 or no multiple of 4; ctb_log2 outside 5..7;
 * ctb_width / ctb_height not ceil(size >> ctb_log2); unit_pitch or mvf_pitch < width / 4; n_comp not 1 or 3; hs or vs above 1; a negative
 * count; a record array or its ctu_first_* missing while its count is positive; mvf, ref_poc, slice_idx or a tile map missing; a mandatory
 * output missing (bs[*][0], max_len_p, max_len_q; with n_comp == 3 also bs[*][1..2]) */
enum { VVC355_BS_REC_E_FRAME = -1, VVC355_BS_REC_E_SIZE = -2, VVC355_BS_REC_E_CTB = -3, VVC355_BS_REC_E_GRID = -4, VVC355_BS_REC_E_PITCH = -5,
       VVC355_BS_REC_E_COMP = -6, VVC355_BS_REC_E_SHIFT = -7, VVC355_BS_REC_E_COUNT = -8, VVC355_BS_REC_E_RECORDS = -9,
       VVC355_BS_REC_E_TABLES = -10, VVC355_BS_REC_E_OUTPUT = -11 };
/* One launch on `stream`, one workgroup per CTU, no device scratch.  The host copy of the frame is checked before any HIP call.
 * returns 0, or a negative VVC355_BS_REC_E_* with NOTHING launched */
int vvc355_deblock_bs_rec_pass(void *stream, const vvc355_bs_rec_frame *frame_dev, const vvc355_bs_rec_frame *frame_host);

/*
 * The QP tables of vvc355_deblock_frame from the same records (qp_rec.hip): fc->tab.qp[LUMA] as set_qp_y paints it over every coding unit
 * (set_cb_tab, vvc_ctu.c:144-177) and fc->tab.qp[CB] / [CR] as set_qp_c_tab paints them over every chroma transform block (set_tb_tab,
 * :179-185, called from set_cu_tabs :1241-1250).  The values travel in two sidecars paired with the records BY INDEX (as vvc355_tb_levels
 * is paired with the TB records): cu_qp[i] belongs to cu[i], tu_qp_c[i] to tu[i]; the record structs and their pad_ bytes are unchanged.
 * tu_qp_c is read only for tree-1 records (flags bit 7); the entries of tree-0 records are never looked at.  The bytes are copied, not
 * interpreted: QpY may be negative, the chroma values carry qp_bd_offset as cu->qp[] does, and for a joint Cb-Cr transform unit with both
 * flags coded the caller stores cu->qp[JCBCR] in both, as set_qp_c_tab does.
 *
 * The outputs plug into vvc355_deblock_frame unchanged: qp_y with min_cb_log2 = 2 and min_cb_width = unit_pitch, qp_c[k] with
 * min_tu_width = unit_pitch (a coarser MinCbLog2SizeY only means coarser record coordinates).  Every entry with ux < width / 4 and
 * uy < height / 4 is written in one launch: the value of the record that covers the unit (a coding-unit record for qp_y, a tree-1
 * transform-unit record for qp_c), or 0 where no record does.  The pitch padding (ux >= width / 4) is not touched.  With n_comp == 1 only
 * qp_y is written; tu, ctu_first_tu, tu_qp_c and qp_c are not looked at and may be 0.
 *
 * Records are NOT trusted, exactly as in vvc355_deblock_bs_rec_pass: a malformed record (w or h zero or no multiple of 4, x0 or y0 no
 * multiple of 4, a rectangle not inside the CTU it is filed under) paints nothing, a CTU's range in ctu_first_* is clamped to the arrays
 * and to 65535 records, and the sidecars are read only at indices of records that painted.  No implicit padding: 104 bytes.
 */
typedef struct vvc355_qp_rec_frame {
    uint64_t cu, tu;                      /* DEVICE vvc355_cu_rec[n_cu] / vvc355_tu_rec[n_tu]: the arrays vvc355_deblock_bs_rec_pass takes */
    uint64_t ctu_first_cu, ctu_first_tu;  /* DEVICE int32[ctb_width * ctb_height + 1] each */
    uint64_t cu_qp;                       /* DEVICE int8[n_cu]: cu->qp[LUMA] of cu[i] (what set_qp_y leaves in the table) */
    uint64_t tu_qp_c;                     /* DEVICE int8[n_tu][2]: what set_qp_c_tab paints for the Cb / Cr block of tu[i];
                                             read only for tree-1 records (flags bit 7); 0 allowed with n_comp == 1 */
    uint64_t qp_y, qp_c[2];               /* OUTPUTS, int8 per 4x4 luma unit, row pitch unit_pitch */
    int32_t  n_cu, n_tu, unit_pitch;
    int32_t  width, height, ctb_width, ctb_height;
    uint8_t  ctb_log2, n_comp, pad_[2];
} vvc355_qp_rec_frame;

/* what vvc355_deblock_qp_rec_pass returns for a frame it refuses: no frame; width or height <= 0 or no multiple of 4; ctb_log2 outside 5..7;
 * ctb_width / ctb_height not ceil(size >> ctb_log2); unit_pitch < width / 4; n_comp not 1 or 3; a negative count; cu or ctu_first_cu missing
 * while n_cu > 0, or (n_comp == 3) tu or ctu_first_tu missing while n_tu > 0; cu_qp missing while n_cu > 0, or (n_comp == 3) tu_qp_c
 * missing while n_tu > 0; qp_y missing, or (n_comp == 3) qp_c[0] or qp_c[1] */
enum { VVC355_QP_REC_E_FRAME = -1, VVC355_QP_REC_E_SIZE = -2, VVC355_QP_REC_E_CTB = -3, VVC355_QP_REC_E_GRID = -4, VVC355_QP_REC_E_PITCH = -5,
       VVC355_QP_REC_E_COMP = -6, VVC355_QP_REC_E_COUNT = -7, VVC355_QP_REC_E_RECORDS = -8, VVC355_QP_REC_E_SIDECAR = -9,
       VVC355_QP_REC_E_OUTPUT = -10 };
/* One launch on `stream`, one workgroup per CTU, no device scratch, no atomics.  The host copy of the frame is checked before any HIP call.
 * returns 0, or a negative VVC355_QP_REC_E_* with NOTHING launched */
int vvc355_deblock_qp_rec_pass(void *stream, const vvc355_qp_rec_frame *frame_dev, const vvc355_qp_rec_frame *frame_host);

/* ------------------------------------------------------------------ MvField table from prediction-unit records (mvf_unit.hip) */

/*
 * The MvField table written from ONE fixed-size record per prediction unit, the reference's three storage rules run on the device.
 * vvc355_tab_fill_pass takes one vvc355_mv_rec per rectangle of equal motion, which for a regular unit is one call of ff_vvc_store_mvf /
 * ff_vvc_store_mv; for the two kinds whose field is computed per 4x4 block — ff_vvc_store_sb_mvs (vvc_mvs.c:402-446) from control
 * points, ff_vvc_store_gpm_mvf (:448-491) from two candidates and a partition — the host would have to run the derivation and upload up
 * to one 32-byte record per 4x4 block (8 KiB for a 64x64 affine unit whose inputs are 48 bytes).  Here such a unit is one 64-byte record:
 *   VVC355_MVF_PLAIN   every entry of the rectangle gets body[0..5] (a vvc355_mvfield) verbatim, pad bytes included: ff_vvc_store_mvf,
 *                      ff_vvc_store_mv, one sub-block of a sub-block temporal merge unit, an intra unit (a zero MvField: PF_INTRA).
 *   VVC355_MVF_AFFINE  body = cp_mv[list][control point][x, y] (mi->mv[list][cp]), aux = motion_model_idc (1: 4 parameters, 2: 6),
 *                      pf = pred_flag | hpel_if_idx << 2 | bcw_idx << 4.  Per list in pred_flag: SubblockParams of init_subblock_params
 *                      (:338-359), the fallback decision of is_fallback_mode (:313-336, per list), then per 4x4 sub-block (sbx, sby) the
 *                      position 2 + 4 * sb (cb >> 1 under fallback), mv = mv_scale + d_hor * x_pos + d_ver * y_pos, ff_vvc_round_mv(., 0, 7)
 *                      and the clip to [-2^17, 2^17 - 1].  The entry has pred_flag, hpel_if_idx, bcw_idx and BOTH ref_idx from the
 *                      record, ciip_flag 0 and pad 0; the motion of a list not in pred_flag is 0 (the reference leaves what its stack
 *                      held there, and in that list's ref_idx).  Where link != VVC355_MVF_LINK_NONE the pass also writes, into
 *                      affine_cus[link], prof_flags (bit l = cb_prof_flag[l] of derive_cb_prof_flag_lx :282-298: 0 with prof_disabled,
 *                      under fallback, with equal control points, or for a list not in pred_flag; the other six bits 0) and all 64
 *                      diff_mv of derive_subblock_diff_mvs (:361-379: rounded with shift 8, clipped to +-31; zeros where the flag is 0).
 *                      No other byte of that vvc355_affine_cu is written.  Two records must not link the same vvc355_affine_cu.
 *   VVC355_MVF_GPM     body = pu->gpm_mv[0..1] (two vvc355_mvfield), aux = gpm_partition_idx.  Per 4x4 block motion_idx and s_type
 *                      (:469-471); the entry is gpm_mv[0] verbatim, gpm_mv[1] verbatim (s_type 1, or s_type 2 with both parts in one
 *                      list), or the combination: gpm_mv[0] with pred_flag = PF_BI and mv / ref_idx of list gpm_mv[1].pred_flag - 1 from
 *                      gpm_mv[1].
 * All results are byte-exact.  Placement: the rectangles of one picture's records do not overlap; every covered entry (x >> 2, y >> 2)
 * is written whole (24 bytes); entries no record covers keep their bytes.  Records are grouped per CTU in raster order as for
 * vvc355_tab_fill: ctu_first[rs] .. ctu_first[rs + 1] is CTU rs's range (clamped to n_units and to 65535 records; a ctu_first that
 * decreases makes that CTU's range empty).
 *
 * Records are NOT trusted.  A malformed record is skipped — no entry and no vvc355_affine_cu is written for it, and of the record only
 * the fields the check needs are read.  vvc355_mvf_unit_check is that check (the same predicate the kernel runs), in this order:
 *   _R_SIDE      w or h zero, no multiple of 4, or above 128
 *   _R_PLACE     x0 or y0 negative or no multiple of 4, or the rectangle not inside the picture
 *   _R_CTU       the rectangle not inside the CTU it is filed under
 *   _R_PAD       pad_ != 0                      _R_KIND       kind above VVC355_MVF_GPM
 *   _R_AFF_SHAPE a side below 8 or no power of two             _R_AFF_MODEL  aux not 1 or 2
 *   _R_AFF_PRED  pf & 3 == 0                    _R_AFF_LINK   link neither VVC355_MVF_LINK_NONE nor below n_affine_cus
 *   _R_GPM_SHAPE a side outside 8..64           _R_GPM_RATIO  one side 8 or more times the other
 *   _R_GPM_PART  aux above 63                   _R_GPM_PRED   a part whose pred_flag is not 1 or 2
 * Domain: control points lie within the 18-bit motion range [-2^17, 2^17 - 1]; beyond it the reference's int arithmetic may overflow,
 * which is undefined there (this pass wraps).  No implicit padding: the record is 64 bytes (16-byte aligned in the array), the frame 64.
 */
enum { VVC355_MVF_PLAIN = 0, VVC355_MVF_AFFINE = 1, VVC355_MVF_GPM = 2 };
#define VVC355_MVF_LINK_NONE 0xFFFFFFFFu
typedef struct vvc355_mvf_unit {
    int16_t  x0, y0;              /* luma samples, multiples of 4 */
    uint8_t  w, h;                /* multiples of 4, up to 128 */
    uint8_t  kind;                /* VVC355_MVF_* */
    uint8_t  aux;                 /* AFFINE: motion_model_idc; GPM: gpm_partition_idx; PLAIN: not read */
    uint32_t link;                /* AFFINE: index into frame.affine_cus, or VVC355_MVF_LINK_NONE; other kinds: not read */
    uint8_t  pf;                  /* AFFINE: pred_flag | hpel_if_idx << 2 | bcw_idx << 4 */
    int8_t   ref_idx[2];          /* AFFINE */
    uint8_t  pad_;                /* 0 */
    int32_t  body[12];            /* see above; what a kind does not use is not read */
} vvc355_mvf_unit;
typedef struct vvc355_mvf_unit_frame {
    uint64_t units;               /* DEVICE vvc355_mvf_unit[n_units], 16-byte aligned */
    uint64_t ctu_first;           /* DEVICE int32[ctb_width * ctb_height + 1] */
    uint64_t mvf;                 /* DEVICE vvc355_mvfield per 4x4 luma unit, row pitch mvf_pitch, 8-byte aligned: the OUTPUT */
    uint64_t affine_cus;          /* DEVICE vvc355_affine_cu[n_affine_cus], 16-byte aligned, or 0: prof_flags and diff_mv are OUTPUTS */
    int32_t  n_units, n_affine_cus;
    int32_t  mvf_pitch;
    int32_t  width, height, ctb_width, ctb_height;     /* luma picture size; CTUs per row / column */
    uint8_t  ctb_log2;
    uint8_t  prof_disabled;       /* ph_prof_disabled_flag */
    uint8_t  pad_[2];
} vvc355_mvf_unit_frame;

/* what vvc355_mvf_unit_pass returns for a frame it refuses, in the order checked: no frame (either copy); width or height <= 0, no
 * multiple of 4 or above 32764; a negative count; ctb_log2 outside 5..7; ctb_width / ctb_height not ceil(size >> ctb_log2); mvf_pitch <
 * ceil(width / 4); with n_units > 0, units, ctu_first or mvf missing or misaligned (16 / 4 / 8 bytes); with n_affine_cus > 0, affine_cus
 * missing or not 16-byte aligned */
enum { VVC355_MVF_UNIT_E_FRAME = -1, VVC355_MVF_UNIT_E_SIZE = -2, VVC355_MVF_UNIT_E_COUNT = -3, VVC355_MVF_UNIT_E_CTB = -4,
       VVC355_MVF_UNIT_E_GRID = -5, VVC355_MVF_UNIT_E_PITCH = -6, VVC355_MVF_UNIT_E_RECORDS = -7, VVC355_MVF_UNIT_E_AFFINE = -8 };
/* which rule a record breaks (vvc355_mvf_unit_check; see above) */
enum { VVC355_MVF_UNIT_R_SIDE = 1, VVC355_MVF_UNIT_R_PLACE = 2, VVC355_MVF_UNIT_R_CTU = 3, VVC355_MVF_UNIT_R_PAD = 4,
       VVC355_MVF_UNIT_R_KIND = 5, VVC355_MVF_UNIT_R_AFF_SHAPE = 6, VVC355_MVF_UNIT_R_AFF_MODEL = 7, VVC355_MVF_UNIT_R_AFF_PRED = 8,
       VVC355_MVF_UNIT_R_AFF_LINK = 9, VVC355_MVF_UNIT_R_GPM_SHAPE = 10, VVC355_MVF_UNIT_R_GPM_RATIO = 11,
       VVC355_MVF_UNIT_R_GPM_PART = 12, VVC355_MVF_UNIT_R_GPM_PRED = 13 };
/* One launch on `stream`, one workgroup per CTU, no device scratch, no atomics, no host synchronisation: it can be captured in a graph.
 * The host copy of the frame is checked before any HIP call.  n_units == 0 launches nothing and returns 0.
 * returns 0, or a negative VVC355_MVF_UNIT_E_* with NOTHING launched */
int vvc355_mvf_unit_pass(void *stream, const vvc355_mvf_unit_frame *frame_dev, const vvc355_mvf_unit_frame *frame_host);
/* HOST only, no HIP call: 0 for a record the pass would place when filed under CTU ctu_rs of `frame` (of which width, height, ctb_log2,
 * ctb_width, ctb_height and n_affine_cus are read), or the VVC355_MVF_UNIT_R_* of the first rule it breaks; -1 without a record or a
 * frame, with ctb_log2 outside 5..7 or ctu_rs outside the CTU grid */
int vvc355_mvf_unit_check(const vvc355_mvf_unit *rec, const vvc355_mvf_unit_frame *frame, int ctu_rs);

/* ------------------------------------------------------------------ SAO stage driver (loopfilter.hip) */

/*
 * SAO of a whole picture straight from the decoder's per-CTB tables: what ff_vvc_sao_filter (vvc_filter.c:154-300) does per
 * CTB — picture-border flags, the "unfilterable edge" flags from slice indices and tile boundaries (:177-215), the
 * per-component type / band position / edge class / offsets — then band_filter, or edge_filter + edge_restore.  No job
 * array; CTBs with SAO switched off are copied.  Reads the deblocked picture (src), writes another (dst), so the
 * reference's saved border lines (sao_pixel_buffer_h / _v, :100-152) are not needed.
 */
typedef struct vvc355_sao_ctb {
    int16_t  offset_val[3][5];    /* SAOParams.offset_val */
    uint8_t  type_idx[3];         /* 0 not applied, 1 band, 2 edge (SAO_NOT_APPLIED / SAO_BAND / SAO_EDGE) */
    uint8_t  band_position[3], eo_class[3];
    uint8_t  pad_;
} vvc355_sao_ctb;

typedef struct vvc355_sao_frame {
    uint64_t dst[3], src[3];      /* post- and pre-SAO planes (the reference filters in place from saved border lines) */
    uint64_t sao;                 /* vvc355_sao_ctb per CTB, raster order (fc->tab.sao) */
    uint64_t slice_idx;           /* int16 per CTB (fc->tab.slice_idx) */
    uint64_t ctb_to_col_bd, ctb_to_row_bd;   /* int16 per CTB column (ctb_width + 1 entries) / row (pps->ctb_to_col_bd, _row_bd) */
    int32_t  dst_stride[3], src_stride[3];   /* bytes */
    int32_t  width, height, ctb_width, ctb_height;
    uint8_t  ctb_log2, hs, vs, n_comp;
    uint8_t  lfase;               /* pps_loop_filter_across_slices_enabled_flag */
    uint8_t  no_tile_filter;      /* num_tiles_in_pic > 1 && !pps_loop_filter_across_tiles_enabled_flag */
    uint8_t  pad_[2];
} vvc355_sao_frame;

void vvc355_sao_frame_pass(void *stream, int bd, const vvc355_sao_frame *frame_dev, const vvc355_sao_frame *frame_host);

/* ------------------------------------------------------------------ ALF stage driver (alf.hip) */

/*
 * ALF of a whole picture straight from the decoder's per-CTB tables: what ff_vvc_alf_filter (vvc_filter.c:1254-1318) does per
 * CTB — edges[] from picture borders, tile boundaries and slice indices (:1264-1278; they become the replication flags of
 * alf_prepare_buffer, :1105-1137), filter-set selection (alf_get_coeff_and_clip :1142-1169, alf_filter_chroma :1195-1210,
 * alf_filter_cc :1212-1227) — as a device-side builder of the vvc355_alf_job arrays, followed by the three batched kernels.
 * CTB components with ALF off pass through (a zero filter).  work_dev: DEVICE scratch of vvc355_alf_frame_work_bytes().
 */
typedef struct vvc355_alf_ctb {
    uint8_t ctb_flag[3];          /* alf_ctb_flag[] (ALFParams, vvc_ctu.h:453-459) */
    uint8_t filt_set_idx_y;       /* AlfCtbFiltSetIdxY: < 16 fixed filter sets, else 16 + index into the slice's luma APS list */
    uint8_t alt_idx[2];           /* alf_ctb_filter_alt_idx[] */
    uint8_t cc_idc[2];            /* alf_ctb_cc_cb_idc / _cr_idc */
} vvc355_alf_ctb;

/* what one slice signals (sh_alf_aps_id_luma[], sh_alf_aps_id_chroma, sh_alf_cc_cb / cr_aps_id resolved to the APS tables) */
typedef struct vvc355_alf_slice {
    uint64_t luma_coeff[8];       /* VVCALF.luma_coeff of sh_alf_aps_id_luma[k]: int16 [25][12] */
    uint64_t luma_clip_idx[8];    /* VVCALF.luma_clip_idx: uint8 [25][12] */
    uint64_t chroma_coeff;        /* VVCALF.chroma_coeff: int16 [8][6] */
    uint64_t chroma_clip_idx;     /* VVCALF.chroma_clip_idx: uint8 [8][6] */
    uint64_t cc_coeff[2];         /* VVCALF.cc_coeff[0 / 1]: int16 [4][7]; 0 = no APS */
} vvc355_alf_slice;

typedef struct vvc355_alf_frame {
    uint64_t dst[3], src[3];      /* post- and pre-ALF planes */
    uint64_t alf;                 /* vvc355_alf_ctb per CTB, raster order (fc->tab.alf) */
    uint64_t slices;              /* vvc355_alf_slice per slice */
    uint64_t slice_idx;           /* int16 per CTB (fc->tab.slice_idx) */
    uint64_t ctb_to_col_bd, ctb_to_row_bd;   /* int16 per CTB column (+1) / row (+1) */
    int32_t  dst_stride[3], src_stride[3];   /* bytes */
    int32_t  width, height, ctb_width, ctb_height;
    uint8_t  ctb_log2, hs, vs, n_comp;
    uint8_t  lfase, lfate;        /* pps_loop_filter_across_slices / _tiles_enabled_flag */
    uint8_t  pad_[2];
} vvc355_alf_frame;

size_t vvc355_alf_frame_work_bytes(int n_ctbs);
void vvc355_alf_frame_pass(void *stream, int bd, const vvc355_alf_frame *frame_dev, const vvc355_alf_frame *frame_host, void *work_dev);
/* The two halves of the pass on their own: the descriptor builder (per-CTB jobs and parameter blocks into work_dev — it reads only the ALF
 * tables, so it can run any time after they are on the device, like the other job builders) and the filter kernels (which read the
 * planes).  vvc355_alf_frame_pass = build, then filter, on the same stream. */
void vvc355_alf_frame_build(void *stream, int bd, const vvc355_alf_frame *frame_dev, const vvc355_alf_frame *frame_host, void *work_dev);
void vvc355_alf_frame_filter(void *stream, int bd, const vvc355_alf_frame *frame_host, const void *work_dev);

/* ------------------------------------------------------------------ LFNST and transform-type selection on device (itx.hip) */

/*
 * The two steps the reference does in host C between dequant and the table's inverse transform, itransform (vvc_intra.c:431-476):
 *   ilfnst_transform (:65-127)       gather by the 4x4 diagonal scan, ff_vvc_inv_lfnst_1d, scatter into the top-left 4x4 / 8x8 L-shape
 *                                    (transposed for pred_mode_intra > 34), max_scan := 3 or 7
 *   derive_transform_type (:130-164) implicit / explicit MTS -> (trh, trv)
 * Flattened: pred_mode_intra = what derive_ilfnst_pred_mode_intra (:34-62) returns; tu_flags = VVC355_TU_* of the coding unit and SPS.
 */
enum { VVC355_TU_MTS_ENABLED = 1, VVC355_TU_EXPLICIT_MTS_INTRA = 2, VVC355_TU_ISP = 4, VVC355_TU_SBT = 8, VVC355_TU_SBT_HORIZONTAL = 16,
       VVC355_TU_SBT_POS = 32, VVC355_TU_INTRA = 64, VVC355_TU_MIP = 128 };

/* One transform block that carries LFNST: the scaling process (same fields as vvc355_dequant_job, window min 0 .. max) and then
 * ilfnst_transform, in place on coeffs.  The inverse transform that follows takes nzw = nzh = 4 (4-wide / 4-high blocks) or 8. */
typedef struct vvc355_lfnst_job {
    uint64_t coeffs;
    uint64_t scale_matrix;
    uint8_t  log2_w, log2_h, max_x, max_y;
    uint8_t  qp, dequant, dep_quant, bit_depth, range, log2_matrix_size;   /* dequant = 0: coefficients are already scaled */
    int16_t  dc;
    int8_t   pred_mode_intra;
    uint8_t  lfnst_idx;      /* 1 or 2 */
    uint8_t  pad_[2];
} vvc355_lfnst_job;
void vvc355_lfnst_batch(void *stream, const vvc355_lfnst_job *jobs_dev, int n_jobs);
/* synchronous forms (host pointers) */
int  vvc355_ilfnst_transform(int *coeffs, int w, int h, int pred_mode_intra, int lfnst_idx, int log2_transform_range);
/* returns trh | trv << 4; the batched transform entries apply the same rule on the device when a job sets VVC355_ITX_DERIVE_TYPE */
int  vvc355_derive_transform_type(int tu_flags, int mts_idx, int lfnst_idx, int c_idx, int w, int h);

/* ------------------------------------------------------------------ RECON stage driver: in-order CTU interpreter + wavefront (intra.hip) */

/*
 * ff_vvc_reconstruct (vvc_intra.c:498-527) for a whole picture: every CTU's coding units are walked in decoding order — intra
 * prediction (predict_intra :245-274 -> intra_pred / intra_cclm_pred) reading neighbours that earlier blocks have written, then
 * the residual of the transform unit — and CTUs are released in wavefront order: a CTU starts when its left, upper-left, upper and
 * upper-right neighbours are done (the reference's scheduler waits for left + upper-right, vvc_thread.c:156-184, whose own
 * dependencies cover the other two).  The walk is a command list per CTU, one command per reference call in the reference's order:
 *   MARK   add_reconstructed_area(lc, c_idx > 0, x0, y0, w, h)                                   (luma coordinates, :188-206)
 *   PRED   intra.intra_pred(lc, x0, y0, w, h, c_idx)                                             (luma coordinates, like the slot)
 *   CCLM   intra.intra_cclm_pred(lc, x0, y0, w, h)
 *   RESID  itx.add_residual / add_residual_joint of transform block (tb->x0, tb->y0 luma coordinates; w, h = tb_width, tb_height)
 *   CIIP   inter.put_ciip after the PRED of a combined inter / intra coding unit (ff_vvc_predict_ciip, vvc_inter.c:915; luma
 *          coordinates): resid = the inter prediction of the batched stage (w x h pixels of the component, packed rows),
 *          joint = the intra weight ciip_derive_intra_weight (:530-548) gives
 * Neighbour availability is derived on the device the way ff_vvc_get_top_available / _left_available do (:574-648), in a pass over
 * the CTU's list that runs before the CTU waits for its neighbours (the answers depend on the list alone, not on samples): the
 * areas the MARK commands record — for the current CTU only, as in the reference (:508) — are kept as a bitmap of 4x4-luma-sample
 * units, and the length of the covered run above / left of a block is what the reference's walk over its area list returns for the
 * areas a decoder produces (disjoint blocks of one partitioning in coding order, inside the CTU, positions and sizes multiples of
 * four luma samples except the 1- and 2-row intra sub-partitions); ctb_up / ctb_left flags come from the slice and tile tables
 * (ff_vvc_decode_neighbour, vvc_ctu.c:2468), the wide-angle mapping (:693) from the command's mode.
 * Residuals are the outputs of the batched transform stage (vvc355_itx_*_batch with store_coeffs): the inverse transform does
 * not depend on neighbours, so only prediction + add is serialised.  Transform blocks of coding units that are not intra-coded
 * are added by the batched stage itself (dst != 0) before this pass; their CTUs need no commands.
 */
enum { VVC355_RECON_MARK = 0, VVC355_RECON_PRED = 1, VVC355_RECON_CCLM = 2, VVC355_RECON_RESID = 3, VVC355_RECON_CIIP = 4 };
typedef struct vvc355_recon_cmd {
    uint64_t resid;            /* RESID: DEVICE int32[w * h] */
    int16_t  x0, y0, w, h;
    int16_t  cu_x0, cu_y0;     /* lc->cu->x0, y0: end_of_ctb_x / _y of the availability process */
    int16_t  cb_width, cb_height;
    int8_t   mode;             /* cu->intra_pred_mode_y / _c as parsed (before the wide-angle mapping); CCLM: 81, 82, 83 */
    uint8_t  kind, c_idx, ref_idx, is_mip, mip_mode, mip_transposed, isp_split, bdpcm_flag;
    uint8_t  joint;            /* RESID of a chroma block (c_idx 1, 2; a luma RESID is a plain add: the add ignores its joint byte):
                                * bit 0 = add_residual_joint, bit 1 = c_sign negative, bit 2 = shift;
                                * bit 3 = chroma residual scaling (itransform's chroma_scale, vvc_intra.c:449: chroma block of more than 4 samples in
                                * a slice with sh_lmcs_used_flag and ph_chroma_residual_scale_flag): the residual — after the joint sign / shift,
                                * vvc_intra.c:180-182 — goes through lmcs_scale_chroma (vvc_intra_template.c:431) with the scale of the 64x64
                                * unit of (cu_x0, cu_y0), derived from the reconstructed luma left of and above that unit (:390-429) and kept
                                * for the rest of the CTU as lc->lmcs does (reset per CTU, vvc_intra.c:509-510); needs frame.lmcs_model */
    uint8_t  pad_[6];          /* written by the pass itself (the commands live in DEVICE memory, read-write): the availability answers of
                                * its pre-pass — whatever the host puts here is overwritten */
} vvc355_recon_cmd;
/*
 * flags: what the host knows about a CTU's place in the dependency web (0 = an ordinary CTU: it waits for its left, upper-left, upper
 * and upper-right neighbours that have commands, and is walked on LDS tiles by one wave per channel type).
 *   LIGHT      the CTU's commands are MARKs and RESIDs only and none touches luma: the chroma residuals of inter coding units that chroma
 *              residual scaling keeps in the walk (their scale needs the reconstructed luma of a neighbouring CTU the walk writes).  Such a
 *              CTU is not staged in LDS; its blocks (disjoint, so their order does not matter: several are added at a time) go straight
 *              on the planes, and it waits for nothing but
 *   LUMA_LEFT / LUMA_UP   the LUMA of its left / upper neighbour CTU (set when that neighbour's luma is written by the walk: the 64x64
 *              units on that edge read its last column / row, lmcs_derive_chroma_scale vvc_intra_template.c:401-410).  Ordinary CTUs
 *              publish their luma as soon as their luma commands are done, ahead of their chroma.
 */
enum { VVC355_RECON_CTU_LIGHT = 1, VVC355_RECON_CTU_LUMA_LEFT = 2, VVC355_RECON_CTU_LUMA_UP = 4 };
typedef struct vvc355_recon_ctu { uint32_t first_cmd, n_cmd, flags; } vvc355_recon_ctu;
typedef struct vvc355_recon_frame {
    uint64_t plane[3];            /* component planes, predicted / reconstructed in place */
    uint64_t cmds, ctus;          /* vvc355_recon_cmd[], vvc355_recon_ctu per CTU (raster order; n_cmd = 0: nothing to do) */
    uint64_t order;               /* int32 raster indices of the CTUs that have commands, n_work entries, every CTU after the CTUs it waits for
                                   * (see flags above): ascending raster order qualifies; vvc355_recon_order() gives the order that keeps
                                   * the longest dependency chains moving */
    uint64_t state;               /* DEVICE scratch of vvc355_recon_state_bytes(): ticket counter + per-CTU done flags */
    uint64_t slice_idx, ctb_to_col_bd, ctb_to_row_bd;    /* int16 per CTB / per CTB column (+1) / per CTB row (+1) */
    int32_t  stride[3];           /* bytes */
    int32_t  width, height, ctb_width, ctb_height, n_work;
    uint8_t  ctb_log2, hs, vs;
    uint8_t  wpp;                 /* sps_entropy_coding_sync_enabled_flag */
    uint8_t  collocated;          /* sps_chroma_vertical_collocated_flag */
    uint8_t  pad_;
    uint16_t workgroups;          /* persistent workgroups of the pass (each holds 77 KB of LDS while it walks or waits); 0 = 192, the fastest for one
                                   * picture alone — a host that keeps several pictures in flight does better with fewer (about 96 with eight) */
    uint64_t lmcs_model;          /* 0, or DEVICE vvc355_lmcs_model: the picture's LMCS model for RESID commands with joint bit 3 (chroma residual scaling) */
} vvc355_recon_frame;
size_t vvc355_recon_state_bytes(int n_ctus);
/*
 * HOST helper: the ticket order of a picture's CTUs (vvc355_recon_frame.order) from the per-CTU table, no device work.  Workgroups take
 * CTUs in this order and hold their slot while they wait for neighbours, so raster order lets the workgroups pile up behind the first
 * unfinished chain while CTUs further down that wait for nothing are not started.  This is list scheduling, longest remaining chain first:
 * a CTU's weight = its commands (a quarter for LIGHT CTUs) + the heaviest chain of CTUs waiting for it; among the CTUs whose predecessors
 * are all placed the heaviest goes next.  Returns n_work (the CTUs with commands); order has room for ctb_width * ctb_height entries.
 */
int vvc355_recon_order(const vvc355_recon_ctu *ctus_host, int ctb_width, int ctb_height, int32_t *order_host);
void vvc355_recon_frame_pass(void *stream, int bd, const vvc355_recon_frame *frame_dev, const vvc355_recon_frame *frame_host);
/*
 * HOST helper, O(n), no device work: is order_host[0 .. n_work) a ticket order vvc355_recon_frame_pass can run?  The pass takes the order on
 * trust, and a CTU placed before a CTU it waits for makes its workgroup spin on a flag nobody is left to set: a GPU hang, not an error (the
 * reference's scheduler cannot get there: it derives the order itself, vvc_thread.c:156-184).  Returns 0 when the order lists every CTU
 * that has commands exactly once, no other CTU, and every CTU after the CTUs it waits for (the rule of the flags above, the one
 * vvc355_recon_order uses); otherwise what is wrong first: arguments (no table, no order with n_work > 0, a grid or n_work below 0); an
 * index outside the grid; a CTU without commands; a CTU listed twice; a CTU with commands not listed; a CTU ahead of one it waits for.
 */
enum { VVC355_RECON_ORDER_E_ARGS = -1, VVC355_RECON_ORDER_E_RANGE = -2, VVC355_RECON_ORDER_E_EMPTY = -3, VVC355_RECON_ORDER_E_DUPLICATE = -4,
       VVC355_RECON_ORDER_E_MISSING = -5, VVC355_RECON_ORDER_E_DEPENDENCY = -6 };
int vvc355_recon_order_check(const vvc355_recon_ctu *ctus_host, int ctb_width, int ctb_height, const int32_t *order_host, int n_work);

/* ------------------------------------------------------------------ one picture, one call (picture.cpp) */

/*
 * The launch sequence of a picture's record-path stages: what the reference spreads over its per-CTU task stages (vvc_thread.c:432-565, :592-598:
 * run_inter, run_recon, run_lmcs, run_deblock_v, run_deblock_h, run_sao, run_alf) and their progress waits, as one host call on one stream.  Every stage is a pair
 * (DEVICE address, HOST address) of the frame descriptor its own entry takes; host == 0 skips the stage.  Order:
 *   before the reference waits (these read only uploaded records):
 *     tab_fill, the inter / affine / gpm / ciip BUILDS, intra_tb, bs_rec, qp_rec, the ALF build
 *   the stream waits for refs[0 .. n_refs)
 *   after them:
 *     the inter / affine / gpm / ciip PREDICTS,
 *     inter_tb and ts_tb: with channels 3 each; with a lmcs_scale stage inter_tb(1), ts_tb(1), lmcs_vpdu_scale_pass, inter_tb(2), ts_tb(2),
 *     recon, lmcs (inverse mapping), deblock_v, deblock_h, sao, the ALF filter, and `done` is recorded.
 * The WHOLE picture is validated before the first launch: every stage's own host check (the stages that return a code), a stage given
 * without a device address, vvc355_recon_order_check on recon_ctus_host / recon_order_host where both are given (with the recon frame's
 * grid and n_work), and the picture's own rules — ciip.cmds, when set, is recon.cmds; a scale_table of inter_tb / ts_tb is lmcs_scale.scale
 * and that stage is present; n_refs is 0..32 and no reference is 0; while `stream` is capturing a graph n_refs and done are 0 (a captured
 * wait would tie the graph to one event).  On a refusal NOTHING is launched and no event is touched; the value is
 * -(stage << 8 | -code): VVC355_PIC_STAGE(r) gives the VVC355_PIC_STAGE_* id and VVC355_PIC_CODE(r) the stage's own negative code (every
 * code of every stage fits 8 bits).  A picture with no stage, no reference and no `done` returns 0 without any HIP call.
 * `pic` and the descriptors it names are HOST memory and are read during the call only.  No implicit padding: 568 bytes.
 */
typedef struct vvc355_stage_ref { uint64_t dev, host; } vvc355_stage_ref;
typedef struct vvc355_picture {
    vvc355_stage_ref tab_fill;     /* vvc355_tab_fill (the motion records; any of its tables) */
    vvc355_stage_ref inter, affine, gpm, ciip;     /* vvc355_inter_frame, _affine_frame, _gpm_frame, _ciip_frame */
    vvc355_stage_ref intra_tb;     /* vvc355_intra_tb_frame */
    vvc355_stage_ref bs_rec, qp_rec;               /* vvc355_bs_rec_frame, vvc355_qp_rec_frame */
    vvc355_stage_ref alf;          /* vvc355_alf_frame; needs alf_work */
    vvc355_stage_ref inter_tb, ts_tb;              /* vvc355_inter_tb_frame, vvc355_ts_tb_frame */
    vvc355_stage_ref lmcs_scale;   /* vvc355_lmcs_scale_frame: chroma residual scaling, splits the TB passes into luma / chroma calls */
    vvc355_stage_ref recon;        /* vvc355_recon_frame */
    vvc355_stage_ref lmcs;         /* vvc355_lmcs_frame */
    vvc355_stage_ref deblock_v, deblock_h;         /* vvc355_deblock_frame with vertical = 1 / 0 */
    vvc355_stage_ref sao;          /* vvc355_sao_frame */
    uint64_t alf_work;             /* DEVICE scratch of vvc355_alf_frame_work_bytes() */
    uint64_t recon_ctus_host, recon_order_host;    /* HOST copies of recon.ctus / recon.order, or 0: not checked */
    uint64_t refs[32];             /* events (vvc355_event_create) of the reference pictures: their `done` */
    uint64_t done;                 /* event recorded after the last stage ("decoded"), or 0 */
    int32_t  n_refs, pad_;
} vvc355_picture;
enum { VVC355_PIC_STAGE_PICTURE = 1, VVC355_PIC_STAGE_TAB_FILL, VVC355_PIC_STAGE_INTER, VVC355_PIC_STAGE_AFFINE, VVC355_PIC_STAGE_GPM,
       VVC355_PIC_STAGE_CIIP, VVC355_PIC_STAGE_INTRA_TB, VVC355_PIC_STAGE_BS_REC, VVC355_PIC_STAGE_QP_REC, VVC355_PIC_STAGE_ALF,
       VVC355_PIC_STAGE_INTER_TB, VVC355_PIC_STAGE_TS_TB, VVC355_PIC_STAGE_LMCS_SCALE, VVC355_PIC_STAGE_RECON, VVC355_PIC_STAGE_RECON_ORDER,
       VVC355_PIC_STAGE_LMCS, VVC355_PIC_STAGE_DEBLOCK_V, VVC355_PIC_STAGE_DEBLOCK_H, VVC355_PIC_STAGE_SAO };
/* codes of VVC355_PIC_STAGE_PICTURE (the picture's own rules, checked first); VVC355_PIC_E_NO_DEVICE_FRAME is reported under the id of
 * the stage that has a host descriptor and no device address (the ALF stage: or no alf_work), before any stage's own check runs */
enum { VVC355_PIC_E_NO_DEVICE_FRAME = -1, VVC355_PIC_E_PICTURE = -2, VVC355_PIC_E_CIIP_CMDS = -3, VVC355_PIC_E_SCALE_TABLE = -4,
       VVC355_PIC_E_REFS = -5, VVC355_PIC_E_CAPTURE = -6 };
#define VVC355_PIC_ERROR(stage, code) (-(((stage) << 8) | -(code)))
#define VVC355_PIC_STAGE(ret)         ((-(ret)) >> 8)
#define VVC355_PIC_CODE(ret)          (-((-(ret)) & 255))
int vvc355_picture_pass(void *stream, int bd, const vvc355_picture *pic);   /* pic is HOST memory */

#ifdef __cplusplus
}
#endif
#endif /* VVC_MI355_H */
