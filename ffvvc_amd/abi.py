"""ctypes binding of libvvc_mi355.so (the C ABI declared in include/vvc_mi355.h).

The library is the product: there is no CPU fallback.  Loading fails loudly when the in-tree
shared object has not been built (``python -c 'import __graft_entry__ as g; g.build()'``).
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvvc_mi355.so")

_C = {
    "i": ctypes.c_int,
    "p": ctypes.c_void_p,
    "q": ctypes.c_ssize_t,     # ptrdiff_t / intptr_t
    "z": ctypes.c_size_t,
    "u": ctypes.c_uint32,
    "v": None,
}

# name (without the vvc355_/orc_ prefix) -> (return code, argument codes).
# The CPU oracle used by the tests exports the same slot signatures under the orc_ prefix, so the
# table is shared between the two libraries (tests/conftest.py).
SLOT_SIGNATURES = {
    # ---- ALF
    "alf_filter_luma":          ("v", "ipqpqiippi"),
    "alf_filter_chroma":        ("v", "ipqpqiippi"),
    "alf_filter_cc":            ("v", "ipqpqiiiipi"),
    "alf_classify":             ("v", "ipppqiiip"),
    "alf_recon_coeff_and_clip": ("v", "ippppippp"),
    # ---- inter
    "put":                ("v", "iiiippqippi"),
    "put_uni":            ("v", "iiiipqpqippi"),
    "put_uni_w":          ("v", "iiiipqpqiiiippi"),
    "avg":                ("v", "ipqppii"),
    "w_avg":              ("v", "ipqppiiiiiii"),
    "put_ciip":           ("v", "ipqiipqi"),
    "put_gpm":            ("v", "ipqiipppii"),
    "fetch_samples":      ("v", "ippqii"),
    "bdof_fetch_samples": ("v", "ippqiiii"),
    "prof_grad_filter":   ("v", "ippqpqiii"),
    "apply_prof":         ("v", "ipppp"),
    "apply_prof_uni":     ("v", "ipqppp"),
    "apply_prof_uni_w":   ("v", "ipqpppiii"),
    "apply_bdof":         ("v", "ipqppii"),
    "sad":                ("i", "ppiiii"),
    "dmvr":               ("v", "iiippqiqqi"),
    # ---- LMCS / SAO / deblock
    "lmcs_filter":        ("v", "ipqiip"),
    "sao_band_filter":    ("v", "ippqqpiii"),
    "sao_edge_filter":    ("v", "ippqpiii"),
    "sao_edge_restore":   ("v", "iippqqpipiippp"),
    "lf_filter_luma":     ("v", "iipqppppppi"),
    "lf_filter_chroma":   ("v", "iipqppppppi"),
    "lf_ladf_level":      ("i", "iipq"),
    # ---- inverse transform / residual (no leading bd where the reference slot is bit-depth independent)
    "itx":                  ("i", "iiiipzzqq"),
    "inv_lfnst_1d":         ("v", "ppiiiii"),
    "dequant":              ("v", "piiiiiiiiiiipii"),
    "ilfnst_transform":     ("i", "piiiii"),
    "derive_transform_type": ("i", "iiiiii"),
    "add_residual":         ("v", "ippiiq"),
    "add_residual_joint":   ("v", "ippiiqii"),
    "pred_residual_joint":  ("v", "piiii"),
    "transform_bdpcm":      ("v", "piiii"),
    # ---- intra (leaf predictors: stride in PIXELS)
    "pred_planar":        ("v", "ipppiiq"),
    "pred_dc":            ("v", "ipppiiq"),
    "pred_v":             ("v", "ippiiq"),
    "pred_h":             ("v", "ippiiq"),
    "pred_angular_v":     ("v", "ipppiiqiiiii"),
    "pred_angular_h":     ("v", "ipppiiqiiiii"),
    "pred_mip":           ("v", "ipppiiqii"),
    "intra_pred_flat":    ("v", "ip"),
}

# flattened "fat" slots whose signatures differ between the product (needs staging bounds) and the oracle
FLAT_SIGNATURES = {
    "intra_cclm_pred_flat":    ("v", "ipii"),
    "lmcs_scale_chroma_flat":  ("v", "ipppii"),
}

RUNTIME_SIGNATURES = {
    "device_count":   ("i", ""),
    "set_device":     ("v", "i"),
    "malloc":         ("p", "z"),
    "free":           ("v", "p"),
    "upload":         ("v", "ppz"),
    "download":       ("v", "ppz"),
    "copy_async":     ("v", "pppz"),
    "host_alloc":     ("p", "z"),
    "host_free":      ("v", "p"),
    "download_async": ("v", "pppz"),
    "stream_create":  ("p", ""),
    "stream_destroy": ("v", "p"),
    "stream_sync":    ("v", "p"),
    "graph_begin":    ("v", "p"),
    "graph_end":      ("p", "p"),
    "graph_launch":   ("v", "pp"),
    "graph_destroy":  ("v", "p"),
    "event_create":   ("p", ""),
    "event_destroy":  ("v", "p"),
    "event_record":   ("v", "pp"),
    "stream_wait_event": ("v", "pp"),
    "event_query":    ("i", "p"),
    "version":        ("p", ""),
    "set_error_policy": ("v", "i"),
    "last_error":     ("i", ""),
    "last_error_string": ("p", ""),
    "clear_error":    ("v", ""),
}

BATCH_SIGNATURES = {
    "alf_luma_batch":   ("v", "piipi"),
    "alf_chroma_batch": ("v", "pipi"),
    "alf_cc_batch":     ("v", "pipi"),
    "mc_batch":         ("v", "pipiii"),
    "blend_batch":      ("v", "pipiii"),
    "bdof_batch":       ("v", "pipi"),
    "sao_batch":        ("v", "pipiii"),
    "sao_ctb_batch":    ("v", "pipii"),
    "deblock_batch":    ("v", "pipi"),
    "lmcs_batch":       ("v", "pipiii"),
    "itx_batch":        ("v", "pipii"),
    "itx_shape_batch":  ("v", "pipiii"),
    "dequant_batch":    ("v", "ppi"),
    "intra_pred_batch": ("v", "pipii"),
    "cclm_batch":       ("v", "pipi"),
    "lmcs_chroma_resid_batch": ("v", "pipip"),
    "lmcs_vpdu_scale_pass": ("v", "pipp"),
    "pred_fused_batch": ("v", "pipi"),
    "bipred_batch":     ("v", "pipi"),
    "bipred_chroma_batch": ("v", "pipi"),
    "affine_batch":     ("v", "pipi"),
    "gpm_batch":        ("v", "pipi"),
    "inter_frame_build": ("v", "ppp"),
    "inter_frame_predict": ("v", "pipp"),
    "inter_frame_pass": ("v", "pipp"),
    "affine_frame_build": ("v", "ppp"),
    "affine_frame_predict": ("v", "pipp"),
    "affine_frame_pass": ("v", "pipp"),
    "gpm_frame_build":  ("v", "ppp"),
    "gpm_frame_predict": ("v", "pipp"),
    "gpm_frame_pass":   ("v", "pipp"),
    "gpm_weights":      ("v", "iiiiip"),
    # the inter half of the CIIP coding units from 32-byte records (vvc355_ciip_cu): job array + RECON command patch, one prediction launch
    "ciip_frame_build": ("i", "ppp"),
    "ciip_frame_predict": ("i", "pipp"),
    "ciip_frame_pass":  ("i", "pipp"),
    "deblock_frame_pass": ("v", "pipp"),
    "sao_frame_pass":   ("v", "pipp"),
    "alf_frame_pass":   ("v", "pippp"),
    "alf_frame_build":  ("v", "pippp"),
    "alf_frame_filter": ("v", "pipp"),
    "deblock_bs_pass":  ("v", "ppp"),
    "alf_frame_work_bytes": ("z", "i"),
    "lfnst_batch":      ("v", "ppi"),
    "recon_frame_pass": ("v", "pipp"),
    "recon_state_bytes": ("z", "i"),
    "recon_order":      ("i", "piip"),
    "tab_fill_pass":    ("v", "ppp"),
    "itx_frame_build":  ("v", "ppp"),
    # packed coefficient levels (vvc355_tb_levels): the transform entries that read them, the int32 adapter, and the host C packer
    "itx_shape_batch_lv": ("v", "pipppiii"),
    "itx_batch_lv":     ("v", "pipppii"),
    "levels_expand":    ("v", "ppppi"),
    "levels_pack":      ("i", "piippu"),
    # the intra transform stage from 16-byte records (vvc355_intra_tu): scaling + LFNST + transform in one kernel, no job array
    "intra_tb_pass":    ("i", "ppp"),
    # the transform stage of the other coding units from 16-byte records (vvc355_inter_tu): transform + (scaled, joint) residual add
    "inter_tb_pass":    ("i", "pppi"),
    # the transform-skip / BDPCM blocks from 16-byte records (vvc355_ts_tu): BDPCM on the levels + scaling + (scaled, joint) residual add
    "ts_tb_pass":       ("i", "pppi"),
    # boundary strengths and luma filter lengths straight from the unit records of tab_fill_pass (vvc355_bs_rec_frame): no side tables
    "deblock_bs_rec_pass": ("i", "ppp"),
    # the QP tables of deblock_frame_pass from the same records and two sidecars of one / two bytes per record (vvc355_qp_rec_frame)
    "deblock_qp_rec_pass": ("i", "ppp"),
    # the MvField table from one 64-byte record per prediction unit (vvc355_mvf_unit_frame): plain, affine (from control points, with the
    # PROF switches and offsets of the affine stage's records) and GPM units; the second entry is the record check, host only
    "mvf_unit_pass":    ("i", "ppp"),
    "mvf_unit_check":   ("i", "ppi"),
    # inverse luma mapping of a whole picture from the per-CTB slice index and the per-slice flags (vvc355_lmcs_frame): no job array
    "lmcs_frame_pass":  ("i", "pipp"),
    # a decoded picture's checksums where it lies (vvc355_pic_digest_frame): framecrc's Adler-32, the SEI's checksum and CRC per component
    "pic_digest_work_bytes": ("z", "pi"),
    "pic_digest_pass":  ("i", "pipp"),
    # the hand-over of a decoded picture (vvc355_pic_output_frame): crop and repack on the device, planar or semi-planar, as stored, 16 or 8 bit
    "pic_output_pass":  ("i", "pipp"),
    # the hand-back of collocated motion (vvc355_col_mvf_frame): one packed 16-byte entry per 8x8 luma block, DMVR refinement overlaid from
    # the inter stage's jobs and records; the two host helpers unpack an entry and put a picture's entries into a host MvField table
    "col_mvf_pass":     ("i", "ppp"),
    "col_mv_unpack":    ("v", "pppp"),
    "col_mvf_scatter":  ("v", "piiipi"),
    # is a ticket order one recon_frame_pass can run?  (host only)
    "recon_order_check": ("i", "piipi"),
    # every record-path stage of a picture in the documented order, validated as a whole before the first launch (vvc355_picture, HOST memory)
    "picture_pass":     ("i", "pip"),
    # the recorder (include/vvc_mi355_rec.h, host only): parsed units -> RECON commands, CTU table, ticket order, the three TB record lists
    # with their side records and level stream, arena slots; KEEP decided over the whole picture in end_picture
    "rec_create":       ("p", ""),
    "rec_destroy":      ("v", "p"),
    "rec_begin_picture": ("i", "pp"),
    "rec_ctu":          ("i", "piipi"),
    "rec_end_picture":  ("i", "pp"),
    "rec_fill_arena":   ("i", "pp"),
    "rec_bind":         ("i", "pz"),
    # the unit entry of the recorder: rec_ctu that also takes CIIP units and a vvc355_rec_pu per coding unit, and after end_picture the
    # cu / tu records with their QP sidecars, the motion records and the four inter-unit lists in raster CTU order
    "rec_ctu_units":    ("i", "piiippi"),
    "rec_units":        ("i", "pp"),
    # the transform-unit records the deblocking passes need (pcm bit, one chroma record per ISP unit, thin ISP partitions merged)
    "rec_deblock_units": ("i", "pp"),
}


def bind(lib: ctypes.CDLL, prefix: str, table: dict) -> None:
    """Attach restype/argtypes for every entry of `table` found under `prefix` in `lib`."""
    for name, (ret, args) in table.items():
        fn = getattr(lib, prefix + name)        # AttributeError = missing symbol: loud on purpose
        fn.restype = _C[ret]
        fn.argtypes = [_C[a] for a in args]


_lib = None


def load() -> ctypes.CDLL:
    """Load libvvc_mi355.so (once) and bind every declared entry point."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP extension first (__graft_entry__.build()); "
                "this package has no CPU fallback")
        lib = ctypes.CDLL(LIB_PATH)
        bind(lib, "vvc355_", SLOT_SIGNATURES)
        bind(lib, "vvc355_", RUNTIME_SIGNATURES)
        bind(lib, "vvc355_", BATCH_SIGNATURES)
        bind(lib, "vvc355_", FLAT_SIGNATURES)
        _lib = lib
    return _lib


class AlfJob(ctypes.Structure):
    """Mirror of vvc355_alf_job (include/vvc_mi355.h)."""
    _fields_ = [
        ("dst", ctypes.c_uint64), ("src", ctypes.c_uint64), ("coeff", ctypes.c_uint64),
        ("clip", ctypes.c_uint64), ("class_to_filt", ctypes.c_uint64),
        ("dst_stride", ctypes.c_int32), ("src_stride", ctypes.c_int32),
        ("w", ctypes.c_int16), ("h", ctypes.c_int16), ("vb_pos", ctypes.c_int16),
        ("ext_l", ctypes.c_int8), ("ext_r", ctypes.c_int8), ("ext_t", ctypes.c_int8), ("ext_b", ctypes.c_int8),
        ("hs", ctypes.c_int8), ("vs", ctypes.c_int8), ("pad_", ctypes.c_int8 * 4),
    ]


class McJob(ctypes.Structure):
    """Mirror of vvc355_mc_job."""
    _fields_ = [
        ("dst", ctypes.c_uint64), ("src", ctypes.c_uint64),
        ("dst_stride", ctypes.c_int32), ("src_stride", ctypes.c_int32),
        ("w", ctypes.c_int16), ("h", ctypes.c_int16),
        ("hf", ctypes.c_int8 * 8), ("vf", ctypes.c_int8 * 8),
        ("kind", ctypes.c_uint8), ("chroma", ctypes.c_uint8), ("hfrac", ctypes.c_uint8), ("vfrac", ctypes.c_uint8),
        ("denom", ctypes.c_int16), ("wx", ctypes.c_int16), ("ox", ctypes.c_int16), ("pad_", ctypes.c_int16),
    ]


class BlendJob(ctypes.Structure):
    """Mirror of vvc355_blend_job."""
    _fields_ = [
        ("dst", ctypes.c_uint64), ("src0", ctypes.c_uint64), ("src1", ctypes.c_uint64), ("aux", ctypes.c_uint64),
        ("dst_stride", ctypes.c_int32), ("src0_stride", ctypes.c_int32), ("src1_stride", ctypes.c_int32),
        ("step_x", ctypes.c_int32), ("step_y", ctypes.c_int32),
        ("w", ctypes.c_int16), ("h", ctypes.c_int16), ("mode", ctypes.c_int16), ("denom", ctypes.c_int16),
        ("w0", ctypes.c_int16), ("w1", ctypes.c_int16), ("o0", ctypes.c_int16), ("o1", ctypes.c_int16),
        ("pad_", ctypes.c_int32),
    ]


class SaoJob(ctypes.Structure):
    """Mirror of vvc355_sao_job."""
    _fields_ = [
        ("dst", ctypes.c_uint64), ("src", ctypes.c_uint64),
        ("dst_stride", ctypes.c_int32), ("src_stride", ctypes.c_int32),
        ("w", ctypes.c_int16), ("h", ctypes.c_int16), ("offset_val", ctypes.c_int16 * 5),
        ("type", ctypes.c_uint8), ("eo", ctypes.c_uint8), ("band_position", ctypes.c_uint8), ("restore", ctypes.c_uint8),
        ("borders", ctypes.c_uint8 * 4), ("vert_edge", ctypes.c_uint8 * 2), ("horiz_edge", ctypes.c_uint8 * 2),
        ("diag_edge", ctypes.c_uint8 * 4), ("pad_", ctypes.c_uint8 * 2),
    ]


class DeblockJob(ctypes.Structure):
    """Mirror of vvc355_deblock_job."""
    _fields_ = [
        ("pix", ctypes.c_uint64), ("stride", ctypes.c_int32),
        ("beta", ctypes.c_int32 * 4), ("tc", ctypes.c_int32 * 4),
        ("no_p", ctypes.c_uint8 * 4), ("no_q", ctypes.c_uint8 * 4),
        ("max_len_p", ctypes.c_uint8 * 4), ("max_len_q", ctypes.c_uint8 * 4),
        ("dir", ctypes.c_uint8), ("chroma", ctypes.c_uint8), ("flag", ctypes.c_uint8), ("pad_", ctypes.c_uint8),
    ]


class ItxJob(ctypes.Structure):
    """Mirror of vvc355_itx_job."""
    _fields_ = [
        ("coeffs", ctypes.c_uint64), ("dst", ctypes.c_uint64), ("dst_stride", ctypes.c_int32),
        ("trh", ctypes.c_uint8), ("trv", ctypes.c_uint8), ("log2_w", ctypes.c_uint8), ("log2_h", ctypes.c_uint8),
        ("nzw", ctypes.c_uint8), ("nzh", ctypes.c_uint8), ("range", ctypes.c_uint8), ("bd", ctypes.c_uint8),
        ("store_coeffs", ctypes.c_uint8), ("dq_flags", ctypes.c_uint8), ("dq_qp", ctypes.c_uint8), ("log2_matrix_size", ctypes.c_uint8),
        ("scale_matrix", ctypes.c_uint64), ("dc", ctypes.c_int16),
        ("mts_flags", ctypes.c_uint8), ("tu_flags", ctypes.c_uint8), ("mts_idx", ctypes.c_uint8), ("lfnst_idx", ctypes.c_uint8),
        ("c_idx", ctypes.c_uint8), ("pad_", ctypes.c_uint8),
    ]


class LfnstJob(ctypes.Structure):
    """Mirror of vvc355_lfnst_job."""
    _fields_ = [
        ("coeffs", ctypes.c_uint64), ("scale_matrix", ctypes.c_uint64),
        ("log2_w", ctypes.c_uint8), ("log2_h", ctypes.c_uint8), ("max_x", ctypes.c_uint8), ("max_y", ctypes.c_uint8),
        ("qp", ctypes.c_uint8), ("dequant", ctypes.c_uint8), ("dep_quant", ctypes.c_uint8), ("bit_depth", ctypes.c_uint8),
        ("range", ctypes.c_uint8), ("log2_matrix_size", ctypes.c_uint8), ("dc", ctypes.c_int16),
        ("pred_mode_intra", ctypes.c_int8), ("lfnst_idx", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 2),
    ]


class ReconCmd(ctypes.Structure):
    """Mirror of vvc355_recon_cmd (and of the oracle's orc_recon_cmd)."""
    _fields_ = [
        ("resid", ctypes.c_uint64),
        ("x0", ctypes.c_int16), ("y0", ctypes.c_int16), ("w", ctypes.c_int16), ("h", ctypes.c_int16),
        ("cu_x0", ctypes.c_int16), ("cu_y0", ctypes.c_int16), ("cb_width", ctypes.c_int16), ("cb_height", ctypes.c_int16),
        ("mode", ctypes.c_int8), ("kind", ctypes.c_uint8), ("c_idx", ctypes.c_uint8), ("ref_idx", ctypes.c_uint8),
        ("is_mip", ctypes.c_uint8), ("mip_mode", ctypes.c_uint8), ("mip_transposed", ctypes.c_uint8), ("isp_split", ctypes.c_uint8),
        ("bdpcm_flag", ctypes.c_uint8), ("joint", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 6),
    ]


class ReconCtu(ctypes.Structure):
    """Mirror of vvc355_recon_ctu."""
    _fields_ = [("first_cmd", ctypes.c_uint32), ("n_cmd", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class ReconFrame(ctypes.Structure):
    """Mirror of vvc355_recon_frame (and of the oracle's orc_recon_frame)."""
    _fields_ = [
        ("plane", ctypes.c_uint64 * 3), ("cmds", ctypes.c_uint64), ("ctus", ctypes.c_uint64), ("order", ctypes.c_uint64), ("state", ctypes.c_uint64),
        ("slice_idx", ctypes.c_uint64), ("ctb_to_col_bd", ctypes.c_uint64), ("ctb_to_row_bd", ctypes.c_uint64),
        ("stride", ctypes.c_int32 * 3), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ctb_width", ctypes.c_int32),
        ("ctb_height", ctypes.c_int32), ("n_work", ctypes.c_int32),
        ("ctb_log2", ctypes.c_uint8), ("hs", ctypes.c_uint8), ("vs", ctypes.c_uint8), ("wpp", ctypes.c_uint8), ("collocated", ctypes.c_uint8),
        ("pad_", ctypes.c_uint8), ("workgroups", ctypes.c_uint16), ("lmcs_model", ctypes.c_uint64),
    ]


class LmcsModel(ctypes.Structure):
    """Mirror of vvc355_lmcs_model / orc_lmcs_model."""
    _fields_ = [("pivot", ctypes.c_uint16 * 17), ("chroma_scale_coeff", ctypes.c_uint16 * 16), ("min_bin_idx", ctypes.c_uint8), ("max_bin_idx", ctypes.c_uint8),
                ("pad_", ctypes.c_uint8 * 4)]


RECON_MARK, RECON_PRED, RECON_CCLM, RECON_RESID, RECON_CIIP = 0, 1, 2, 3, 4
RECON_CTU_LIGHT, RECON_CTU_LUMA_LEFT, RECON_CTU_LUMA_UP = 1, 2, 4
TU_MTS_ENABLED, TU_EXPLICIT_MTS_INTRA, TU_ISP, TU_SBT, TU_SBT_HORIZONTAL, TU_SBT_POS, TU_INTRA, TU_MIP = 1, 2, 4, 8, 16, 32, 64, 128
ITX_DERIVE_TYPE = 1


class BipredJob(ctypes.Structure):
    """Mirror of vvc355_bipred_job (and of the oracle's orc_bipred_job)."""
    _fields_ = [
        ("dst", ctypes.c_uint64), ("ref0", ctypes.c_uint64), ("ref1", ctypes.c_uint64), ("rec", ctypes.c_uint64),
        ("dst_stride", ctypes.c_int32), ("ref0_stride", ctypes.c_int32), ("ref1_stride", ctypes.c_int32),
        ("mv", ctypes.c_int32 * 4),
        ("x", ctypes.c_int16), ("y", ctypes.c_int16), ("w", ctypes.c_int16), ("h", ctypes.c_int16),
        ("pic_w", ctypes.c_int16), ("pic_h", ctypes.c_int16),
        ("denom", ctypes.c_int16), ("w0", ctypes.c_int16), ("w1", ctypes.c_int16), ("o0", ctypes.c_int16), ("o1", ctypes.c_int16),
        ("chroma", ctypes.c_uint8), ("hs", ctypes.c_uint8), ("vs", ctypes.c_uint8), ("dmvr", ctypes.c_uint8),
        ("bdof", ctypes.c_uint8), ("hf_idx", ctypes.c_uint8), ("vf_idx", ctypes.c_uint8), ("weight_flag", ctypes.c_uint8),
        ("pred_flag", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 5),
        ("lmcs_lut", ctypes.c_uint64),
    ]


class RefPic(ctypes.Structure):
    """Mirror of vvc355_ref_pic."""
    _fields_ = [("plane", ctypes.c_uint64 * 3), ("stride", ctypes.c_int32 * 3), ("pad_", ctypes.c_int32)]


class InterPu(ctypes.Structure):
    """Mirror of vvc355_inter_pu."""
    _fields_ = [("x0", ctypes.c_int16), ("y0", ctypes.c_int16), ("cb_width", ctypes.c_int16), ("cb_height", ctypes.c_int16),
                ("num_sb_x", ctypes.c_uint8), ("num_sb_y", ctypes.c_uint8), ("dmvr_flag", ctypes.c_uint8), ("bdof_flag", ctypes.c_uint8),
                ("ciip_flag", ctypes.c_uint8), ("hpel_if_idx", ctypes.c_uint8), ("slice", ctypes.c_uint8), ("pad_", ctypes.c_uint8),
                ("first_job", ctypes.c_uint32)]


class InterSlice(ctypes.Structure):
    """Mirror of vvc355_inter_slice."""
    _fields_ = [("weighted_pred", ctypes.c_uint8), ("weighted_bipred", ctypes.c_uint8), ("log2_denom", ctypes.c_uint8 * 2),
                ("lmcs_used", ctypes.c_uint8), ("pad_", ctypes.c_uint8),
                ("weight", ctypes.c_int16 * 16 * 3 * 2), ("offset", ctypes.c_int16 * 16 * 3 * 2)]


class InterFrame(ctypes.Structure):
    """Mirror of vvc355_inter_frame."""
    _fields_ = [("dst", ctypes.c_uint64 * 3), ("mvf", ctypes.c_uint64), ("refs", ctypes.c_uint64), ("pus", ctypes.c_uint64), ("slices", ctypes.c_uint64),
                ("jobs_luma", ctypes.c_uint64), ("jobs_chroma", ctypes.c_uint64), ("records", ctypes.c_uint64), ("dmvr_mvf", ctypes.c_uint64),
                ("dst_stride", ctypes.c_int32 * 3), ("mvf_stride", ctypes.c_int32), ("n_pus", ctypes.c_int32), ("n_jobs", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("hs", ctypes.c_uint8), ("vs", ctypes.c_uint8), ("chroma_format_idc", ctypes.c_uint8), ("pixel_shift", ctypes.c_uint8),
                ("pad_", ctypes.c_uint8 * 4), ("lmcs_fwd_lut", ctypes.c_uint64)]


class AffineCu(ctypes.Structure):
    """Mirror of vvc355_affine_cu."""
    _fields_ = [("x0", ctypes.c_int16), ("y0", ctypes.c_int16), ("cb_width", ctypes.c_int16), ("cb_height", ctypes.c_int16),
                ("num_sb_x", ctypes.c_uint8), ("num_sb_y", ctypes.c_uint8), ("prof_flags", ctypes.c_uint8), ("slice", ctypes.c_uint8),
                ("first_job", ctypes.c_uint32), ("diff_mv", ctypes.c_int16 * 16 * 2 * 2)]


class AffineFrame(ctypes.Structure):
    """Mirror of vvc355_affine_frame."""
    _fields_ = [("pic", InterFrame), ("cus", ctypes.c_uint64), ("jobs_luma", ctypes.c_uint64), ("jobs_chroma", ctypes.c_uint64),
                ("n_cus", ctypes.c_int32), ("n_jobs", ctypes.c_int32)]


class GpmFrame(ctypes.Structure):
    """Mirror of vvc355_gpm_frame."""
    _fields_ = [("pic", InterFrame), ("cus", ctypes.c_uint64), ("jobs", ctypes.c_uint64), ("n_cus", ctypes.c_int32), ("n_jobs", ctypes.c_int32)]


class CiipCu(ctypes.Structure):
    """Mirror of vvc355_ciip_cu."""
    _fields_ = [("x0", ctypes.c_int16), ("y0", ctypes.c_int16), ("cb_width", ctypes.c_int16), ("cb_height", ctypes.c_int16),
                ("hpel_if_idx", ctypes.c_uint8), ("slice", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 2), ("first_job", ctypes.c_uint32),
                ("scratch_off", ctypes.c_uint32), ("cmd", ctypes.c_uint32 * 3)]


class CiipFrame(ctypes.Structure):
    """Mirror of vvc355_ciip_frame."""
    _fields_ = [("pic", InterFrame), ("cus", ctypes.c_uint64), ("jobs", ctypes.c_uint64), ("scratch", ctypes.c_uint64), ("cmds", ctypes.c_uint64),
                ("slice_idx", ctypes.c_uint64), ("ctb_to_col_bd", ctypes.c_uint64), ("ctb_to_row_bd", ctypes.c_uint64),
                ("n_cus", ctypes.c_int32), ("n_jobs", ctypes.c_int32), ("scratch_len", ctypes.c_int32), ("n_slices", ctypes.c_int32),
                ("n_cmds", ctypes.c_int32), ("ctb_width", ctypes.c_int32), ("ctb_height", ctypes.c_int32),
                ("ctb_log2", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 3)]


CIIP_NO_CMD = 0xFFFFFFFF             # vvc355_ciip_cu.cmd[c]: the component has no VVC355_RECON_CIIP command
# what vvc355_ciip_frame_build / _pass return for a frame they refuse (VVC355_CIIP_E_*)
(CIIP_E_FRAME, CIIP_E_SIZE, CIIP_E_CTB, CIIP_E_GRID, CIIP_E_COUNT, CIIP_E_DEPTH, CIIP_E_FORMAT, CIIP_E_RECORDS, CIIP_E_JOBS,
 CIIP_E_TABLES, CIIP_E_CMDS) = -1, -2, -3, -4, -5, -6, -7, -8, -9, -10, -11


class GpmJob(ctypes.Structure):
    """Mirror of vvc355_gpm_job (and of the oracle's orc_gpm_job)."""
    _fields_ = [("base", BipredJob), ("weights", ctypes.c_uint64), ("step_x", ctypes.c_int32), ("step_y", ctypes.c_int32)]


class BipredResult(ctypes.Structure):
    """Mirror of vvc355_bipred_result."""
    _fields_ = [("mv", ctypes.c_int32 * 4), ("bdof", ctypes.c_int32), ("min_sad", ctypes.c_int32),
                ("searched", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class SaoCtb(ctypes.Structure):
    """Mirror of vvc355_sao_ctb."""
    _fields_ = [("offset_val", (ctypes.c_int16 * 5) * 3), ("type_idx", ctypes.c_uint8 * 3), ("band_position", ctypes.c_uint8 * 3),
                ("eo_class", ctypes.c_uint8 * 3), ("pad_", ctypes.c_uint8)]


class SaoFrame(ctypes.Structure):
    """Mirror of vvc355_sao_frame (and of the oracle's orc_sao_frame)."""
    _fields_ = [
        ("dst", ctypes.c_uint64 * 3), ("src", ctypes.c_uint64 * 3), ("sao", ctypes.c_uint64), ("slice_idx", ctypes.c_uint64),
        ("ctb_to_col_bd", ctypes.c_uint64), ("ctb_to_row_bd", ctypes.c_uint64),
        ("dst_stride", ctypes.c_int32 * 3), ("src_stride", ctypes.c_int32 * 3),
        ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ctb_width", ctypes.c_int32), ("ctb_height", ctypes.c_int32),
        ("ctb_log2", ctypes.c_uint8), ("hs", ctypes.c_uint8), ("vs", ctypes.c_uint8), ("n_comp", ctypes.c_uint8),
        ("lfase", ctypes.c_uint8), ("no_tile_filter", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 2),
    ]


class AlfCtb(ctypes.Structure):
    """Mirror of vvc355_alf_ctb."""
    _fields_ = [("ctb_flag", ctypes.c_uint8 * 3), ("filt_set_idx_y", ctypes.c_uint8), ("alt_idx", ctypes.c_uint8 * 2),
                ("cc_idc", ctypes.c_uint8 * 2)]


class AlfSlice(ctypes.Structure):
    """Mirror of vvc355_alf_slice."""
    _fields_ = [("luma_coeff", ctypes.c_uint64 * 8), ("luma_clip_idx", ctypes.c_uint64 * 8), ("chroma_coeff", ctypes.c_uint64),
                ("chroma_clip_idx", ctypes.c_uint64), ("cc_coeff", ctypes.c_uint64 * 2)]


class AlfFrame(ctypes.Structure):
    """Mirror of vvc355_alf_frame (and of the oracle's orc_alf_frame)."""
    _fields_ = [
        ("dst", ctypes.c_uint64 * 3), ("src", ctypes.c_uint64 * 3), ("alf", ctypes.c_uint64), ("slices", ctypes.c_uint64),
        ("slice_idx", ctypes.c_uint64), ("ctb_to_col_bd", ctypes.c_uint64), ("ctb_to_row_bd", ctypes.c_uint64),
        ("dst_stride", ctypes.c_int32 * 3), ("src_stride", ctypes.c_int32 * 3),
        ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ctb_width", ctypes.c_int32), ("ctb_height", ctypes.c_int32),
        ("ctb_log2", ctypes.c_uint8), ("hs", ctypes.c_uint8), ("vs", ctypes.c_uint8), ("n_comp", ctypes.c_uint8),
        ("lfase", ctypes.c_uint8), ("lfate", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 2),
    ]


class MvField(ctypes.Structure):
    """Mirror of vvc355_mvfield (= the reference's MvField, vvc_ctu.h:195-202)."""
    _fields_ = [("mv", (ctypes.c_int32 * 2) * 2), ("ref_idx", ctypes.c_int8 * 2), ("hpel_if_idx", ctypes.c_uint8),
                ("bcw_idx", ctypes.c_uint8), ("pred_flag", ctypes.c_uint8), ("ciip_flag", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 2)]


class GpmCu(ctypes.Structure):
    """Mirror of vvc355_gpm_cu (gpm_mv: two MvField)."""
    _fields_ = [("x0", ctypes.c_int16), ("y0", ctypes.c_int16), ("cb_width", ctypes.c_int16), ("cb_height", ctypes.c_int16),
                ("partition_idx", ctypes.c_uint8), ("slice", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 2), ("first_job", ctypes.c_uint32),
                ("gpm_mv", MvField * 2)]


class BsFrame(ctypes.Structure):
    """Mirror of vvc355_bs_frame (and of the oracle's orc_bs_frame)."""
    _fields_ = [
        ("mvf", ctypes.c_uint64), ("ref_poc", ctypes.c_uint64), ("slice_idx", ctypes.c_uint64),
        ("ctb_to_col_bd", ctypes.c_uint64), ("ctb_to_row_bd", ctypes.c_uint64),
        ("tu_coded_flag", ctypes.c_uint64 * 3), ("tu_joint_cbcr", ctypes.c_uint64), ("pcmf", ctypes.c_uint64 * 2),
        ("tb_pos_x0", ctypes.c_uint64 * 2), ("tb_pos_y0", ctypes.c_uint64 * 2), ("tb_width", ctypes.c_uint64 * 2), ("tb_height", ctypes.c_uint64 * 2),
        ("cb_pos_x", ctypes.c_uint64), ("cb_pos_y", ctypes.c_uint64), ("cb_width", ctypes.c_uint64), ("cb_height", ctypes.c_uint64),
        ("msf", ctypes.c_uint64), ("iaf", ctypes.c_uint64),
        ("bs", (ctypes.c_uint64 * 3) * 2), ("max_len_p", ctypes.c_uint64 * 2), ("max_len_q", ctypes.c_uint64 * 2),
        ("width", ctypes.c_int32), ("height", ctypes.c_int32),
        ("min_tu_width", ctypes.c_int32), ("min_pu_width", ctypes.c_int32), ("min_cb_width", ctypes.c_int32), ("ctb_width", ctypes.c_int32),
        ("ctb_log2", ctypes.c_uint8), ("min_cb_log2", ctypes.c_uint8), ("hs", ctypes.c_uint8), ("vs", ctypes.c_uint8), ("n_comp", ctypes.c_uint8),
        ("lfase", ctypes.c_uint8), ("lfate", ctypes.c_uint8), ("pad_", ctypes.c_uint8),
    ]


class DeblockFrame(ctypes.Structure):
    """Mirror of vvc355_deblock_frame (and of the oracle's orc_deblock_frame)."""
    _fields_ = [
        ("plane", ctypes.c_uint64 * 3), ("bs", ctypes.c_uint64 * 3),
        ("max_len_p", ctypes.c_uint64), ("max_len_q", ctypes.c_uint64), ("tb_size_c", ctypes.c_uint64),
        ("qp_y", ctypes.c_uint64), ("qp_c", ctypes.c_uint64 * 2), ("db_params", ctypes.c_uint64),
        ("stride", ctypes.c_int32 * 3), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
        ("min_tu_width", ctypes.c_int32), ("min_cb_width", ctypes.c_int32), ("ctb_width", ctypes.c_int32),
        ("ladf_lower_bound", ctypes.c_int32 * 5),
        ("min_cb_log2", ctypes.c_uint8), ("ctb_log2", ctypes.c_uint8), ("hs", ctypes.c_uint8), ("vs", ctypes.c_uint8),
        ("n_comp", ctypes.c_uint8), ("vertical", ctypes.c_uint8), ("qp_bd_offset", ctypes.c_uint8), ("ladf_enabled", ctypes.c_uint8),
        ("num_ladf_intervals", ctypes.c_uint8), ("ladf_lowest_qp_offset", ctypes.c_int8), ("ladf_qp_offset", ctypes.c_int8 * 4),
        ("pad_", ctypes.c_uint8 * 6),
    ]


class AffineJob(ctypes.Structure):
    """Mirror of vvc355_affine_job (and of the oracle's orc_affine_job)."""
    _fields_ = [
        ("dst", ctypes.c_uint64), ("ref0", ctypes.c_uint64), ("ref1", ctypes.c_uint64), ("diff_mv", ctypes.c_uint64),
        ("dst_stride", ctypes.c_int32), ("ref0_stride", ctypes.c_int32), ("ref1_stride", ctypes.c_int32),
        ("mv", ctypes.c_int32 * 4),
        ("x", ctypes.c_int16), ("y", ctypes.c_int16), ("pic_w", ctypes.c_int16), ("pic_h", ctypes.c_int16),
        ("denom", ctypes.c_int16), ("w0", ctypes.c_int16), ("w1", ctypes.c_int16), ("o0", ctypes.c_int16), ("o1", ctypes.c_int16),
        ("pred_flag", ctypes.c_uint8), ("prof0", ctypes.c_uint8), ("prof1", ctypes.c_uint8), ("weight_flag", ctypes.c_uint8),
        ("pad_", ctypes.c_uint8 * 6),
        ("lmcs_lut", ctypes.c_uint64),
    ]


class DequantJob(ctypes.Structure):
    """Mirror of vvc355_dequant_job."""
    _fields_ = [
        ("coeffs", ctypes.c_uint64), ("scale_matrix", ctypes.c_uint64),
        ("log2_w", ctypes.c_uint8), ("log2_h", ctypes.c_uint8), ("min_x", ctypes.c_uint8), ("min_y", ctypes.c_uint8),
        ("max_x", ctypes.c_uint8), ("max_y", ctypes.c_uint8),
        ("qp", ctypes.c_uint8), ("ts", ctypes.c_uint8), ("dep_quant", ctypes.c_uint8), ("bit_depth", ctypes.c_uint8),
        ("range", ctypes.c_uint8), ("log2_matrix_size", ctypes.c_uint8),
        ("dc", ctypes.c_int16), ("pad_", ctypes.c_uint8 * 2),
    ]


class IntraJob(ctypes.Structure):
    """Mirror of vvc355_intra_job (and of the oracle's orc_intra_job)."""
    _fields_ = [
        ("plane", ctypes.c_uint64), ("stride", ctypes.c_int32),
        ("x", ctypes.c_int16), ("y", ctypes.c_int16), ("w", ctypes.c_int16), ("h", ctypes.c_int16),
        ("mode", ctypes.c_int16), ("cb_width", ctypes.c_int16), ("cb_height", ctypes.c_int16),
        ("left_avail", ctypes.c_int16), ("top_avail", ctypes.c_int16),
        ("plane_w", ctypes.c_int16), ("plane_h", ctypes.c_int16),
        ("c_idx", ctypes.c_uint8), ("ref_idx", ctypes.c_uint8), ("is_mip", ctypes.c_uint8), ("mip_mode", ctypes.c_uint8),
        ("mip_transposed", ctypes.c_uint8), ("isp_split", ctypes.c_uint8), ("bdpcm_flag", ctypes.c_uint8),
        ("cand_up_left", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 6),
    ]


class CclmJob(ctypes.Structure):
    """Mirror of vvc355_cclm_job / orc_cclm_job."""
    _fields_ = [
        ("luma", ctypes.c_uint64), ("cb", ctypes.c_uint64), ("cr", ctypes.c_uint64),
        ("luma_stride", ctypes.c_int32), ("cb_stride", ctypes.c_int32), ("cr_stride", ctypes.c_int32),
        ("x0", ctypes.c_int16), ("y0", ctypes.c_int16), ("width", ctypes.c_int16), ("height", ctypes.c_int16),
        ("top_avail_c", ctypes.c_int16), ("left_avail_c", ctypes.c_int16),
        ("mode", ctypes.c_uint8), ("hs", ctypes.c_uint8), ("vs", ctypes.c_uint8), ("avail_t", ctypes.c_uint8),
        ("avail_l", ctypes.c_uint8), ("collocated", ctypes.c_uint8), ("ctu_boundary", ctypes.c_uint8), ("pad_", ctypes.c_uint8),
    ]


class LmcsScaleJob(ctypes.Structure):
    """Mirror of vvc355_lmcs_scale_job / orc_lmcs_scale_job."""
    _fields_ = [
        ("luma", ctypes.c_uint64), ("luma_stride", ctypes.c_int32),
        ("x_vpdu", ctypes.c_int16), ("y_vpdu", ctypes.c_int16), ("pic_w", ctypes.c_int16), ("pic_h", ctypes.c_int16),
        ("size_y", ctypes.c_int16),
        ("avail_t", ctypes.c_uint8), ("avail_l", ctypes.c_uint8), ("min_bin_idx", ctypes.c_uint8), ("max_bin_idx", ctypes.c_uint8),
        ("pivot", ctypes.c_uint16 * 17), ("chroma_scale_coeff", ctypes.c_uint16 * 16), ("pad_", ctypes.c_uint16 * 6),
    ]


class ItxTu(ctypes.Structure):
    """Mirror of vvc355_itx_tu."""
    _fields_ = [("coeff_off", ctypes.c_uint32), ("x0", ctypes.c_int16), ("y0", ctypes.c_int16),
                ("log2_w", ctypes.c_uint8), ("log2_h", ctypes.c_uint8), ("nzw", ctypes.c_uint8), ("nzh", ctypes.c_uint8),
                ("c_idx", ctypes.c_uint8), ("qp", ctypes.c_uint8), ("flags", ctypes.c_uint8), ("tr", ctypes.c_uint8)]


LEVELS_INT32 = 1                     # vvc355_tb_levels.flags bit 0: the block's levels are int32 at job.coeffs
LEVELS_E_RANGE, LEVELS_E_ZERO_OUT = -1, -2


class TbLevels(ctypes.Structure):
    """Mirror of vvc355_tb_levels (the side record of a block's packed levels)."""
    _fields_ = [("groups", ctypes.c_uint64), ("first", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class IntraTu(ctypes.Structure):
    """Mirror of vvc355_intra_tu (one transform block of an intra coding unit)."""
    _fields_ = [("coeff_off", ctypes.c_uint32),
                ("log2_w", ctypes.c_uint8), ("log2_h", ctypes.c_uint8), ("nzw", ctypes.c_uint8), ("nzh", ctypes.c_uint8),
                ("c_idx", ctypes.c_uint8), ("qp", ctypes.c_uint8), ("flags", ctypes.c_uint8), ("tu_flags", ctypes.c_uint8),
                ("mts_idx", ctypes.c_uint8), ("lfnst_idx", ctypes.c_uint8), ("pred_mode_intra", ctypes.c_int8), ("pad_", ctypes.c_uint8)]


INTRA_TU_DEP_QUANT, INTRA_TU_LFNST = 1, 2
INTRA_TB_E_CLASS, INTRA_TB_E_BD, INTRA_TB_E_RANGE, INTRA_TB_E_LEVELS, INTRA_TB_E_MODE = -1, -2, -3, -4, -5


class IntraTbFrame(ctypes.Structure):
    """Mirror of vvc355_intra_tb_frame."""
    _fields_ = [("tus", ctypes.c_uint64), ("coeffs", ctypes.c_uint64), ("lv", ctypes.c_uint64), ("levels", ctypes.c_uint64),
                ("n_tus", ctypes.c_int32), ("class_first", ctypes.c_int32 * 6),
                ("range", ctypes.c_uint8), ("bd", ctypes.c_uint8), ("launch_mode", ctypes.c_uint8), ("pad_", ctypes.c_uint8)]


class InterTu(ctypes.Structure):
    """Mirror of vvc355_inter_tu (one coded transform block outside the in-order pass)."""
    _fields_ = [("coeff_off", ctypes.c_uint32), ("x0", ctypes.c_int16), ("y0", ctypes.c_int16),
                ("log2_w", ctypes.c_uint8), ("log2_h", ctypes.c_uint8), ("nzw", ctypes.c_uint8), ("nzh", ctypes.c_uint8),
                ("qp", ctypes.c_uint8), ("tu_flags", ctypes.c_uint8), ("flags", ctypes.c_uint8), ("joint_mts", ctypes.c_uint8)]


# vvc355_inter_tu.flags: bits 0-1 c_idx, then these; joint_mts = joint (bits 0-3) | mts_idx << 4
INTER_TU_DEP_QUANT, INTER_TU_KEEP, INTER_TU_UNIT_DX, INTER_TU_UNIT_DY = 4, 8, 16, 32
INTER_TB_BINS = 26
(INTER_TB_E_BINS, INTER_TB_E_BD, INTER_TB_E_RANGE, INTER_TB_E_LEVELS, INTER_TB_E_SIZE_Y, INTER_TB_E_SHIFT, INTER_TB_E_CHANNELS,
 INTER_TB_E_ORDER) = -1, -2, -3, -4, -5, -6, -7, -8


class InterTbFrame(ctypes.Structure):
    """Mirror of vvc355_inter_tb_frame."""
    _fields_ = [("tus", ctypes.c_uint64), ("coeffs", ctypes.c_uint64), ("lv", ctypes.c_uint64), ("levels", ctypes.c_uint64),
                ("plane", ctypes.c_uint64 * 3), ("scale_table", ctypes.c_uint64), ("stride", ctypes.c_int32 * 3),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("n_tus", ctypes.c_int32),
                ("hs", ctypes.c_uint8), ("vs", ctypes.c_uint8), ("size_y", ctypes.c_uint8), ("range", ctypes.c_uint8), ("bd", ctypes.c_uint8),
                ("pad_", ctypes.c_uint8 * 3), ("bin_first", (ctypes.c_int32 * (INTER_TB_BINS + 1)) * 2)]


class TsTu(ctypes.Structure):
    """Mirror of vvc355_ts_tu (one coded transform-skip block, BDPCM included)."""
    _fields_ = [("coeff_off", ctypes.c_uint32), ("x0", ctypes.c_int16), ("y0", ctypes.c_int16),
                ("log2_w", ctypes.c_uint8), ("log2_h", ctypes.c_uint8), ("nzw", ctypes.c_uint8), ("nzh", ctypes.c_uint8),
                ("qp", ctypes.c_uint8), ("pad_", ctypes.c_uint8), ("flags", ctypes.c_uint8), ("joint", ctypes.c_uint8)]


# vvc355_ts_tu.flags: bits 0-1 c_idx, then these; joint = bits 0-3 of vvc355_recon_cmd.joint
TS_TU_BDPCM, TS_TU_KEEP, TS_TU_UNIT_DX, TS_TU_UNIT_DY, TS_TU_VERTICAL = 4, 8, 16, 32, 64
TS_TB_CLASSES = 4
(TS_TB_E_CLASS, TS_TB_E_BD, TS_TB_E_RANGE, TS_TB_E_LEVELS, TS_TB_E_SIZE_Y, TS_TB_E_SHIFT, TS_TB_E_CHANNELS,
 TS_TB_E_ORDER) = -1, -2, -3, -4, -5, -6, -7, -8


class TsTbFrame(ctypes.Structure):
    """Mirror of vvc355_ts_tb_frame."""
    _fields_ = [("tus", ctypes.c_uint64), ("coeffs", ctypes.c_uint64), ("lv", ctypes.c_uint64), ("levels", ctypes.c_uint64),
                ("plane", ctypes.c_uint64 * 3), ("scale_table", ctypes.c_uint64), ("stride", ctypes.c_int32 * 3),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("n_tus", ctypes.c_int32),
                ("hs", ctypes.c_uint8), ("vs", ctypes.c_uint8), ("size_y", ctypes.c_uint8), ("range", ctypes.c_uint8), ("bd", ctypes.c_uint8),
                ("pad_", ctypes.c_uint8 * 3), ("class_first", (ctypes.c_int32 * (TS_TB_CLASSES + 1)) * 2)]


class ItxFrame(ctypes.Structure):
    """Mirror of vvc355_itx_frame."""
    _fields_ = [("tus", ctypes.c_uint64), ("jobs", ctypes.c_uint64), ("coeffs", ctypes.c_uint64), ("plane", ctypes.c_uint64 * 3),
                ("stride", ctypes.c_int32 * 3), ("n_tus", ctypes.c_int32),
                ("range", ctypes.c_uint8), ("bd", ctypes.c_uint8), ("pixel_shift", ctypes.c_uint8), ("tu_flags", ctypes.c_uint8),
                ("resid_jobs", ctypes.c_uint64), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("hs", ctypes.c_uint8), ("vs", ctypes.c_uint8), ("size_y", ctypes.c_uint8), ("pad_", ctypes.c_uint8),
                ("scale_table", ctypes.c_uint64)]


class LmcsScaleFrame(ctypes.Structure):
    """Mirror of vvc355_lmcs_scale_frame / orc_lmcs_scale_frame."""
    _fields_ = [("luma", ctypes.c_uint64), ("scale", ctypes.c_uint64), ("model", ctypes.c_uint64), ("slice_idx", ctypes.c_uint64),
                ("ctb_to_col_bd", ctypes.c_uint64), ("ctb_to_row_bd", ctypes.c_uint64),
                ("luma_stride", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ctb_width", ctypes.c_int32),
                ("ctb_log2", ctypes.c_uint8), ("size_y", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 6)]


class CuRec(ctypes.Structure):
    """Mirror of vvc355_cu_rec / vvc355_tu_rec (same layout)."""
    _fields_ = [("x0", ctypes.c_int16), ("y0", ctypes.c_int16), ("w", ctypes.c_uint8), ("h", ctypes.c_uint8), ("flags", ctypes.c_uint8), ("pad_", ctypes.c_uint8)]


class MvRec(ctypes.Structure):
    """Mirror of vvc355_mv_rec."""
    _fields_ = [("x0", ctypes.c_int16), ("y0", ctypes.c_int16), ("w", ctypes.c_uint8), ("h", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 2), ("mvf", ctypes.c_int32 * 6)]


class TabFill(ctypes.Structure):
    """Mirror of vvc355_tab_fill / orc_tab_fill."""
    _fields_ = [("cu", ctypes.c_uint64), ("tu", ctypes.c_uint64), ("mv", ctypes.c_uint64),
                ("n_cu", ctypes.c_int32), ("n_tu", ctypes.c_int32), ("n_mv", ctypes.c_int32), ("unit_pitch", ctypes.c_int32), ("mvf_pitch", ctypes.c_int32),
                ("hs", ctypes.c_uint8), ("vs", ctypes.c_uint8), ("ctb_log2", ctypes.c_uint8), ("pad_", ctypes.c_uint8),
                ("ctu_first_cu", ctypes.c_uint64), ("ctu_first_tu", ctypes.c_uint64), ("ctu_first_mv", ctypes.c_uint64),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ctb_width", ctypes.c_int32), ("ctb_height", ctypes.c_int32),
                ("mvf", ctypes.c_uint64),
                ("tu_coded_flag", ctypes.c_uint64 * 3), ("tu_joint_cbcr", ctypes.c_uint64), ("pcmf", ctypes.c_uint64 * 2),
                ("tb_pos_x0", ctypes.c_uint64 * 2), ("tb_pos_y0", ctypes.c_uint64 * 2), ("tb_width", ctypes.c_uint64 * 2), ("tb_height", ctypes.c_uint64 * 2),
                ("cb_pos_x", ctypes.c_uint64), ("cb_pos_y", ctypes.c_uint64), ("cb_width", ctypes.c_uint64), ("cb_height", ctypes.c_uint64),
                ("msf", ctypes.c_uint64), ("iaf", ctypes.c_uint64)]


class BsRecFrame(ctypes.Structure):
    """Mirror of vvc355_bs_rec_frame."""
    _fields_ = [("cu", ctypes.c_uint64), ("tu", ctypes.c_uint64), ("ctu_first_cu", ctypes.c_uint64), ("ctu_first_tu", ctypes.c_uint64),
                ("mvf", ctypes.c_uint64), ("ref_poc", ctypes.c_uint64), ("slice_idx", ctypes.c_uint64),
                ("ctb_to_col_bd", ctypes.c_uint64), ("ctb_to_row_bd", ctypes.c_uint64),
                ("bs", (ctypes.c_uint64 * 3) * 2), ("max_len_p", ctypes.c_uint64 * 2), ("max_len_q", ctypes.c_uint64 * 2),
                ("tb_width_c", ctypes.c_uint64), ("tb_height_c", ctypes.c_uint64),
                ("n_cu", ctypes.c_int32), ("n_tu", ctypes.c_int32), ("unit_pitch", ctypes.c_int32), ("mvf_pitch", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ctb_width", ctypes.c_int32), ("ctb_height", ctypes.c_int32),
                ("ctb_log2", ctypes.c_uint8), ("hs", ctypes.c_uint8), ("vs", ctypes.c_uint8), ("n_comp", ctypes.c_uint8),
                ("lfase", ctypes.c_uint8), ("lfate", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 2)]


# what vvc355_deblock_bs_rec_pass returns for a frame it refuses (VVC355_BS_REC_E_*)
(BS_REC_E_FRAME, BS_REC_E_SIZE, BS_REC_E_CTB, BS_REC_E_GRID, BS_REC_E_PITCH, BS_REC_E_COMP, BS_REC_E_SHIFT, BS_REC_E_COUNT,
 BS_REC_E_RECORDS, BS_REC_E_TABLES, BS_REC_E_OUTPUT) = -1, -2, -3, -4, -5, -6, -7, -8, -9, -10, -11


class QpRecFrame(ctypes.Structure):
    """Mirror of vvc355_qp_rec_frame."""
    _fields_ = [("cu", ctypes.c_uint64), ("tu", ctypes.c_uint64), ("ctu_first_cu", ctypes.c_uint64), ("ctu_first_tu", ctypes.c_uint64),
                ("cu_qp", ctypes.c_uint64), ("tu_qp_c", ctypes.c_uint64), ("qp_y", ctypes.c_uint64), ("qp_c", ctypes.c_uint64 * 2),
                ("n_cu", ctypes.c_int32), ("n_tu", ctypes.c_int32), ("unit_pitch", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ctb_width", ctypes.c_int32), ("ctb_height", ctypes.c_int32),
                ("ctb_log2", ctypes.c_uint8), ("n_comp", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 2)]


# what vvc355_deblock_qp_rec_pass returns for a frame it refuses (VVC355_QP_REC_E_*)
(QP_REC_E_FRAME, QP_REC_E_SIZE, QP_REC_E_CTB, QP_REC_E_GRID, QP_REC_E_PITCH, QP_REC_E_COMP, QP_REC_E_COUNT, QP_REC_E_RECORDS,
 QP_REC_E_SIDECAR, QP_REC_E_OUTPUT) = -1, -2, -3, -4, -5, -6, -7, -8, -9, -10


MVF_PLAIN, MVF_AFFINE, MVF_GPM = 0, 1, 2          # VVC355_MVF_*: vvc355_mvf_unit.kind
MVF_LINK_NONE = 0xFFFFFFFF                        # VVC355_MVF_LINK_NONE


class MvfUnit(ctypes.Structure):
    """Mirror of vvc355_mvf_unit (body: a MvField | cp_mv[2][3][2] | two MvField)."""
    _fields_ = [("x0", ctypes.c_int16), ("y0", ctypes.c_int16), ("w", ctypes.c_uint8), ("h", ctypes.c_uint8), ("kind", ctypes.c_uint8),
                ("aux", ctypes.c_uint8), ("link", ctypes.c_uint32), ("pf", ctypes.c_uint8), ("ref_idx", ctypes.c_int8 * 2),
                ("pad_", ctypes.c_uint8), ("body", ctypes.c_int32 * 12)]


class MvfUnitFrame(ctypes.Structure):
    """Mirror of vvc355_mvf_unit_frame."""
    _fields_ = [("units", ctypes.c_uint64), ("ctu_first", ctypes.c_uint64), ("mvf", ctypes.c_uint64), ("affine_cus", ctypes.c_uint64),
                ("n_units", ctypes.c_int32), ("n_affine_cus", ctypes.c_int32), ("mvf_pitch", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ctb_width", ctypes.c_int32), ("ctb_height", ctypes.c_int32),
                ("ctb_log2", ctypes.c_uint8), ("prof_disabled", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 2)]


# what vvc355_mvf_unit_pass returns for a frame it refuses (VVC355_MVF_UNIT_E_*)
(MVF_UNIT_E_FRAME, MVF_UNIT_E_SIZE, MVF_UNIT_E_COUNT, MVF_UNIT_E_CTB, MVF_UNIT_E_GRID, MVF_UNIT_E_PITCH, MVF_UNIT_E_RECORDS,
 MVF_UNIT_E_AFFINE) = -1, -2, -3, -4, -5, -6, -7, -8
# which rule a record breaks (vvc355_mvf_unit_check, VVC355_MVF_UNIT_R_*)
(MVF_UNIT_R_SIDE, MVF_UNIT_R_PLACE, MVF_UNIT_R_CTU, MVF_UNIT_R_PAD, MVF_UNIT_R_KIND, MVF_UNIT_R_AFF_SHAPE, MVF_UNIT_R_AFF_MODEL,
 MVF_UNIT_R_AFF_PRED, MVF_UNIT_R_AFF_LINK, MVF_UNIT_R_GPM_SHAPE, MVF_UNIT_R_GPM_RATIO, MVF_UNIT_R_GPM_PART,
 MVF_UNIT_R_GPM_PRED) = range(1, 14)


class LmcsFrame(ctypes.Structure):
    """Mirror of vvc355_lmcs_frame."""
    _fields_ = [("plane", ctypes.c_uint64), ("inv_lut", ctypes.c_uint64), ("slice_idx", ctypes.c_uint64), ("slice_lmcs_used", ctypes.c_uint64),
                ("stride", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ctb_width", ctypes.c_int32),
                ("ctb_height", ctypes.c_int32), ("n_slices", ctypes.c_int32), ("ctb_log2", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 3)]


# what vvc355_lmcs_frame_pass returns for a frame it refuses (VVC355_LMCS_FRAME_E_*)
(LMCS_FRAME_E_FRAME, LMCS_FRAME_E_BD, LMCS_FRAME_E_SIZE, LMCS_FRAME_E_CTB, LMCS_FRAME_E_GRID, LMCS_FRAME_E_STRIDE, LMCS_FRAME_E_COUNT,
 LMCS_FRAME_E_TABLES) = -1, -2, -3, -4, -5, -6, -7, -8

# VVC355_DIGEST_*: the bits of vvc355_pic_digest_frame.what
DIGEST_ADLER32, DIGEST_CHECKSUM, DIGEST_CRC = 1, 2, 4


class PicDigestResult(ctypes.Structure):
    """Mirror of vvc355_pic_digest_result."""
    _fields_ = [("adler32", ctypes.c_uint32), ("plane_adler32", ctypes.c_uint32 * 3), ("checksum", ctypes.c_uint32 * 3),
                ("crc", ctypes.c_uint16 * 3), ("n_comp", ctypes.c_uint16)]


class PicDigestFrame(ctypes.Structure):
    """Mirror of vvc355_pic_digest_frame."""
    _fields_ = [("plane", ctypes.c_uint64 * 3), ("result", ctypes.c_uint64), ("work", ctypes.c_uint64), ("stride", ctypes.c_int32 * 3),
                ("width", ctypes.c_int32 * 3), ("height", ctypes.c_int32 * 3), ("n_comp", ctypes.c_uint8), ("what", ctypes.c_uint8),
                ("pad_", ctypes.c_uint8 * 2)]


# what vvc355_pic_digest_pass returns for a frame it refuses (VVC355_PIC_DIGEST_E_*)
(PIC_DIGEST_E_FRAME, PIC_DIGEST_E_BD, PIC_DIGEST_E_WHAT, PIC_DIGEST_E_SIZE, PIC_DIGEST_E_STRIDE, PIC_DIGEST_E_TABLES) = -1, -2, -3, -4, -5, -6

# VVC355_OUT_*: vvc355_pic_output_frame.layout, and the bits of .flags
OUT_PLANAR, OUT_SEMI = 0, 1
OUT_SWAP_UV = 1


class PicOutputFrame(ctypes.Structure):
    """Mirror of vvc355_pic_output_frame."""
    _fields_ = [("src", ctypes.c_uint64 * 3), ("dst", ctypes.c_uint64 * 3), ("src_stride", ctypes.c_int32 * 3), ("dst_stride", ctypes.c_int32 * 3),
                ("width", ctypes.c_int32 * 3), ("height", ctypes.c_int32 * 3), ("n_comp", ctypes.c_uint8), ("layout", ctypes.c_uint8),
                ("out_bits", ctypes.c_uint8), ("flags", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 4)]


# what vvc355_pic_output_pass returns for a frame it refuses (VVC355_PIC_OUTPUT_E_*)
(PIC_OUTPUT_E_FRAME, PIC_OUTPUT_E_BD, PIC_OUTPUT_E_FORMAT, PIC_OUTPUT_E_SIZE, PIC_OUTPUT_E_STRIDE, PIC_OUTPUT_E_PLANES,
 PIC_OUTPUT_E_OVERLAP) = -1, -2, -3, -4, -5, -6, -7

COL_MVF_COMPRESS = 1                 # VVC355_COL_MVF_COMPRESS: vvc355_col_mvf_frame.flags bit 0


class ColMv(ctypes.Structure):
    """Mirror of vvc355_col_mv: [list][x, y]."""
    _fields_ = [("w", (ctypes.c_uint32 * 2) * 2)]


class ColMvfFrame(ctypes.Structure):
    """Mirror of vvc355_col_mvf_frame."""
    _fields_ = [("mvf", ctypes.c_uint64), ("col", ctypes.c_uint64), ("jobs_luma", ctypes.c_uint64), ("records", ctypes.c_uint64),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("mvf_stride", ctypes.c_int32), ("col_stride", ctypes.c_int32),
                ("n_jobs", ctypes.c_int32), ("flags", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 3)]


# what vvc355_col_mvf_pass returns for a frame it refuses (VVC355_COL_MVF_E_*)
(COL_MVF_E_FRAME, COL_MVF_E_SIZE, COL_MVF_E_STRIDE, COL_MVF_E_TABLES, COL_MVF_E_JOBS, COL_MVF_E_FLAGS, COL_MVF_E_OVERLAP) = -1, -2, -3, -4, -5, -6, -7

# what vvc355_recon_order_check returns for an order it refuses (VVC355_RECON_ORDER_E_*)
(RECON_ORDER_E_ARGS, RECON_ORDER_E_RANGE, RECON_ORDER_E_EMPTY, RECON_ORDER_E_DUPLICATE, RECON_ORDER_E_MISSING,
 RECON_ORDER_E_DEPENDENCY) = -1, -2, -3, -4, -5, -6


class StageRef(ctypes.Structure):
    """Mirror of vvc355_stage_ref: (DEVICE address, HOST address) of a stage's frame descriptor; host == 0 skips the stage."""
    _fields_ = [("dev", ctypes.c_uint64), ("host", ctypes.c_uint64)]


PIC_STAGES = ("tab_fill", "inter", "affine", "gpm", "ciip", "intra_tb", "bs_rec", "qp_rec", "alf", "inter_tb", "ts_tb", "lmcs_scale",
              "recon", "lmcs", "deblock_v", "deblock_h", "sao")


class Picture(ctypes.Structure):
    """Mirror of vvc355_picture (HOST memory)."""
    _fields_ = [(n, StageRef) for n in PIC_STAGES] + [
        ("alf_work", ctypes.c_uint64), ("recon_ctus_host", ctypes.c_uint64), ("recon_order_host", ctypes.c_uint64),
        ("refs", ctypes.c_uint64 * 32), ("done", ctypes.c_uint64), ("n_refs", ctypes.c_int32), ("pad_", ctypes.c_int32)]


# VVC355_PIC_STAGE_*: which stage refused the picture
(PIC_STAGE_PICTURE, PIC_STAGE_TAB_FILL, PIC_STAGE_INTER, PIC_STAGE_AFFINE, PIC_STAGE_GPM, PIC_STAGE_CIIP, PIC_STAGE_INTRA_TB,
 PIC_STAGE_BS_REC, PIC_STAGE_QP_REC, PIC_STAGE_ALF, PIC_STAGE_INTER_TB, PIC_STAGE_TS_TB, PIC_STAGE_LMCS_SCALE, PIC_STAGE_RECON,
 PIC_STAGE_RECON_ORDER, PIC_STAGE_LMCS, PIC_STAGE_DEBLOCK_V, PIC_STAGE_DEBLOCK_H, PIC_STAGE_SAO) = range(1, 20)
# codes of PIC_STAGE_PICTURE (VVC355_PIC_E_*)
PIC_E_NO_DEVICE_FRAME, PIC_E_PICTURE, PIC_E_CIIP_CMDS, PIC_E_SCALE_TABLE, PIC_E_REFS, PIC_E_CAPTURE = -1, -2, -3, -4, -5, -6


def pic_stage(ret: int) -> int:
    """VVC355_PIC_STAGE(ret)."""
    return (-ret) >> 8


def pic_code(ret: int) -> int:
    """VVC355_PIC_CODE(ret)."""
    return -((-ret) & 255)


class LmcsResidJob(ctypes.Structure):
    """Mirror of vvc355_lmcs_resid_job / orc_lmcs_resid_job."""
    _fields_ = [
        ("dst", ctypes.c_uint64), ("resid", ctypes.c_uint64), ("luma", ctypes.c_uint64),
        ("dst_stride", ctypes.c_int32), ("luma_stride", ctypes.c_int32),
        ("w", ctypes.c_int16), ("h", ctypes.c_int16), ("x_vpdu", ctypes.c_int16), ("y_vpdu", ctypes.c_int16),
        ("pic_w", ctypes.c_int16), ("pic_h", ctypes.c_int16), ("size_y", ctypes.c_int16),
        ("avail_l", ctypes.c_uint8), ("avail_t", ctypes.c_uint8), ("joint", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 7),
    ]


class PredJob(ctypes.Structure):
    """Mirror of vvc355_pred_job."""
    _fields_ = [
        ("dst", ctypes.c_uint64), ("src0", ctypes.c_uint64), ("src1", ctypes.c_uint64),
        ("dst_stride", ctypes.c_int32), ("src0_stride", ctypes.c_int32), ("src1_stride", ctypes.c_int32),
        ("hf0", ctypes.c_int8 * 8), ("vf0", ctypes.c_int8 * 8), ("hf1", ctypes.c_int8 * 8), ("vf1", ctypes.c_int8 * 8),
        ("w", ctypes.c_uint8), ("h", ctypes.c_uint8), ("chroma", ctypes.c_uint8), ("frac", ctypes.c_uint8),
        ("mode", ctypes.c_uint8), ("pad0_", ctypes.c_uint8),
        ("denom", ctypes.c_int16), ("w0", ctypes.c_int16), ("w1", ctypes.c_int16), ("o0", ctypes.c_int16), ("o1", ctypes.c_int16),
        ("pad1_", ctypes.c_int16 * 2),
    ]


# ---- the recorder (include/vvc_mi355_rec.h): its input PODs, its result and what it returns for input it refuses

class RecTb(ctypes.Structure):
    """Mirror of vvc355_rec_tb (one transform block as the parser left it; levels = HOST int32[w * h])."""
    _fields_ = [("levels", ctypes.c_uint64), ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("w", ctypes.c_int16), ("h", ctypes.c_int16),
                ("c_idx", ctypes.c_uint8), ("ts", ctypes.c_uint8), ("has_coeffs", ctypes.c_uint8), ("pad0_", ctypes.c_uint8),
                ("min_x", ctypes.c_uint8), ("min_y", ctypes.c_uint8), ("max_x", ctypes.c_uint8), ("max_y", ctypes.c_uint8),
                ("pad1_", ctypes.c_uint32)]


class RecTu(ctypes.Structure):
    """Mirror of vvc355_rec_tu (tbs = HOST vvc355_rec_tb[n_tbs])."""
    _fields_ = [("tbs", ctypes.c_uint64), ("n_tbs", ctypes.c_int32), ("x0", ctypes.c_int32), ("y0", ctypes.c_int32),
                ("w", ctypes.c_int16), ("h", ctypes.c_int16), ("coded_flag", ctypes.c_uint8 * 3), ("joint_cbcr_residual_flag", ctypes.c_uint8),
                ("pad_", ctypes.c_uint32)]


class RecCu(ctypes.Structure):
    """Mirror of vvc355_rec_cu (tus = HOST vvc355_rec_tu[n_tus], decoding order)."""
    _fields_ = [("tus", ctypes.c_uint64), ("n_tus", ctypes.c_int32), ("x0", ctypes.c_int32), ("y0", ctypes.c_int32),
                ("w", ctypes.c_int16), ("h", ctypes.c_int16),
                ("pred_mode", ctypes.c_uint8), ("tree_type", ctypes.c_uint8), ("coded_flag", ctypes.c_uint8), ("ciip_flag", ctypes.c_uint8),
                ("mode_y", ctypes.c_int8), ("mode_c", ctypes.c_int8), ("ref_idx", ctypes.c_uint8),
                ("mip_flag", ctypes.c_uint8), ("mip_mode", ctypes.c_uint8), ("mip_transposed", ctypes.c_uint8), ("mip_chroma_direct", ctypes.c_uint8),
                ("isp_type", ctypes.c_uint8), ("bdpcm", ctypes.c_uint8 * 3), ("lfnst_idx", ctypes.c_uint8), ("apply_lfnst", ctypes.c_uint8 * 3),
                ("mts_idx", ctypes.c_uint8), ("sbt_flag", ctypes.c_uint8), ("sbt_horizontal", ctypes.c_uint8), ("sbt_pos", ctypes.c_uint8),
                ("qp", ctypes.c_int8 * 4), ("pad_", ctypes.c_uint8 * 5)]


class RecParams(ctypes.Structure):
    """Mirror of vvc355_rec_params."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("ctb_log2", ctypes.c_uint8), ("bit_depth", ctypes.c_uint8), ("log2_transform_range", ctypes.c_uint8), ("chroma_format_idc", ctypes.c_uint8),
                ("qp_bd_offset", ctypes.c_int8), ("sps_min_qp_prime_ts", ctypes.c_uint8),
                ("mts_enabled", ctypes.c_uint8), ("explicit_mts_intra", ctypes.c_uint8), ("explicit_mts_inter", ctypes.c_uint8),
                ("ph_joint_cbcr_sign_flag", ctypes.c_uint8), ("ph_chroma_residual_scale_flag", ctypes.c_uint8), ("pack_levels", ctypes.c_uint8),
                ("pad_", ctypes.c_uint8 * 28)]


class RecResult(ctypes.Structure):
    """Mirror of vvc355_rec_result: HOST addresses into the recorder's buffers, valid until its next begin_picture."""
    _fields_ = [("cmds", ctypes.c_uint64), ("ctus", ctypes.c_uint64), ("order", ctypes.c_uint64),
                ("intra", ctypes.c_uint64), ("inter", ctypes.c_uint64), ("ts", ctypes.c_uint64),
                ("intra_lv", ctypes.c_uint64), ("inter_lv", ctypes.c_uint64), ("ts_lv", ctypes.c_uint64), ("levels", ctypes.c_uint64),
                ("n_levels", ctypes.c_uint64), ("arena_len", ctypes.c_uint64),
                ("n_cmds", ctypes.c_int32), ("n_ctus", ctypes.c_int32), ("n_work", ctypes.c_int32),
                ("n_intra", ctypes.c_int32), ("n_inter", ctypes.c_int32), ("n_ts", ctypes.c_int32),
                ("class_first", ctypes.c_int32 * 6), ("bin_first", (ctypes.c_int32 * (INTER_TB_BINS + 1)) * 2),
                ("ts_first", (ctypes.c_int32 * (TS_TB_CLASSES + 1)) * 2),
                ("keep", ctypes.c_int32), ("batched_scaled", ctypes.c_int32), ("walk_scaled", ctypes.c_int32), ("late_keep", ctypes.c_int32)]


REC_SLICE_DEP_QUANT, REC_SLICE_LMCS = 1, 2
(REC_E_ARGS, REC_E_STATE, REC_E_PARAMS, REC_E_CTU_RANGE, REC_E_CTU_TWICE, REC_E_CU_RECT, REC_E_TB_RECT, REC_E_SIDE, REC_E_C_IDX, REC_E_LEVELS,
 REC_E_CIIP, REC_E_NOMEM) = range(-1, -13, -1)


class RecPu(ctypes.Structure):
    """Mirror of vvc355_rec_pu (motion = HOST int32: MvFields, control points or the two GPM MvFields, by kind)."""
    _fields_ = [("motion", ctypes.c_uint64), ("kind", ctypes.c_uint8), ("merge_subblock_flag", ctypes.c_uint8),
                ("num_sb_x", ctypes.c_uint8), ("num_sb_y", ctypes.c_uint8), ("dmvr_flag", ctypes.c_uint8), ("bdof_flag", ctypes.c_uint8),
                ("hpel_if_idx", ctypes.c_uint8), ("bcw_idx", ctypes.c_uint8), ("pred_flag", ctypes.c_uint8), ("motion_model_idc", ctypes.c_uint8),
                ("gpm_partition_idx", ctypes.c_uint8), ("ref_idx", ctypes.c_int8 * 2), ("pad_", ctypes.c_uint8 * 11)]


class RecUnitsResult(ctypes.Structure):
    """Mirror of vvc355_rec_units_result: HOST addresses with the lifetime of RecResult."""
    _fields_ = [("cu", ctypes.c_uint64), ("cu_qp", ctypes.c_uint64), ("tu", ctypes.c_uint64), ("tu_qp_c", ctypes.c_uint64),
                ("ctu_first_cu", ctypes.c_uint64), ("ctu_first_tu", ctypes.c_uint64), ("mvf", ctypes.c_uint64), ("ctu_first_mvf", ctypes.c_uint64),
                ("inter", ctypes.c_uint64), ("affine", ctypes.c_uint64), ("gpm", ctypes.c_uint64), ("ciip", ctypes.c_uint64),
                ("n_cu", ctypes.c_int32), ("n_tu", ctypes.c_int32), ("n_mvf", ctypes.c_int32), ("n_inter", ctypes.c_int32),
                ("n_affine", ctypes.c_int32), ("n_gpm", ctypes.c_int32), ("n_ciip", ctypes.c_int32),
                ("n_inter_jobs", ctypes.c_int32), ("n_affine_jobs", ctypes.c_int32), ("n_gpm_jobs", ctypes.c_int32), ("n_ciip_jobs", ctypes.c_int32),
                ("ciip_scratch_len", ctypes.c_int32)]


class RecDeblockTus(ctypes.Structure):
    """Mirror of vvc355_rec_deblock_tus: the transform-unit records the deblocking passes need (HOST addresses)."""
    _fields_ = [("tu", ctypes.c_uint64), ("tu_qp_c", ctypes.c_uint64), ("ctu_first_tu", ctypes.c_uint64), ("n_tu", ctypes.c_int32), ("pad_", ctypes.c_int32)]


RECU_E_ARGS, RECU_E_MIXED, RECU_E_CIIP_SHAPE, RECU_E_MOTION, RECU_E_COUNT = range(-21, -26, -1)
