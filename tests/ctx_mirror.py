"""ctypes mirrors of include/vvc_mi355_ctx.h (the decoder state the four context-taking DSP slots read) and of the DSP table."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ReconstructedArea(ctypes.Structure):
    _fields_ = [("x", ctypes.c_int), ("y", ctypes.c_int), ("w", ctypes.c_int), ("h", ctypes.c_int)]


class SAOParams(ctypes.Structure):
    _fields_ = [("offset_abs", (ctypes.c_int * 4) * 3), ("offset_sign", (ctypes.c_int * 4) * 3), ("band_position", ctypes.c_uint8 * 3),
                ("eo_class", ctypes.c_int * 3), ("offset_val", (ctypes.c_int16 * 5) * 3), ("type_idx", ctypes.c_uint8 * 3)]


class CodingUnit(ctypes.Structure):
    _fields_ = [("x0", ctypes.c_int), ("y0", ctypes.c_int), ("cb_width", ctypes.c_int), ("cb_height", ctypes.c_int),
                ("intra_pred_mode_y", ctypes.c_int), ("intra_pred_mode_c", ctypes.c_int),
                ("intra_luma_ref_idx", ctypes.c_uint8), ("isp_split_type", ctypes.c_uint8), ("mip_chroma_direct_flag", ctypes.c_uint8),
                ("bdpcm_flag", ctypes.c_uint8 * 3)]


class Lmcs(ctypes.Structure):
    _fields_ = [("min_bin_idx", ctypes.c_uint8), ("max_bin_idx", ctypes.c_uint8), ("pivot", ctypes.c_uint16 * 17), ("chroma_scale_coeff", ctypes.c_uint16 * 16)]


class VVCFrameContext(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p * 3), ("linesize", ctypes.c_int * 3), ("width", ctypes.c_int), ("height", ctypes.c_int),
                ("bit_depth", ctypes.c_int), ("hshift", ctypes.c_uint8 * 3), ("vshift", ctypes.c_uint8 * 3),
                ("ctb_log2_size_y", ctypes.c_uint8), ("min_cb_log2_size_y", ctypes.c_uint8), ("min_cb_width", ctypes.c_int),
                ("sps_entropy_coding_sync_enabled_flag", ctypes.c_uint8), ("sps_chroma_vertical_collocated_flag", ctypes.c_uint8),
                ("imf", ctypes.c_void_p), ("imm", ctypes.c_void_p), ("imtf", ctypes.c_void_p), ("lmcs", Lmcs)]


class NA(ctypes.Structure):
    _fields_ = [("cand_up_left", ctypes.c_int)]


class LmcsCache(ctypes.Structure):
    _fields_ = [("x_vpdu", ctypes.c_int), ("y_vpdu", ctypes.c_int), ("chroma_scale", ctypes.c_int)]


class VVCLocalContext(ctypes.Structure):
    _fields_ = [("fc", ctypes.POINTER(VVCFrameContext)), ("cu", ctypes.POINTER(CodingUnit)),
                ("ras", (ReconstructedArea * 1024) * 2), ("num_ras", ctypes.c_int * 2), ("na", NA),
                ("ctb_left_flag", ctypes.c_uint8), ("ctb_up_flag", ctypes.c_uint8), ("end_of_tiles_x", ctypes.c_int), ("lmcs", LmcsCache)]


# The DSP table (VVC355DSPContext, member order of the reference's VVCDSPContext, vvcdsp.h:160-168) as an array of pointers:
# inter 3 * 56 + 11 + sad + 4 dmvr, intra 10, itx 3 + 441 + 1, lmcs 1, lf 6, sao 20, alf 5
TABLE_POINTERS = 3 * 56 + 16 + 10 + 445 + 1 + 6 + 20 + 5
INTRA0 = 3 * 56 + 16                         # first pointer of the intra sub-table: intra_cclm_pred, lmcs_scale_chroma, intra_pred, ...
SAO0 = INTRA0 + 10 + 445 + 1 + 6             # first pointer of the SAO sub-table; edge_restore[2] are its entries 18 and 19
LC = ctypes.POINTER(VVCLocalContext)
CCLM_FN = ctypes.CFUNCTYPE(None, LC, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int)
LMCS_SCALE_FN = ctypes.CFUNCTYPE(None, LC, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int)
INTRA_PRED_FN = ctypes.CFUNCTYPE(None, LC, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int)


def context_slots(tab):
    """(intra_cclm_pred, lmcs_scale_chroma, intra_pred) of a filled table, callable with a mirror context."""
    return CCLM_FN(tab[INTRA0 + 0]), LMCS_SCALE_FN(tab[INTRA0 + 1]), INTRA_PRED_FN(tab[INTRA0 + 2])


def load_host():
    lib = ctypes.CDLL(os.path.join(ROOT, "ffvvc_amd", "libvvc_mi355_host.so"))
    return lib
