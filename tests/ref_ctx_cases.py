"""Deterministic cases for the slots that take the decoder's context: intra.intra_pred, intra.intra_cclm_pred,
intra.lmcs_scale_chroma, and the two availability functions they all ask (ff_vvc_get_top_available / _left_available).

Same discipline as tests/ref_cases.py (whose generator this module uses): seed 0 is the committed list, other seeds are rounds of
the sweep; the planes a call may write are handed over whole and compared whole.  The cases are cut from small pictures of
tests/recon_cases.ReconWork: valid partitions walked in decoding order, the only order in which the reference's search through
the reconstructed areas is defined.  Every picture has an interior 2 x 2 CTU corner, a tile column boundary and partial CTUs at
the right and bottom edges.  A case is the decoder state at one call, as the mirror structs of tests/ctx_mirror.py, plus the call's
arguments; a *side* is a callable side(case, lc) that makes the call on that state:

    reference      ref_<slot>_ctx / ref_*_available of oracle/ref_shim_intra.c: real slot on real structs
    project, CPU   vvc355_ctx_flatten_* of the host shim, then the oracle's orc_*_flat
    project, GPU   the slot of the installed table (ff_vvc_dsp_init_mi355_ctx)

The picture's planes hold random samples everywhere: what lies in areas that are not reconstructed yet is different from any
value a substitution would produce, so a side that reads a sample the reference does not read differs.
"""
import ctypes

import numpy as np

import ctx_mirror as cm
import recon_cases
import ref_cases
from ffvvc_amd import abi
from ref_cases import Gen, GROUP

SLOTS = ("intra_pred", "intra_cclm_pred", "lmcs_scale_chroma", "top_available", "left_available")
DEVICE_SLOTS = SLOTS[:3]
UNBOUNDED = 16384          # a request larger than any picture
KEEP_INTRA, KEEP_LMCS = 3, 2          # one call in so many becomes a case: the device test replays the lists call by call, a few hundred per bit depth
LC = cm.LC

# (ctb_log2, width, height, hshift, vshift, slices, tiles, wavefront, collocated chroma, bit depth): 5 x 3, 4 x 3 and 3 x 2 CTUs
PICTURES = [
    (5, 136, 72, 1, 1, 3, True, 0, 0, 8),
    (5, 136, 72, 0, 0, 1, True, 1, 0, 10),
    (5, 136, 72, 1, 0, 2, False, 0, 1, 12),
    (6, 200, 136, 1, 0, 2, True, 0, 0, 8),
    (6, 200, 136, 1, 1, 1, False, 1, 1, 10),
    (6, 200, 136, 0, 0, 3, True, 0, 0, 12),
    (7, 264, 136, 1, 1, 2, True, 1, 1, 12),
    (7, 264, 136, 0, 0, 1, True, 0, 0, 8),
    (7, 264, 136, 1, 0, 2, False, 1, 0, 10),
]


class GenRng:
    """The three draws recon_cases uses, on the counter-based generator of ref_cases (no numpy random stream in a digest)."""

    def __init__(self, g):
        self.g = g

    def random(self):
        return float(self.g.u64(1)[0] >> np.uint64(11)) / float(1 << 53)

    def integers(self, lo, hi=None, size=None):
        lo, hi = (0, lo) if hi is None else (lo, hi)
        return self.g.ints(int(lo), int(hi), None if size is None else (size,) if np.isscalar(size) else size)

    def choice(self, seq, size=None, replace=True):
        seq = list(seq)
        if size is None:
            return seq[self.g.ints(0, len(seq))]
        assert not replace
        out = []
        for _ in range(size):
            out.append(seq.pop(self.g.ints(0, len(seq))))
        return np.array(out)


class Picture:
    """One partition with its planes, tables and LMCS model: shared, read-only, by the cases cut from it."""

    def __init__(self, g, cfg, idx):
        self.ctb_log2, self.w, self.h, self.hs, self.vs, n_slices, tiles, self.wpp, self.collocated, self.bd = cfg
        self.idx = idx
        rng = GenRng(g)
        self.work = recon_cases.ReconWork(rng, self.w, self.h, self.ctb_log2, self.hs, self.vs, intra_frac=0.9, n_slices=n_slices, tiles=tiles,
                                          cclm_frac=0.3, isp_p=0.3 if self.hs + self.vs else 0.6, lmcs=True,
                                          min_cu=4 if self.hs + self.vs == 0 else 8)          # 4-sample coding units where chroma keeps 4 samples too
        self.planes = [ref_cases.pixels(g, (self.h >> (self.vs if c else 0), self.w >> (self.hs if c else 0)), self.bd, "uniform") for c in range(3)]
        self.min_cb_w = self.w // 4
        n_cb = ((self.h + 3) // 4) * self.min_cb_w
        self.tabs = [np.zeros(n_cb, np.uint8) for _ in range(3)]          # imf, imm, imtf: a call patches the entry it reads
        # LMCS model: increasing pivots; every other picture uses a narrow bin range
        cuts = np.sort(rng.choice(np.arange(1, 1 << self.bd), size=15, replace=False))
        self.pivot = [0] + [int(v) for v in cuts] + [min(1 << self.bd, 65535)]
        self.scale_coeff = [g.ints(1024, 4096) for _ in range(16)]
        self.bins = (g.ints(4, 7), g.ints(8, 11)) if idx & 1 else (0, 15)
        self.angular = 7 * idx          # running angular mode of _walk

    def frame_context(self, planes):
        fc = cm.VVCFrameContext()
        fc.width, fc.height, fc.bit_depth, fc.ctb_log2_size_y, fc.min_cb_log2_size_y, fc.min_cb_width = self.w, self.h, self.bd, self.ctb_log2, 2, self.min_cb_w
        for c in range(3):
            fc.hshift[c], fc.vshift[c] = (self.hs, self.vs) if c else (0, 0)
            fc.data[c], fc.linesize[c] = planes[c].ctypes.data, planes[c].strides[0]
        fc.sps_entropy_coding_sync_enabled_flag, fc.sps_chroma_vertical_collocated_flag = self.wpp, self.collocated
        fc.imf, fc.imm, fc.imtf = (t.ctypes.data for t in self.tabs)
        fc.lmcs.min_bin_idx, fc.lmcs.max_bin_idx = self.bins
        for i in range(17):
            fc.lmcs.pivot[i] = self.pivot[i]
        for i in range(16):
            fc.lmcs.chroma_scale_coeff[i] = self.scale_coeff[i]
        return fc

    def digest(self, hasher):
        hasher.update(repr((self.ctb_log2, self.w, self.h, self.hs, self.vs, self.wpp, self.collocated, self.bd, self.pivot, self.scale_coeff, self.bins)).encode())
        for p in self.planes:
            hasher.update(p.tobytes())


class CtxCase:
    """The decoder state at one call.  `ras` are the CTU's reconstructed areas so far ([luma, chroma] arrays of x, y, w, h); `ctu` is
    (ctb_left_flag, ctb_up_flag, end_of_tiles_x); `cu` the coding unit's members; `mip` what the tables hold at the block
    (imf, imm, imtf); `args` the integer arguments after the context; `coeff` / `cache` belong to lmcs_scale_chroma."""
    __slots__ = ("slot", "key", "params", "pic", "ras", "ctu", "cu", "cand_up_left", "mip", "args", "coeff", "cache", "ret")

    def __init__(self, slot, pic, ras, ctu, cu, cand_up_left, mip, args, params, coeff=None, cache=(-1, -1, 0)):
        self.slot, self.pic, self.ras, self.ctu, self.cu, self.cand_up_left, self.mip, self.args = slot, pic, ras, ctu, cu, cand_up_left, mip, args
        self.key, self.coeff, self.cache, self.ret = (pic.bd,), coeff, cache, slot.endswith("available")
        self.params = dict(picture=pic.idx, bd=pic.bd, ctb=1 << pic.ctb_log2, chroma=(pic.hs, pic.vs), args=args, cu=cu, ctu=ctu, areas=[len(r) for r in ras], **params)


def _walk(slot, pic, g, out, wide):
    work = pic.work
    ctb, w = 1 << pic.ctb_log2, pic.w
    for rs in work.order:
        rs = int(rs)
        rx, ry = rs % work.ncx, rs // work.ncx
        # ff_vvc_decode_neighbour (vvc_ctu.c:2468-2495)
        left_tile = rx > 0 and work.col_bd[rx] != work.col_bd[rx - 1]
        upper_tile = ry > 0 and work.row_bd[ry] != work.row_bd[ry - 1]
        upper_slice = ry > 0 and work.slice_idx[rs] != work.slice_idx[rs - work.ncx]
        end_of_tiles_x = min(rx * ctb + ctb, w) if work.col_bd[rx] != work.col_bd[rx + 1] else w
        ctu = (int(rx > 0 and not left_tile), int(ry > 0 and not upper_tile and not upper_slice), int(end_of_tiles_x))
        ras = [[], []]
        luma_mip = {}
        first, n = int(work.ctus[rs]["first_cmd"]), int(work.ctus[rs]["n_cmd"])
        for k in range(n):
            c = work.cmds[first + k]
            kind, c_idx = int(c["kind"]), int(c["c_idx"])
            x0, y0, bw, bh = int(c["x0"]), int(c["y0"]), int(c["w"]), int(c["h"])
            if kind == abi.RECON_MARK:
                sx, sy = (pic.hs, pic.vs) if c_idx else (0, 0)
                ras[int(c_idx > 0)].append((x0 >> sx, y0 >> sy, bw >> sx, bh >> sy))
                continue
            snap = [np.array(r, np.int32).reshape(-1, 4) for r in ras]
            cu = dict(x0=int(c["cu_x0"]), y0=int(c["cu_y0"]), cb_width=int(c["cb_width"]), cb_height=int(c["cb_height"]),
                      intra_pred_mode_y=int(c["mode"]), intra_pred_mode_c=int(c["mode"]), intra_luma_ref_idx=int(c["ref_idx"]),
                      isp_split_type=int(c["isp_split"]), mip_chroma_direct_flag=0, bdpcm_flag=[0, 0, 0])
            # ff_vvc_set_neighbour_available (vvc_ctu.c:2497-2510)
            x0b, y0b = x0 & (ctb - 1), y0 & (ctb - 1)
            cand_up, cand_left = bool(ctu[1] or y0b), bool(ctu[0] or x0b)
            cul = int((cand_left and cand_up) if (x0b or y0b) else (ctu[0] and ctu[1]))
            if kind == abi.RECON_PRED:
                mip = (int(c["is_mip"]), int(c["mip_mode"]), int(c["mip_transposed"]))
                if c_idx == 0:
                    luma_mip[(cu["x0"], cu["y0"])] = mip
                    cu["mip_chroma_direct_flag"] = g.ints(0, 2)          # not read for luma
                    cu["bdpcm_flag"][0] = int(c["bdpcm_flag"])
                else:
                    lm = luma_mip.get((cu["x0"], cu["y0"]), (0, 0, 0))
                    if lm[0]:          # chroma of a MIP coding unit: the table says MIP; at 4:4:4 half of them take it over (MipChromaDirectFlag)
                        direct = int(pic.hs == 0 and pic.vs == 0 and (cu["x0"] >> 3) & 1)
                        mip, cu["mip_chroma_direct_flag"] = lm, direct
                    elif int(c["mode"]) in (18, 50) and bw <= 32 and bh <= 32 and (cu["y0"] >> 3) & 1:
                        cu["bdpcm_flag"][c_idx] = 1          # chroma BDPCM: horizontal / vertical without PDPC
                sx, sy = (pic.hs, pic.vs) if c_idx else (0, 0)
                # the shape the wide-angle mapping looks at, and the modes it remaps for that shape, the most extreme first
                nw, nh = (cu["cb_width"], cu["cb_height"]) if cu["isp_split_type"] and not c_idx else (bw >> sx, bh >> sy)
                remapped = sorted((m for m in range(2, 67) if ref_cases.wide_angle(m, nw, nh) != m), reverse=nw > nh)
                steer = c_idx == 0 and not mip[0] and not cu["bdpcm_flag"][0]
                rare = ((cu["isp_split_type"] and cu["cb_width"] == 4) or                          # 1-wide ISP parts,
                        (steer and max(nw, nh) >= 8 * min(nw, nh)) or                            # blocks of 8:1 and 16:1, which alone reach the outermost modes,
                        (y0b == 0 and ctu[1] and ctu[2] < w and ctu[2] - x0 < bw + bh))          # and top-row requests an interior tile end clips: all of them
                if slot == "intra_pred" and (g.ints(0, KEEP_INTRA) == 0 or rare):
                    shape = (nw > nh, max(nw, nh) // min(nw, nh))          # orientation and aspect ratio: what the mapping depends on
                    if steer and remapped and (shape[1] >= 8 or wide.setdefault(shape, 0) & 1 == 0):
                        # a non-square block: every other one of its ratio (every one of the few 8:1 and 16:1 blocks) walks the modes the
                        # mapping moves for that ratio, the outermost first (those no flatter block reaches), so that every mode
                        # -14 .. -1 and 67 .. 80 occurs
                        step = wide.setdefault(shape, 0) // (1 if shape[1] >= 8 else 2)
                        cu["intra_pred_mode_y"] = remapped[step % len(remapped)]
                    elif steer and remapped:
                        # the other non-square blocks walk through all angular modes, wide and tall ones on their own (any mode is legal
                        # on any block) ...
                        cu["intra_pred_mode_y"] = 2 + wide.setdefault(shape[0], 0) % 65
                        wide[shape[0]] += 1
                    elif steer and len(out) & 3:
                        # ... and so do three square blocks in four; the rest keep the partition's own random modes, planar and DC among them
                        cu["intra_pred_mode_y"] = 2 + pic.angular % 65
                        pic.angular += 1
                    if steer and remapped:
                        wide[shape] += 1
                    prm = dict(mode=cu["intra_pred_mode_c" if c_idx else "intra_pred_mode_y"], ref_idx=cu["intra_luma_ref_idx"], isp=cu["isp_split_type"],
                               mip=mip, c_idx=c_idx, rs=rs, cmd=k)
                    out.append(CtxCase(slot, pic, snap, ctu, cu, cul, mip, (x0, y0, bw, bh, c_idx), prm))
                elif slot.endswith("available") and c_idx < 2:
                    side = (bw >> sx) if slot[0] == "t" else (bh >> sy)
                    for target in (1, side, UNBOUNDED):
                        out.append(CtxCase(slot, pic, snap, ctu, cu, cul, mip, (x0 >> sx, y0 >> sy, target, c_idx), dict(c_idx=c_idx)))
            elif kind == abi.RECON_CCLM and slot == "intra_cclm_pred":
                out.append(CtxCase(slot, pic, snap, ctu, cu, cul, (0, 0, 0), (x0, y0, bw, bh), dict(mode=int(c["mode"]))))
            elif kind == abi.RECON_CCLM and slot.endswith("available"):          # the chroma blocks CCLM predicts are blocks of the picture too
                side = (bw >> pic.hs) if slot[0] == "t" else (bh >> pic.vs)
                for target in (1, side, UNBOUNDED):
                    out.append(CtxCase(slot, pic, snap, ctu, cu, cul, (0, 0, 0), (x0 >> pic.hs, y0 >> pic.vs, target, 1), dict(c_idx=1)))
            elif kind == abi.RECON_RESID and (int(c["joint"]) & 8) and slot == "lmcs_scale_chroma" and g.ints(0, KEEP_LMCS) == 0:
                coeff = ref_cases.field(g, (bh, bw), -(1 << (pic.bd + 1)), (1 << (pic.bd + 1)) - 1, ref_cases.dist_cycle(len(out)), np.int32)
                out.append(CtxCase(slot, pic, snap, ctu, cu, cul, (0, 0, 0), (bw, bh, cu["x0"], cu["y0"]), dict(cache="cold"), coeff=coeff))
    return out


_pictures = {}


def pictures(seed=0):
    if seed not in _pictures:
        _pictures[seed] = [Picture(Gen(f"ctx-picture-{i}", seed), cfg, i) for i, cfg in enumerate(PICTURES)]
        if len(_pictures) > 2:
            del _pictures[min(k for k in _pictures if k != seed and k != 0)]
    return _pictures[seed]


def cases(slot, seed=0):
    out, wide = [], {}          # wide: luma blocks met so far per non-square shape (_walk steers their modes)
    for pic in pictures(seed):
        pic.angular = 7 * pic.idx
        _walk(slot, pic, Gen(f"{slot}-{pic.idx}", seed), out, wide)
    return out


def with_cache(case, scale):
    """The lmcs_scale_chroma case once more, with the reference's per-VPDU cache already holding this unit's scale."""
    size = min(1 << case.pic.ctb_log2, 64)
    c = CtxCase(case.slot, case.pic, case.ras, case.ctu, case.cu, case.cand_up_left, case.mip, case.args, dict(cache="matching"), coeff=case.coeff,
                cache=(case.args[2] & ~(size - 1), case.args[3] & ~(size - 1), int(scale)))
    return c


def groups(slot, seed=0):
    by_key = {}
    for c in cases(slot, seed):
        by_key.setdefault(c.key, []).append(c)
    return [(f"{slot}/{key[0]}/{k // GROUP}", lst[k:k + GROUP]) for key, lst in by_key.items() for k in range(0, len(lst), GROUP)]


# ---------------------------------------------------------------------------------------------------------------- running

def context(case, planes):
    """(lc, objects to keep alive) for one call on `planes`."""
    pic = case.pic
    fc = pic.frame_context(planes)
    lc = cm.VVCLocalContext()
    lc.fc = ctypes.pointer(fc)
    cu = cm.CodingUnit()
    for name, v in case.cu.items():
        if name == "bdpcm_flag":
            for i in range(3):
                cu.bdpcm_flag[i] = v[i]
        else:
            setattr(cu, name, v)
    lc.cu = ctypes.pointer(cu)
    for t in range(2):
        a = np.ascontiguousarray(case.ras[t][:1024])
        lc.num_ras[t] = len(a)
        if len(a):
            ctypes.memmove(ctypes.addressof(lc.ras[t]), a.ctypes.data, a.nbytes)
    lc.na.cand_up_left = case.cand_up_left
    lc.ctb_left_flag, lc.ctb_up_flag, lc.end_of_tiles_x = case.ctu
    lc.lmcs.x_vpdu, lc.lmcs.y_vpdu, lc.lmcs.chroma_scale = case.cache
    if case.slot == "intra_pred":          # the table entries the call reads (the tables are the picture's: valid until the next context())
        at = (case.args[1] >> 2) * pic.min_cb_w + (case.args[0] >> 2)
        for t, v in zip(pic.tabs, case.mip):
            t[at] = v
    return lc, (fc, cu)


def run(case, side):
    """Call `side` on private copies of the picture's planes; returns what counts as the result: the three planes whole, for
    lmcs_scale_chroma the scaled block as well, for the availability functions the return value."""
    pic = case.pic
    planes = [p.copy() for p in pic.planes]
    lc, keep = context(case, planes)
    res = side(case, lc)
    outs = planes
    if case.slot == "lmcs_scale_chroma":
        outs = planes + [res]
    elif case.ret:
        outs = [np.array([res], np.int64)]
    del keep
    return outs


def input_digest(hasher, case):
    hasher.update(repr((case.slot, case.args, sorted(case.cu.items()), case.ctu, case.cand_up_left, case.mip, case.cache)).encode())
    for r in case.ras:
        hasher.update(np.ascontiguousarray(r).tobytes())
    if case.coeff is not None:
        hasher.update(case.coeff.tobytes())


def group_input_digest(hasher, cases_):
    seen = set()
    for c in cases_:
        if id(c.pic) not in seen:
            seen.add(id(c.pic))
            c.pic.digest(hasher)
        input_digest(hasher, c)


def first_difference(case, want, got):
    for i, (x, y) in enumerate(zip(want, got)):
        if not np.array_equal(x, y):
            bad = np.argwhere(x != y)
            at = tuple(bad[0])
            return f"{case.slot} {case.params}: output #{i} differs in {len(bad)} elements, first at {list(map(int, at))}: want {x[at]} got {y[at]}"
    return None


# ---------------------------------------------------------------------------------------------------------------- sides

def reference_side(ref):
    ref.ref_intra_pred_ctx.argtypes = [LC] + [ctypes.c_int] * 5
    ref.ref_intra_cclm_pred_ctx.argtypes = [LC] + [ctypes.c_int] * 4
    ref.ref_lmcs_scale_chroma_ctx.argtypes = [LC, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 4
    for name in ("ref_top_available", "ref_left_available"):
        getattr(ref, name).argtypes = [LC] + [ctypes.c_int] * 4
    for name in ("ref_intra_pred_ctx", "ref_intra_cclm_pred_ctx", "ref_lmcs_scale_chroma_ctx"):
        getattr(ref, name).restype = None

    def side(case, lc):
        if case.slot == "lmcs_scale_chroma":
            dst = np.full_like(case.coeff, 0x5A5A5A)
            ref.ref_lmcs_scale_chroma_ctx(lc, dst.ctypes.data, case.coeff.ctypes.data, *case.args)
            side.cache = (lc.lmcs.x_vpdu, lc.lmcs.y_vpdu, lc.lmcs.chroma_scale)
            return dst
        name = {"intra_pred": "ref_intra_pred_ctx", "intra_cclm_pred": "ref_intra_cclm_pred_ctx"}.get(case.slot, "ref_" + case.slot)
        return getattr(ref, name)(lc, *case.args)
    return side


def oracle_side(orc, host):
    """The project's CPU path: the host shim flattens the context into a job, the oracle's flat form runs it."""
    host.vvc355_ctx_flatten_intra_pred.argtypes = [LC] + [ctypes.c_int] * 5 + [ctypes.POINTER(abi.IntraJob)]
    host.vvc355_ctx_flatten_cclm.argtypes = [LC] + [ctypes.c_int] * 4 + [ctypes.POINTER(abi.CclmJob)]
    host.vvc355_ctx_flatten_lmcs_scale.argtypes = [LC, ctypes.c_int, ctypes.c_int, ctypes.POINTER(abi.LmcsScaleJob)]
    for name in ("vvc355_ctx_flatten_intra_pred", "vvc355_ctx_flatten_cclm", "vvc355_ctx_flatten_lmcs_scale"):
        getattr(host, name).restype = None
    for name in ("vvc355_ctx_top_available", "vvc355_ctx_left_available"):
        getattr(host, name).argtypes = [LC] + [ctypes.c_int] * 4
    orc.orc_intra_pred_flat.argtypes = [ctypes.c_int, ctypes.c_void_p]
    orc.orc_intra_cclm_pred_flat.argtypes = [ctypes.c_int, ctypes.c_void_p]
    orc.orc_lmcs_scale_chroma_flat.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    orc.orc_lmcs_chroma_scale_flat.argtypes = [ctypes.c_int, ctypes.c_void_p]

    def side(case, lc):
        bd = case.pic.bd
        if case.slot == "intra_pred":
            j = abi.IntraJob()
            host.vvc355_ctx_flatten_intra_pred(lc, *case.args, ctypes.byref(j))
            return orc.orc_intra_pred_flat(bd, ctypes.addressof(j))
        if case.slot == "intra_cclm_pred":
            j = abi.CclmJob()
            host.vvc355_ctx_flatten_cclm(lc, *case.args, ctypes.byref(j))
            return orc.orc_intra_cclm_pred_flat(bd, ctypes.addressof(j))
        if case.slot == "lmcs_scale_chroma":
            j = abi.LmcsScaleJob()
            host.vvc355_ctx_flatten_lmcs_scale(lc, case.args[2], case.args[3], ctypes.byref(j))
            dst = np.full_like(case.coeff, 0x5A5A5A)
            orc.orc_lmcs_scale_chroma_flat(bd, ctypes.addressof(j), dst.ctypes.data, case.coeff.ctypes.data, case.args[0], case.args[1])
            side.scale = orc.orc_lmcs_chroma_scale_flat(bd, ctypes.addressof(j))
            return dst
        return getattr(host, "vvc355_ctx_" + case.slot)(lc, *case.args)
    return side


def table_side(host):
    """The project's device path: the slots of the installed table, called with the mirror context."""
    host.ff_vvc_dsp_init_mi355.argtypes = [ctypes.c_void_p, ctypes.c_int]
    host.ff_vvc_dsp_init_mi355_ctx.argtypes = [ctypes.c_void_p, ctypes.c_int]
    tables = {}

    def slots(bd):
        if bd not in tables:
            tab = (ctypes.c_void_p * cm.TABLE_POINTERS)()
            host.ff_vvc_dsp_init_mi355(tab, bd)
            host.ff_vvc_dsp_init_mi355_ctx(tab, bd)
            tables[bd] = (tab,) + cm.context_slots(tab)
        return tables[bd]

    def side(case, lc):
        _, cclm_fn, lmcs_fn, pred_fn = slots(case.pic.bd)
        if case.slot == "intra_pred":
            return pred_fn(lc, *case.args)
        if case.slot == "intra_cclm_pred":
            return cclm_fn(lc, *case.args)
        dst = np.full_like(case.coeff, 0x5A5A5A)
        lmcs_fn(lc, dst.ctypes.data, case.coeff.ctypes.data, *case.args)
        return dst
    return side
