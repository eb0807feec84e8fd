"""Cases for vvc355_pic_output_pass: what the output planes of a picture must be, as a vectorised numpy function that shares nothing with the
kernel, the scalar restatement it is checked against on the CPU (the three formulas of the header, and the byte positions of
libavutil/pixdesc.c's NV12 / NV21 / P010 / P012 descriptors), the directed shapes, the legal (layout, out_bits, SWAP_UV) combinations, and the
device plumbing of a run.  Used by tests/test_pic_output_cpu.py, tests/test_pic_output_gpu.py and tools/pic_output_time.py."""
import ctypes

import numpy as np

import pic_digest_cases as dc
from ffvvc_amd import abi, batch

SEED = 0x0D7B07
SENTINEL = 0x5A                  # the byte of the destination before the pass: pitch padding and the slack around a plane keep it
SLACK = 64                       # bytes in front of a destination plane's first row and behind its last
SEG_BYTES = 4096                 # pic_output.hip: kOutSeg, the bytes of destination address one wave takes per step


# ---------------------------------------------------------------------------------------------------------------- expected values

def convert(plane, bd, out_bits):
    """The destination samples of a plane of stored samples (uint8 at bd 8, uint16 above): as stored, in the high bits of 16, or rounded to 8."""
    s = np.asarray(plane)
    assert s.dtype == (np.uint8 if bd == 8 else np.uint16)
    if out_bits == bd:
        return s.copy()
    if out_bits == 16:
        return ((s.astype(np.uint32) << (16 - bd)) & 0xFFFF).astype(np.uint16)
    assert out_bits == 8 and bd in (10, 12)
    return np.minimum((s.astype(np.uint32) + (1 << (bd - 9))) >> (bd - 8), 255).astype(np.uint8)


def out_planes(planes, bd, layout, out_bits, swap=False):
    """The output planes (contiguous sample arrays, rows without pitch) of `planes`: one per component, or luma and the interleaved pair."""
    conv = [convert(p, bd, out_bits) for p in planes]
    if layout == abi.OUT_PLANAR:
        assert not swap
        return conv
    assert len(conv) == 3 and conv[1].shape == conv[2].shape
    first, second = (conv[2], conv[1]) if swap else (conv[1], conv[2])
    h, w = first.shape
    pair = np.empty((h, 2 * w), first.dtype)
    pair[:, 0::2], pair[:, 1::2] = first, second
    return [conv[0], pair]


def sample_bytes(a):
    """The bytes of output samples: one per sample at 8 bit, two, low byte first, above."""
    a = np.ascontiguousarray(a)
    return a.astype(np.uint8 if a.dtype == np.uint8 else "<u2").view(np.uint8).reshape(a.shape[0], -1)


# ---------------------------------------------------------------------------------------------------------------- plain restatements

def convert_scalar(s, bd, out_bits):
    """One sample, as include/vvc_mi355.h states it."""
    s = int(s)
    if out_bits == bd:
        return s
    if out_bits == 16:
        return (s << (16 - bd)) & 0xFFFF
    return min((s + (1 << (bd - 9))) >> (bd - 8), 255)


# libavutil/pixdesc.c, AVComponentDescriptor { plane, step, offset, shift, depth } of Y, U, V: where a component's sample lies (byte `offset`
# of every `step` bytes of a row of `plane`) and where its value lies in the little-endian word read there (value << shift)
PIXDESC = {
    "nv12": ((0, 1, 0, 0, 8), (1, 2, 0, 0, 8), (1, 2, 1, 0, 8)),
    "nv21": ((0, 1, 0, 0, 8), (1, 2, 1, 0, 8), (1, 2, 0, 0, 8)),
    "p010le": ((0, 2, 0, 6, 10), (1, 4, 0, 6, 10), (1, 4, 2, 6, 10)),
    "p012le": ((0, 2, 0, 4, 12), (1, 4, 0, 4, 12), (1, 4, 2, 4, 12)),
}


def pixdesc_scalar(planes, bd, name):
    """The bytes of the two planes of semi-planar format `name`, written sample by sample at the descriptor's positions; the value of a sample
    is the header's formula (convert_scalar), which for the P01x formats is value << shift."""
    desc = PIXDESC[name]
    word = 1 if desc[0][4] == 8 else 2
    out_bits = 8 if word == 1 else 16
    hy, wy = planes[0].shape
    hc, wc = planes[1].shape
    out = [np.zeros((hy, wy * word), np.uint8), np.zeros((hc, 2 * wc * word), np.uint8)]
    for c, (plane, step, offset, shift, depth) in enumerate(desc):
        for y in range(planes[c].shape[0]):
            for x in range(planes[c].shape[1]):
                d = convert_scalar(planes[c][y, x], bd, out_bits)
                if word == 2 and depth == bd:
                    assert d == (int(planes[c][y, x]) << shift) & 0xFFFF
                for k in range(word):
                    out[plane][y, x * step + offset + k] = (d >> (8 * k)) & 0xFF
    return out


def unpack(outs, bd, layout, out_bits, swap=False):
    """The source planes back from output planes that lose nothing (out_bits == bd or 16): the inverse of out_planes()."""
    assert out_bits in (bd, 16)
    if layout == abi.OUT_SEMI:
        a, b = outs[1][:, 0::2], outs[1][:, 1::2]
        outs = [outs[0]] + ([b, a] if swap else [a, b])
    if out_bits == bd:
        return [np.ascontiguousarray(o) for o in outs]
    return [(np.asarray(o) >> (16 - bd)).astype(np.uint8 if bd == 8 else np.uint16) for o in outs]


# ---------------------------------------------------------------------------------------------------------------- shapes and modes

def modes(bd, n_comp=3):
    """Every legal (layout, out_bits, swap) at this bit depth."""
    out = []
    for out_bits in sorted({bd, 16, 8} if bd > 8 else {8, 16}):
        out.append((abi.OUT_PLANAR, out_bits, False))
        if n_comp == 3:
            out += [(abi.OUT_SEMI, out_bits, False), (abi.OUT_SEMI, out_bits, True)]
    return out


def mode_name(bd, mode):
    layout, out_bits, swap = mode
    return f"bd {bd} {'semi' if layout else 'planar'} out {out_bits}{' swapped' if swap else ''}"


# name, (width, height, chroma format)
SHAPES = [("1x1 4:4:4", (1, 1, 444)), ("2x2 4:2:0", (2, 2, 420)), ("3x5 4:2:2", (3, 5, 422)), ("17x3 4:4:4", (17, 3, 444)),
          ("257x257 4:2:0", (257, 257, 420)), ("200x136 4:0:0", (200, 136, 400))]


def random_planes(seed, bd, dims):
    rng = np.random.default_rng([SEED, seed, bd])
    return [rng.integers(0, 1 << bd, size=(h, w), dtype=np.int64).astype(np.uint8 if bd == 8 else np.uint16) for (w, h) in dims]


def row_segs(rowbytes):
    return (rowbytes + 15 + SEG_BYTES - 1) // SEG_BYTES


def frame_of(bd, dims, src, src_stride, dst, dst_stride, layout, out_bits, swap=False):
    """abi.PicOutputFrame of device (or made-up) addresses; dst / dst_stride per OUTPUT plane."""
    f = abi.PicOutputFrame()
    for c, (w, h) in enumerate(dims):
        f.src[c], f.src_stride[c], f.width[c], f.height[c] = src[c], src_stride[c], w, h
    for p, (d, s) in enumerate(zip(dst, dst_stride)):
        f.dst[p], f.dst_stride[p] = d, s
    f.n_comp, f.layout, f.out_bits, f.flags = len(dims), layout, out_bits, abi.OUT_SWAP_UV if swap else 0
    return f


def valid_frame(bd=10, layout=abi.OUT_SEMI, out_bits=16):
    """A host frame with made-up addresses that the pass accepts, for the refusals (nothing may be launched)."""
    spx, dpx = (1 if bd == 8 else 2), (2 if out_bits > 8 else 1)
    dims = dc.chroma_dims(416, 240, 420)
    src = [0x100000, 0x200000, 0x300000]
    if layout == abi.OUT_SEMI:
        return frame_of(bd, dims, src, [512 * spx, 256 * spx, 256 * spx], [0x400000, 0x500000], [416 * dpx, 416 * dpx], layout, out_bits)
    return frame_of(bd, dims, src, [512 * spx, 256 * spx, 256 * spx], [0x400000, 0x500000, 0x600000], [416 * dpx, 208 * dpx, 208 * dpx], layout, out_bits)


# ---------------------------------------------------------------------------------------------------------------- device plumbing

class OutRun:
    """One frame on device source planes: a destination allocation per output plane, SENTINEL everywhere, the first row SLACK + start[p]
    bytes in (so start[p] is the row's offset in its 16-byte line), rows at pitch[p] (None: the row's bytes plus one sample; "compact": the
    row's bytes)."""

    def __init__(self, lib, bd, dims, src_ptrs, src_strides, mode, pitch=None, start=None):
        self.lib, self.bd, self.dims, self.mode = lib, bd, list(dims), mode
        layout, out_bits, swap = mode
        self.dpx = 2 if out_bits > 8 else 1
        self.out_dims = [dims[0], (2 * dims[1][0], dims[1][1])] if layout == abi.OUT_SEMI else list(dims)       # in output samples
        self.rowbytes = [w * self.dpx for (w, h) in self.out_dims]
        if pitch == "compact":
            pitch = self.rowbytes
        self.pitch = [(pitch[p] if pitch else None) or self.rowbytes[p] + self.dpx for p in range(len(self.out_dims))]
        self.start = list(start) if start else [0] * len(self.out_dims)
        assert all(s % self.dpx == 0 and 0 <= s < 16 for s in self.start) and all(p >= r and p % self.dpx == 0 for p, r in zip(self.pitch, self.rowbytes))
        self.images = [np.full(SLACK + st + (h - 1) * pt + rb + SLACK, SENTINEL, np.uint8)
                       for (w, h), pt, rb, st in zip(self.out_dims, self.pitch, self.rowbytes, self.start)]
        self.bufs = [batch.DeviceBuffer.from_host(img) for img in self.images]
        assert all(b.ptr % 16 == 0 for b in self.bufs)
        self.frame = frame_of(bd, dims, src_ptrs, src_strides, [b.ptr + SLACK + st for b, st in zip(self.bufs, self.start)], self.pitch, layout, out_bits, swap)
        self.d_frame = batch.DeviceBuffer.from_host(np.frombuffer(bytes(self.frame), np.uint8))

    @classmethod
    def on(cls, pic, mode, pitch=None, start=None):
        return cls(pic.lib, pic.bd, pic.dims, pic.ptrs(), pic.pitch, mode, pitch, start)

    def segments(self):
        """Segments as the kernel counts them (one wave's step each)."""
        return sum(h * row_segs(rb) for (w, h), rb in zip(self.out_dims, self.rowbytes))

    def issue(self, stream=None):
        return self.lib.vvc355_pic_output_pass(stream, self.bd, self.d_frame.ptr, ctypes.addressof(self.frame))

    def reset(self):
        for b, img in zip(self.bufs, self.images):
            self.lib.vvc355_upload(b.ptr, img.ctypes.data, img.nbytes)

    def download(self):
        return [b.to_host(np.uint8, img.shape) for b, img in zip(self.bufs, self.images)]

    def expected_images(self, planes):
        """Every byte of the destination allocations after the pass on source samples `planes`: the rows, and SENTINEL everywhere else."""
        out = []
        for p, o in enumerate(out_planes(planes, self.bd, *self.mode)):
            img = self.images[p].copy()
            (w, h), first = self.out_dims[p], SLACK + self.start[p]
            data = sample_bytes(o)
            assert data.shape == (h, self.rowbytes[p])
            for y in range(h):
                img[first + y * self.pitch[p]:first + y * self.pitch[p] + self.rowbytes[p]] = data[y]
            out.append(img)
        return out

    def mismatch(self, planes):
        """'' where the destination allocations hold exactly what they must, otherwise where the first difference lies."""
        for p, (got, want) in enumerate(zip(self.download(), self.expected_images(planes))):
            if not np.array_equal(got, want):
                at = int(np.flatnonzero(got != want)[0])
                rel = at - SLACK - self.start[p]
                return (f"{mode_name(self.bd, self.mode)}, output plane {p}: byte {at} of the allocation (row {rel // self.pitch[p]}, byte {rel % self.pitch[p]} "
                        f"of a row of {self.rowbytes[p]} at pitch {self.pitch[p]}) is {got[at]:#x}, expected {want[at]:#x}; {int((got != want).sum())} bytes differ")
        return ""

    def run(self, planes, stream=None):
        assert self.issue(stream) == 0
        self.lib.vvc355_stream_sync(stream)
        assert self.lib.vvc355_last_error() == 0
        return self.mismatch(planes)
