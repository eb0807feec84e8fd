"""CPU: what vvc355_pic_output_pass is before any HIP call — the layout and the codes as the header states them, the numpy expectation of
pic_output_cases pinned against the definitions (a scalar loop restates the three formulas and writes every sample at the byte position
libavutil/pixdesc.c's NV12 / NV21 / P010 / P012 descriptors give it; unpacking gives the planes back; the premises are counted), and the
refusal of every kind of malformed frame with its own code, in the stated order, in a child process with a stream pointer no runtime could
use, so that a launch that should not have happened cannot hide."""
import ctypes
import subprocess
import sys

import numpy as np

import pic_digest_cases as dc
import pic_output_cases as oc
from conftest import ROOT
from ffvvc_amd import abi
from test_pic_digest_cpu import SIZES, _header, _members
from test_picture_cpu import _enum


def test_layout_matches_the_header():
    text = _header()
    assert ctypes.sizeof(abi.PicOutputFrame) == 104 and "vvc355_pic_output_frame {    /* 104 bytes, no implicit padding */" in text
    members = _members(text, "vvc355_pic_output_frame")
    assert [m[1] for m in members] == [n for n, _ in abi.PicOutputFrame._fields_]
    off = 0
    for ctype, ident, n in members:                 # no implicit padding: every member starts where the one before ends
        field = getattr(abi.PicOutputFrame, ident)
        assert field.offset == off and off % SIZES[ctype] == 0, ident
        assert field.size == SIZES[ctype] * max(n, 1), ident
        off += field.size
    assert off == 104
    offs = {n: getattr(abi.PicOutputFrame, n).offset for n, _ in abi.PicOutputFrame._fields_}
    assert offs == dict(src=0, dst=24, src_stride=48, dst_stride=60, width=72, height=84, n_comp=96, layout=97, out_bits=98, flags=99, pad_=100)
    assert abi.BATCH_SIGNATURES["pic_output_pass"] == ("i", "pipp")
    for name, sig in dict(host_alloc=("p", "z"), host_free=("v", "p"), download_async=("v", "pppz")).items():
        assert abi.RUNTIME_SIGNATURES[name] == sig, name
    # declared next to the digest, and the stream-ordered download next to vvc355_download
    assert text.index("int vvc355_pic_digest_pass(") < text.index("vvc355_pic_output_frame") < text.index("vvc355_lmcs_filter(")
    assert text.index("vvc355_download(") < text.index("vvc355_download_async(") < text.index("vvc355_stream_create(")


def test_codes_are_the_headers():
    text = _header()
    codes = _enum(text, "VVC355_PIC_OUTPUT_E_")
    names = ("FRAME", "BD", "FORMAT", "SIZE", "STRIDE", "PLANES", "OVERLAP")
    assert len(codes) == len(names)
    for i, n in enumerate(names):
        assert codes["VVC355_PIC_OUTPUT_E_" + n] == getattr(abi, "PIC_OUTPUT_E_" + n) == -(i + 1), n
    assert _enum(text, "VVC355_OUT_") == dict(VVC355_OUT_PLANAR=abi.OUT_PLANAR, VVC355_OUT_SEMI=abi.OUT_SEMI, VVC355_OUT_SWAP_UV=abi.OUT_SWAP_UV)
    assert (abi.OUT_PLANAR, abi.OUT_SEMI, abi.OUT_SWAP_UV) == (0, 1, 1)
    # the definitions are cited where they are stated
    assert "libavutil/pixdesc.c" in text and "swscale_unscaled.c:237-264" in text


# ---------------------------------------------------------------------------------------------------------------- the expectation, pinned

def test_convert_is_the_scalar_formula_and_meets_its_premises():
    rng = np.random.default_rng(oc.SEED)
    # 16 -> 8: every stored value, those above the bit depth included (nothing is masked)
    every = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16).reshape(256, 256)
    for bd in (10, 12):
        got = oc.convert(every, bd, 8)
        want = np.array([oc.convert_scalar(s, bd, 8) for s in range(1 << 16)]).reshape(256, 256)
        assert got.dtype == np.uint8 and np.array_equal(got, want), bd
        top = (1 << bd) - 1
        in_range = np.arange(1 << bd)
        unclipped = (in_range + (1 << (bd - 9))) >> (bd - 8)
        # premises: inputs INSIDE the bit depth round to 256 and are clipped; a carry crosses a byte boundary of the sum
        assert int((unclipped == 256).sum()) == 1 << (bd - 9) and unclipped[top] == 256 and oc.convert_scalar(top, bd, 8) == 255 == got.flat[top]
        carries = int((((in_range & 0xFF) + (1 << (bd - 9))) > 0xFF).sum())         # the rounding constant carries out of the low byte
        assert carries == (1 << (bd - 8)) * (1 << (bd - 9)) and oc.convert_scalar(0xFF, bd, 8) == (0x100 >> (bd - 8)) == got.flat[0xFF]
        assert got.flat[0xFFFF] == 255 and got.flat[0] == 0 and got.flat[(1 << (bd - 9)) - 1] == 0 and got.flat[1 << (bd - 9)] == 1
        # 16 -> 16
        got = oc.convert(every, bd, 16)
        want = np.array([oc.convert_scalar(s, bd, 16) for s in range(1 << 16)]).reshape(256, 256)
        assert got.dtype == np.uint16 and np.array_equal(got, want) and got.flat[0xFFFF] == (0xFFC0 if bd == 10 else 0xFFF0) and got.flat[top] == got.flat[0xFFFF]
        assert np.array_equal(oc.convert(every, bd, bd), every)
    b = np.arange(256, dtype=np.uint32).astype(np.uint8).reshape(16, 16)
    assert np.array_equal(oc.convert(b, 8, 16), b.astype(np.uint16) * 256) and np.array_equal(oc.convert(b, 8, 8), b)
    assert [oc.convert_scalar(s, 8, 16) for s in (0, 1, 255)] == [0, 0x100, 0xFF00]
    assert oc.convert(rng.integers(0, 1024, (3, 5)).astype(np.uint16), 10, 8).dtype == np.uint8


def test_semi_planar_bytes_are_pixdescs():
    """NV12 / NV21 from 8 bit, P010 from 10 bit, P012 from 12 bit: every sample at (plane, x * step + offset), the value << shift, low byte first."""
    for name, bd, mode in (("nv12", 8, (abi.OUT_SEMI, 8, False)), ("nv21", 8, (abi.OUT_SEMI, 8, True)),
                           ("p010le", 10, (abi.OUT_SEMI, 16, False)), ("p012le", 12, (abi.OUT_SEMI, 16, False))):
        planes = oc.random_planes(1, bd, dc.chroma_dims(13, 7, 420))
        got = [oc.sample_bytes(o) for o in oc.out_planes(planes, bd, *mode)]
        want = oc.pixdesc_scalar(planes, bd, name)
        assert len(got) == 2 and all(np.array_equal(g, w) for g, w in zip(got, want)), name
    # an 8-bit NV12 proxy of a 10-bit picture: the same positions, the rounded value
    planes = oc.random_planes(2, 10, dc.chroma_dims(13, 7, 420))
    planes[1][0, :3] = (1023, 1022, 1021)
    got = [oc.sample_bytes(o) for o in oc.out_planes(planes, 10, abi.OUT_SEMI, 8)]
    want = oc.pixdesc_scalar(planes, 10, "nv12")
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and list(got[1][0, 0:6:2]) == [255, 255, 255]
    # and NV24: chroma as wide as luma
    planes = oc.random_planes(3, 8, dc.chroma_dims(5, 3, 444))
    pair = oc.out_planes(planes, 8, abi.OUT_SEMI, 8)[1]
    assert pair.shape == (3, 10) and np.array_equal(pair[:, 0::2], planes[1]) and np.array_equal(pair[:, 1::2], planes[2])


def test_unpacking_gives_the_planes_back():
    for bd in (8, 10, 12):
        for fmt in (420, 422, 444, 400):
            dims = dc.chroma_dims(19, 6, fmt)
            planes = oc.random_planes(4, bd, dims)
            for mode in oc.modes(bd, len(dims)):
                outs = oc.out_planes(planes, bd, *mode)
                assert [o.dtype.itemsize for o in outs] == [2 if mode[1] > 8 else 1] * len(outs)
                if mode[1] in (bd, 16):
                    back = oc.unpack(outs, bd, *mode)
                    assert len(back) == len(planes) and all(np.array_equal(a, b) for a, b in zip(back, planes)), (bd, fmt, mode)
    assert len(oc.modes(8)) == 6 and len(oc.modes(10)) == len(oc.modes(12)) == 9 and len(oc.modes(10, 1)) == 3
    planes = oc.random_planes(5, 10, dc.chroma_dims(4, 2, 444))
    a, b = oc.out_planes(planes, 10, abi.OUT_SEMI, 16)[1], oc.out_planes(planes, 10, abi.OUT_SEMI, 16, True)[1]
    assert np.array_equal(a[:, 0::2], b[:, 1::2]) and np.array_equal(a[:, 1::2], b[:, 0::2]) and not np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- refusals, in a child

CHILD = f"""
import ctypes, sys
sys.path[:0] = [{ROOT!r}, {ROOT + "/tests"!r}]
import pic_output_cases as oc
from ffvvc_amd import abi
lib = abi.load()
STREAM = 0x5EED0001          # no stream of any runtime: a launch on it would not return
"""


def test_pic_output_pass_refuses_malformed_frames_before_any_hip_call():
    body = """
P, S = abi.OUT_PLANAR, abi.OUT_SEMI

def frame(bd=10, layout=S, out_bits=16, **kw):
    f = oc.valid_frame(bd, layout, out_bits)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(f, k)[v[0]] = v[1]
        else:
            setattr(f, k, v)
    return f

def run(f, bd=10, dev_ptr=0xf000):
    return lib.vvc355_pic_output_pass(STREAM, bd, dev_ptr, ctypes.addressof(f) if f is not None else None)

E = lambda n: getattr(abi, "PIC_OUTPUT_E_" + n)
# 1. no frame, n_comp
assert run(None) == E("FRAME") and run(frame(), dev_ptr=None) == E("FRAME")
for n in (0, 2, 4, 255):
    assert run(frame(n_comp=n)) == E("FRAME"), n
# 2. bd
for bd in (0, 9, 11, 16):
    assert run(frame(), bd) == E("BD"), bd
# 3. layout, out_bits, flags, pad bytes, the conditions of SEMI
for kw in (dict(layout=2), dict(layout=255), dict(out_bits=0), dict(out_bits=12), dict(out_bits=9), dict(out_bits=32), dict(flags=2), dict(flags=3),
           dict(flags=0x80), dict(pad_=(0, 1)), dict(pad_=(3, 1)), dict(n_comp=1), dict(width=(2, 207)), dict(height=(1, 119)), dict(dst=(2, 0x600000))):
    assert run(frame(**kw)) == E("FORMAT"), kw
assert run(frame(12, out_bits=10), 12) == E("FORMAT") and run(frame(8, out_bits=10), 8) == E("FORMAT") and run(frame(8, out_bits=12), 8) == E("FORMAT")
assert run(frame(layout=P, flags=abi.OUT_SWAP_UV)) == E("FORMAT")         # exchange dst[1] and dst[2] instead
# 4. sizes
for layout in (P, S):
    for c in range(3):
        for kw in (dict(width=(c, 0)), dict(width=(c, -8)), dict(height=(c, 0)), dict(height=(c, -1)), dict(width=(c, 1 << 16)), dict(height=(c, 1 << 16))):
            f = frame(layout=layout, **kw)
            if layout == S and c:                   # keep the pair's sizes equal: the size is what is refused
                f.width[3 - c], f.height[3 - c] = f.width[c], f.height[c]
            assert run(f) == E("SIZE"), (layout, kw)
# 5. strides: smaller than a row, no multiple of the sample size, 8 MiB or more; a span of 2 GiB or more
for c in range(3):
    w = oc.valid_frame().width[c]
    for kw in (dict(src_stride=(c, 2 * w - 2)), dict(src_stride=(c, 0)), dict(src_stride=(c, -1024)), dict(src_stride=(c, 2 * w + 1)), dict(src_stride=(c, 1 << 23))):
        assert run(frame(**kw)) == E("STRIDE"), kw
        assert run(frame(layout=P, **kw)) == E("STRIDE"), kw
    f = frame(src_stride=(c, 1 << 22))
    f.height[c] = 512
    if c:
        f.height[3 - c] = 512
        f.src_stride[3 - c] = 1 << 20
    assert run(f) == E("STRIDE"), c
for p, row in ((0, 832), (1, 832)):              # SEMI at 16 bit: both rows are 416 samples of two bytes
    for kw in (dict(dst_stride=(p, row - 2)), dict(dst_stride=(p, 0)), dict(dst_stride=(p, -832)), dict(dst_stride=(p, row + 1)), dict(dst_stride=(p, 1 << 23))):
        assert run(frame(**kw)) == E("STRIDE"), kw
for p, row in ((0, 416), (1, 208), (2, 208)):    # PLANAR at 8 bit from 10: rows of one byte per sample, any stride from a row up
    for kw in (dict(dst_stride=(p, row - 1)), dict(dst_stride=(p, 0)), dict(dst_stride=(p, 1 << 23))):
        assert run(frame(layout=P, out_bits=8, **kw)) == E("STRIDE"), kw
assert run(frame(8, out_bits=8, src_stride=(0, 415)), 8) == E("STRIDE")
f = frame(dst_stride=(0, 1 << 22))
f.height[0] = 512
assert run(f) == E("STRIDE")
# 6. pointers: missing, or not aligned to the sample size
for c in range(3):
    assert run(frame(src=(c, 0))) == E("PLANES") and run(frame(src=(c, 0x100001 + (c << 20)))) == E("PLANES"), c
    assert run(frame(layout=P, dst=(c, 0))) == E("PLANES") and run(frame(layout=P, dst=(c, 0x400001 + (c << 20)))) == E("PLANES"), c
for p in range(2):
    assert run(frame(dst=(p, 0))) == E("PLANES") and run(frame(dst=(p, 0x400001 + (p << 20)))) == E("PLANES"), p
# 7. a destination span that overlaps a source span: in place, by one byte at either end, and across components
g = oc.valid_frame()
src_span = [g.src_stride[c] * (g.height[c] - 1) + 2 * g.width[c] for c in range(3)]
dst_span = [g.dst_stride[p] * (g.height[p] - 1) + 832 for p in range(2)]
for p in range(2):
    for c in range(3):
        assert run(frame(dst=(p, g.src[c]))) == E("OVERLAP"), (p, c)
        assert run(frame(dst=(p, g.src[c] + src_span[c] - 2))) == E("OVERLAP"), (p, c)
        assert run(frame(dst=(p, g.src[c] - dst_span[p] + 2))) == E("OVERLAP"), (p, c)
assert run(frame(layout=P, out_bits=10, dst=(2, g.src[0] + 64))) == E("OVERLAP")
# the order of the checks is the order of the codes
bad = dict(layout=7, width=(0, 0), src_stride=(0, 1), src=(0, 0))
assert run(frame(n_comp=2, **bad), 9) == E("FRAME") and run(frame(**bad), 9) == E("BD") and run(frame(**bad)) == E("FORMAT")
del bad["layout"]
assert run(frame(**bad)) == E("SIZE")
del bad["width"]
assert run(frame(**bad)) == E("STRIDE")
del bad["src_stride"]
assert run(frame(**bad)) == E("PLANES")
assert run(frame(src=(0, 0), dst=(0, g.src[1]))) == E("PLANES") and run(frame(dst=(0, g.src[1]))) == E("OVERLAP")
assert [E(n) for n in ("FRAME", "BD", "FORMAT", "SIZE", "STRIDE", "PLANES", "OVERLAP")] == [-1, -2, -3, -4, -5, -6, -7]
"""
    r = subprocess.run([sys.executable, "-c", CHILD + body + "\nprint('validated')\n"], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-1500:])
    assert b"validated" in r.stdout
