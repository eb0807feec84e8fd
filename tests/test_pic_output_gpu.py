"""GPU: vvc355_pic_output_pass against the numpy expectation of pic_output_cases (tests/test_pic_output_cpu.py pins it to the header's formulas
and to libavutil/pixdesc.c's byte positions).  Every comparison is exact and covers every byte of the destination allocations: the rows, the
pitch padding and the slack in front of and behind every plane.

1. the directed shapes at 8, 10 and 12 bit with every legal (layout, out_bits, SWAP_UV); 2. an alignment sweep: source and destination
starts inside a 16-byte line, widths around the 16-byte slots; 3. special values; 4. a 1920x1080 picture to P010 and to 8-bit NV12; 5. a
crop by offset source pointers; 6. stream order behind vvc355_lmcs_frame_pass and in front of vvc355_pic_digest_pass; 7. graph capture; 8. a
refused frame; 9. vvc355_download_async into vvc355_host_alloc memory behind the pass."""
import ctypes

import numpy as np
import pytest

import pic_digest_cases as dc
import pic_output_cases as oc
import picture_cases as pcs
from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- 1. directed shapes

@pytest.mark.parametrize("shape", oc.SHAPES, ids=[s[0] for s in oc.SHAPES])
def test_directed_shapes(dev, shape):
    name, (w, h, fmt) = shape
    dims = dc.chroma_dims(w, h, fmt)
    runs = 0
    for bd in (8, 10, 12):
        px = 1 if bd == 8 else 2
        planes = oc.random_planes(oc.SHAPES.index(shape), bd, dims)
        pic = dc.DevicePicture(bd, planes, start=[px * s for s in (1, 3, 7)][:len(dims)])          # odd sample addresses
        assert all((p // px) % 2 == 1 for p in pic.ptrs())
        for mode in oc.modes(bd, len(dims)):
            dpx = 2 if mode[1] > 8 else 1
            n_out = 2 if mode[0] == abi.OUT_SEMI else len(dims)
            start = [dpx * s for s in (1, 5, 3)][:n_out]
            widest = max(dims[0][0], 2 * dims[-1][0] if mode[0] == abi.OUT_SEMI else 0) * dpx
            # destination pitches: one sample more than a row, and 101 bytes where the sample size and the rows allow
            for pitch in [None] + ([[101] * n_out] if dpx == 1 and widest <= 101 else []):
                run = oc.OutRun.on(pic, mode, pitch=pitch, start=start)
                assert max(run.rowbytes) == widest and (pitch or run.pitch == [r + dpx for r in run.rowbytes])
                bad = run.run(planes)
                assert not bad, f"{name}, pitch {run.pitch}: {bad}"
                runs += 1
    assert runs >= (2 + 3 + 3 if fmt == 400 else 6 + 9 + 9)


# ---------------------------------------------------------------------------------------------------------------- 2. alignment sweep

WIDTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
# byte offsets inside a 16-byte line, in SAMPLES of the plane's size (x1 at 8 bit, x2 at 16): Y, Cb, Cr each at another
SRC_OFFSETS = ((0, 0, 0), (1, 3, 6), (7, 2, 5), (4, 7, 1))
DST_OFFSETS = ((0, 0, 0), (1, 2, 5), (7, 4, 3), (6, 5, 1))
SWEEP_MODES = [(10, (abi.OUT_SEMI, 16, False)), (10, (abi.OUT_SEMI, 8, False)), (8, (abi.OUT_PLANAR, 8, False)), (8, (abi.OUT_SEMI, 16, False))]


@pytest.mark.parametrize("bd,mode", SWEEP_MODES, ids=[oc.mode_name(bd, m) for bd, m in SWEEP_MODES])
def test_alignment_sweep(dev, bd, mode):
    """Two-row 4:4:4 pictures in ONE source buffer uploaded once and ONE destination buffer downloaded once: every width x source offsets x
    destination offsets is a frame of its own with a destination region of its own; all are issued, then everything is compared."""
    layout, out_bits, swap = mode
    spx, dpx = (1 if bd == 8 else 2), (2 if out_bits > 8 else 1)
    n_out = 2 if layout == abi.OUT_SEMI else 3
    wmax = max(WIDTHS)
    src_pitch = 16 * ((wmax * spx + 15) // 16 + 2) + spx                     # rows of a picture at different offsets in their lines
    comp_bytes = 16 + 2 * src_pitch
    rng = np.random.default_rng([oc.SEED, 77, bd])
    src_image = rng.integers(0, 256, 3 * comp_bytes, dtype=np.int64).astype(np.uint8)
    if bd > 8:                                                                  # samples inside the bit depth, wherever a plane starts
        src_image[1::2] &= (1 << (bd - 8)) - 1
    d_src = batch.DeviceBuffer.from_host(src_image)
    region = 16 * ((16 + 2 * (2 * wmax * dpx + dpx) + 15) // 16 + 1)            # bytes of destination per output plane of a frame
    combos = [(w, so, do) for w in WIDTHS for so in SRC_OFFSETS for do in DST_OFFSETS]
    dst_image = np.full(len(combos) * n_out * region, oc.SENTINEL, np.uint8)
    want = dst_image.copy()
    d_dst = batch.DeviceBuffer.from_host(dst_image)
    assert d_src.ptr % 16 == 0 and d_dst.ptr % 16 == 0
    frames = (abi.PicOutputFrame * len(combos))()
    for i, (w, so, do) in enumerate(combos):
        src_at = [c * comp_bytes + so[c] * spx for c in range(3)]
        planes = []
        for c in range(3):
            rows = [src_image[src_at[c] + y * src_pitch:src_at[c] + y * src_pitch + w * spx] for y in range(2)]
            planes.append(np.stack(rows).view(np.uint8 if bd == 8 else "<u2").astype(np.uint8 if bd == 8 else np.uint16))
        outs = oc.out_planes(planes, bd, *mode)
        dst_at, dst_pitch = [], []
        for p, o in enumerate(outs):
            data = oc.sample_bytes(o)
            pitch = data.shape[1] + dpx                                           # the second row at another offset than the first
            at = (i * n_out + p) * region + do[p] * dpx
            assert at + pitch + data.shape[1] <= (i * n_out + p + 1) * region
            for y in range(2):
                want[at + y * pitch:at + y * pitch + data.shape[1]] = data[y]
            dst_at.append(at)
            dst_pitch.append(pitch)
        frames[i] = oc.frame_of(bd, [(w, 2)] * 3, [d_src.ptr + a for a in src_at], [src_pitch] * 3, [d_dst.ptr + a for a in dst_at], dst_pitch,
                                layout, out_bits, swap)
    d_frames = batch.DeviceBuffer.from_host(np.frombuffer(bytes(frames), np.uint8))
    size = ctypes.sizeof(abi.PicOutputFrame)
    for i in range(len(combos)):
        assert dev.vvc355_pic_output_pass(None, bd, d_frames.ptr + i * size, ctypes.addressof(frames[i])) == 0, combos[i]
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    got = d_dst.to_host(np.uint8, dst_image.shape)
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        i, p = divmod(at // region, n_out)
        pytest.fail(f"width {combos[i][0]}, source offsets {combos[i][1]}, destination offsets {combos[i][2]}, output plane {p}: byte {at % region} of its "
                    f"region is {got[at]:#x}, expected {want[at]:#x}; {int((got != want).sum())} bytes differ in all")
    assert np.array_equal(d_src.to_host(np.uint8, src_image.shape), src_image)


# ---------------------------------------------------------------------------------------------------------------- 3. special values

@pytest.mark.parametrize("bd,value", [(8, 0), (10, 0), (12, 0), (8, 0xFF), (10, 0x3FF), (12, 0xFFF), (10, 0xFFFF)],
                         ids=["zeros 8", "zeros 10", "zeros 12", "0xFF at 8", "0x3FF at 10", "0xFFF at 12", "0xFFFF as stored at 10"])
def test_special_values(dev, bd, value):
    dims = dc.chroma_dims(70, 6, 420)
    planes = [np.full((h, w), value, np.uint8 if bd == 8 else np.uint16) for (w, h) in dims]
    pic = dc.DevicePicture(bd, planes)
    for mode in oc.modes(bd):
        outs = oc.out_planes(planes, bd, *mode)
        if value and mode[1] == 8 and bd > 8:
            assert all((o == 255).all() for o in outs)                          # the clip: 255, not 0
        if value == 0xFFFF and mode[1] == 16:
            assert all((o == 0xFFC0).all() for o in outs)
        if value == 0:
            assert not any(o.any() for o in outs)
        bad = oc.OutRun.on(pic, mode).run(planes)
        assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- 4. a 1080p picture

def test_1080p_to_p010_and_to_8_bit_nv12(dev):
    bd = 10
    dims = dc.chroma_dims(1920, 1080, 420)
    planes = oc.random_planes(100, bd, dims)
    pic = dc.DevicePicture(bd, planes, fill=0x3C)
    before = [img.copy() for img in pic.images]
    for out_bits in (16, 8):
        mode = (abi.OUT_SEMI, out_bits, False)
        row = 1920 * (2 if out_bits == 16 else 1)
        run = oc.OutRun.on(pic, mode, pitch=[row + 256, row + 256])           # pitch padding to keep
        assert run.segments() >= 1080 + 540 and all(img.nbytes > h * row for img, (w, h) in zip(run.images, run.out_dims))
        bad = run.run(planes)
        assert not bad, bad
        assert all(np.array_equal(a, b) for a, b in zip(pic.download(), before)), "the pass wrote to a source plane"


# ---------------------------------------------------------------------------------------------------------------- 5. a crop

def test_crop_by_offset_source_pointers(dev):
    x0, y0, w, h = 6, 10, 100, 50
    for bd in (8, 10):
        dims = dc.chroma_dims(200, 136, 420)
        planes = oc.random_planes(200, bd, dims)
        pic = dc.DevicePicture(bd, planes)
        win = [(x0, y0, w, h), (x0 // 2, y0 // 2, w // 2, h // 2), (x0 // 2, y0 // 2, w // 2, h // 2)]
        ptrs = [p + y * pitch + x * pic.px for p, pitch, (x, y, _, _) in zip(pic.ptrs(), pic.pitch, win)]
        crop = [np.ascontiguousarray(pl[y:y + ch, x:x + cw]) for pl, (x, y, cw, ch) in zip(planes, win)]
        for mode in ((abi.OUT_PLANAR, bd, False), (abi.OUT_SEMI, 16, False)):
            run = oc.OutRun(dev, bd, [(cw, ch) for (_, _, cw, ch) in win], ptrs, pic.pitch, mode)
            bad = run.run(crop)
            assert not bad, bad
            assert run.mismatch([pl[:ch, :cw] for pl, (_, _, cw, ch) in zip(planes, win)]), "the window is not the picture's corner"


# ---------------------------------------------------------------------------------------------------------------- 6. stream order

def test_output_follows_lmcs_and_the_digest_follows_the_output(dev):
    """No numpy in the comparison: the digest of the packed plane is the digest of the source window, both taken on the stream."""
    c = pcs.lmcs_case(1)
    k = pcs.Keep()
    image = pcs.lmcs_bytes(c, c.plane)
    d_plane = k.up(image)
    lf_ptr, lf = k.frame(pcs.lmcs_frame(c, d_plane.ptr, k.up(c.lut).ptr, k.up(c.slice_idx).ptr, k.up(c.used).ptr))
    dims = [(c.width, c.height)]
    out = oc.OutRun(dev, c.bd, dims, [d_plane.ptr], [c.pitch], (abi.OUT_PLANAR, c.bd, False), pitch="compact")
    assert out.pitch == [c.width * c.isz] and out.pitch[0] < c.pitch
    of_source = dc.Run(dev, c.bd, dims, [d_plane.ptr], [c.pitch])
    of_output = dc.Run(dev, c.bd, dims, [out.frame.dst[0]], out.pitch)
    s = dev.vvc355_stream_create()
    try:
        assert dev.vvc355_lmcs_frame_pass(s, c.bd, lf_ptr, ctypes.addressof(lf)) == 0
        assert out.issue(s) == 0                                   # no synchronisation in between
        assert of_output.issue(s) == 0 and of_source.issue(s) == 0
        dev.vvc355_stream_sync(s)
        assert dev.vvc355_last_error() == 0
    finally:
        dev.vvc355_stream_destroy(s)
    got, intact = of_output.result()
    want, intact_too = of_source.result()
    assert intact and intact_too
    assert got == want, dc.describe(got, want)
    assert all(want["crc"][:1]) and want != dc.expected([c.plane], c.bd)          # the mapped plane, not the one uploaded


# ---------------------------------------------------------------------------------------------------------------- 7. graph capture

def test_pass_captured_in_a_graph(dev):
    bd = 10
    dims = dc.chroma_dims(257, 257, 420)
    planes = oc.random_planes(300, bd, dims)
    others = [np.ascontiguousarray(p[::-1]) ^ 0x155 for p in planes]
    pic = dc.DevicePicture(bd, planes)
    run = oc.OutRun.on(pic, (abi.OUT_SEMI, 16, False))
    s = dev.vvc355_stream_create()
    try:
        dev.vvc355_graph_begin(s)
        ret = run.issue(s)
        g = dev.vvc355_graph_end(s)
        assert ret == 0 and g
        dev.vvc355_stream_sync(s)
        assert all(np.array_equal(a, b) for a, b in zip(run.download(), run.images)), "recorded, not run"
        for rep, src in enumerate((planes, others, planes)):
            pic.upload(src)
            dev.vvc355_graph_launch(g, s)
            dev.vvc355_stream_sync(s)
            assert dev.vvc355_last_error() == 0
            bad = run.mismatch(src)
            assert not bad, f"replay {rep}: {bad}"
        assert run.mismatch(others)
        dev.vvc355_graph_destroy(g)
    finally:
        dev.vvc355_stream_destroy(s)


# ---------------------------------------------------------------------------------------------------------------- 8. a refused frame

def test_refused_frame_leaves_the_destination_untouched(dev):
    bd = 8
    dims = dc.chroma_dims(4, 4, 420)
    planes = oc.random_planes(400, bd, dims)
    pic = dc.DevicePicture(bd, planes)
    run = oc.OutRun.on(pic, (abi.OUT_SEMI, 8, False))
    for field, value, code in (("layout", 2, abi.PIC_OUTPUT_E_FORMAT), ("n_comp", 2, abi.PIC_OUTPUT_E_FRAME), ("out_bits", 10, abi.PIC_OUTPUT_E_FORMAT),
                               ("flags", 2, abi.PIC_OUTPUT_E_FORMAT)):
        keep = getattr(run.frame, field)
        setattr(run.frame, field, value)
        assert run.issue() == code, field
        setattr(run.frame, field, keep)
    for field, c, value, code in (("dst_stride", 1, 3, abi.PIC_OUTPUT_E_STRIDE), ("dst", 2, run.frame.dst[1], abi.PIC_OUTPUT_E_FORMAT),
                                  ("src", 1, 0, abi.PIC_OUTPUT_E_PLANES), ("dst", 0, run.frame.src[2], abi.PIC_OUTPUT_E_OVERLAP),
                                  ("width", 0, 0, abi.PIC_OUTPUT_E_SIZE)):
        keep = getattr(run.frame, field)[c]
        getattr(run.frame, field)[c] = value
        assert run.issue() == code, field
        getattr(run.frame, field)[c] = keep
    assert run.lib.vvc355_pic_output_pass(None, 9, run.d_frame.ptr, ctypes.addressof(run.frame)) == abi.PIC_OUTPUT_E_BD
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    assert all(np.array_equal(a, b) for a, b in zip(run.download(), run.images)), "a refused frame wrote to the destination"
    bad = run.run(planes)
    assert not bad, f"the same frame once it is valid: {bad}"


# ---------------------------------------------------------------------------------------------------------------- 9. stream-ordered download

def test_download_async_into_pinned_memory_behind_the_pass(dev):
    bd = 10
    dims = dc.chroma_dims(200, 136, 420)
    planes = oc.random_planes(500, bd, dims)
    pic = dc.DevicePicture(bd, planes)
    run = oc.OutRun.on(pic, (abi.OUT_SEMI, 16, False))
    sizes = [img.nbytes for img in run.images]
    host = dev.vvc355_host_alloc(sum(sizes))
    assert host
    try:
        ctypes.memset(host, 0xEE, sum(sizes))
        s = dev.vvc355_stream_create()
        try:
            assert run.issue(s) == 0
            at = 0
            for b, n in zip(run.bufs, sizes):                      # behind the pass, no synchronisation in between
                dev.vvc355_download_async(s, host + at, b.ptr, n)
                at += n
            dev.vvc355_stream_sync(s)
            assert dev.vvc355_last_error() == 0
        finally:
            dev.vvc355_stream_destroy(s)
        got = np.frombuffer(ctypes.string_at(host, sum(sizes)), np.uint8)
        want = np.concatenate(run.expected_images(planes))
        assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
    finally:
        dev.vvc355_host_free(host)
    assert dev.vvc355_last_error() == 0
