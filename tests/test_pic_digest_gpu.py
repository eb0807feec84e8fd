"""GPU: vvc355_pic_digest_pass against zlib's Adler-32 with start value 0, binascii.crc_hqx with initial value 0x1D0F and the numpy checksum
of pic_digest_cases (tests/test_pic_digest_cpu.py pins those three to their definitions).  Every comparison is exact.

1. the directed shapes at 8, 10 and 12 bit with every digest asked for; 2. saturated and all-zero pictures; 3. a 1920x1080 picture: the
pitch padding does not count, nothing but the result and the work buffer is written, the picture spans many waves' shares; 4. subsets of
`what`; 5. a crop by offset plane pointers; 6. stream order behind vvc355_lmcs_frame_pass; 7. graph capture; 8. a refused frame."""
import ctypes

import numpy as np
import pytest

import pic_digest_cases as dc
import picture_cases as pcs
from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu

SEG_BYTES = 4096                    # pic_digest.hip: kDigestSeg, the bytes of address one wave takes per step


def _check(got, want, what):
    assert got == want, f"{what}: {dc.describe(got, want)}"


def _segments(pic):
    """Segments of a picture as the partials kernel counts them: per row, the 4 KiB pieces of its bytes plus 15."""
    return sum(h * ((w * pic.px + 15 + SEG_BYTES - 1) // SEG_BYTES) for (w, h) in pic.dims)


# ---------------------------------------------------------------------------------------------------------------- 1. directed shapes

@pytest.mark.parametrize("case", dc.CASES, ids=[c["name"] for c in dc.CASES])
def test_directed_shapes(dev, case):
    for bd in case["bds"]:
        planes = dc.case_planes(case, bd)
        pic = dc.DevicePicture(bd, planes, case.get("pitch"), case.get("start"))
        if case.get("start"):
            assert all(p % 16 == s % 16 for p, s in zip(pic.ptrs(), pic.start))        # the planes start where the case says
        host = pic.host_planes()
        assert all(np.array_equal(a, b) for a, b in zip(host, planes))
        want = dc.expected(host, bd)
        assert want["crc"][0] != 0 or want["checksum"][0] != 0
        _check(dc.Run.on(pic).run(), want, f"{case['name']} at {bd} bit")


# ---------------------------------------------------------------------------------------------------------------- 2. saturation, length

@pytest.mark.parametrize("bd,w,h,fmt,value", [(8, 1024, 512, 420, 0xFF), (10, 600, 400, 444, 0xFFFF), (8, 200, 136, 420, 0), (10, 200, 136, 420, 0)],
                         ids=["1024x512 of 0xFF", "600x400 of 0xFFFF as stored", "zeros 8 bit", "zeros 10 bit"])
def test_saturated_and_zero_pictures(dev, bd, w, h, fmt, value):
    planes = [np.full((ph, pw), value, np.uint8 if bd == 8 else np.uint16) for (pw, ph) in dc.chroma_dims(w, h, fmt)]
    want = dc.expected(planes, bd)
    if value == 0:
        assert want["adler32"] == 0 and want["plane_adler32"] == [0, 0, 0] and all(want["crc"]) and all(want["checksum"])
    if value == 0xFFFF:
        assert planes[0].nbytes > 1 << 16                       # stored bytes, nothing masked: where an unreduced length product fails
    _check(dc.Run.on(dc.DevicePicture(bd, planes)).run(), want, f"{w}x{h} of {value:#x}")


# ---------------------------------------------------------------------------------------------------------------- 3. a 1080p picture

def test_1080p_padding_does_not_count_and_nothing_else_is_written(dev):
    bd = 10
    rng = np.random.default_rng(dc.SEED + 100)
    planes = [rng.integers(0, 1 << bd, size=(h, w), dtype=np.int64).astype(np.uint16) for (w, h) in dc.chroma_dims(1920, 1080, 420)]
    pic = dc.DevicePicture(bd, planes, fill=0x3C)
    assert pic.pitch == [batch.plane_pitch(w, 2) for (w, h) in pic.dims] and pic.pitch[1] > pic.dims[1][0] * 2         # there is padding
    run = dc.Run.on(pic)
    # many workgroups, and a wave's share is more than one segment: the running element is joined across segments and across waves
    assert run.groups >= 64 and _segments(pic) >= 2 * run.groups * dc.WAVES_PER_GROUP
    want = dc.expected(planes, bd)
    first = run.run()                                            # asserts the sentinels around the result and behind the work buffer
    _check(first, want, "1080p")
    before = [img.copy() for img in pic.images]
    assert all(np.array_equal(a, b) for a, b in zip(pic.download(), before)), "the pass wrote to a plane"
    pic.upload(planes, fill=0xE7)                                # other garbage in the padding and behind the planes
    assert any(not np.array_equal(a, b) for a, b in zip(pic.images, before))
    _check(run.run(), first, "1080p, other padding")


# ---------------------------------------------------------------------------------------------------------------- 4. subsets of `what`

def test_what_subsets(dev):
    case = next(c for c in dc.CASES if c["name"] == "200x136 4:2:0")
    for bd in (8, 10):
        planes = dc.case_planes(case, bd)
        pic = dc.DevicePicture(bd, planes)
        full = dc.Run.on(pic).run()
        _check(full, dc.expected(planes, bd), f"{bd} bit, everything")
        for what in (abi.DIGEST_ADLER32, abi.DIGEST_CHECKSUM, abi.DIGEST_CRC, abi.DIGEST_ADLER32 | abi.DIGEST_CRC):
            got = dc.Run.on(pic, what).run()
            want = dc.expected(planes, bd, what)
            _check(got, want, f"{bd} bit, what = {what}")
            # the fields asked for are those of the full run, the others 0
            assert got["adler32"] == (full["adler32"] if what & 1 else 0) and got["checksum"] == (full["checksum"] if what & 2 else [0, 0, 0])
            assert got["crc"] == (full["crc"] if what & 4 else [0, 0, 0]) and got["n_comp"] == 3


# ---------------------------------------------------------------------------------------------------------------- 5. a crop

def test_crop_by_offset_plane_pointers(dev):
    x0, y0, w, h = 3, 5, 333, 77
    for bd in (8, 10):
        rng = np.random.default_rng(dc.SEED + 200 + bd)
        planes = [rng.integers(0, 1 << bd, size=(240, 416), dtype=np.int64).astype(np.uint8 if bd == 8 else np.uint16) for _ in range(3)]
        pic = dc.DevicePicture(bd, planes)
        ptrs = [p + y0 * pitch + x0 * pic.px for p, pitch in zip(pic.ptrs(), pic.pitch)]
        crop = [dc.samples_of(dc.rect_bytes(pic.pitched(c), x0 * pic.px, y0, w * pic.px, h), bd, w, h) for c in range(3)]
        assert all(np.array_equal(a, p[y0:y0 + h, x0:x0 + w]) for a, p in zip(crop, planes))
        want = dc.expected([np.ascontiguousarray(c) for c in crop], bd)
        _check(dc.Run(dev, bd, [(w, h)] * 3, ptrs, pic.pitch).run(), want, f"crop at {bd} bit")
        assert want != dc.expected(planes, bd)


# ---------------------------------------------------------------------------------------------------------------- 6. stream order

def test_digest_follows_lmcs_frame_pass_on_its_stream(dev):
    c = pcs.lmcs_case(1)
    k = pcs.Keep()
    image = pcs.lmcs_bytes(c, c.plane)
    d_plane = k.up(image)
    lf_ptr, lf = k.frame(pcs.lmcs_frame(c, d_plane.ptr, k.up(c.lut).ptr, k.up(c.slice_idx).ptr, k.up(c.used).ptr))
    run = dc.Run(dev, c.bd, [(c.width, c.height)], [d_plane.ptr], [c.pitch])
    s = dev.vvc355_stream_create()
    try:
        assert dev.vvc355_lmcs_frame_pass(s, c.bd, lf_ptr, ctypes.addressof(lf)) == 0
        assert run.issue(s) == 0                                 # no synchronisation in between
        dev.vvc355_stream_sync(s)
        assert dev.vvc355_last_error() == 0
    finally:
        dev.vvc355_stream_destroy(s)
    mapped = d_plane.to_host(np.uint8, image.shape)
    assert not np.array_equal(mapped, image)
    got, intact = run.result()
    assert intact
    plane = dc.samples_of(dc.rect_bytes(mapped, 0, 0, c.width * c.isz, c.height), c.bd, c.width, c.height)
    assert np.array_equal(plane, pcs.lmcs_expected(c))
    _check(got, dc.expected([plane], c.bd), "the mapped plane")
    assert got != dc.expected([c.plane], c.bd)


# ---------------------------------------------------------------------------------------------------------------- 7. graph capture

def test_pass_captured_in_a_graph(dev):
    bd = 10
    case = next(c for c in dc.CASES if c["name"] == "257x257")
    planes = dc.case_planes(case, bd)
    others = [np.ascontiguousarray(p[::-1]) ^ 0x155 for p in planes]
    pic = dc.DevicePicture(bd, planes)
    run = dc.Run.on(pic)
    s = dev.vvc355_stream_create()
    try:
        dev.vvc355_graph_begin(s)
        ret = run.issue(s)
        g = dev.vvc355_graph_end(s)
        assert ret == 0 and g
        dev.vvc355_stream_sync(s)
        raw = run.d_result.to_host(np.uint8, run.result_image.shape)
        assert (raw == dc.SENTINEL).all(), "recorded, not run"
        for rep, src in enumerate((planes, others, planes)):
            pic.upload(src)
            dev.vvc355_graph_launch(g, s)
            dev.vvc355_stream_sync(s)
            assert dev.vvc355_last_error() == 0
            got, intact = run.result()
            assert intact
            _check(got, dc.expected(src, bd), f"replay {rep}")
        assert dc.expected(planes, bd) != dc.expected(others, bd)
        dev.vvc355_graph_destroy(g)
    finally:
        dev.vvc355_stream_destroy(s)


# ---------------------------------------------------------------------------------------------------------------- 8. a refused frame

def test_refused_frame_leaves_the_result_untouched(dev):
    case = next(c for c in dc.CASES if c["name"] == "4x4 with 2x2 chroma")
    pic = dc.DevicePicture(8, dc.case_planes(case, 8))
    run = dc.Run.on(pic)
    for field, value, code in (("what", 0, abi.PIC_DIGEST_E_WHAT), ("n_comp", 2, abi.PIC_DIGEST_E_FRAME), ("work", 0, abi.PIC_DIGEST_E_TABLES)):
        keep = getattr(run.frame, field)
        setattr(run.frame, field, value)
        assert run.issue() == code, field
        setattr(run.frame, field, keep)
    run.frame.stride[1] = 1
    assert run.issue() == abi.PIC_DIGEST_E_STRIDE
    run.frame.stride[1] = pic.pitch[1]
    assert run.lib.vvc355_pic_digest_pass(None, 9, run.d_frame.ptr, ctypes.addressof(run.frame)) == abi.PIC_DIGEST_E_BD
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    raw = run.d_result.to_host(np.uint8, run.result_image.shape)
    assert (raw == dc.SENTINEL).all(), "a refused frame wrote to the result"
    _check(run.run(), dc.expected(pic.host_planes(), 8), "the same frame once it is valid")
