"""Cases for vvc355_pic_digest_pass: what the digests of a picture must be, by code that shares nothing with the kernels (zlib's Adler-32
with start value 0, binascii.crc_hqx with initial value 0x1D0F, a numpy checksum), the plain restatements those three are checked against
on the CPU, the helper that turns a pitched plane into the bytes of a rectangle, the directed shapes, and the device plumbing of a run.
Used by tests/test_pic_digest_cpu.py, tests/test_pic_digest_gpu.py and tools/pic_digest_time.py."""
import binascii
import ctypes
import zlib

import numpy as np

from ffvvc_amd import abi, batch

SEED = 0x5EEDD16E
FILL = 0xC3                      # the byte of pitch padding and of the slack around a plane
SENTINEL = 0xA5                  # the byte around the result and behind the work buffer
SLACK = 64                       # bytes behind a plane's last row and around the result
CRC_INIT = 0x1D0F                # the SEI's register 0xFFFF with its 16 appended zero bits, as crc_hqx's initial value
PART_BYTES = 20                  # one element of the work buffer (pic_digest.hip: kDigestPartDwords), one per workgroup and component
WAVES_PER_GROUP = 4              # each with a share of its own


# ---------------------------------------------------------------------------------------------------------------- expected values

def rect_bytes(image, x_bytes, y, row_bytes, height):
    """The bytes of a rectangle of a pitched plane (`image`: uint8, rows x pitch): its rows one after the other, without the pitch."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 2
    assert 0 <= x_bytes and x_bytes + row_bytes <= image.shape[1] and 0 <= y and y + height <= image.shape[0]
    return np.ascontiguousarray(image[y:y + height, x_bytes:x_bytes + row_bytes]).tobytes()


def plane_bytes(plane, bd):
    """The bytes of a contiguous plane of samples: one per sample at 8 bit, two, low byte first, above."""
    return np.ascontiguousarray(plane).astype(np.uint8 if bd == 8 else "<u2").tobytes()


def samples_of(data, bd, width, height):
    return np.frombuffer(data, np.uint8 if bd == 8 else "<u2").reshape(height, width)


def checksum_numpy(plane, bd):
    """picture_checksum of the decoded picture hash SEI over a (height, width) plane of samples as stored."""
    s = np.asarray(plane).astype(np.uint32)
    h, w = s.shape
    x, y = np.arange(w, dtype=np.uint32)[None, :], np.arange(h, dtype=np.uint32)[:, None]
    mask = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8)
    total = int(((s & 0xFF) ^ mask).sum(dtype=np.uint64))
    if bd > 8:
        total += int(((s >> 8) ^ mask).sum(dtype=np.uint64))
    return total & 0xFFFFFFFF


def expected(planes, bd, what=7):
    """The vvc355_pic_digest_result of `planes` (contiguous (height, width) sample arrays) as a dict; fields `what` leaves out are 0."""
    data = [plane_bytes(p, bd) for p in planes]
    out = dict(adler32=0, plane_adler32=[0, 0, 0], checksum=[0, 0, 0], crc=[0, 0, 0], n_comp=len(planes))
    if what & abi.DIGEST_ADLER32:
        out["adler32"] = zlib.adler32(b"".join(data), 0)
        out["plane_adler32"][:len(data)] = [zlib.adler32(d, 0) for d in data]
    if what & abi.DIGEST_CHECKSUM:
        out["checksum"][:len(data)] = [checksum_numpy(p, bd) for p in planes]
    if what & abi.DIGEST_CRC:
        out["crc"][:len(data)] = [binascii.crc_hqx(d, CRC_INIT) for d in data]
    return out


# ---------------------------------------------------------------------------------------------------------------- plain restatements

def sei_crc_bit_serial(data):
    """The SEI's loop as the standard writes it: crc = 0xFFFF, two zero bytes appended, one bit at a time, most significant first."""
    crc = 0xFFFF
    padded = bytes(data) + b"\0\0"
    for bit_idx in range(len(padded) * 8):
        crc_msb = (crc >> 15) & 1
        bit_val = (padded[bit_idx >> 3] >> (7 - (bit_idx & 7))) & 1
        crc = (((crc << 1) + bit_val) & 0xFFFF) ^ (crc_msb * 0x1021)
    return crc


def adler_scalar(data, a=0, b=0):
    for v in data:
        a = (a + v) % 65521
        b = (b + a) % 65521
    return b << 16 | a


def checksum_scalar(plane, bd):
    total = 0
    for y in range(plane.shape[0]):
        for x in range(plane.shape[1]):
            mask = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8)
            s = int(plane[y, x])
            total += (s & 0xFF) ^ mask
            if bd > 8:
                total += (s >> 8) ^ mask
    return total & 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------- the directed shapes

def chroma_dims(w, h, fmt):
    """(width, height) per component of a w x h picture: 400 (luma only), 420, 422 or 444."""
    if fmt == 400:
        return [(w, h)]
    hs, vs = {420: (1, 1), 422: (1, 0), 444: (0, 0)}[fmt]
    return [(w, h)] + [((w + hs) >> hs, (h + vs) >> vs)] * 2


# name, bit depths, dims per component, pitch in BYTES per component (None: plane_pitch), byte offset of the plane in its allocation
CASES = [
    dict(name="1x1 luma only", bds=(8, 10, 12), dims=chroma_dims(1, 1, 400)),
    dict(name="4x4 with 2x2 chroma", bds=(8, 10, 12), dims=chroma_dims(4, 4, 420)),
    dict(name="13x7 pitch 101 at odd addresses", bds=(8,), dims=chroma_dims(13, 7, 444), pitch=[101] * 3, start=[1, 3, 15]),
    dict(name="257x257", bds=(8, 10, 12), dims=chroma_dims(257, 257, 420)),                # x >> 8 and y >> 8 not 0
    dict(name="200x136 4:2:0", bds=(8, 10, 12), dims=chroma_dims(200, 136, 420)),
    dict(name="200x136 4:2:2", bds=(8, 10, 12), dims=chroma_dims(200, 136, 422)),
    dict(name="200x136 4:4:4", bds=(8, 10, 12), dims=chroma_dims(200, 136, 444)),
    dict(name="4099x1", bds=(8, 10, 12), dims=chroma_dims(4099, 1, 420)),                  # one row, more than one 4 KiB segment
    # rows of exactly one segment that start at every offset of a 16-byte line in turn: the second segment of a row is empty, then one byte, ...
    dict(name="4096x19 pitch 4097", bds=(8,), dims=chroma_dims(4096, 19, 400), pitch=[4097]),
    # 16-bit rows of several segments with a head and a tail, the start moving by 10 bytes per row
    dict(name="4500x5 pitch 9002 from byte 6", bds=(10,), dims=chroma_dims(4500, 5, 400), pitch=[9002], start=[6]),
]


def case_planes(case, bd):
    rng = np.random.default_rng([SEED, CASES.index(case), bd])
    return [rng.integers(0, 1 << bd, size=(h, w), dtype=np.int64).astype(np.uint8 if bd == 8 else np.uint16) for (w, h) in case["dims"]]


def frame_of(bd, dims, planes, strides, result, work, what=7):
    """abi.PicDigestFrame of device (or made-up) addresses."""
    f = abi.PicDigestFrame()
    for c, (w, h) in enumerate(dims):
        f.plane[c], f.stride[c], f.width[c], f.height[c] = planes[c], strides[c], w, h
    f.result, f.work, f.n_comp, f.what = result, work, len(dims), what
    return f


def valid_frame(bd=10):
    """A host frame with made-up addresses that the pass accepts, for the refusals (nothing may be launched)."""
    px = 1 if bd == 8 else 2
    return frame_of(bd, chroma_dims(416, 240, 420), [0x10000, 0x90000, 0xD0000], [512 * px, 256 * px, 256 * px], 0xF0000, 0xF1000)


# ---------------------------------------------------------------------------------------------------------------- device plumbing

def result_dict(r):
    return dict(adler32=r.adler32, plane_adler32=list(r.plane_adler32), checksum=list(r.checksum), crc=list(r.crc), n_comp=r.n_comp)


class DevicePicture:
    """Planes of samples on the device as a decoder holds them: rows at a pitch, the padding and SLACK bytes behind the last row filled
    with `fill`, the first sample `start[c]` bytes into the allocation.  images[c] is the host copy of allocation c (uint8, flat)."""

    def __init__(self, bd, planes, pitch=None, start=None, fill=FILL):
        self.bd, self.px = bd, 1 if bd == 8 else 2
        self.dims = [(p.shape[1], p.shape[0]) for p in planes]
        self.pitch = [(pitch[c] if pitch else None) or batch.plane_pitch(w, self.px) for c, (w, h) in enumerate(self.dims)]
        self.start = list(start) if start else [0] * len(planes)
        self.images, self.bufs = [], []
        for c, p in enumerate(planes):
            self.images.append(self._image(c, p, fill))
            self.bufs.append(batch.DeviceBuffer.from_host(self.images[-1]))
        self.lib = self.bufs[0].lib

    def _image(self, c, plane, fill):
        (w, h), pitch = self.dims[c], self.pitch[c]
        assert pitch >= w * self.px
        img = np.full(self.start[c] + h * pitch + SLACK, fill, np.uint8)
        rows = img[self.start[c]:self.start[c] + h * pitch].reshape(h, pitch)
        rows[:, :w * self.px] = np.frombuffer(plane_bytes(plane, self.bd), np.uint8).reshape(h, w * self.px)
        return img

    def upload(self, planes, fill=FILL):
        """Other samples (same shapes), other padding."""
        for c, p in enumerate(planes):
            self.images[c] = self._image(c, p, fill)
            self.lib.vvc355_upload(self.bufs[c].ptr, self.images[c].ctypes.data, self.images[c].nbytes)

    def ptrs(self):
        return [b.ptr + s for b, s in zip(self.bufs, self.start)]

    def pitched(self, c):
        """Rows x pitch view of the host copy of plane c, for rect_bytes()."""
        (w, h) = self.dims[c]
        return self.images[c][self.start[c]:self.start[c] + h * self.pitch[c]].reshape(h, self.pitch[c])

    def host_planes(self):
        """The samples as the pitched host copies hold them, through rect_bytes()."""
        return [samples_of(rect_bytes(self.pitched(c), 0, 0, w * self.px, h), self.bd, w, h) for c, (w, h) in enumerate(self.dims)]

    def download(self):
        return [b.to_host(np.uint8, img.shape) for b, img in zip(self.bufs, self.images)]


class Run:
    """One frame on a DevicePicture (or on any device planes): result and work buffer with sentinel bytes around them."""

    def __init__(self, lib, bd, dims, ptrs, strides, what=7):
        self.lib, self.bd = lib, bd
        self.result_image = np.full(SLACK + ctypes.sizeof(abi.PicDigestResult) + SLACK, SENTINEL, np.uint8)
        self.d_result = batch.DeviceBuffer.from_host(self.result_image)
        self.frame = frame_of(bd, dims, ptrs, strides, self.d_result.ptr + SLACK, 0x1000, what)       # any `work` while sizing
        self.work_bytes = lib.vvc355_pic_digest_work_bytes(ctypes.addressof(self.frame), bd)
        assert self.work_bytes > 0 and self.work_bytes % (PART_BYTES * len(dims)) == 0
        self.groups = self.work_bytes // (PART_BYTES * len(dims))                                 # workgroups of the partials kernel
        self.work_image = np.full(self.work_bytes + SLACK, SENTINEL, np.uint8)
        self.d_work = batch.DeviceBuffer.from_host(self.work_image)
        self.frame.work = self.d_work.ptr
        self.d_frame = batch.DeviceBuffer.from_host(np.frombuffer(bytes(self.frame), np.uint8))

    @classmethod
    def on(cls, pic, what=7):
        return cls(pic.lib, pic.bd, pic.dims, pic.ptrs(), pic.pitch, what)

    def issue(self, stream=None):
        return self.lib.vvc355_pic_digest_pass(stream, self.bd, self.d_frame.ptr, ctypes.addressof(self.frame))

    def result(self):
        """(the result as a dict, the sentinels around it and behind the work buffer are intact) after the caller's synchronisation."""
        raw = self.d_result.to_host(np.uint8, self.result_image.shape)
        n = ctypes.sizeof(abi.PicDigestResult)
        r = abi.PicDigestResult.from_buffer_copy(raw[SLACK:SLACK + n].tobytes())
        work = self.d_work.to_host(np.uint8, self.work_image.shape)
        intact = bool((raw[:SLACK] == SENTINEL).all() and (raw[SLACK + n:] == SENTINEL).all() and (work[self.work_bytes:] == SENTINEL).all())
        return result_dict(r), intact

    def run(self, stream=None):
        assert self.issue(stream) == 0
        self.lib.vvc355_stream_sync(stream)
        assert self.lib.vvc355_last_error() == 0
        got, intact = self.result()
        assert intact, "bytes around the result or behind the work buffer were written"
        return got


def describe(got, want):
    """The fields that differ, in hex."""
    out = []
    for k in want:
        if got[k] != want[k]:
            fmt = (lambda v: [hex(i) for i in v]) if isinstance(want[k], list) else hex
            out.append(f"{k}: got {fmt(got[k])}, want {fmt(want[k])}")
    return "; ".join(out)
