"""CPU: what vvc355_pic_digest_pass is before any HIP call — the layouts and codes as the header states them, the premises of the expected
values in pic_digest_cases (the stdlib CRC with initial value 0x1D0F is the SEI's bit-serial loop, Adler-32 with start value 0 is the
two-line loop, the numpy checksum is the double loop), and the refusal of every kind of malformed frame with its own code, in a child
process with a stream pointer no runtime could use, so that a launch that should not have happened cannot hide."""
import binascii
import ctypes
import re
import subprocess
import sys
import zlib

import numpy as np

import pic_digest_cases as dc
from conftest import ROOT
from ffvvc_amd import abi


def _header():
    return open(f"{ROOT}/include/vvc_mi355.h").read()


def _members(text, name):
    """[(type, member, array length or 0)] of `typedef struct name { ... } name;` in the header."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for ctype, decl in re.findall(r"(\w+)\s+([^;]+);", body):
        for m in decl.split(","):
            ident, _, n = m.strip().partition("[")
            out.append((ctype, ident, int(n.rstrip("]")) if n else 0))
    return out


SIZES = dict(uint64_t=8, uint32_t=4, int32_t=4, uint16_t=2, uint8_t=1)


def test_layouts_match_the_header():
    text = _header()
    for cls, name, size in ((abi.PicDigestResult, "vvc355_pic_digest_result", 36), (abi.PicDigestFrame, "vvc355_pic_digest_frame", 80)):
        assert ctypes.sizeof(cls) == size and f"{size} bytes, no implicit padding" in text
        members = _members(text, name)
        assert [m[1] for m in members] == [n for n, _ in cls._fields_], name
        off = 0
        for ctype, ident, n in members:                 # no implicit padding: every member starts where the one before ends
            field = getattr(cls, ident)
            assert field.offset == off and off % SIZES[ctype] == 0, (name, ident)
            assert field.size == SIZES[ctype] * max(n, 1), (name, ident)
            off += field.size
        assert off == size
    offs = {n: getattr(abi.PicDigestFrame, n).offset for n, _ in abi.PicDigestFrame._fields_}
    assert offs == dict(plane=0, result=24, work=32, stride=40, width=52, height=64, n_comp=76, what=77, pad_=78)
    offs = {n: getattr(abi.PicDigestResult, n).offset for n, _ in abi.PicDigestResult._fields_}
    assert offs == dict(adler32=0, plane_adler32=4, checksum=16, crc=28, n_comp=34)
    assert abi.BATCH_SIGNATURES["pic_digest_pass"] == ("i", "pipp") and abi.BATCH_SIGNATURES["pic_digest_work_bytes"] == ("z", "pi")
    # declared next to vvc355_lmcs_frame_pass
    assert text.index("int vvc355_lmcs_frame_pass(") < text.index("vvc355_pic_digest_result") < text.index("vvc355_lmcs_filter(")


def test_codes_are_the_headers():
    import test_picture_cpu
    text = _header()
    codes = test_picture_cpu._enum(text, "VVC355_PIC_DIGEST_E_")
    names = ("FRAME", "BD", "WHAT", "SIZE", "STRIDE", "TABLES")
    assert len(codes) == len(names)
    for i, n in enumerate(names):
        assert codes["VVC355_PIC_DIGEST_E_" + n] == getattr(abi, "PIC_DIGEST_E_" + n) == -(i + 1), n
    bits = test_picture_cpu._enum(text, "VVC355_DIGEST_")
    assert bits == dict(VVC355_DIGEST_ADLER32=abi.DIGEST_ADLER32, VVC355_DIGEST_CHECKSUM=abi.DIGEST_CHECKSUM, VVC355_DIGEST_CRC=abi.DIGEST_CRC)
    assert (abi.DIGEST_ADLER32, abi.DIGEST_CHECKSUM, abi.DIGEST_CRC) == (1, 2, 4)
    # the definitions are cited where they are stated
    assert "libavformat/framecrcenc.c:53" in text and "H.274" in text and "0x1D0F" in text


# ---------------------------------------------------------------------------------------------------------------- premises of the expected values

def test_crc_hqx_from_0x1d0f_is_the_seis_bit_serial_crc():
    data = np.random.default_rng(dc.SEED).integers(0, 256, 1000, dtype=np.uint8).tobytes()
    for n in range(1001):
        assert binascii.crc_hqx(data[:n], dc.CRC_INIT) == dc.sei_crc_bit_serial(data[:n]), n
    for d in (b"\0" * 300, b"\xff" * 300):
        assert binascii.crc_hqx(d, dc.CRC_INIT) == dc.sei_crc_bit_serial(d)
    assert binascii.crc_hqx(b"", dc.CRC_INIT) == dc.CRC_INIT == dc.sei_crc_bit_serial(b"")


def test_adler_with_start_value_0_is_the_scalar_loop_and_joins_by_length():
    rng = np.random.default_rng(dc.SEED + 1)
    for n in (0, 1, 2, 15, 16, 17, 5552, 5553, 70000):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert zlib.adler32(d, 0) == dc.adler_scalar(d), n
    assert zlib.adler32(b"\0" * 1000, 0) == 0 and zlib.adler32(b"\0" * 1000) != 0
    # the rule the kernels join pieces by, on pieces longer than 65 550 bytes of 0xFF (where an unreduced length product leaves 32 bits)
    left, right = b"\xff" * 70001, rng.integers(200, 256, 131077, dtype=np.uint8).tobytes()
    l, r = zlib.adler32(left, 0), zlib.adler32(right, 0)
    a = ((l & 0xFFFF) + (r & 0xFFFF)) % 65521
    b = ((l >> 16) + (r >> 16) + (len(right) % 65521) * (l & 0xFFFF)) % 65521
    assert zlib.adler32(left + right, 0) == b << 16 | a


def test_numpy_checksum_is_the_double_loop():
    rng = np.random.default_rng(dc.SEED + 2)
    for bd in (8, 10):
        plane = rng.integers(0, 1 << bd, size=(260, 300), dtype=np.int64).astype(np.uint8 if bd == 8 else np.uint16)      # both >> 8 terms not 0
        assert dc.checksum_numpy(plane, bd) == dc.checksum_scalar(plane, bd), bd
    stored = np.full((3, 5), 0xFFFF, np.uint16)            # as stored: nothing is masked to the bit depth
    assert dc.checksum_numpy(stored, 10) == dc.checksum_scalar(stored, 10) != dc.checksum_numpy(stored & 0x3FF, 10)


def test_rect_bytes_and_expected():
    rng = np.random.default_rng(dc.SEED + 3)
    plane = rng.integers(0, 1 << 10, size=(6, 9), dtype=np.int64).astype(np.uint16)
    image = np.full((8, 40), dc.FILL, np.uint8)
    image[1:7, 4:22] = plane.view(np.uint8).reshape(6, 18)
    data = dc.rect_bytes(image, 4, 1, 18, 6)
    assert data == dc.plane_bytes(plane, 10) and np.array_equal(dc.samples_of(data, 10, 9, 6), plane)
    want = dc.expected([plane], 10)
    assert want["adler32"] == want["plane_adler32"][0] == zlib.adler32(data, 0) and want["crc"][0] == dc.sei_crc_bit_serial(data)
    assert want["n_comp"] == 1 and want["plane_adler32"][1:] == [0, 0] and want["crc"][1:] == [0, 0]
    only = dc.expected([plane], 10, abi.DIGEST_CHECKSUM)
    assert only["checksum"][0] == want["checksum"][0] and only["adler32"] == 0 and only["crc"] == [0, 0, 0]
    three = dc.expected([plane, plane[:3], plane[:2]], 10)
    assert three["adler32"] == zlib.adler32(dc.plane_bytes(plane, 10) + dc.plane_bytes(plane[:3], 10) + dc.plane_bytes(plane[:2], 10), 0)
    assert dc.chroma_dims(7, 5, 420) == [(7, 5), (4, 3), (4, 3)] and dc.chroma_dims(7, 5, 422) == [(7, 5), (4, 5), (4, 5)]


# ---------------------------------------------------------------------------------------------------------------- refusals, in a child

CHILD = f"""
import ctypes, sys
sys.path[:0] = [{ROOT!r}, {ROOT + "/tests"!r}]
import pic_digest_cases as dc
from ffvvc_amd import abi
lib = abi.load()
STREAM = 0x5EED0001          # no stream of any runtime: a launch on it would not return
"""


def test_pic_digest_pass_refuses_malformed_frames_before_any_hip_call():
    body = """
def frame(bd=10, **kw):
    f = dc.valid_frame(bd)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(f, k)[v[0]] = v[1]
        else:
            setattr(f, k, v)
    return f

def run(f, bd=10, dev_ptr=0xf000):
    host = ctypes.addressof(f) if f is not None else None
    ret = lib.vvc355_pic_digest_pass(STREAM, bd, dev_ptr, host)
    if dev_ptr:                                     # the size of the work buffer says the same: 0 for a frame the pass refuses
        assert (lib.vvc355_pic_digest_work_bytes(host, bd) == 0) == (ret != 0), ret
    return ret

E = lambda n: getattr(abi, "PIC_DIGEST_E_" + n)
assert run(None) == E("FRAME") and run(frame(), dev_ptr=None) == E("FRAME")
for n in (0, 2, 4, 255):
    assert run(frame(n_comp=n)) == E("FRAME"), n
for bd in (0, 9, 11, 16):
    assert run(frame(), bd) == E("BD"), bd
for kw in (dict(what=0), dict(what=8), dict(what=15), dict(what=0x80), dict(pad_=(0, 1)), dict(pad_=(1, 1))):
    assert run(frame(**kw)) == E("WHAT"), kw
for c in range(3):
    for kw in (dict(width=(c, 0)), dict(width=(c, -8)), dict(height=(c, 0)), dict(height=(c, -1)), dict(width=(c, 1 << 16)), dict(height=(c, 1 << 16))):
        assert run(frame(**kw)) == E("SIZE"), kw
    # a stride smaller than a row, no multiple of the pixel size, 8 MiB or more; a plane span of 2 GiB or more
    w = dc.valid_frame().width[c]
    for kw in (dict(stride=(c, 2 * w - 2)), dict(stride=(c, 0)), dict(stride=(c, -1024)), dict(stride=(c, 2 * w + 1)), dict(stride=(c, 1 << 23))):
        assert run(frame(**kw)) == E("STRIDE"), kw
    f = frame(stride=(c, 1 << 22))
    f.height[c] = 512
    assert run(f) == E("STRIDE"), c
    assert run(frame(plane=(c, 0))) == E("TABLES"), c
    assert run(frame(plane=(c, 0x10001))) == E("TABLES"), c         # a 16-bit plane at an odd address
assert run(frame(bd=8, stride=(0, 415)), 8) == E("STRIDE")
for name in ("result", "work"):
    assert run(frame(**{name: 0})) == E("TABLES"), name
    assert run(frame(**{name: 0xF0002})) == E("TABLES"), name
# a luma-only frame does not look at the chroma members
f = frame(n_comp=1, width=(1, 0), stride=(2, -1), plane=(1, 0))
assert f.n_comp == 1 and lib.vvc355_pic_digest_work_bytes(ctypes.addressof(f), 10) > 0
# the order of the checks is the order of the codes
assert run(frame(n_comp=2, what=0, width=(0, 0)), 9) == E("FRAME") and run(frame(what=0, width=(0, 0)), 9) == E("BD")
assert run(frame(what=0, width=(0, 0), stride=(0, 1))) == E("WHAT") and run(frame(width=(0, 0), stride=(0, 1), result=0)) == E("SIZE")
assert run(frame(stride=(0, 1), result=0)) == E("STRIDE")
codes = [E(n) for n in ("FRAME", "BD", "WHAT", "SIZE", "STRIDE", "TABLES")]
assert codes == [-1, -2, -3, -4, -5, -6]
# valid frames: the work buffer has a size, bounded whatever the picture
for bd in (8, 10, 12):
    f = dc.valid_frame(bd)
    n = lib.vvc355_pic_digest_work_bytes(ctypes.addressof(f), bd)
    assert 0 < n < 128 << 10 and n % (3 * dc.PART_BYTES) == 0, (bd, n)
big = dc.frame_of(10, dc.chroma_dims(65535, 16000, 444), [0x10000] * 3, [131072] * 3, 0xF0000, 0xF1000)
assert 0 < lib.vvc355_pic_digest_work_bytes(ctypes.addressof(big), 10) < 128 << 10
tiny = dc.frame_of(8, dc.chroma_dims(1, 1, 400), [0x10001], [1], 0xF0000, 0xF1000)
assert lib.vvc355_pic_digest_work_bytes(ctypes.addressof(tiny), 8) == dc.PART_BYTES
"""
    r = subprocess.run([sys.executable, "-c", CHILD + body + "\nprint('validated')\n"], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-1500:])
    assert b"validated" in r.stdout
