"""Packed coefficient levels (vvc355_tb_levels, include/vvc_mi355.h) restated in numpy: the packer, the unpacker and random blocks.

A block's levels become 4x4 groups of int16 (slot (y & 3) * 4 + (x & 3)) on a grid of ceil(min(w, 32) / 4) x ceil(min(h, 32) / 4)
tiles; bit gy * gw + gx of the side record's mask marks a coded tile, and the coded tiles follow each other in bit order."""
import numpy as np

from ffvvc_amd import abi

DCT2 = 0
LV_DTYPE = np.dtype([("groups", "<u8"), ("first", "<u4"), ("flags", "<u4")])


def grid(w, h):
    return (min(w, 32) + 3) // 4, (min(h, 32) + 3) // 4


def pack(c):
    """int32 levels (h, w) -> (mask, groups (n, 16) int16), or None when the block must stay on the int32 path."""
    h, w = c.shape
    if np.any(c[32:, :]) or np.any(c[:, 32:]) or c.min(initial=0) < -32768 or c.max(initial=0) > 32767:
        return None
    gw, gh = grid(w, h)
    pad = np.zeros((gh * 4, gw * 4), np.int64)
    hh, ww = min(h, 32), min(w, 32)
    pad[:hh, :ww] = c[:hh, :ww]
    tiles = pad.reshape(gh, 4, gw, 4).transpose(0, 2, 1, 3).reshape(gh * gw, 16)
    coded = np.any(tiles != 0, axis=1)
    mask = 0
    for b in np.flatnonzero(coded):
        mask |= 1 << int(b)
    return mask, tiles[coded].astype(np.int16)


def unpack(mask, stream, first, w, h):
    """The inverse: a block's int32 levels (h, w) from its mask and the stream (int16, groups of 16)."""
    gw, gh = grid(w, h)
    pad = np.zeros((gh * 4, gw * 4), np.int32)
    k = first
    for b in range(gw * gh):
        if mask >> b & 1:
            gy, gx = divmod(b, gw)
            pad[gy * 4:gy * 4 + 4, gx * 4:gx * 4 + 4] = stream[k * 16:(k + 1) * 16].reshape(4, 4)
            k += 1
    out = np.zeros((h, w), np.int32)
    hh, ww = min(h, 32), min(w, 32)
    out[:hh, :ww] = pad[:hh, :ww]
    return out


def pack_all(blocks, force_int32=()):
    """Pack a list of blocks into one stream: (levels int16, 32-byte aligned length; side records LV_DTYPE).  Blocks that do not fit,
    and the indices in force_int32, get flags bit 0 and no groups."""
    lv = np.zeros(len(blocks), LV_DTYPE)
    parts, n = [], 0
    for i, c in enumerate(blocks):
        p = None if i in force_int32 else pack(c)
        lv[i]["first"] = n
        if p is None:
            lv[i]["flags"] = abi.LEVELS_INT32
            continue
        lv[i]["groups"] = p[0]
        parts.append(p[1])
        n += len(p[1])
    levels = np.concatenate(parts).ravel() if parts else np.zeros(0, np.int16)
    return np.concatenate([levels, np.zeros(16, np.int16)]).astype(np.int16), lv


def laplace_levels(rng, shape, scale=1.1):
    """Sparse levels with a Laplacian magnitude distribution (about half of them zero)."""
    mag = np.floor(-np.log(np.clip(rng.random(shape), 1e-9, None)) * scale).astype(np.int64)
    return (mag * rng.choice([-1, 1], size=shape)).astype(np.int32)


def windowed_block(rng, w, h, nzw, nzh, bits=None):
    """Levels inside [0, nzw) x [0, nzh) only: Laplacian, or uniform of `bits` bits."""
    c = np.zeros((h, w), np.int32)
    if bits is None:
        c[:nzh, :nzw] = laplace_levels(rng, (nzh, nzw), scale=float(rng.choice([0.5, 1.1, 4.0])))
    else:
        c[:nzh, :nzw] = rng.integers(-(1 << bits), 1 << bits, size=(nzh, nzw))
    return c


def nz_limits(trh, trv, w, h):
    return min(32 if trh == DCT2 else 16, w), min(32 if trv == DCT2 else 16, h)
