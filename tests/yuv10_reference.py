"""10-bit 4:2:0 in 16-bit words (include/avd.h: AVD_FMT_P010, AVD_FMT_I010), restated in numpy.

The definition is a narrowing followed by the 8-bit 4:2:0 path: every little-endian 16-bit word s becomes one 8-bit sample,

    P010 (the 10 bits in the HIGH bits of the word)   s8 = min(255, (s + 128) >> 8)
    I010 (the 10 bits in the LOW bits)                s8 = min(255, (s + 2) >> 2)

-- total over all 65536 words, so that no input is undefined -- and the NV12 / I420 picture of those samples goes through libswscale's table
converter as tests/yuv_tables_reference.py restates it (nearest chroma, limited or full range).  With the low six bits of a P010 word zero
both are (v10 + 2) >> 2 clipped to 255: what libswscale's 16-bit input path is believed to hand its one-tap vertical output (v << 5, then
(x + 64) >> 7).  That restatement is from memory, and parity with a real libswscale is UNPINNED, as for every other layout.
The packers go from 10-bit (Y, U, V) planes to each layout and `planes_of` back."""
import numpy as np

from tests import yuv_tables_reference as ytr

P010, I010 = 0x30, 0x31
LAYOUTS = (P010, I010)
NAMES = {P010: "p010", I010: "i010"}


def narrow_p010(s) -> np.ndarray:
    """uint16 words with the sample in the high bits -> uint8; formed in 32 bits, so that s + 128 cannot wrap"""
    s = np.asarray(s)
    assert s.dtype == np.uint16
    return np.minimum(255, (s.astype(np.int64) + 128) >> 8).astype(np.uint8)


def narrow_i010(s) -> np.ndarray:
    """uint16 words with the sample in the low bits -> uint8"""
    s = np.asarray(s)
    assert s.dtype == np.uint16
    return np.minimum(255, (s.astype(np.int64) + 2) >> 2).astype(np.uint8)


NARROW = {P010: narrow_p010, I010: narrow_i010}


def pack(fmt: int, y10, u10, v10):
    """10-bit (Y [..., H, W], U and V [..., H/2, W/2]) -> the clip in layout fmt: (y, uv uint16[..., H/2, W]) with the samples shifted into the
    high bits (P010) or (y, u, v) as they are (I010)"""
    y10, u10, v10 = (np.asarray(p, np.uint16) for p in (y10, u10, v10))
    assert max(int(y10.max()), int(u10.max()), int(v10.max())) < 1024
    if fmt == I010:
        return y10, u10, v10
    assert fmt == P010, fmt
    uv = np.empty(u10.shape[:-1] + (2 * u10.shape[-1],), np.uint16)
    uv[..., 0::2], uv[..., 1::2] = u10 << 6, v10 << 6
    return y10 << 6, uv


def planes_of(fmt: int, clip):
    """the words of a clip, plane by plane as (Y, U, V) -- NOT shifted back: what the narrowing is defined on"""
    if fmt == I010:
        return tuple(np.asarray(p) for p in clip)
    y, uv = (np.asarray(p) for p in clip)
    return y, uv[..., 0::2], uv[..., 1::2]


def unpack(fmt: int, clip):
    """the inverse of pack: -> 10-bit (Y, U, V)"""
    y, u, v = planes_of(fmt, clip)
    return (y, u, v) if fmt == I010 else (y >> 6, u >> 6, v >> 6)


def narrowed_i420(fmt: int, clip):
    """-> the 8-bit I420 picture (y, u, v) of the clip's samples"""
    return tuple(NARROW[fmt](p) for p in planes_of(fmt, clip))


def narrowed_nv12(fmt: int, clip):
    """-> the 8-bit NV12 picture (y, uv) of the clip's samples"""
    y, u, v = narrowed_i420(fmt, clip)
    uv = np.empty(u.shape[:-1] + (2 * u.shape[-1],), np.uint8)
    uv[..., 0::2], uv[..., 1::2] = u, v
    return y, uv


def to_bgr(fmt: int, clip, full_range: bool) -> np.ndarray:
    """narrow, then the table converter of the 8-bit path -> uint8[..., H, W, 3]"""
    return ytr.nv12_to_bgr(*narrowed_nv12(fmt, clip), full_range)


def widen(v8, rem) -> np.ndarray:
    """8-bit samples -> 10-bit values that narrow back to them: 4 v8 - 2 + rem with rem in 0 .. 3 (clipped at 0), i.e. v10 mod 4 = 2, 3 (rounded
    up) or 0, 1 (rounded down)"""
    v10 = np.maximum(0, 4 * np.asarray(v8).astype(np.int64) - 2 + np.asarray(rem))
    assert int(v10.max()) <= 1021
    return v10.astype(np.uint16)


def random_planes10(n: int, h: int, w: int, seed: int):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1024, (n, h, w), dtype=np.uint16), rng.integers(0, 1024, (n, h // 2, w // 2), dtype=np.uint16),
            rng.integers(0, 1024, (n, h // 2, w // 2), dtype=np.uint16))


def enum_planes10(n: int, h: int, w: int, seed: int):
    """10-bit (Y, U, V) whose NARROWED leading 2 x 2 cells enumerate ytr.enum_cells() as ytr.enum_planes lays them out: every 8-bit sample of
    that content is widened with a low remainder that cycles 0 .. 3 along each plane, so both rounding directions occur on every level"""
    y8, uv8 = ytr.enum_planes(n, h, w, seed)
    cyc = lambda a: (np.arange(a.size) % 4).reshape(a.shape)
    u8, v8 = uv8[..., 0::2], uv8[..., 1::2]
    return widen(y8, cyc(y8)), widen(u8, cyc(u8)), widen(v8, (cyc(v8) + 1) % 4)
