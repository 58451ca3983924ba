"""The 4:2:2 conversion of the fused ingest (include/avd.h: AVD_FMT_YUYV422 / _UYVY422 / _I422 / _NV16), restated in numpy.

Pixel (y, x) has luma Y[y][x] and the chroma sample U[y][x >> 1], V[y][x >> 1] of its OWN row; its BGR triple is what libswscale's table
converter gives: B = T[Y + ob(U)], G = T[Y + og(U, V)], R = T[Y + or(V)], with the very tables of the 4:2:0 path
(tests/yuv_tables_reference.py::tables), limited or full range.  The four layouts differ only in where the samples lie; the packers below
go from (Y, U, V) to each of them and `planes_of` back.  tests/test_yuv422_host.py ties this file to the pinned 4:2:0 converters through two
identities (row doubling, chroma-row pairs).  Parity with a real libswscale is UNPINNED, as for 4:2:0."""
import numpy as np

from tests import yuv_tables_reference as ytr

YUYV422, UYVY422, I422, NV16 = 0x20, 0x21, 0x22, 0x23
LAYOUTS = (YUYV422, UYVY422, I422, NV16)
NAMES = {YUYV422: "yuyv422", UYVY422: "uyvy422", I422: "i422", NV16: "nv16"}


def to_bgr(y, u, v, full_range: bool) -> np.ndarray:
    """y uint8[..., H, W], u and v uint8[..., H, W/2] -> uint8[..., H, W, 3] by table lookups; H may be odd"""
    t = ytr.tables(bool(full_range))
    y, u, v = np.asarray(y), np.asarray(u), np.asarray(v)
    h, w = y.shape[-2:]
    assert w % 2 == 0 and u.shape[-2:] == (h, w // 2) == v.shape[-2:], (y.shape, u.shape, v.shape)
    u, v = np.repeat(u, 2, axis=-1), np.repeat(v, 2, axis=-1)              # a pixel pair shares the sample of its own row
    base = t["yoffs"] + y.astype(np.int64)
    out = np.empty(y.shape + (3,), np.uint8)
    out[..., 0] = t["ytab"][base + t["b_off"][u]]
    out[..., 1] = t["ytab"][base + t["gu_off"][u] + t["gv_off"][v]]
    out[..., 2] = t["ytab"][base + t["r_off"][v]]
    return out


def pack(fmt: int, y, u, v):
    """(Y, U, V) -> the clip in layout fmt: uint8[..., H, W, 2] (packed), (y, u, v) (I422) or (y, uv uint8[..., H, W]) (NV16)"""
    y, u, v = np.asarray(y), np.asarray(u), np.asarray(v)
    if fmt == I422:
        return y, u, v
    if fmt == NV16:
        uv = np.empty(y.shape, np.uint8)
        uv[..., 0::2], uv[..., 1::2] = u, v
        return y, uv
    out = np.empty(y.shape + (2,), np.uint8)
    luma, chroma = (0, 1) if fmt == YUYV422 else (1, 0)       # YUYV: Y0 U Y1 V;  UYVY: U Y0 V Y1
    assert fmt in (YUYV422, UYVY422), fmt
    out[..., luma] = y
    out[..., 0::2, chroma] = u
    out[..., 1::2, chroma] = v
    return out


def planes_of(fmt: int, clip):
    """the inverse of pack: -> (Y, U, V)"""
    if fmt == I422:
        return tuple(np.asarray(p) for p in clip)
    if fmt == NV16:
        y, uv = (np.asarray(p) for p in clip)
        return y, uv[..., 0::2], uv[..., 1::2]
    a = np.asarray(clip)
    luma, chroma = (0, 1) if fmt == YUYV422 else (1, 0)
    return a[..., luma], a[..., 0::2, chroma], a[..., 1::2, chroma]


def clip_to_bgr(fmt: int, clip, full_range: bool) -> np.ndarray:
    return to_bgr(*planes_of(fmt, clip), full_range)


def random_planes(n: int, h: int, w: int, seed: int):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, h, w), dtype=np.uint8), rng.integers(0, 256, (n, h, w // 2), dtype=np.uint8),
            rng.integers(0, 256, (n, h, w // 2), dtype=np.uint8))


def enum_planes(n: int, h: int, w: int, seed: int):
    """Seeded random (Y, U, V) whose leading pixel pairs -- row-major, frame after frame -- enumerate ENUM_LEVELS^3 (Y, U, V): every triple
    once, both ends of either range's index window among them.  More pairs than triples, so the rest is random."""
    cells = ytr.enum_cells()
    assert w % 2 == 0 and n * h * (w // 2) > len(cells), (n, h, w)
    y, u, v = random_planes(n, h, w, seed)
    y.reshape(-1, 2)[:len(cells)] = cells[:, :1]
    u.reshape(-1)[:len(cells)] = cells[:, 1]
    v.reshape(-1)[:len(cells)] = cells[:, 2]
    return y, u, v
