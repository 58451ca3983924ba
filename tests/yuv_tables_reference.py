"""libswscale's table-driven yuv420 -> BGR24 converter (yuv2rgb.c), restated LITERALLY in numpy, for both ranges.

What cv2.VideoCapture.retrieve() runs on a decoded 4:2:0 picture of the picture's own size: ff_yuv2rgb_c_init_tables builds ONE clip table
and, per chroma value, a pointer into it; yuv2rgb_c_24_bgr looks every pixel up, with the nearest chroma sample (a 2 x 2 cell shares U, V).
This file keeps the tables as tables -- the clip table `ytab`, the per-V offsets of R, the per-U offsets of B, the per-U and per-V offsets
whose sum is G's -- where the library evaluates them arithmetically from a handful of integers (csrc/avd_tables.cpp: build_yuv_consts).
It is written from the published algorithm, not from that function, and shares nothing with it:

    crv, cbu, cgu, cgv = 104597, 132201, -25675, -53279              ff_yuv2rgb_coeffs[SWS_CS_DEFAULT] (BT.601), 16.16
    limited range:  cy = (65536 * 255) / 219,  oy = 16 << 16         the luma excursion 16 .. 235 stretched to 0 .. 255
    full range:     cy = 65536, oy = 0, every chroma coefficient c -> (c * 224) / 255      (C division: truncating)
    contrast = saturation = 1 << 16, brightness = 0: identities
    c -> (c * 65536 + 0x8000) / cy                                   "scale coefficients by cy", C division
    ytab[i] = clip_uint8((yb + 0x8000) >> 16),  yb = -(384 << 16) - HEADROOM * cy - oy + i * cy
    yoffs = (full range ? 384 : 326) + HEADROOM
    table_rV[V] = ytab + yoffs + ((V * crv) >> 16) - (crv >> 9), likewise bU with cbu; gU, gV with cgu, cgv (arithmetic shifts)
    B = table_bU[U][Y],  G = (table_gU[U] + table_gV[V])[Y],  R = table_rV[V][Y]

With full_range=False it equals oracle/avd_oracle.c's avdo_nv12_to_bgr24 bit for bit (tests/test_fullrange_host.py), which ties it to the
pinned converter.  Parity of either range with a real libswscale is UNPINNED: there is none to compare with, and x86 builds dispatch to
SIMD code that differs from the C tables by +-1."""
import functools

import numpy as np

HEADROOM = 512
ENUM_LEVELS = (0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 240, 254, 255)


def _cdiv(a: int, b: int) -> int:
    """C's integer division: truncates toward zero"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


@functools.lru_cache(maxsize=None)
def tables(full_range: bool):
    """-> dict: ytab uint8[1024 + 2 * HEADROOM], yoffs, r_off[256] (by V), b_off[256] (by U), gu_off[256], gv_off[256] (offsets from
    ytab + yoffs), and the rescaled integers cy, crv, cbu, cgu, cgv, oy"""
    crv, cbu, cgu, cgv = 104597, 132201, -25675, -53279
    cy, oy = 1 << 16, 0
    if full_range:
        crv, cbu, cgu, cgv = (_cdiv(c * 224, 255) for c in (crv, cbu, cgu, cgv))
    else:
        cy, oy = _cdiv(cy * 255, 219), 16 << 16
    crv, cbu, cgu, cgv = (_cdiv(c * 65536 + 0x8000, cy) for c in (crv, cbu, cgu, cgv))
    size = 1024 + 2 * HEADROOM
    yb0 = -(384 << 16) - HEADROOM * cy - oy
    ytab = np.array([min(max((yb0 + i * cy + 0x8000) >> 16, 0), 255) for i in range(size)], np.uint8)     # Python's >> floors, as C's does here
    off = lambda c: np.array([((s * c) >> 16) - (c >> 9) for s in range(256)], np.int64)
    return dict(ytab=ytab, yoffs=(384 if full_range else 326) + HEADROOM, r_off=off(crv), b_off=off(cbu), gu_off=off(cgu), gv_off=off(cgv),
                cy=cy, crv=crv, cbu=cbu, cgu=cgu, cgv=cgv, oy=oy)


def nv12_to_bgr(y: np.ndarray, uv: np.ndarray, full_range: bool) -> np.ndarray:
    """y uint8[..., H, W], uv uint8[..., H/2, W] (U, V interleaved) -> uint8[..., H, W, 3], by table lookups"""
    t = tables(bool(full_range))
    y, uv = np.asarray(y), np.asarray(uv)
    h, w = y.shape[-2:]
    assert uv.shape[-2:] == (h // 2, w) and h % 2 == 0 and w % 2 == 0
    u = np.repeat(np.repeat(uv[..., 0::2], 2, axis=-2), 2, axis=-1)             # nearest chroma: a 2 x 2 cell shares its sample
    v = np.repeat(np.repeat(uv[..., 1::2], 2, axis=-2), 2, axis=-1)
    base = t["yoffs"] + y.astype(np.int64)
    out = np.empty(y.shape + (3,), np.uint8)
    out[..., 0] = t["ytab"][base + t["b_off"][u]]
    out[..., 1] = t["ytab"][base + t["gu_off"][u] + t["gv_off"][v]]
    out[..., 2] = t["ytab"][base + t["r_off"][v]]
    return out


def consts(full_range: bool) -> dict:
    """The integers an arithmetic evaluation of the tables needs, derived from the TABLES' construction: value = clip8((c0 + (Y + off) * cy) >> 16)
    with off the table offsets, whose constant parts are kr = -(crv >> 9), kb = -(cbu >> 9), kg = -(cgu >> 9) - (cgv >> 9)."""
    t = tables(bool(full_range))
    c0 = -(384 << 16) - HEADROOM * t["cy"] - t["oy"] + t["yoffs"] * t["cy"] + 0x8000         # ytab[yoffs + i] = clip8((c0 + i * cy) >> 16)
    return dict(cy=t["cy"], crv=t["crv"], cbu=t["cbu"], cgu=t["cgu"], cgv=t["cgv"], c0=c0, kr=int(t["r_off"][0]), kb=int(t["b_off"][0]),
                kg=int(t["gu_off"][0] + t["gv_off"][0]))


def offset_ranges(full_range: bool) -> dict:
    """per channel (min, max) of the table offset over U, V in 0 .. 255"""
    t = tables(bool(full_range))
    g = t["gu_off"][:, None] + t["gv_off"][None, :]
    return {"R": (int(t["r_off"].min()), int(t["r_off"].max())), "B": (int(t["b_off"].min()), int(t["b_off"].max())), "G": (int(g.min()), int(g.max()))}


def index_window(full_range: bool):
    """(min, max) of Y + offset over Y, U, V in 0 .. 255: what a table indexed by it must hold"""
    r = offset_ranges(full_range).values()
    return min(lo for lo, _ in r), max(hi for _, hi in r) + 255


# ---- test content ------------------------------------------------------------------------------------------------------------------------
def enum_cells():
    """(Y, U, V) over ENUM_LEVELS^3, int array [2197, 3], Y slowest"""
    lv = np.array(ENUM_LEVELS)
    return np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), -1).reshape(-1, 3)


def enum_frames(h: int, w: int) -> int:
    """frames of h x w it takes to hold one 2 x 2 cell per enumerated triple"""
    return -(-len(enum_cells()) // ((h // 2) * (w // 2)))


def enum_planes(n: int, h: int, w: int, seed: int):
    """NV12 planes (y uint8[n, h, w], uv uint8[n, h/2, w]) of seeded random bytes whose leading 2 x 2 cells -- row-major over the cell grid,
    frame after frame -- enumerate ENUM_LEVELS^3: every triple is there once, both ends of the full-range index window among them
    ((0, 0, .) and (255, 255, .)).  n > enum_frames(h, w), so at least one frame is random throughout."""
    cells = enum_cells()
    per = (h // 2) * (w // 2)
    assert h % 2 == 0 and w % 2 == 0 and n > enum_frames(h, w), (n, h, w)
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    uv = rng.integers(0, 256, (n, h // 2, w), dtype=np.uint8)
    yc = y.reshape(n, h // 2, 2, w // 2, 2).transpose(0, 1, 3, 2, 4).reshape(n * per, 4).copy()      # [cell][4 luma samples]
    cc = uv.reshape(n * per, 2).copy()                                                             # [cell][U, V]
    yc[:len(cells)] = cells[:, :1]
    cc[:len(cells)] = cells[:, 1:]
    y = np.ascontiguousarray(yc.reshape(n, h // 2, w // 2, 2, 2).transpose(0, 1, 3, 2, 4).reshape(n, h, w))
    return y, np.ascontiguousarray(cc.reshape(n, h // 2, w))
