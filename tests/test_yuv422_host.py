"""4:2:2 pictures (AVD_FMT_YUYV422 / _UYVY422 / _I422 / _NV16), the parts that need no GPU: the four values in header, library-side header and
binding; the definition (tests/yuv422_reference.py) tied to the pinned 4:2:0 converters through the row-doubling and the chroma-row-pairs
identities; the refusals of from_picture / from_frame_list / check_clip in their documented order; the staging plan of host clips; the
table-fill eligibility of lists; the descriptors the binding builds; a C422 .y4m written and read back.  The host logic runs in a stand-alone
program (tests/ingest_check.cpp, built with the address and undefined-behaviour sanitizers by tests/ingest_host_kit.py, which also
holds the case writers, the answer reader and the texts every layout shares)."""
import ctypes
import os
import re

import numpy as np
import pytest

import avd_hip
from avd_hip import _lib, sources
from tests import yuv422_reference as ref
from tests import yuv_tables_reference as ytr
from tests.ingest_host_kit import (ARG, BASE, BGR, DEVICE, FULL, HOST, I420, NV12, OK, PLANES, PX, ROOT, T_GEOM, T_MEM, T_SMALL, UNSUPPORTED,  # noqa: F401
                                   binding, frame_list, list_addrs, parse, picture, program, r256, row_bytes, t_format, t_reserved, t_rotate)

YUYV, UYVY, I422, NV16 = ref.LAYOUTS
NEW = ref.LAYOUTS
T_TURNED = "a turned 4:2:2 picture is not on the path: the conversion does not commute with quarter turns"
T_SHARE = "the U and V planes of an I422 picture share their strides"
T_EVEN = {YUYV: "YUYV422 needs even width", UYVY: "UYVY422 needs even width", I422: "I422 needs even width", NV16: "NV16 needs even width"}
T_NULL = {YUYV: "null frame pointer", UYVY: "null frame pointer", I422: "null I422 plane pointer", NV16: "null NV16 plane pointer"}
T_STRIDES = {YUYV: "strides smaller than the frame", UYVY: "strides smaller than the frame", I422: "strides smaller than the I422 planes",
             NV16: "strides smaller than the NV16 planes"}
parse_p = parse_l = parse


# ---- the values -----------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree_on_the_four_values(program):
    hdr = open(os.path.join(ROOT, "include", "avd.h")).read()
    names = ("AVD_FMT_YUYV422", "AVD_FMT_UYVY422", "AVD_FMT_I422", "AVD_FMT_NV16")
    for name, value in zip(names, (0x20, 0x21, 0x22, 0x23)):
        assert int(re.search(r"^#define %s\s+(0x[0-9a-fA-F]+)\s*$" % name, hdr, re.M).group(1), 16) == value
        assert getattr(_lib, name) == value == getattr(avd_hip, name)
        assert _lib.LAYOUT[value].planes == PLANES[value]
    a = parse(program(["A"])[0])
    assert a["picture_size"] == ctypes.sizeof(_lib.AvdPicture) == 104
    assert a["list_size"] == ctypes.sizeof(_lib.AvdFrameList) == 80
    assert tuple(a[name] for name in names) == NEW == (0x20, 0x21, 0x22, 0x23)
    for text in ("14 yuyv_scalar, 15 yuyv_tables, 16 i422_scalar, 17 i422_tables, 18 nv16_scalar, 19 nv16_tables", "UNPINNED", "YV16",
                 "FFmpeg up to 7.0", "could not be determined", "4:4:4 and 10-bit"):
        assert text in hdr, text
    own = open(os.path.join(ROOT, "include", "avd_frame_list.h")).read()
    assert "AVD_FMT_I422: Y, U, V; AVD_FMT_NV16: Y, interleaved UV" in own


# ---- the definition -------------------------------------------------------------------------------------------------------------------------
def _doubled_nv12(y, u, v):
    """the NV12 picture of height 2h whose luma rows 2r and 2r + 1 are both Y[r] and whose chroma row r is the 4:2:2 picture's"""
    return np.repeat(y, 2, axis=-2), ref.pack(NV16, y, u, v)[1]


def test_reference_equals_the_pinned_converter_by_row_doubling(oracle):
    """limited range, against avdo_nv12_to_bgr24; odd height and enumerated content"""
    for y, u, v in (ref.random_planes(2, 33, 48, 1), ref.enum_planes(2, 37, 64, 2)):
        y2, uv2 = _doubled_nv12(y, u, v)
        want = oracle.nv12_to_bgr(y2, uv2)[:, 0::2]
        assert np.array_equal(ref.to_bgr(y, u, v, False), want)
        assert np.array_equal(oracle.nv12_to_bgr(y2, uv2)[:, 1::2], want)          # the odd rows say the same


@pytest.mark.parametrize("full_range", (False, True), ids=("limited", "full"))
def test_reference_equals_the_table_restatement_for_both_ranges(full_range):
    y, u, v = ref.enum_planes(2, 37, 64, 3)
    # the content reaches both ends of the range's index window
    t = ytr.tables(full_range)
    yy, uu, vv = y.astype(np.int64), np.repeat(u, 2, -1), np.repeat(v, 2, -1)
    idx = np.stack([yy + t["b_off"][uu], yy + t["gu_off"][uu] + t["gv_off"][vv], yy + t["r_off"][vv]])
    assert (int(idx.min()), int(idx.max())) == ytr.index_window(full_range)
    want = ytr.nv12_to_bgr(*_doubled_nv12(y, u, v), full_range)[:, 0::2]
    assert np.array_equal(ref.to_bgr(y, u, v, full_range), want)
    # every layout carries the same samples
    for fmt in NEW:
        clip = ref.pack(fmt, y, u, v)
        for a, b in zip(ref.planes_of(fmt, clip), (y, u, v)):
            assert np.array_equal(a, b), ref.NAMES[fmt]
        assert np.array_equal(ref.clip_to_bgr(fmt, clip, full_range), want)
    assert not np.array_equal(ref.to_bgr(y, u, v, True), ref.to_bgr(y, u, v, False))


@pytest.mark.parametrize("full_range", (False, True), ids=("limited", "full"))
def test_chroma_row_pairs_give_the_420_result(full_range):
    """a 4:2:2 picture of even height whose chroma rows 2k and 2k + 1 are equal is the I420 / NV12 picture on chroma rows k"""
    y4, uv4 = ytr.enum_planes(ytr.enum_frames(36, 64) + 1, 36, 64, 4)
    u, v = np.repeat(uv4[..., 0::2], 2, axis=-2), np.repeat(uv4[..., 1::2], 2, axis=-2)
    assert np.array_equal(ref.to_bgr(y4, u, v, full_range), ytr.nv12_to_bgr(y4, uv4, full_range))


def test_packed_byte_positions():
    y = np.array([[[10, 11, 12, 13]]], np.uint8)
    u, v = np.array([[[20, 21]]], np.uint8), np.array([[[30, 31]]], np.uint8)
    assert ref.pack(YUYV, y, u, v).reshape(-1).tolist() == [10, 20, 11, 30, 12, 21, 13, 31]
    assert ref.pack(UYVY, y, u, v).reshape(-1).tolist() == [20, 10, 30, 11, 21, 12, 31, 13]
    assert ref.pack(NV16, y, u, v)[1].reshape(-1).tolist() == [20, 30, 21, 31]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NEW, ids=lambda f: ref.NAMES[f])
def test_accepted_as_described(program, fmt):
    p = parse_p(program([picture(fmt)])[0])
    assert (p["status"], p["why"], p["format"], p["planes"], p["px"], p["full"]) == (OK, "", fmt, PLANES[fmt], PX[fmt], 0)
    # the chroma planes have h rows; the height may be ODD, the range flag is taken out of the format
    p = parse_p(program([picture(fmt | FULL, h=33, w=34)])[0])
    assert (p["status"], p["format"], p["full"]) == (OK, fmt, 1)
    assert (p["sub_rows"], p["sub_row"]) == (33, 17 if fmt == I422 else 34)
    l = parse_l(program([frame_list(fmt | FULL, list_addrs(fmt), h=33, w=34)])[0])
    assert (l["status"], l["format"], l["planes"], l["px"], l["full"], l["sub_rows"]) == (OK, fmt, PLANES[fmt], PX[fmt], 1, 33)
    # the limits themselves, and n = 0 asking for no planes
    assert parse_p(program([picture(fmt, h=16383, w=16384, n=1)])[0])["status"] == OK
    assert parse_p(program([picture(fmt, h=32, w=32)])[0])["status"] == OK
    assert parse_p(program([picture(fmt, n=0, planes=(0, 0, 0))])[0])["status"] == OK


@pytest.mark.parametrize("fmt", NEW, ids=lambda f: ref.NAMES[f])
def test_refusal_table_of_a_picture(program, fmt):
    rb = row_bytes(fmt, 64)
    short0 = [rb[0] - 1, rb[1], rb[2]]
    table = [
        (picture(fmt, rotate=4), ARG, t_rotate("picture")),
        (picture(fmt, reserved=1), ARG, t_reserved("picture")),
        (picture(fmt, rotate=1), UNSUPPORTED, T_TURNED),
        (picture(fmt | FULL, rotate=2), UNSUPPORTED, T_TURNED),
        (picture(fmt, rotate=3), UNSUPPORTED, T_TURNED),
        (picture(fmt, mem=2), ARG, T_MEM),
        (picture(fmt, w=16386), ARG, T_GEOM),
        (picture(fmt, h=16385), ARG, T_GEOM),
        (picture(fmt, h=0), ARG, T_GEOM),
        (picture(fmt, n=-1), ARG, T_GEOM),
        (picture(fmt, w=63), UNSUPPORTED, T_EVEN[fmt]),
        (picture(fmt, h=31), UNSUPPORTED, T_SMALL),
        (picture(fmt, w=30), UNSUPPORTED, T_SMALL),
        (picture(fmt, planes=(0,) + BASE[1:]), ARG, T_NULL[fmt]),
        (picture(fmt, rs=short0), ARG, T_STRIDES[fmt]),
        (picture(fmt, fs=[rb[0] * 48 - 1, rb[1] * 48, rb[2] * 48]), ARG, T_STRIDES[fmt]),
        # pairs of faults: the documented order
        (picture(fmt, rotate=4, reserved=1, mem=2), ARG, t_rotate("picture")),
        (picture(fmt, rotate=1, reserved=1), ARG, t_reserved("picture")),
        (picture(fmt, rotate=1, mem=2), UNSUPPORTED, T_TURNED),
        (picture(fmt, rotate=1, w=63), UNSUPPORTED, T_TURNED),
        (picture(fmt, mem=2, w=16386), ARG, T_MEM),
        (picture(fmt, w=16385, h=31), ARG, T_GEOM),
        (picture(fmt, w=31), UNSUPPORTED, T_EVEN[fmt]),                           # evenness before the 32 x 32 minimum, as for 4:2:0
        (picture(fmt, h=31, planes=(0, 0, 0)), UNSUPPORTED, T_SMALL),
        (picture(fmt, planes=(0,) + BASE[1:], rs=short0), ARG, T_NULL[fmt]),
        (picture(fmt | 0x200), ARG, t_format("picture")),
        (picture(fmt | 0x200 | FULL), ARG, t_format("picture")),
    ]
    if PLANES[fmt] >= 2:
        table += [
            (picture(fmt, planes=(BASE[0], 0, BASE[2])), ARG, T_NULL[fmt]),
            (picture(fmt, rs=[rb[0], rb[1] - 1, rb[2] - 1]), ARG, T_STRIDES[fmt]),
            # the chroma planes have h rows: a frame stride that held h/2 of them is too small
            (picture(fmt, fs=[rb[0] * 48, rb[1] * 24, rb[2] * 24]), ARG, T_STRIDES[fmt]),
            (picture(fmt, fs=[rb[0] * 48, rb[1] * 48 - 1, rb[2] * 48 - 1]), ARG, T_STRIDES[fmt]),
        ]
    if fmt == I422:
        table += [
            (picture(fmt, planes=(BASE[0], BASE[1], 0)), ARG, T_NULL[fmt]),
            (picture(fmt, rs=[64, 32, 48]), ARG, T_SHARE),
            (picture(fmt, fs=[64 * 48, 32 * 48, 32 * 49]), ARG, T_SHARE),
            (picture(fmt, rotate=1, rs=[64, 32, 48]), UNSUPPORTED, T_TURNED),     # the turn before the strides
            (picture(fmt, rs=[64, 32, 48], mem=2), ARG, T_SHARE),                 # the descriptor's before check_clip's
            (picture(fmt, rs=[64, 32, 48], w=63), ARG, T_SHARE),
        ]
    elif fmt == NV16:
        table += [(picture(fmt, planes=(BASE[0], BASE[1], 0), rs=[64, 64, 1], fs=[64 * 48, 64 * 48, 2]), OK, "")]     # plane 2 is not looked at
    else:
        table += [(picture(fmt, planes=(BASE[0], 0, 0), rs=[128, 1, 2], fs=[128 * 48, 3, 4]), OK, "")]                  # one plane
    got = program([t[0] for t in table])
    for (line, status, why), g in zip(table, got):
        p = parse_p(g)
        assert (p["status"], p["why"]) == (status, why), (line, g)


@pytest.mark.parametrize("fmt", NEW, ids=lambda f: ref.NAMES[f])
def test_refusal_table_of_a_frame_list(program, fmt):
    a = list_addrs(fmt)
    rb = row_bytes(fmt, 64)
    holed = [list(pl) for pl in a]
    holed[-1][1] = 0
    table = [
        (frame_list(fmt, a, rotate=-1), ARG, t_rotate("frame_list")),
        (frame_list(fmt, a, reserved=7), ARG, t_reserved("frame_list")),
        (frame_list(fmt, a, rotate=3), UNSUPPORTED, T_TURNED),
        (frame_list(fmt, a, mem=-1), ARG, T_MEM),
        (frame_list(fmt, a, h=16385), ARG, T_GEOM),
        (frame_list(fmt, a, w=34 + 1), UNSUPPORTED, T_EVEN[fmt]),
        (frame_list(fmt, a, w=30), UNSUPPORTED, T_SMALL),
        (frame_list(fmt, a, null_arrays=1 << (PLANES[fmt] - 1)), ARG, "null plane array of a frame list"),
        (frame_list(fmt, holed), ARG, "null plane pointer in a frame list"),
        (frame_list(fmt, a, rs=[rb[0] - 1, rb[1], rb[2]]), ARG, T_STRIDES[fmt]),
        (frame_list(fmt, a, rotate=3, reserved=1), ARG, t_reserved("frame_list")),
        (frame_list(fmt, a, rotate=3, mem=5), UNSUPPORTED, T_TURNED),
        (frame_list(fmt, holed, rs=[rb[0] - 1, rb[1], rb[2]]), ARG, "null plane pointer in a frame list"),
        (frame_list(fmt | 0x200, a), ARG, t_format("frame_list")),
    ]
    if fmt == I422:
        table += [(frame_list(fmt, a, rs=[64, 32, 48]), ARG, T_SHARE), (frame_list(fmt, a, rs=[64, 48, 32], rotate=1), UNSUPPORTED, T_TURNED),
                  (frame_list(fmt, a, rs=[64, 31, 31]), ARG, T_STRIDES[fmt])]
    got = program([t[0] for t in table])
    for (line, status, why), g in zip(table, got):
        l = parse_l(g)
        assert (l["status"], l["why"]) == (status, why), (line, g)


def test_neighbouring_layout_values_stay_refused(program):
    for layout in (3, 7, 0x0F, 0x14, 0x1F, 0x24, 0x2F, 0xFF):
        for fmt in (layout, layout | FULL):
            p = parse_p(program([picture(fmt)])[0])
            assert (p["status"], p["why"]) == (ARG, t_format("picture")), hex(fmt)
            l = parse_l(program([frame_list(fmt, [[BASE[0]], [BASE[1]], [BASE[2]]])])[0])
            assert (l["status"], l["why"]) == (ARG, t_format("frame_list")), hex(fmt)


# ---- staging --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", (YUYV, UYVY), ids=lambda f: ref.NAMES[f])
def test_a_packed_clip_is_one_span_of_2w_byte_rows(program, fmt):
    n, h, w = 2, 41, 48
    p = parse_p(program([picture(fmt, n=n, h=h, w=w)])[0])
    assert (p["nspans"], p["off"], p["bytes"], p["plane_off"]) == (1, [0], [n * h * w * 2], [0])
    rs = w * 2 + 32
    p = parse_p(program([picture(fmt, n=n, h=h, w=w, rs=[rs] * 3, fs=[rs * h + 64] * 3)])[0])
    assert p["bytes"] == [(rs * h + 64) * (n - 1) + rs * (h - 1) + w * 2]
    p = parse_p(program([picture(fmt, mem=DEVICE, n=n, h=h, w=w)])[0])
    assert (p["status"], p["nspans"], p["total"]) == (OK, 0, 0)


def test_a_dense_i422_frame_stack_is_one_span(program):
    """a .y4m map: Y, U, V of a frame adjacent, frame after frame (an odd height, a FRAME marker between the pictures)"""
    n, h, w = 3, 41, 48
    hw, c = h * w, h * (w // 2)
    for marker in (0, 6):
        fs = 2 * hw + marker
        planes = (BASE[0], BASE[0] + hw, BASE[0] + hw + c)
        p = parse_p(program([picture(I422, n=n, h=h, w=w, planes=planes, fs=[fs] * 3)])[0])
        assert p["status"] == OK and p["nspans"] == 1
        assert p["bytes"] == [fs * (n - 1) + 2 * hw] and p["off"] == [0] and p["plane_off"] == [0, hw, hw + c]
        assert p["copied"] == fs * (n - 1) + 2 * hw
    # YV16: the pointers exchanged, the same span
    p = parse_p(program([picture(I422, n=1, h=h, w=w, planes=(BASE[0], BASE[0] + hw + c, BASE[0] + hw))])[0])
    assert (p["nspans"], p["bytes"], p["plane_off"]) == (1, [2 * hw], [0, hw + c, hw])


def test_separate_i422_planes_are_three_spans_and_nv16_two(program):
    n, h, w = 2, 33, 34
    ys, cs = n * h * w, n * h * (w // 2)
    p = parse_p(program([picture(I422, n=n, h=h, w=w)])[0])
    assert (p["status"], p["nspans"], p["bytes"]) == (OK, 3, [ys, cs, cs])
    assert p["off"] == [0, r256(ys), r256(ys) + r256(cs)] == p["plane_off"] and p["copied"] == ys + 2 * cs
    p = parse_p(program([picture(NV16, n=n, h=h, w=w)])[0])
    assert (p["status"], p["nspans"], p["bytes"], p["off"], p["plane_off"]) == (OK, 2, [ys, ys], [0, r256(ys)], [0, r256(ys)])
    assert p["copied"] == 2 * ys and p["total"] == 2 * r256(ys)


def test_a_frame_listed_twice_is_copied_once(program):
    h, w = 41, 48
    for fmt in NEW:
        a = list_addrs(fmt, 2)
        twice = [[pl[0], pl[1], pl[0]] for pl in a]
        l = parse_l(program([frame_list(fmt, twice, h=h, w=w)])[0])
        frame = sum(h * r for r in row_bytes(fmt, w)[:PLANES[fmt]])
        assert l["status"] == OK and l["nspans"] == 2 * PLANES[fmt] and l["copied"] == 2 * frame, ref.NAMES[fmt]
        for p in range(PLANES[fmt]):
            assert l["plane_off"][p * 3] == l["plane_off"][p * 3 + 2]
    # I422 frames that are views of one dense stack: one span, as the strided clip
    hw, c = h * w, h * (w // 2)
    views = [[BASE[0] + f * 2 * hw + o for f in range(3)] for o in (0, hw, hw + c)]
    l = parse_l(program([frame_list(I422, views, h=h, w=w)])[0])
    assert (l["nspans"], l["bytes"], l["copied"]) == (1, [6 * hw], 6 * hw)


# ---- table-fill eligibility of a list -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NEW, ids=lambda f: ref.NAMES[f])
def test_list_vec_eligible(program, fmt):
    a = list_addrs(fmt, 3)
    rb = row_bytes(fmt, 64)
    assert parse_l(program([frame_list(fmt, a, mem=DEVICE)])[0])["given"] == 1
    assert parse_l(program([frame_list(fmt, a, mem=DEVICE, h=33)])[0])["given"] == 1           # an odd height changes nothing
    for plane in range(PLANES[fmt]):
        for delta in (1, 4, 8):
            off = [list(pl) for pl in a]
            off[plane][1] += delta
            # the chroma planes of I422 are read 8 bytes at a time: 8 mod 16 is still the table fill, 4 mod 8 is not
            want = 1 if fmt == I422 and plane > 0 and delta == 8 else 0
            assert parse_l(program([frame_list(fmt, off, mem=DEVICE)])[0])["given"] == want, (plane, delta)
    assert parse_l(program([frame_list(fmt, a, mem=DEVICE, w=72)])[0])["given"] == 0
    assert parse_l(program([frame_list(fmt, a, mem=DEVICE, rs=[rb[0] + 8, rb[1], rb[2]])])[0])["given"] == 0
    assert parse_l(program([frame_list(fmt, a, mem=DEVICE, rs=[rb[0] + 16, rb[1], rb[2]])])[0])["given"] == 1
    if PLANES[fmt] > 1:
        assert parse_l(program([frame_list(fmt, a, mem=DEVICE, rs=[rb[0], rb[1] + 8, rb[2] + 8])])[0])["given"] == (1 if fmt == I422 else 0)
        assert parse_l(program([frame_list(fmt, a, mem=DEVICE, rs=[rb[0], rb[1] + 4, rb[2] + 4])])[0])["given"] == 0
    # host frames are judged where they are staged: separately allocated ones land on 256-byte boundaries
    off = [[v + 3 for v in pl] for pl in a]
    l = parse_l(program([frame_list(fmt, off)])[0])
    assert (l["given"], l["staged"]) == (0, 1)


# ---- the binding's descriptors ----------------------------------------------------------------------------------------------------------------
def test_pixels_takes_the_four_layouts():
    y, u, v = ref.random_planes(2, 33, 48, 5)
    for fmt in NEW:
        clip = ref.pack(fmt, y, u, v)
        assert avd_hip.Pixels(clip, fmt).fmt == fmt
    with pytest.raises(ValueError, match="tuple of 3 planes"):
        avd_hip.Pixels((y, u), I422)
    with pytest.raises(ValueError, match="tuple of 2 planes"):
        avd_hip.Pixels((y, u, v), NV16)
    for bad in (NV12, I420, 0x1F, 0x24):
        with pytest.raises(ValueError, match="fmt must be"):
            avd_hip.Pixels(y, bad)


def test_pixels_descriptors(binding):
    n, h, w = 2, 33, 48
    y, u, v = ref.random_planes(n, h, w, 6)
    for fmt in (YUYV, UYVY):
        a = ref.pack(fmt, y, u, v)
        p, cnt, keep = binding._picture(avd_hip.Pixels(a, fmt), 0, True)
        assert (p.format, p.n, p.h, p.w, cnt) == (fmt | FULL, n, h, w, n) and keep is a
        assert (p.plane[0], p.row_stride[0], p.frame_stride[0]) == (a.ctypes.data, 2 * w, 2 * w * h)
        padded = np.zeros((n, h, w + 8, 2), np.uint8)[:, :, :w]
        p, _, keep = binding._picture(avd_hip.Pixels(padded, fmt))
        assert keep is padded and p.row_stride[0] == 2 * (w + 8)
        with pytest.raises(ValueError, match=r"uint8\[N,H,W,2\]"):
            binding._picture(avd_hip.Pixels(np.zeros((n, h, w, 3), np.uint8), fmt))
    p, cnt, _ = binding._picture(avd_hip.Pixels((y, u, v), I422))
    assert (p.format, p.h, p.w, cnt) == (I422, h, w, n)
    assert [p.plane[i] for i in range(3)] == [y.ctypes.data, u.ctypes.data, v.ctypes.data]
    assert list(p.row_stride) == [w, w // 2, w // 2] and list(p.frame_stride) == [w * h, w // 2 * h, w // 2 * h]
    yy, uv = ref.pack(NV16, y, u, v)
    p, _, _ = binding._picture(avd_hip.Pixels((yy, uv), NV16), 0, True)
    assert (p.format, list(p.row_stride)[:2], list(p.frame_stride)[:2]) == (NV16 | FULL, [w, w], [w * h, w * h])
    # chroma planes of h / 2 rows are not a 4:2:2 picture, and the untagged tuples remain 4:2:0
    with pytest.raises(ValueError, match="chroma planes must be"):
        binding._picture(avd_hip.Pixels((y[:, :32], u[:, :16], v[:, :16]), I422))
    with pytest.raises(ValueError, match="chroma plane must be"):
        binding._picture(avd_hip.Pixels((y[:, :32], uv[:, :16]), NV16))
    assert binding._picture((y[:, :32], u[:, :16], v[:, :16]))[0].format == I420
    assert binding._picture((y[:, :32], uv[:, :16]))[0].format == NV12
    with pytest.raises(ValueError, match="same row and frame strides"):
        binding._picture(avd_hip.Pixels((y, u, np.zeros((n, h, w), np.uint8)[..., :w // 2]), I422))


def test_frame_list_descriptors(binding):
    h, w = 33, 48
    y, u, v = ref.random_planes(3, h, w, 7)
    for fmt in NEW:
        clip = ref.pack(fmt, y, u, v)
        if PLANES[fmt] == 1:
            frames = [np.ascontiguousarray(f) for f in clip]
        else:
            frames = [tuple(np.ascontiguousarray(pl[f]) for pl in clip) for f in range(3)]
        L, n, keep = binding._frame_list(frames, fmt, 0, True)
        assert (L.format, L.n, L.h, L.w, n, L.mem) == (fmt | FULL, 3, h, w, 3, HOST)
        assert list(L.row_stride)[:PLANES[fmt]] == row_bytes(fmt, w)[:PLANES[fmt]]
        for pl in range(PLANES[fmt]):
            tab = ctypes.cast(L.plane[pl], ctypes.POINTER(ctypes.c_void_p * 3)).contents
            assert list(tab) == [(f if PLANES[fmt] == 1 else f[pl]).ctypes.data for f in frames]
        E, n0, _ = binding._frame_list([], fmt)
        assert (n0, E.h, E.w, list(E.row_stride)[:PLANES[fmt]]) == (0, 32, 32, row_bytes(fmt, 32)[:PLANES[fmt]])
    with pytest.raises(ValueError, match=r"plane 1 must be uint8\[33, 24\]"):
        binding._frame_list([(y[0], u[0, :16], v[0, :16])], I422)
    with pytest.raises(ValueError, match="fmt must be"):
        binding._frame_list([y[0]], 0x24)


# ---- a C422 file ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,full_range", [(33, False), (36, True)])
def test_c422_y4m_written_and_read_back(tmp_path, h, full_range):
    n, w = 3, 48
    y, u, v = ref.random_planes(n, h, w, 8)
    path = str(tmp_path / "clip.y4m")
    sources.write_y4m(path, y, ref.pack(NV16, y, u, v)[1], fps=(25, 1), full_range=full_range)
    header = open(path, "rb").readline()
    assert b" C422" in header.split(b" XCOLORRANGE")[0] and (b"XCOLORRANGE=FULL" in header) == full_range
    assert os.path.getsize(path) == len(header) + n * (6 + 2 * w * h)
    for planar in (False, True):                               # a 4:2:2 file yields its own planes either way
        src = sources.open_source(path, planar=planar)
        assert isinstance(src, sources.Y4mSource) and src.surface == "i422"
        assert (src.width, src.height, src.frame_count, src.fps, src.full_range, src.rotate) == (w, h, n, 25.0, full_range, 0)
        got = list(src.sampled(1))
        assert len(got) == n
        for f, (gy, gu, gv) in enumerate(got):
            assert gy.shape == (h, w) and gu.shape == (h, w // 2) == gv.shape
            assert np.array_equal(gy, y[f]) and np.array_equal(gu, u[f]) and np.array_equal(gv, v[f])
            # views of the map, adjacent: what the staging plan merges into one copy
            assert gu.ctypes.data - gy.ctypes.data == h * w and gv.ctypes.data - gu.ctypes.data == h * (w // 2)
        assert [np.array_equal(a[0], y[i]) for i, a in zip((0, 2), src.sampled(2))] == [True, True]
        src.close()


def test_y4m_refusals_stay(tmp_path):
    for name, header in (("deep", b"YUV4MPEG2 W64 H64 F25:1 C422p10\n"), ("oddw", b"YUV4MPEG2 W63 H64 F25:1 C422\n"),
                         ("odd420", b"YUV4MPEG2 W64 H63 F25:1 C420\n"), ("c444", b"YUV4MPEG2 W64 H64 F25:1 C444\n"),
                         ("mono", b"YUV4MPEG2 W64 H64 F25:1 Cmono\n")):
        p = tmp_path / (name + ".y4m")
        p.write_bytes(header)
        assert sources.open_source(str(p)) is None, name
    # a 4:2:0 file is what it was
    y, uv = np.zeros((1, 34, 48), np.uint8), np.zeros((1, 17, 48), np.uint8)
    path = str(tmp_path / "c420.y4m")
    sources.write_y4m(path, y, uv)
    assert b"C420jpeg" in open(path, "rb").readline()
    assert sources.open_source(path).surface == "nv12" and sources.open_source(path, planar=True).surface == "i420"
