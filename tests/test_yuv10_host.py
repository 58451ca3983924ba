"""10-bit 4:2:0 pictures in 16-bit words (AVD_FMT_P010 / _I010), the parts that need no GPU: the two values in header, library-side header and
binding; the definition (tests/yuv10_reference.py) over all 65536 words and tied to the pinned 8-bit converter; the refusals of from_picture /
from_frame_list / check_clip in their documented order, the 2-byte alignment check last; the staging plan of host clips; the table-fill
eligibility of lists; the descriptors the binding builds and the dtypes it refuses.  The host logic runs in a stand-alone program
(tests/ingest_check.cpp, built with the address and undefined-behaviour sanitizers by tests/ingest_host_kit.py, which also
holds the case writers, the answer reader and the texts every layout shares)."""
import ctypes
import os
import re

import numpy as np
import pytest

import avd_hip
from avd_hip import _lib
from tests import yuv10_reference as ref
from tests import yuv_tables_reference as ytr
from tests.ingest_host_kit import (ARG, BASE, DEVICE, FULL, HOST, I420, NV12, OK, PLANES, ROOT, T_GEOM, T_MEM, T_ODD, T_SMALL, UNSUPPORTED,  # noqa: F401
                                   binding, frame_list, list_addrs, parse, picture, program, r256, row_bytes, t_format, t_reserved, t_rotate)

P010, I010 = ref.LAYOUTS
NEW = ref.LAYOUTS
T_SHARE = "the U and V planes of an I010 picture share their strides"
T_EVEN = {P010: "P010 needs even width and height", I010: "I010 needs even width and height"}
T_NULL = {P010: "null P010 plane pointer", I010: "null I010 plane pointer"}
T_STRIDES = {P010: "strides smaller than the P010 planes", I010: "strides smaller than the I010 planes"}
parse_p = parse_l = parse


# ---- the values -----------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree_on_the_two_values(program):
    hdr = open(os.path.join(ROOT, "include", "avd.h")).read()
    for name, value in zip(("AVD_FMT_P010", "AVD_FMT_I010"), (0x30, 0x31)):
        assert int(re.search(r"^#define %s\s+(0x[0-9a-fA-F]+)\s*$" % name, hdr, re.M).group(1), 16) == value
        assert getattr(_lib, name) == value == getattr(avd_hip, name)
        assert _lib.LAYOUT[value].planes == PLANES[value] and _lib.LAYOUT[value].handed == "planes"
    a = parse(program(["A"])[0])
    assert a["picture_size"] == ctypes.sizeof(_lib.AvdPicture) == 104
    assert a["list_size"] == ctypes.sizeof(_lib.AvdFrameList) == 80
    assert (a["AVD_FMT_P010"], a["AVD_FMT_I010"]) == NEW == (0x30, 0x31)
    assert re.search(r"^#define AVD_ABI_VERSION 3\b", hdr, re.M)
    for text in ("20 p010_scalar, 21 p010_tables, 22 i010_scalar", "23 i010_tables, 24 p010_strip, 25 i010_strip", "UNPINNED", "yuv420p10le",
                 "min(255, (s + 128) >> 8)", "min(255, (s + 2) >> 2)", "index the table at 256", "0x24 .. 0x2F and 0x32 .. 0xFF stay AVD_ERR_ARG",
                 "4:4:4 and 10-bit 4:2:2", T_ODD[:40]):
        assert text in hdr, text
    assert _lib._FMT_NAMES.endswith("AVD_FMT_P010 or AVD_FMT_I010")


# ---- the definition -------------------------------------------------------------------------------------------------------------------------
def test_p010_narrowing_over_all_words():
    s = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    got = ref.narrow_p010(s).astype(np.int64)
    v10 = s.astype(np.int64) >> 6
    assert np.array_equal(got, np.minimum(255, (v10 + 2) >> 2))                        # the low six bits never change it ...
    assert np.array_equal(got, ref.narrow_p010(s & np.uint16(0xFFC0)))                 # ... nor does clearing them
    assert set(got.tolist()) == set(range(256))
    assert got[0xFFFF] == 255 and got[0xFF80] == 255 and got[0xFF7F] == 255 and got[0xFE80] == 255 and got[0xFE7F] == 254
    assert got[0] == 0 and got[0x7F] == 0 and got[0x80] == 1


def test_i010_narrowing_over_all_words():
    s = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    got = ref.narrow_i010(s).astype(np.int64)
    assert set(got[:1024].tolist()) == set(range(256))                                 # every value is reached by a 10-bit sample
    assert got[1021] == got[1022] == got[1023] == 255 and got[1020] == 255 and got[1017] == 254
    v = np.arange(4, 1016)
    assert np.array_equal(got[v][v % 4 == 1], v[v % 4 == 1] // 4) and np.array_equal(got[v][v % 4 == 2], v[v % 4 == 2] // 4 + 1)     # down, up
    assert np.array_equal(got[v][v % 4 == 0], v[v % 4 == 0] // 4) and np.array_equal(got[v][v % 4 == 3], v[v % 4 == 3] // 4 + 1)
    assert (got[1024:] == 255).all() and got[0xFFFF] == 255 and got[0xFFFE] == 255     # no 16-bit wrap: 0xFFFE + 2 is not 0
    assert np.all(np.diff(got) >= 0)


def test_packers_and_word_positions():
    y = np.array([[[1, 2], [3, 1023]]], np.uint16)
    u, v = np.array([[[512]]], np.uint16), np.array([[[64]]], np.uint16)
    py, puv = ref.pack(P010, y, u, v)
    assert py.reshape(-1).tolist() == [64, 128, 192, 0xFFC0] and puv.reshape(-1).tolist() == [0x8000, 0x1000]
    assert py.dtype == np.uint16 and py.tobytes()[:2] == b"\x40\x00" or py.dtype.byteorder == ">"      # little-endian words on this host
    for fmt in NEW:
        clip = ref.pack(fmt, y, u, v)
        for a, b in zip(ref.unpack(fmt, clip), (y, u, v)):
            assert np.array_equal(a, b)
    assert ref.narrowed_nv12(P010, (py, puv))[1].reshape(-1).tolist() == [128, 16]
    assert [p.reshape(-1).tolist() for p in ref.narrowed_i420(I010, (y, u, v))] == [[0, 1, 1, 255], [128], [16]]


@pytest.mark.parametrize("full_range", (False, True), ids=("limited", "full"))
def test_enumerated_content_reaches_both_ends_of_the_index_window(full_range):
    h, w = 36, 64
    n = ytr.enum_frames(h, w) + 1
    y10, u10, v10 = ref.enum_planes10(n, h, w, 3)
    y8, uv8 = ytr.enum_planes(n, h, w, 3)
    for fmt in NEW:
        clip = ref.pack(fmt, y10, u10, v10)
        ny, nuv = ref.narrowed_nv12(fmt, clip)
        assert np.array_equal(ny, y8) and np.array_equal(nuv, uv8), ref.NAMES[fmt]         # the narrowed cells enumerate ytr.enum_cells()
        t = ytr.tables(full_range)
        yy = ny.astype(np.int64)
        uu = np.repeat(np.repeat(nuv[..., 0::2], 2, -2), 2, -1)
        vv = np.repeat(np.repeat(nuv[..., 1::2], 2, -2), 2, -1)
        idx = np.stack([yy + t["b_off"][uu], yy + t["gu_off"][uu] + t["gv_off"][vv], yy + t["r_off"][vv]])
        assert (int(idx.min()), int(idx.max())) == ytr.index_window(full_range)
        assert np.array_equal(ref.to_bgr(fmt, clip, full_range), ytr.nv12_to_bgr(y8, uv8, full_range))
    # both rounding directions occur: remainders 0, 1 (down) and 2, 3 (up)
    for p in (y10, u10, v10):
        assert set((p.reshape(-1)[1000:2000] % 4).tolist()) == {0, 1, 2, 3}


def test_reference_equals_the_pinned_converter_on_widened_planes(oracle):
    """to_bgr of 8-bit planes widened exactly (v8 << 2, P010 v8 << 8) is the pinned 8-bit converter's frame"""
    h, w = 36, 64
    n = ytr.enum_frames(h, w) + 1
    y8, uv8 = ytr.enum_planes(n, h, w, 4)
    want = oracle.nv12_to_bgr(y8, uv8)
    u8, v8 = uv8[..., 0::2], uv8[..., 1::2]
    i010 = tuple(p.astype(np.uint16) << 2 for p in (y8, u8, v8))
    assert np.array_equal(ref.to_bgr(I010, i010, False), want)
    p010 = (y8.astype(np.uint16) << 8, uv8.astype(np.uint16) << 8)
    assert np.array_equal(ref.to_bgr(P010, p010, False), want)
    assert np.array_equal(ref.to_bgr(P010, ref.pack(P010, *i010), False), want)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NEW, ids=lambda f: ref.NAMES[f])
def test_accepted_as_described(program, fmt):
    p = parse_p(program([picture(fmt)])[0])
    assert (p["status"], p["why"], p["format"], p["planes"], p["px"], p["full"]) == (OK, "", fmt, PLANES[fmt], 2, 0)
    assert (p["sub_rows"], p["sub_row"]) == (24, row_bytes(fmt, 64)[1])
    for rotate in (1, 2, 3):                                                              # a turn and the range flag are allowed
        p = parse_p(program([picture(fmt | FULL, h=34, w=36, rotate=rotate)])[0])
        assert (p["status"], p["format"], p["full"], p["sub_rows"], p["sub_row"]) == (OK, fmt, 1, 17, row_bytes(fmt, 36)[1])
    l = parse_l(program([frame_list(fmt | FULL, list_addrs(fmt), h=34, w=36, rotate=3)])[0])
    assert (l["status"], l["format"], l["planes"], l["px"], l["full"], l["sub_rows"]) == (OK, fmt, PLANES[fmt], 2, 1, 17)
    assert parse_p(program([picture(fmt, h=16384, w=16384, n=1)])[0])["status"] == OK
    assert parse_p(program([picture(fmt, h=32, w=32)])[0])["status"] == OK
    assert parse_p(program([picture(fmt, n=0, planes=(0, 0, 0))])[0])["status"] == OK


@pytest.mark.parametrize("fmt", NEW, ids=lambda f: ref.NAMES[f])
def test_refusal_table_of_a_picture(program, fmt):
    rb = row_bytes(fmt, 64)
    short0 = [rb[0] - 2, rb[1], rb[2]]
    fs = [rb[0] * 48, rb[1] * 24, rb[2] * 24]
    table = [
        (picture(fmt, rotate=4), ARG, t_rotate("picture")),
        (picture(fmt, reserved=1), ARG, t_reserved("picture")),
        (picture(fmt, mem=2), ARG, T_MEM),
        (picture(fmt, w=16386), ARG, T_GEOM),
        (picture(fmt, h=16386), ARG, T_GEOM),
        (picture(fmt, h=0), ARG, T_GEOM),
        (picture(fmt, n=-1), ARG, T_GEOM),
        (picture(fmt, w=63), UNSUPPORTED, T_EVEN[fmt]),
        (picture(fmt, h=47), UNSUPPORTED, T_EVEN[fmt]),
        (picture(fmt, h=30), UNSUPPORTED, T_SMALL),
        (picture(fmt, w=30), UNSUPPORTED, T_SMALL),
        (picture(fmt, planes=(0,) + BASE[1:]), ARG, T_NULL[fmt]),
        (picture(fmt, planes=(BASE[0], 0, BASE[2])), ARG, T_NULL[fmt]),
        (picture(fmt, rs=short0), ARG, T_STRIDES[fmt]),
        (picture(fmt, rs=[64, rb[1], rb[2]]), ARG, T_STRIDES[fmt]),                       # w bytes a row would do for 8-bit luma, not here
        (picture(fmt, rs=[rb[0], rb[1] - 2, rb[2] - 2]), ARG, T_STRIDES[fmt]),
        (picture(fmt, fs=[fs[0] - 2, fs[1], fs[2]]), ARG, T_STRIDES[fmt]),
        (picture(fmt, fs=[fs[0], fs[1] - 2, fs[2] - 2]), ARG, T_STRIDES[fmt]),
        # the new check, last: an odd plane base, row stride or frame stride
        (picture(fmt, planes=(BASE[0] + 1,) + BASE[1:]), ARG, T_ODD),
        (picture(fmt, planes=(BASE[0], BASE[1] + 1, BASE[2])), ARG, T_ODD),
        (picture(fmt, rs=[rb[0] + 1, rb[1], rb[2]]), ARG, T_ODD),
        (picture(fmt, rs=[rb[0], rb[1] + 1, rb[2] + 1]), ARG, T_ODD),
        (picture(fmt, fs=[fs[0] + 1, fs[1], fs[2]]), ARG, T_ODD),
        (picture(fmt, fs=[fs[0], fs[1] + 1, fs[2] + 1]), ARG, T_ODD),
        (picture(fmt, n=1, fs=[fs[0] + 1, fs[1] + 1, fs[2] + 1]), OK, ""),                # one frame: its frame strides are not looked at
        (picture(fmt, planes=(BASE[0] + 2, BASE[1] + 2, BASE[2] + 2), rs=[rb[0] + 2, rb[1] + 2, rb[2] + 2]), OK, ""),
        # pairs of faults: the documented order
        (picture(fmt, rotate=4, reserved=1, mem=2), ARG, t_rotate("picture")),
        (picture(fmt, reserved=1, mem=2), ARG, t_reserved("picture")),
        (picture(fmt, mem=2, w=16386), ARG, T_MEM),
        (picture(fmt, w=16386, h=31), ARG, T_GEOM),
        (picture(fmt, w=31), UNSUPPORTED, T_EVEN[fmt]),                                   # evenness before the 32 x 32 minimum
        (picture(fmt, h=30, planes=(0, 0, 0)), UNSUPPORTED, T_SMALL),
        (picture(fmt, planes=(0,) + BASE[1:], rs=short0), ARG, T_NULL[fmt]),
        (picture(fmt, planes=(BASE[0] + 1,) + BASE[1:], rs=short0), ARG, T_STRIDES[fmt]),  # short strides before odd ones
        (picture(fmt, planes=(BASE[0] + 1, 0, BASE[2])), ARG, T_NULL[fmt]),
        (picture(fmt, planes=(BASE[0] + 1,) + BASE[1:], w=63), UNSUPPORTED, T_EVEN[fmt]),
        (picture(fmt, rs=[rb[0] - 1, rb[1], rb[2]]), ARG, T_STRIDES[fmt]),                # short AND odd: short
        (picture(fmt | 0x200), ARG, t_format("picture")),
        (picture(fmt | 0x200 | FULL), ARG, t_format("picture")),
    ]
    if fmt == I010:
        table += [
            (picture(fmt, planes=(BASE[0], BASE[1], 0)), ARG, T_NULL[fmt]),
            (picture(fmt, planes=(BASE[0], BASE[1], BASE[2] + 1)), ARG, T_ODD),
            (picture(fmt, rs=[128, 64, 96]), ARG, T_SHARE),
            (picture(fmt, fs=[fs[0], fs[1], fs[2] + 2]), ARG, T_SHARE),
            (picture(fmt, rs=[128, 64, 96], mem=2), ARG, T_SHARE),                        # the descriptor's before check_clip's
            (picture(fmt, rs=[128, 64, 96], w=63), ARG, T_SHARE),
            (picture(fmt, rs=[128, 64, 96], rotate=5), ARG, t_rotate("picture")),
            (picture(fmt, planes=(BASE[0], BASE[2], BASE[1])), OK, ""),                   # V first: the pointers exchanged
        ]
    else:
        table += [(picture(fmt, planes=(BASE[0], BASE[1], 1), rs=[128, 128, 1], fs=[128 * 48, 128 * 24, 3]), OK, "")]     # plane 2 is not looked at
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
    odd = [list(pl) for pl in a]
    odd[-1][1] += 1
    table = [
        (frame_list(fmt, a, rotate=-1), ARG, t_rotate("frame_list")),
        (frame_list(fmt, a, reserved=7), ARG, t_reserved("frame_list")),
        (frame_list(fmt, a, mem=-1), ARG, T_MEM),
        (frame_list(fmt, a, h=16386), ARG, T_GEOM),
        (frame_list(fmt, a, w=34 + 1), UNSUPPORTED, T_EVEN[fmt]),
        (frame_list(fmt, a, h=34 + 1), UNSUPPORTED, T_EVEN[fmt]),
        (frame_list(fmt, a, w=30), UNSUPPORTED, T_SMALL),
        (frame_list(fmt, a, null_arrays=1 << (PLANES[fmt] - 1)), ARG, "null plane array of a frame list"),
        (frame_list(fmt, holed), ARG, "null plane pointer in a frame list"),
        (frame_list(fmt, a, rs=[rb[0] - 2, rb[1], rb[2]]), ARG, T_STRIDES[fmt]),
        (frame_list(fmt, a, rs=[rb[0], rb[1] - 2, rb[2] - 2]), ARG, T_STRIDES[fmt]),
        (frame_list(fmt, odd), ARG, T_ODD),                                               # any entry of any plane
        (frame_list(fmt, a, rs=[rb[0] + 1, rb[1], rb[2]]), ARG, T_ODD),
        (frame_list(fmt, a, rs=[rb[0], rb[1] + 1, rb[2] + 1]), ARG, T_ODD),
        (frame_list(fmt, odd, rs=[rb[0] - 2, rb[1], rb[2]]), ARG, T_STRIDES[fmt]),
        (frame_list(fmt, holed, rs=[rb[0] + 1, rb[1], rb[2]]), ARG, "null plane pointer in a frame list"),
        (frame_list(fmt, a, rotate=3, reserved=1), ARG, t_reserved("frame_list")),
        (frame_list(fmt, a, rotate=3), OK, ""),
        (frame_list(fmt | 0x200, a), ARG, t_format("frame_list")),
    ]
    if fmt == I010:
        table += [(frame_list(fmt, a, rs=[128, 64, 96]), ARG, T_SHARE), (frame_list(fmt, a, rs=[128, 62, 62]), ARG, T_STRIDES[fmt])]
    got = program([t[0] for t in table])
    for (line, status, why), g in zip(table, got):
        l = parse_l(g)
        assert (l["status"], l["why"]) == (status, why), (line, g)


def test_neighbouring_layout_values_stay_refused(program):
    for layout in (0x24, 0x2F, 0x32, 0x3F, 0xFF):
        for fmt in (layout, layout | FULL):
            p = parse_p(program([picture(fmt)])[0])
            assert (p["status"], p["why"]) == (ARG, t_format("picture")), hex(fmt)
            l = parse_l(program([frame_list(fmt, [[BASE[0]], [BASE[1]], [BASE[2]]])])[0])
            assert (l["status"], l["why"]) == (ARG, t_format("frame_list")), hex(fmt)


# ---- staging --------------------------------------------------------------------------------------------------------------------------------
def test_p010_is_two_spans(program):
    n, h, w = 2, 34, 48
    ys, cs = n * h * w * 2, n * (h // 2) * w * 2
    p = parse_p(program([picture(P010, n=n, h=h, w=w)])[0])
    assert (p["status"], p["nspans"], p["bytes"], p["off"], p["plane_off"]) == (OK, 2, [ys, cs], [0, r256(ys)], [0, r256(ys)])
    assert p["copied"] == ys + cs == 3 * n * h * w and p["total"] == r256(ys) + r256(cs)
    rs = 2 * w + 32
    p = parse_p(program([picture(P010, n=n, h=h, w=w, rs=[rs] * 3, fs=[rs * h + 64, rs * h // 2 + 64, 0])])[0])
    assert p["bytes"] == [(rs * h + 64) + rs * (h - 1) + 2 * w, (rs * h // 2 + 64) + rs * (h // 2 - 1) + 2 * w]
    p = parse_p(program([picture(P010, mem=DEVICE, n=n, h=h, w=w)])[0])
    assert (p["status"], p["nspans"], p["total"]) == (OK, 0, 0)


def test_a_dense_i010_frame_stack_is_one_span_and_separate_planes_three(program):
    """what libavcodec's yuv420p10le frames look like in one buffer: Y, U, V of a frame adjacent, frame after frame"""
    n, h, w = 3, 34, 48
    yb, cb = 2 * h * w, 2 * (h // 2) * (w // 2)
    fs = yb + 2 * cb
    assert fs == 3 * h * w
    planes = (BASE[0], BASE[0] + yb, BASE[0] + yb + cb)
    p = parse_p(program([picture(I010, n=n, h=h, w=w, planes=planes, fs=[fs] * 3)])[0])
    assert (p["status"], p["nspans"], p["bytes"], p["off"], p["plane_off"]) == (OK, 1, [n * fs], [0], [0, yb, yb + cb])
    assert p["copied"] == 3 * n * h * w
    # V first: the pointers exchanged, the same span
    p = parse_p(program([picture(I010, n=1, h=h, w=w, planes=(BASE[0], BASE[0] + yb + cb, BASE[0] + yb))])[0])
    assert (p["nspans"], p["bytes"], p["plane_off"]) == (1, [fs], [0, yb + cb, yb])
    ys, cs = n * yb, n * cb
    p = parse_p(program([picture(I010, n=n, h=h, w=w)])[0])
    assert (p["status"], p["nspans"], p["bytes"]) == (OK, 3, [ys, cs, cs])
    assert p["off"] == [0, r256(ys), r256(ys) + r256(cs)] == p["plane_off"] and p["copied"] == 3 * n * h * w


def test_a_frame_listed_twice_is_copied_once(program):
    h, w = 34, 48
    for fmt in NEW:
        a = list_addrs(fmt, 2)
        twice = [[pl[0], pl[1], pl[0]] for pl in a]
        l = parse_l(program([frame_list(fmt, twice, h=h, w=w)])[0])
        assert l["status"] == OK and l["nspans"] == 2 * PLANES[fmt] and l["copied"] == 2 * 3 * h * w, ref.NAMES[fmt]
        for p in range(PLANES[fmt]):
            assert l["plane_off"][p * 3] == l["plane_off"][p * 3 + 2]
    # I010 frames that are views of one dense stack: one span, as the strided clip
    yb, cb = 2 * h * w, 2 * (h // 2) * (w // 2)
    views = [[BASE[0] + f * 3 * h * w + o for f in range(3)] for o in (0, yb, yb + cb)]
    l = parse_l(program([frame_list(I010, views, h=h, w=w)])[0])
    assert (l["nspans"], l["bytes"], l["copied"]) == (1, [9 * h * w], 9 * h * w)


# ---- table-fill eligibility of a list -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NEW, ids=lambda f: ref.NAMES[f])
def test_list_vec_eligible(program, fmt):
    a = list_addrs(fmt, 3)
    rb = row_bytes(fmt, 64)
    assert parse_l(program([frame_list(fmt, a, mem=DEVICE)])[0])["given"] == 1
    for plane in range(PLANES[fmt]):
        for delta, want in ((2, 0), (4, 0), (8, 0), (16, 1)):                             # every plane is read 16 bytes at a time, I010's chroma too
            off = [list(pl) for pl in a]
            off[plane][1] += delta
            assert parse_l(program([frame_list(fmt, off, mem=DEVICE)])[0])["given"] == want, (plane, delta)
    assert parse_l(program([frame_list(fmt, a, mem=DEVICE, w=72)])[0])["given"] == 0
    for delta, want in ((2, 0), (8, 0), (16, 1)):
        assert parse_l(program([frame_list(fmt, a, mem=DEVICE, rs=[rb[0] + delta, rb[1], rb[2]])])[0])["given"] == want
        assert parse_l(program([frame_list(fmt, a, mem=DEVICE, rs=[rb[0], rb[1] + delta, rb[2] + delta])])[0])["given"] == want
    # a contiguous I010 frame: its V plane lies at 5wh/2 bytes, a multiple of 16
    if fmt == I010:
        h, w = 34, 48
        views = [[BASE[0] + f * 3 * h * w + o for f in range(2)] for o in (0, 2 * h * w, 5 * h * w // 2)]
        assert parse_l(program([frame_list(fmt, views, mem=DEVICE, h=h, w=w)])[0])["given"] == 1
    # host frames are judged where they are staged: separately allocated ones land on 256-byte boundaries
    off = [[v + 6 for v in pl] for pl in a]
    l = parse_l(program([frame_list(fmt, off)])[0])
    assert (l["given"], l["staged"]) == (0, 1)


# ---- the binding's descriptors ----------------------------------------------------------------------------------------------------------------
def _clips(n, h, w, seed):
    y, u, v = ref.random_planes10(n, h, w, seed)
    return {fmt: ref.pack(fmt, y, u, v) for fmt in NEW}


def test_pixels_takes_the_two_layouts_and_refuses_other_dtypes():
    clips = _clips(2, 34, 48, 5)
    for fmt in NEW:
        assert avd_hip.Pixels(clips[fmt], fmt).fmt == fmt
    y, u, v = clips[I010]
    with pytest.raises(ValueError, match="tuple of 3 planes"):
        avd_hip.Pixels((y, u), I010)
    with pytest.raises(ValueError, match="tuple of 2 planes"):
        avd_hip.Pixels((y, u, v), P010)
    for bad in (np.uint8, np.int16, np.int32, np.float32):                 # numpy int16 is not taken: only torch lacks an unsigned view
        with pytest.raises(ValueError, match="are uint16"):
            avd_hip.Pixels((y, u, v.astype(bad)), I010)
        with pytest.raises(ValueError, match="are uint16"):
            avd_hip.Pixels((clips[P010][0].astype(bad), clips[P010][1]), P010)
    for bad in (NV12, I420, 0x24, 0x2F, 0x32, 0xFF):
        with pytest.raises(ValueError, match="fmt must be"):
            avd_hip.Pixels(y, bad)


def test_pixels_descriptors(binding):
    n, h, w = 2, 34, 48
    clips = _clips(n, h, w, 6)
    y, uv = clips[P010]
    p, cnt, _ = binding._picture(avd_hip.Pixels((y, uv), P010), 1, True)
    assert (p.format, p.n, p.h, p.w, p.rotate, cnt) == (P010 | FULL, n, h, w, 1, n)
    assert [p.plane[i] for i in range(2)] == [y.ctypes.data, uv.ctypes.data]
    assert list(p.row_stride)[:2] == [2 * w, 2 * w] and list(p.frame_stride)[:2] == [2 * w * h, 2 * w * (h // 2)]          # bytes
    y, u, v = clips[I010]
    p, cnt, _ = binding._picture(avd_hip.Pixels((y, u, v), I010), 3)
    assert (p.format, p.h, p.w, p.rotate, cnt) == (I010, h, w, 3, n)
    assert [p.plane[i] for i in range(3)] == [y.ctypes.data, u.ctypes.data, v.ctypes.data]
    assert list(p.row_stride) == [2 * w, w, w] and list(p.frame_stride) == [2 * w * h, w * (h // 2), w * (h // 2)]
    # a row-padded view goes through as it lies, in bytes
    padded = np.zeros((n, h, w + 8), np.uint16)[:, :, :w]
    p, _, keep = binding._picture(avd_hip.Pixels((padded, u, v), I010))
    assert keep[0] is padded and p.row_stride[0] == 2 * (w + 8)
    with pytest.raises(ValueError, match=r"chroma planes must be uint16\[2,17,24\]"):
        binding._picture(avd_hip.Pixels((y, u[:, :, :16], v[:, :, :16]), I010))
    with pytest.raises(ValueError, match=r"chroma plane must be uint16\[2,17,48\]"):
        binding._picture(avd_hip.Pixels((y, clips[P010][1][:, :, :24]), P010))
    with pytest.raises(ValueError, match="same row and frame strides"):
        binding._picture(avd_hip.Pixels((y, u, np.zeros((n, h // 2, w), np.uint16)[..., :w // 2]), I010))
    # the untagged tuples remain NV12 / I420: uint16 planes are not theirs
    with pytest.raises(ValueError, match="planes must be uint8"):
        binding._picture((y, u, v))
    y8 = np.zeros((n, h, w), np.uint8)
    assert binding._picture((y8, np.zeros((n, h // 2, w), np.uint8)))[0].format == NV12
    assert binding._picture((y8, np.zeros((n, h // 2, w // 2), np.uint8), np.zeros((n, h // 2, w // 2), np.uint8)))[0].format == I420


def test_torch_planes_uint16_and_int16_are_the_same_bits(binding):
    torch = pytest.importorskip("torch")
    n, h, w = 2, 34, 48
    y, u, v = _clips(n, h, w, 7)[I010]
    ty, tu, tv = (torch.from_numpy(p.view(np.int16)) for p in (y, u, v))
    p, cnt, _ = binding._picture(avd_hip.Pixels((ty, tu, tv), I010))
    assert (p.format, cnt, p.mem) == (I010, n, HOST)
    assert [p.plane[i] for i in range(3)] == [y.ctypes.data, u.ctypes.data, v.ctypes.data]
    assert list(p.row_stride) == [2 * w, w, w] and list(p.frame_stride) == [2 * w * h, w * (h // 2), w * (h // 2)]
    if hasattr(torch, "uint16"):
        p, _, _ = binding._picture(avd_hip.Pixels(tuple(t.view(torch.uint16) for t in (ty, tu, tv)), I010))
        assert list(p.row_stride) == [2 * w, w, w] and p.plane[0] == y.ctypes.data
    with pytest.raises(ValueError, match="are uint16"):
        avd_hip.Pixels((ty, tu, tv.to(torch.uint8)), I010)
    L, cnt, _ = binding._frame_list([(ty[f], tu[f], tv[f]) for f in range(n)], I010)
    assert (L.format, cnt, list(L.row_stride)) == (I010, n, [2 * w, w, w])


def test_frame_list_descriptors(binding):
    h, w = 34, 48
    clips = _clips(3, h, w, 8)
    for fmt in NEW:
        frames = [tuple(np.ascontiguousarray(pl[f]) for pl in clips[fmt]) for f in range(3)]
        L, n, keep = binding._frame_list(frames, fmt, 1, True)
        assert (L.format, L.n, L.h, L.w, L.rotate, n, L.mem) == (fmt | FULL, 3, h, w, 1, 3, HOST)
        assert list(L.row_stride)[:PLANES[fmt]] == row_bytes(fmt, w)[:PLANES[fmt]]
        for pl in range(PLANES[fmt]):
            tab = ctypes.cast(L.plane[pl], ctypes.POINTER(ctypes.c_void_p * 3)).contents
            assert list(tab) == [f[pl].ctypes.data for f in frames]
        E, n0, _ = binding._frame_list([], fmt)
        assert (n0, E.h, E.w, list(E.row_stride)[:PLANES[fmt]]) == (0, 32, 32, row_bytes(fmt, 32)[:PLANES[fmt]])
        with pytest.raises(ValueError, match="are uint16 arrays"):
            binding._frame_list([tuple(p.astype(np.uint8) for p in frames[0])], fmt)
    y, u, v = clips[I010]
    with pytest.raises(ValueError, match=r"plane 1 must be uint16\[17, 24\]"):
        binding._frame_list([(y[0], u[0, :, :16], v[0, :, :16])], I010)
    with pytest.raises(ValueError, match="fmt must be"):
        binding._frame_list([y[0]], 0x32)
