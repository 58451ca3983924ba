"""RGB producers' layouts (AVD_FMT_RGB24 / _BGRA32 / _RGBA32 / _RGBP), the parts that need no GPU: the four values in header, library-side
header and binding; the refusals of from_picture / from_frame_list / check_clip in their documented order; the staging plan of host clips
(a dense [N,3,H,W] stack is ONE span, separately allocated planes three, a 32-bit clip one span of 4w-byte rows, a frame listed twice crosses
once); the vector-fill eligibility of lists; and the descriptors the binding builds from Pixels and per-frame arrays.  The host logic runs in a
stand-alone program (tests/ingest_check.cpp, built with the address and undefined-behaviour sanitizers by tests/ingest_host_kit.py, which also
holds the case writers, the answer reader and the texts every layout shares)."""
import ctypes
import os
import re

import numpy as np
import pytest

import avd_hip
from avd_hip import _lib
from tests.ingest_host_kit import (ARG, BASE, BGR, DEVICE, FULL, HOST, I420, NV12, OK, PLANES, PX, ROOT, T_GEOM, T_MEM, T_SMALL, UNSUPPORTED,  # noqa: F401
                                   binding, frame_list, list_addrs, parse, picture, program, t_format, t_reserved, t_rotate)

RGB24, BGRA32, RGBA32, RGBP = NEW = (0x10, 0x11, 0x12, 0x13)
T_RANGE = "AVD_FMT_FULL_RANGE describes 4:2:0 samples: an RGB picture has no range"
T_TURNED = "a turned RGB picture is not on the path: producers of RGB hand it over already rotated"
T_SHARE = "the R, G and B planes of an RGBP picture share their strides"
parse_p = parse_l = parse


def t_null(fmt, kind):
    if kind == "frame_list":
        return "null plane pointer in a frame list"
    return "null RGBP plane pointer" if fmt == RGBP else "null frame pointer"


def t_strides(fmt):
    return "strides smaller than the RGBP planes" if fmt == RGBP else "strides smaller than the frame"


# ---- the values -----------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree_on_the_four_values(program):
    hdr = open(os.path.join(ROOT, "include", "avd.h")).read()
    names = ("AVD_FMT_RGB24", "AVD_FMT_BGRA32", "AVD_FMT_RGBA32", "AVD_FMT_RGBP")
    for name, value in zip(names, NEW):
        assert int(re.search(r"^#define %s\s+(0x[0-9a-fA-F]+)\s*$" % name, hdr, re.M).group(1), 16) == value
        assert getattr(_lib, name) == value == getattr(avd_hip, name)
    # the enum of the first three layouts stays as it was
    assert "enum avd_format { AVD_FMT_BGR24 = 0, AVD_FMT_NV12 = 1, AVD_FMT_I420 = 2 };" in hdr
    a = parse(program(["A"])[0])
    assert a["picture_size"] == ctypes.sizeof(_lib.AvdPicture) == 104
    assert a["list_size"] == ctypes.sizeof(_lib.AvdFrameList) == 80
    assert tuple(a[name] for name in names) == NEW
    for text in ("ARGB and ABGR", "gbrp", '"ingest_format" int32[1]', "9 px32_scalar, 10 px32_vec16, 11 rgbp_scalar, 12 rgbp_vec16, 13 rgbp_staged"):
        assert text in hdr, text


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NEW)
def test_accepted_as_described(program, fmt):
    p = parse_p(program([picture(fmt)])[0])
    assert (p["status"], p["why"], p["format"], p["planes"], p["px"]) == (OK, "", fmt, PLANES[fmt], PX[fmt])
    # no evenness rule: an odd picture is fine in every layout
    p = parse_p(program([picture(fmt, h=33, w=35)])[0])
    assert (p["status"], p["format"]) == (OK, fmt)
    l = parse_l(program([frame_list(fmt, list_addrs(fmt), h=33, w=35)])[0])
    assert (l["status"], l["format"], l["planes"], l["px"]) == (OK, fmt, PLANES[fmt], PX[fmt])
    # n = 0 asks for no planes
    assert parse_p(program([picture(fmt, n=0, planes=(0, 0, 0))])[0])["status"] == OK


@pytest.mark.parametrize("fmt", NEW)
def test_refusal_table_of_a_picture(program, fmt):
    px = PX[fmt]
    row = 64 * px
    table = [
        (picture(fmt | FULL), ARG, T_RANGE),
        (picture(fmt, rotate=4), ARG, t_rotate("picture")),
        (picture(fmt, reserved=1), ARG, t_reserved("picture")),
        (picture(fmt, rotate=1), UNSUPPORTED, T_TURNED),
        (picture(fmt, rotate=2), UNSUPPORTED, T_TURNED),
        (picture(fmt, mem=2), ARG, T_MEM),
        (picture(fmt, w=16385), ARG, T_GEOM),
        (picture(fmt, h=0), ARG, T_GEOM),
        (picture(fmt, n=-1), ARG, T_GEOM),
        (picture(fmt, h=31), UNSUPPORTED, T_SMALL),
        (picture(fmt, w=31), UNSUPPORTED, T_SMALL),
        (picture(fmt, planes=(0,) + BASE[1:]), ARG, t_null(fmt, "picture")),
        (picture(fmt, rs=[row - 1] * 3), ARG, t_strides(fmt)),
        (picture(fmt, fs=[row * 47 + row - 1] * 3), ARG, t_strides(fmt)),
        # pairs of faults: the documented order
        (picture(fmt | FULL, rotate=4, reserved=1, mem=2), ARG, T_RANGE),
        (picture(fmt | FULL, rotate=1), ARG, T_RANGE),                        # not "a turned RGB picture"
        (picture(fmt, rotate=4, reserved=1), ARG, t_rotate("picture")),
        (picture(fmt, rotate=1, reserved=1), ARG, t_reserved("picture")),
        (picture(fmt, rotate=1, mem=2), UNSUPPORTED, T_TURNED),
        (picture(fmt, mem=2, w=16385), ARG, T_MEM),
        (picture(fmt, w=16385, h=31), ARG, T_GEOM),
        (picture(fmt, h=31, planes=(0, 0, 0)), UNSUPPORTED, T_SMALL),
        (picture(fmt, planes=(0,) + BASE[1:], rs=[row - 1] * 3), ARG, t_null(fmt, "picture")),
    ]
    if fmt == RGBP:
        table += [
            (picture(fmt, planes=(BASE[0], 0, BASE[2])), ARG, t_null(fmt, "picture")),
            (picture(fmt, planes=(BASE[0], BASE[1], 0)), ARG, t_null(fmt, "picture")),
            (picture(fmt, rs=[64, 80, 64]), ARG, T_SHARE),
            (picture(fmt, rs=[64, 64, 80]), ARG, T_SHARE),
            (picture(fmt, rs=[80, 64, 64]), ARG, T_SHARE),
            (picture(fmt, fs=[64 * 48, 64 * 48, 64 * 49]), ARG, T_SHARE),
            (picture(fmt, fs=[64 * 49, 64 * 48, 64 * 48]), ARG, T_SHARE),
            (picture(fmt, rotate=1, rs=[64, 80, 64]), UNSUPPORTED, T_TURNED),   # the turn before the strides, as BGR's before I420's
            (picture(fmt, rs=[64, 80, 64], mem=2), ARG, T_SHARE),               # the descriptor's before check_clip's
        ]
    else:
        # one plane: what planes 1 and 2 say is not looked at
        table += [(picture(fmt, planes=(BASE[0], 0, 0), rs=[row, 1, 2], fs=[row * 48, 3, 4]), OK, "")]
    got = program([t[0] for t in table])
    for (line, status, why), g in zip(table, got):
        p = parse_p(g)
        assert (p["status"], p["why"]) == (status, why), (line, g)


@pytest.mark.parametrize("fmt", NEW)
def test_refusal_table_of_a_frame_list(program, fmt):
    a = list_addrs(fmt)
    row = 64 * PX[fmt]
    holed = [list(pl) for pl in a]
    holed[-1][1] = 0
    table = [
        (frame_list(fmt | FULL, a), ARG, T_RANGE),
        (frame_list(fmt, a, rotate=-1), ARG, t_rotate("frame_list")),
        (frame_list(fmt, a, reserved=7), ARG, t_reserved("frame_list")),
        (frame_list(fmt, a, rotate=3), UNSUPPORTED, T_TURNED),
        (frame_list(fmt, a, mem=-1), ARG, T_MEM),
        (frame_list(fmt, a, h=16385), ARG, T_GEOM),
        (frame_list(fmt, a, w=31), UNSUPPORTED, T_SMALL),
        (frame_list(fmt, a, null_arrays=1 << (PLANES[fmt] - 1)), ARG, "null plane array of a frame list"),
        (frame_list(fmt, holed), ARG, t_null(fmt, "frame_list")),
        (frame_list(fmt, a, rs=[row - 1] * 3), ARG, t_strides(fmt)),
        (frame_list(fmt | FULL, a, rotate=3, reserved=1), ARG, T_RANGE),
        (frame_list(fmt, a, rotate=3, reserved=1), ARG, t_reserved("frame_list")),
        (frame_list(fmt, a, rotate=3, mem=5), UNSUPPORTED, T_TURNED),
        (frame_list(fmt, holed, rs=[row - 1] * 3), ARG, t_null(fmt, "frame_list")),
    ]
    if fmt == RGBP:
        table += [(frame_list(fmt, a, rs=[64, 64, 96]), ARG, T_SHARE), (frame_list(fmt, a, rs=[96, 64, 64]), ARG, T_SHARE),
                  (frame_list(fmt, a, rs=[64, 96, 64], rotate=1), UNSUPPORTED, T_TURNED)]
    got = program([t[0] for t in table])
    for (line, status, why), g in zip(table, got):
        l = parse_l(g)
        assert (l["status"], l["why"]) == (status, why), (line, g)


def test_neighbouring_layout_values_stay_refused(program):
    for layout in (3, 7, 0x0F, 0x14, 0xFF):
        for fmt in (layout, layout | FULL):
            p = parse_p(program([picture(fmt)])[0])
            assert (p["status"], p["why"]) == (ARG, t_format("picture")), hex(fmt)
            l = parse_l(program([frame_list(fmt, [[BASE[0]], [BASE[1]], [BASE[2]]])])[0])
            assert (l["status"], l["why"]) == (ARG, t_format("frame_list")), hex(fmt)
    for fmt in NEW:                                             # bits above the flag
        assert parse_p(program([picture(fmt | 0x200)])[0])["why"] == t_format("picture")


# ---- staging --------------------------------------------------------------------------------------------------------------------------------
def test_a_dense_channels_first_stack_is_one_span(program):
    n, h, w = 3, 40, 48
    hw = h * w
    p = parse_p(program([picture(RGBP, n=n, h=h, w=w, planes=(BASE[0], BASE[0] + hw, BASE[0] + 2 * hw), rs=[w] * 3, fs=[3 * hw] * 3)])[0])
    assert p["status"] == OK and p["nspans"] == 1
    assert p["bytes"] == [n * 3 * hw] and p["off"] == [0] and p["plane_off"] == [0, hw, 2 * hw]
    assert p["copied"] == n * 3 * hw and p["total"] == (n * 3 * hw + 255) // 256 * 256
    # one frame: the three planes touch and merge just the same
    p = parse_p(program([picture(RGBP, n=1, h=h, w=w, planes=(BASE[0], BASE[0] + hw, BASE[0] + 2 * hw), rs=[w] * 3, fs=[3 * hw] * 3)])[0])
    assert (p["nspans"], p["bytes"], p["plane_off"]) == (1, [3 * hw], [0, hw, 2 * hw])
    # a gbrp buffer (G, B, R stored in that order) handed over with permuted pointers: still one span, the planes at their own offsets
    p = parse_p(program([picture(RGBP, n=1, h=h, w=w, planes=(BASE[0] + 2 * hw, BASE[0], BASE[0] + hw), rs=[w] * 3, fs=[3 * hw] * 3)])[0])
    assert (p["nspans"], p["bytes"], p["plane_off"]) == (1, [3 * hw], [2 * hw, 0, hw])


def test_separate_planes_are_three_spans_on_256_byte_boundaries(program):
    n, h, w = 2, 33, 35
    span = w * h * (n - 1) + w * (h - 1) + w
    for planes in (BASE, BASE[::-1]):                           # R,G,B ascending, and in B,G,R address order
        p = parse_p(program([picture(RGBP, n=n, h=h, w=w, planes=planes)])[0])
        assert p["status"] == OK and p["nspans"] == 3 and p["bytes"] == [span] * 3
        assert all(o % 256 == 0 for o in p["off"]) and p["off"] == [0, (span + 255) // 256 * 256, 2 * ((span + 255) // 256 * 256)]
        assert p["copied"] == 3 * span
        # every plane at the start of its own span; the spans are laid out in address order
        order = sorted(range(3), key=lambda i: planes[i])
        assert [p["plane_off"][i] for i in order] == p["off"]


@pytest.mark.parametrize("fmt", (RGB24, BGRA32, RGBA32))
def test_a_packed_clip_is_one_span(program, fmt):
    n, h, w, px = 2, 40, 48, PX[fmt]
    p = parse_p(program([picture(fmt, n=n, h=h, w=w)])[0])
    assert (p["nspans"], p["off"], p["bytes"], p["plane_off"]) == (1, [0], [n * h * w * px], [0])
    # row padding: the span ends with the last ROW's px * w bytes, not with its stride
    rs = w * px + 32
    p = parse_p(program([picture(fmt, n=n, h=h, w=w, rs=[rs] * 3, fs=[rs * h + 64] * 3)])[0])
    assert p["bytes"] == [(rs * h + 64) * (n - 1) + rs * (h - 1) + w * px]
    # a device clip is used in place
    p = parse_p(program([picture(fmt, mem=DEVICE, n=n, h=h, w=w)])[0])
    assert (p["status"], p["nspans"], p["total"]) == (OK, 0, 0)


def test_a_frame_listed_twice_is_copied_once(program):
    h, w = 40, 48
    hw = h * w
    for fmt in NEW:
        a = list_addrs(fmt, 2)
        twice = [[pl[0], pl[1], pl[0]] for pl in a]
        l = parse_l(program([frame_list(fmt, twice, h=h, w=w)])[0])
        plane = hw * PX[fmt]
        assert l["status"] == OK and l["nspans"] == 2 * PLANES[fmt] and l["copied"] == 2 * PLANES[fmt] * plane, fmt
        n = 3
        for p in range(PLANES[fmt]):
            assert l["plane_off"][p * n] == l["plane_off"][p * n + 2]
    # [3,H,W] frames that are views of one dense [N,3,H,W] stack: one span, as the strided clip
    base = BASE[0]
    views = [[base + f * 3 * hw + c * hw for f in range(3)] for c in range(3)]
    l = parse_l(program([frame_list(RGBP, views, h=h, w=w)])[0])
    assert (l["nspans"], l["bytes"], l["copied"]) == (1, [9 * hw], 9 * hw)
    assert l["plane_off"] == [f * 3 * hw + c * hw for c in range(3) for f in range(3)]


# ---- vector-fill eligibility of a list ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NEW)
def test_list_vec_eligible(program, fmt):
    a = list_addrs(fmt, 3)
    assert parse_l(program([frame_list(fmt, a, mem=DEVICE)])[0])["given"] == 1
    # the last plane of ONE frame 8 bytes off (RGBP: a misaligned G plane too) turns the whole list scalar
    for plane in ({RGBP: (1, 2)}.get(fmt, (0,))):
        off = [list(pl) for pl in a]
        off[plane][1] += 8
        assert parse_l(program([frame_list(fmt, off, mem=DEVICE)])[0])["given"] == 0, plane
    # a 32-bit base off by 4 bytes
    off = [list(pl) for pl in a]
    off[0][2] += 4
    assert parse_l(program([frame_list(fmt, off, mem=DEVICE)])[0])["given"] == 0
    # the width and the row stride
    assert parse_l(program([frame_list(fmt, a, mem=DEVICE, w=72)])[0])["given"] == 0
    assert parse_l(program([frame_list(fmt, a, mem=DEVICE, rs=[64 * PX[fmt] + 8] * 3)])[0])["given"] == 0
    assert parse_l(program([frame_list(fmt, a, mem=DEVICE, rs=[64 * PX[fmt] + 16] * 3)])[0])["given"] == 1
    # host frames are judged where they are staged: separately allocated ones land on 256-byte boundaries
    off = [[v + 3 for v in pl] for pl in a]
    l = parse_l(program([frame_list(fmt, off)])[0])
    assert (l["given"], l["staged"]) == (0, 1)


# ---- the binding's descriptors ----------------------------------------------------------------------------------------------------------------
def test_pixels_is_exported_and_tagged():
    assert avd_hip.Pixels is _lib.Pixels
    a = np.zeros((1, 32, 32, 3), np.uint8)
    assert avd_hip.Pixels(a, RGB24).fmt == RGB24 and avd_hip.Pixels(a, RGB24).data is a
    for bad in (NV12, I420, 3, 0x14, None):
        with pytest.raises(ValueError, match="fmt must be"):
            avd_hip.Pixels(a, bad)


def test_pixels_descriptor_of_packed_layouts(binding):
    for fmt, ch in ((RGB24, 3), (BGRA32, 4), (RGBA32, 4)):
        a = np.zeros((2, 40, 48, ch), np.uint8)
        p, n, keep = binding._picture(_lib.Pixels(a, fmt))
        assert keep is a and n == 2
        assert (p.struct_size, p.format, p.mem, p.n, p.h, p.w, p.rotate, p.reserved) == (104, fmt, HOST, 2, 40, 48, 0, 0)
        assert p.plane[0] == a.ctypes.data and not p.plane[1] and not p.plane[2]
        assert (p.row_stride[0], p.frame_stride[0]) == (48 * ch, 40 * 48 * ch)
        # a view with padded rows and frames goes through as it lies
        big = np.zeros((3, 44, 52, ch), np.uint8)
        v = big[1:, 2:42, 1:49]
        p, n, keep = binding._picture(_lib.Pixels(v, fmt))
        assert keep is v and p.plane[0] == v.ctypes.data and (p.row_stride[0], p.frame_stride[0]) == (52 * ch, 44 * 52 * ch)
        # pixels that are not dense are copied once
        p, n, keep = binding._picture(_lib.Pixels(big[:, :, ::2], fmt))
        assert keep.flags.c_contiguous and p.w == 26 and p.row_stride[0] == 26 * ch and p.plane[0] == keep.ctypes.data
        with pytest.raises(ValueError, match=r"uint8\[N,H,W,%d\]" % ch):
            binding._picture(_lib.Pixels(np.zeros((2, 40, 48, 7 - ch), np.uint8), fmt))
        with pytest.raises(ValueError, match="uint8"):
            binding._picture(_lib.Pixels(a.astype(np.int8), fmt))
    # a tagged BGR stack is the untagged one
    a = np.zeros((2, 40, 48, 3), np.uint8)
    assert binding._picture(_lib.Pixels(a, BGR))[0].format == BGR == binding._picture(a)[0].format


def test_pixels_descriptor_of_channels_first_stacks(binding):
    a = np.zeros((2, 3, 40, 48), np.uint8)
    hw = 40 * 48
    p, n, keep = binding._picture(_lib.Pixels(a, RGBP))
    assert keep is a and (p.format, p.n, p.h, p.w) == (RGBP, 2, 40, 48)
    assert [p.plane[c] for c in range(3)] == [a.ctypes.data + c * hw for c in range(3)]
    assert list(p.row_stride) == [48] * 3 and list(p.frame_stride) == [3 * hw] * 3
    # gbrp order by a channel index of negative stride or a permuted view: still no copy, the pointers move
    bgr_planes = a[:, ::-1]
    p, n, keep = binding._picture(_lib.Pixels(bgr_planes, RGBP))
    assert keep is bgr_planes and [p.plane[c] for c in range(3)] == [a.ctypes.data + (2 - c) * hw for c in range(3)]
    # a crop: padded rows, the planes still share their strides
    v = a[:, :, 4:38, 8:44]
    p, n, keep = binding._picture(_lib.Pixels(v, RGBP))
    assert keep is v and (p.h, p.w) == (34, 36) and list(p.row_stride) == [48] * 3 and p.plane[1] - p.plane[0] == hw
    # an interleaved array seen channels first has no dense rows: one copy
    hwc = np.zeros((2, 40, 48, 3), np.uint8)
    p, n, keep = binding._picture(_lib.Pixels(hwc.transpose(0, 3, 1, 2), RGBP))
    assert keep.flags.c_contiguous and keep.shape == (2, 3, 40, 48) and list(p.row_stride) == [48] * 3
    with pytest.raises(ValueError, match=r"uint8\[N,3,H,W\]"):
        binding._picture(_lib.Pixels(hwc, RGBP))
    with pytest.raises(ValueError, match="rotate must be"):
        binding._picture(_lib.Pixels(a, RGBP), 4)
    # the flag is passed on for the library to refuse
    assert binding._picture(_lib.Pixels(a, RGBP), 0, True)[0].format == RGBP | FULL


def test_frame_list_descriptor(binding):
    for fmt, shape in ((RGB24, (40, 48, 3)), (BGRA32, (40, 48, 4)), (RGBA32, (40, 48, 4))):
        frames = [np.zeros(shape, np.uint8) for _ in range(3)]
        L, n, keep = binding._frame_list(frames, fmt)
        assert (L.struct_size, L.format, L.mem, L.n, L.h, L.w) == (80, fmt, HOST, 3, 40, 48) and n == 3
        assert L.row_stride[0] == 48 * shape[2] and not L.plane[1] and not L.plane[2]
        tab = ctypes.cast(L.plane[0], ctypes.POINTER(ctypes.c_void_p * 3)).contents
        assert list(tab) == [f.ctypes.data for f in frames]
        with pytest.raises(ValueError, match="plane 0 must be"):
            binding._frame_list(frames[:2] + [np.zeros((40, 48, 7 - shape[2]), np.uint8)], fmt)
        with pytest.raises(ValueError, match="not dense"):
            binding._frame_list([np.zeros((40, 96, shape[2]), np.uint8)[:, ::2]], fmt)
        with pytest.raises(ValueError, match="share their row strides"):
            binding._frame_list([frames[0], np.zeros((40, 50, shape[2]), np.uint8)[:, :48]], fmt)
        L, n, keep = binding._frame_list([], fmt)
        assert (L.n, L.h, L.w, L.row_stride[0]) == (0, 32, 32, 32 * shape[2])
    # channels first: a [3,H,W] frame contributes its three channel views
    frames = [np.zeros((3, 40, 48), np.uint8) for _ in range(2)]
    L, n, keep = binding._frame_list(frames, RGBP)
    assert (L.format, L.n, L.h, L.w) == (RGBP, 2, 40, 48) and list(L.row_stride) == [48] * 3
    for c in range(3):
        tab = ctypes.cast(L.plane[c], ctypes.POINTER(ctypes.c_void_p * 2)).contents
        assert list(tab) == [f.ctypes.data + c * 40 * 48 for f in frames]
    with pytest.raises(ValueError, match=r"uint8\[3,H,W\]"):
        binding._frame_list([np.zeros((40, 48, 3), np.uint8)], RGBP)
    with pytest.raises(ValueError, match="not dense"):
        binding._frame_list([np.zeros((40, 48, 3), np.uint8).transpose(2, 0, 1)], RGBP)
    with pytest.raises(ValueError, match="fmt must be"):
        binding._frame_list(frames, 0x14)
    with pytest.raises(ValueError, match="uint8"):
        binding._frame_list([f.astype(np.int16) for f in frames], RGBP)


def test_sources_and_the_stream_take_the_layouts():
    from avd_hip import analyzer, sources
    import inspect
    assert inspect.signature(analyzer.FrameAnalyzer.records_stream).parameters["fmt"].default == BGR
    doc = inspect.getsource(sources.FrameSource)
    for name in ("rgb24", "bgra32", "rgba32", "rgbp"):
        assert '"%s"' % name in doc
    from app.analyzers import video
    assert video._RGB_SURFACES == {"rgb24": RGB24, "bgra32": BGRA32, "rgba32": RGBA32, "rgbp": RGBP}
    fa = object.__new__(analyzer.FrameAnalyzer)
    with pytest.raises(ValueError, match="one array per frame"):
        fa.records_stream([], NV12)
