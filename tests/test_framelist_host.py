"""Clips as lists of separately allocated frames (include/avd_frame_list.h), the part that needs no GPU: the descriptor's presence in header,
library and binding, and the host logic of csrc/avd_ingest_clip.h -- from_frame_list's and check_clip's refusals in their documented order, the
staging plan of a host list (list_stage) and the vector-fill eligibility (list_vec_eligible).  tests/ingest_check.cpp is compiled with the
host C++ compiler and the address / undefined-behaviour sanitizers and run as its own process; nothing sanitized is loaded into Python.

The staging rule, restated here and computed independently in `plan`: the spans of all (frame, plane) pairs in address order, merged where they
overlap or touch; every merged span on a 256-byte boundary; a plane at span offset + pointer difference; `copied` the sum of the merged spans,
`total` the end of the last one rounded up to 256.  All addresses are made up: the header never reads through them."""
import ctypes
import os
import re

import pytest

from avd_hip import _lib
from tests.ingest_host_kit import (ARG, BGR, DEVICE, FULL, HOST, I420, NV12, OK, PLANES, ROOT, T_GEOM, T_MEM, T_NULL_ARRAY, T_NULL_ENTRY, UNSUPPORTED,  # noqa: F401
                                   frame_list, parse, picture, program, r256, t_format, t_reserved, t_rotate, t_size)
from tests.ingest_host_kit import T_SMALL as T_32

T_SIZE, T_FORMAT, T_ROTATE, T_RESERVED = (t("frame_list") for t in (t_size, t_format, t_rotate, t_reserved))
T_RANGE = "AVD_FMT_FULL_RANGE describes 4:2:0 samples: a BGR picture has no range"
T_BGR_TURN = "a turned BGR picture is not on the path: cv2 hands BGR over already rotated"
T_UV = "the U and V planes of an I420 picture share their strides"
T_EVEN = {NV12: "NV12 needs even width and height", I420: "I420 needs even width and height"}
T_STRIDES = {BGR: "strides smaller than the frame", NV12: "strides smaller than the planes", I420: "strides smaller than the I420 planes"}


def plane_bytes(fmt, h, w, rows):
    """bytes of each plane of one frame, first to last"""
    if fmt == BGR:
        return [rows[0] * (h - 1) + 3 * w]
    cw = w if fmt == NV12 else w // 2
    return [rows[0] * (h - 1) + w] + [rows[p] * (h // 2 - 1) + cw for p in range(1, PLANES[fmt])]


def tight(fmt, w):
    return {BGR: [3 * w, 0, 0], NV12: [w, w, 0], I420: [w, w // 2, w // 2]}[fmt]


def flist(layout, addrs, h=64, w=64, mem=HOST, rows=None, **kw):
    """addrs: per plane the list of frame addresses; kw: any field, `fmt` (the descriptor's format word, by default the layout) included"""
    n = len(addrs[0])
    d = dict(fmt=layout, mem=mem, n=n, h=h, w=w, rotate=0, reserved=0, size_delta=0, rows=list(rows or tight(layout, w)), null_arrays=0,
             addrs=[list(a) for a in addrs] + [[0] * n] * (3 - len(addrs)))
    d.update(kw)
    return d


def plan(c):
    """the staging rule, from its statement"""
    fmt, n = c["fmt"] & 0xFF, c["n"]
    size = plane_bytes(fmt, c["h"], c["w"], c["rows"])
    items = sorted((c["addrs"][p][f], size[p], p * n + f) for p in range(PLANES[fmt]) for f in range(n))
    spans, plane_off = [], [0] * (PLANES[fmt] * n)             # span: [address, bytes, offset]
    for addr, nbytes, slot in items:
        if spans and addr <= spans[-1][0] + spans[-1][1]:
            spans[-1][1] = max(spans[-1][1], addr - spans[-1][0] + nbytes)
        else:
            spans.append([addr, nbytes, r256(spans[-1][2] + spans[-1][1]) if spans else 0])
        plane_off[slot] = spans[-1][2] + addr - spans[-1][0]
    return dict(nspans=len(spans), off=[s[2] for s in spans], bytes=[s[1] for s in spans], plane_off=plane_off,
                total=r256(spans[-1][2] + spans[-1][1]), copied=sum(s[1] for s in spans))


def run_lists(program, cases):
    lines = [frame_list(c["fmt"], c["addrs"], mem=c["mem"], h=c["h"], w=c["w"], rotate=c["rotate"], reserved=c["reserved"], rs=c["rows"],
                        null_arrays=c["null_arrays"], size_delta=c["size_delta"], n=c["n"]) for c in cases]
    return [parse(g) for g in program(lines)]


def run_strided(program, fmt, n, h, w, bases, rows, frames):
    """-> the staging plan of the STRIDED host clip (from_picture, clip_stage)"""
    g = parse(program([picture(fmt, n=n, h=h, w=w, planes=bases, rs=rows, fs=frames)])[0])
    assert g["status"] == OK, g
    return {k: g[k] for k in ("nspans", "total", "copied")}


# ---- ABI presence ----------------------------------------------------------------------------------------------------------------------------
def test_descriptor_is_the_same_in_header_binding_and_compiler(program):
    hdr = open(os.path.join(ROOT, "include", "avd_frame_list.h")).read()
    body = re.search(r"typedef struct avd_frame_list \{(.*?)\} avd_frame_list;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[\d+\]", "", v.strip().split()[-1].lstrip("*")) for v in decl.split(",")]
    assert names == ["struct_size", "format", "plane", "row_stride", "mem", "n", "h", "w", "rotate", "reserved"]
    assert names == [f[0] for f in _lib.AvdFrameList._fields_]
    a = parse(program(["A"])[0])
    assert a["list_size"] == ctypes.sizeof(_lib.AvdFrameList) == 80
    assert a["list_offsets"] == [getattr(_lib.AvdFrameList, f).offset for f in names[1:]]
    assert a["picture_size"] == ctypes.sizeof(_lib.AvdPicture) == 104            # avd_picture is untouched


def test_the_three_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "avd.h")).read()
    own = open(os.path.join(ROOT, "include", "avd_frame_list.h")).read()
    assert re.search(r'^#include "avd_frame_list.h"$', hdr, re.M)               # whoever includes avd.h has the family
    _lib.build()
    L = _lib.load()
    assert set(re.findall(r"^int (avd_\w+)\(", own, re.M)) == set(_lib.LIST_EXPORTS)
    for name in ("avd_preprocess_frame_list", "avd_analyze_frame_lists", "avd_analyze_frame_lists_async"):
        assert re.search(r"^int %s\(avd_ctx\*" % name, own, re.M), name
        assert name in _lib.LIST_EXPORTS and hasattr(L, name), name
    for name in ("preprocess_frame_list", "analyze_frame_lists", "analyze_frame_lists_async", "ingest_list", "stage_copies"):
        assert callable(getattr(_lib.Context, name)), name
    # the new entry is in the sentence that lists the asynchronous calls any other call drains
    assert re.search(r"avd_analyze_pictures_async and avd_analyze_frame_lists_async: whichever of them is\s+\*?\s*outstanding is drained", hdr)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
A3 = [[0x10000000, 0x10100000], [0x20000000, 0x20100000], [0x30000000, 0x30100000]]


def valid(layout, **kw):
    return flist(layout, A3[:PLANES[layout]], **kw)


def with_addr(c, p, f, a):
    c["addrs"] = [list(x) for x in c["addrs"]]
    c["addrs"][p][f] = a
    return c


# Every row carries the fault it is named after AND at least one fault of a later row: the first in the documented order must win.
REFUSALS = [
    ("struct-size", valid(I420, size_delta=8, fmt=7), (ARG, T_SIZE)),
    ("format-layout", valid(NV12, fmt=7, rotate=4), (ARG, T_FORMAT)),
    ("format-high-bit", valid(NV12, fmt=NV12 | 0x200, rotate=4), (ARG, T_FORMAT)),
    ("full-range-bgr", valid(BGR, fmt=BGR | FULL, rotate=4), (ARG, T_RANGE)),
    ("rotate", valid(I420, rotate=4, reserved=1), (ARG, T_ROTATE)),
    ("rotate-negative", valid(NV12, rotate=-1, reserved=1), (ARG, T_ROTATE)),
    ("reserved", valid(I420, reserved=1, rows=[64, 32, 40]), (ARG, T_RESERVED)),
    ("reserved-bgr-turned", valid(BGR, reserved=1, rotate=1), (ARG, T_RESERVED)),
    ("bgr-turned", valid(BGR, rotate=1, mem=2), (UNSUPPORTED, T_BGR_TURN)),
    ("uv-strides", valid(I420, rows=[64, 32, 40], mem=2), (ARG, T_UV)),
    ("mem", valid(NV12, mem=2, n=-1), (ARG, T_MEM)),
    ("n-negative", valid(NV12, n=-1, h=65), (ARG, T_GEOM)),
    ("h-16386", valid(I420, h=16386, w=30, rows=[30, 15, 15]), (ARG, T_GEOM)),
    ("odd-nv12", valid(NV12, h=31), (UNSUPPORTED, T_EVEN[NV12])),                        # odd AND below 32
    ("odd-i420", valid(I420, w=31, rows=[31, 15, 15], null_arrays=1), (UNSUPPORTED, T_EVEN[I420])),
    ("below-32", valid(I420, h=30, null_arrays=2), (UNSUPPORTED, T_32)),
    ("below-32-bgr", valid(BGR, w=31, rows=[93, 0, 0], null_arrays=1), (UNSUPPORTED, T_32)),
    ("null-array-0", with_addr(valid(NV12, null_arrays=1), 1, 1, 0), (ARG, T_NULL_ARRAY)),
    ("null-array-2", with_addr(valid(I420, null_arrays=4), 0, 0, 0), (ARG, T_NULL_ARRAY)),     # an array before an entry, whatever the plane
    ("null-entry", with_addr(valid(I420, rows=[63, 32, 32]), 2, 1, 0), (ARG, T_NULL_ENTRY)),
    ("null-entry-bgr", with_addr(valid(BGR, rows=[191, 0, 0]), 0, 0, 0), (ARG, T_NULL_ENTRY)),
    ("row-stride-bgr", valid(BGR, rows=[191, 0, 0]), (ARG, T_STRIDES[BGR])),
    ("row-stride-nv12-uv", valid(NV12, rows=[64, 63, 0]), (ARG, T_STRIDES[NV12])),
    ("row-stride-i420-y", valid(I420, rows=[63, 32, 32]), (ARG, T_STRIDES[I420])),
]


def test_refusal_table_in_the_documented_order(program):
    got = run_lists(program, [c for _, c, _ in REFUSALS])
    for (name, _, want), g in zip(REFUSALS, got):
        assert (g["status"], g["why"]) == want, name
        assert g["nspans"] == g["total"] == g["copied"] == 0, name


def test_what_is_not_a_fault(program):
    ok = [valid(BGR), valid(NV12), valid(I420), valid(NV12, mem=DEVICE, rotate=3, fmt=NV12 | FULL),
          valid(I420, n=0, null_arrays=7),                                       # no frames: nothing is looked at
          flist(NV12, [[0x1000, 0x1000], [0x9000, 0x9000]]),                      # a frame twice
          flist(BGR, [[0x900000, 0x100000]])]                                     # descending addresses
    for g in run_lists(program, ok):
        assert (g["status"], g["why"]) == (OK, "")


# ---- staging plan ----------------------------------------------------------------------------------------------------------------------------
def check_plan(g, c):
    want = plan(c)
    assert {k: g[k] for k in want} == want
    assert all(o % 256 == 0 for o in g["off"])
    # every plane at its span's offset plus the pointer difference, inside that span
    fmt, n = c["fmt"] & 0xFF, c["n"]
    size = plane_bytes(fmt, c["h"], c["w"], c["rows"])
    starts = {a for p in range(PLANES[fmt]) for a in c["addrs"][p]}
    for p in range(PLANES[fmt]):
        for f in range(n):
            off, addr = g["plane_off"][p * n + f], c["addrs"][p][f]
            i = max(j for j in range(g["nspans"]) if g["off"][j] <= off)
            assert off - g["off"][i] + size[p] <= g["bytes"][i]
            span_addr = addr - (off - g["off"][i])
            assert span_addr in starts                                           # a span starts at a plane


def test_views_of_a_stack_stage_as_the_strided_clip(program):
    n, h, w = 5, 48, 64
    base = 0x40000000
    # BGR: one dense stack
    c = flist(BGR, [[base + f * 3 * w * h for f in range(n)]], h=h, w=w)
    s = run_strided(program, BGR, n, h, w, [base, 0, 0], [3 * w, 0, 0], [3 * w * h, 0, 0])
    g = run_lists(program, [c])[0]
    check_plan(g, c)
    assert (g["nspans"], g["copied"], g["total"]) == (1, s["copied"], s["total"]) and s["nspans"] == 1 and g["copied"] == n * 3 * w * h
    # I420 from one buffer: Y, U, V of a frame adjacent (a y4m map without markers, a rawvideo pipe)
    pic = w * h * 3 // 2
    ys = [base + f * pic for f in range(n)]
    c = flist(I420, [ys, [a + w * h for a in ys], [a + w * h * 5 // 4 for a in ys]], h=h, w=w)
    s = run_strided(program, I420, n, h, w, [base, base + w * h, base + w * h * 5 // 4], [w, w // 2, w // 2], [pic] * 3)
    g = run_lists(program, [c])[0]
    check_plan(g, c)
    assert (g["nspans"], g["copied"], g["total"]) == (1, s["copied"], s["total"]) and s["nspans"] == 1 and g["copied"] == n * pic
    # NV12 out of two stacks: the strided clip's two spans, the same bytes
    uv0 = 0x50000000
    c = flist(NV12, [[base + f * w * h for f in range(n)], [uv0 + f * w * h // 2 for f in range(n)]], h=h, w=w)
    s = run_strided(program, NV12, n, h, w, [base, uv0, 0], [w, w, 0], [w * h, w * h // 2, 0])
    g = run_lists(program, [c])[0]
    check_plan(g, c)
    assert (g["nspans"], g["copied"], g["total"]) == (2, s["copied"], s["total"]) and s["nspans"] == 2


@pytest.mark.parametrize("fmt", [BGR, NV12, I420])
def test_separately_allocated_frames_in_shuffled_order(program, fmt):
    n, h, w = 4, 48, 64
    order = [2, 0, 3, 1]                                                         # list position -> allocation rank
    addrs = [[0x10000000 * (p + 1) + 0x40000 * order[f] + 16 for f in range(n)] for p in range(PLANES[fmt])]
    c = flist(fmt, addrs, h=h, w=w)
    g = run_lists(program, [c])[0]
    check_plan(g, c)
    assert g["nspans"] == n * PLANES[fmt]
    assert g["copied"] == n * sum(plane_bytes(fmt, h, w, c["rows"]))
    assert sorted(g["bytes"]) == sorted(plane_bytes(fmt, h, w, c["rows"]) * n)


def test_a_repeated_frame_crosses_the_link_once(program):
    h, w = 48, 64
    y = [0x1000000, 0x2000000, 0x2000000, 0x3000000]
    c = flist(NV12, [y, [a + 0x100000 for a in y]], h=h, w=w)
    g = run_lists(program, [c])[0]
    check_plan(g, c)
    assert g["nspans"] == 6 and g["copied"] == 3 * (w * h * 3 // 2)
    assert g["plane_off"][1] == g["plane_off"][2] and g["plane_off"][4 + 1] == g["plane_off"][4 + 2]
    # partly overlapping planes (a sliding window over one buffer) are merged too: no byte twice
    c = flist(BGR, [[0x1000000, 0x1000000 + 3 * w * 10, 0x1000000 + 3 * w * 20]], h=h, w=w)
    g = run_lists(program, [c])[0]
    check_plan(g, c)
    assert g["nspans"] == 1 and g["copied"] == 3 * w * (h + 20)


def test_a_gap_keeps_spans_apart_and_touching_merges(program):
    h, w = 48, 64
    pic = w * h * 3 // 2
    base = 0x7000000
    for gap, nspans in ((6, 2), (1, 2), (0, 1)):                                 # 6: the FRAME\n marker between the pictures of a .y4m file
        ys = [base, base + pic + gap]
        c = flist(I420, [ys, [a + w * h for a in ys], [a + w * h * 5 // 4 for a in ys]], h=h, w=w)
        g = run_lists(program, [c])[0]
        check_plan(g, c)
        assert (g["nspans"], g["copied"]) == (nspans, 2 * pic), gap
        if nspans == 2:
            assert g["off"] == [0, r256(pic)] and g["plane_off"][1] == r256(pic)


def test_row_padded_frames(program):
    h, w = 48, 64
    c = flist(NV12, [[0x1000000, 0x1100000], [0x2000000, 0x2100000]], h=h, w=w, rows=[80, 96, 0])
    g = run_lists(program, [c])[0]
    check_plan(g, c)
    assert sorted(g["bytes"]) == sorted(2 * [80 * (h - 1) + w, 96 * (h // 2 - 1) + w])


# ---- eligibility for the 16-byte fills -------------------------------------------------------------------------------------------------------
def test_one_misaligned_frame_sends_the_list_through_the_scalar_fill(program):
    h, w = 48, 64
    al = lambda fmt: [[0x10000000 * (p + 1) + 0x40000 * f for f in range(4)] for p in range(PLANES[fmt])]
    cases, want = [], []
    for fmt in (BGR, NV12, I420):
        for mem in (HOST, DEVICE):
            cases.append(flist(fmt, al(fmt), h=h, w=w, mem=mem))
            want.append(1)
            for p in range(PLANES[fmt]):
                cases.append(with_addr(flist(fmt, al(fmt), h=h, w=w, mem=mem), p, 2, al(fmt)[p][2] + 1))      # one frame, one plane, one byte off
                want.append(0)
    # the chroma planes of I420 are read 8 bytes at a time: 8 is enough there, not for Y or NV12's chroma
    cases.append(with_addr(flist(I420, al(I420), h=h, w=w, mem=DEVICE), 2, 1, al(I420)[2][1] + 8))
    want.append(1)
    cases.append(with_addr(flist(NV12, al(NV12), h=h, w=w, mem=DEVICE), 1, 1, al(NV12)[1][1] + 8))
    want.append(0)
    cases.append(flist(NV12, al(NV12), h=50, w=70, mem=DEVICE))                  # w % 16 != 0
    want.append(0)
    cases.append(flist(NV12, al(NV12), h=h, w=w, mem=DEVICE, rows=[72, 64, 0]))   # a row stride that is no multiple of 16
    want.append(0)
    for c, wnt, g in zip(cases, want, run_lists(program, cases)):
        assert g["status"] == OK
        # a host list is judged where it is staged: a span lands on a 256-byte boundary, so a separately allocated frame is aligned there
        # whatever its host address; a device list is judged where it lies
        if c["mem"] == DEVICE:
            assert g["given"] == wnt, c
        else:
            assert g["staged"] == 1 and g["given"] == wnt, c


def test_a_staged_frame_inside_a_merged_span_keeps_its_misalignment(program):
    h, w = 48, 64
    base = 0x8000000
    # two touching BGR frames behind a one-byte offset into their buffer: one span, both frames at odd... the second at span + 3wh
    c = flist(BGR, [[base + 1, base + 1 + 3 * w * h + 8]], h=h, w=w)
    g = run_lists(program, [c])[0]
    assert g["nspans"] == 2 and g["staged"] == 1                                # a gap: two spans, both on a boundary
    c = flist(BGR, [[base, base + 3 * w * h - 8]], h=h, w=w)                     # overlapping by 8 bytes: merged, the second frame 8 off
    g = run_lists(program, [c])[0]
    assert g["nspans"] == 1 and g["plane_off"] == [0, 3 * w * h - 8] and g["staged"] == 0
