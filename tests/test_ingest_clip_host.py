"""The ingest host path's one clip type (csrc/avd_ingest_clip.h), without a GPU and without the library: tests/ingest_check.cpp (built with the
address / undefined-behaviour sanitizers by tests/ingest_host_kit.py) is fed one line per clip through each of the three named constructors,
from_public and from_picture, and its answers are compared with what is written out here.

The refusal table (`single_faults`, `MULTI_FAULTS`, `PICTURE_FAULTS`) is the documented check order of include/avd.h: mem, the size range, even
width and height (4:2:0), the 32 x 32 minimum, null planes of a clip that has frames, strides.  Status and text of every row are the library's
source strings, written out.  tests/test_gpu_ingest_entries.py sends the same rows through every public entry point of the library.
The staging plan is computed here from its rule: BGR one span; NV12 the chroma span on the next 256-byte boundary behind the Y span; the three
I420 spans in address order, merged where they overlap or touch, a span that is not merged on the next 256-byte boundary; `copied` the sum of
the spans' bytes, `total` the end of the last span rounded up to 256."""
import copy

import pytest

from tests.ingest_host_kit import ARG, BGR, DEVICE, HOST, I420, NV12, OK, PLANES, T_GEOM, T_MEM, UNSUPPORTED, parse, t_size
from tests.ingest_host_kit import T_SMALL as T_32
from tests.ingest_host_kit import program as _lines

NAMES = {BGR: "bgr", NV12: "nv12", I420: "i420"}
T_EVEN = {NV12: "NV12 needs even width and height", I420: "I420 needs even width and height"}
T_NULL = {BGR: "null frame pointer", NV12: "null plane pointer", I420: "null I420 plane pointer"}
T_STRIDES = {BGR: "strides smaller than the frame", NV12: "strides smaller than the planes", I420: "strides smaller than the I420 planes"}
ADDR = (0x10000000, 0x20000000, 0x30000000)            # stand-ins for plane pointers: the header never reads through them


def tight(fmt, h, w):
    """-> (row strides, frame strides) of exactly-sized planes"""
    if fmt == BGR:
        return [3 * w, 0, 0], [3 * w * h, 0, 0]
    if fmt == NV12:
        return [w, w, 0], [w * h, w * (h // 2), 0]
    return [w, w // 2, w // 2], [w * h, (w // 2) * (h // 2), (w // 2) * (h // 2)]


def clip(fmt, n=2, h=64, w=64, mem=HOST, planes=ADDR, rotate=0):
    rows, frames = tight(fmt, h, w)
    return dict(fmt=fmt, mem=mem, n=n, h=h, w=w, rotate=rotate, planes=list(planes[:PLANES[fmt]]) + [0] * (3 - PLANES[fmt]), rows=rows,
                frames=frames, size_delta=0, reserved=0)


def _set(**kw):
    return lambda c: c.update(kw)


def _size(**kw):
    """another stored size, with the tight strides of THAT size: the size is the only fault"""
    def edit(c):
        c.update(kw)
        c["rows"], c["frames"] = tight(c["fmt"], c["h"], c["w"])
    return edit


def _item(key, i, delta=None):
    def edit(c):
        c[key][i] = 0 if delta is None else c[key][i] + delta
        if c["fmt"] == I420 and i == 1 and key != "planes":
            c[key][2] = c[key][1]                          # U and V share their strides
    return edit


def single_faults(fmt):
    """-> [(name, edit of a valid clip of 2 frames of 64 x 64 with tight strides, (status, text))], one row per fault, in the documented order"""
    rows = [("mem", _set(mem=2), (ARG, T_MEM)), ("n-negative", _set(n=-1), (ARG, T_GEOM)),
            ("h-16386", _size(h=16386), (ARG, T_GEOM)), ("w-16386", _size(w=16386), (ARG, T_GEOM))]
    if fmt != BGR:
        rows += [("h-65", _size(h=65), (UNSUPPORTED, T_EVEN[fmt])), ("w-65", _size(w=65), (UNSUPPORTED, T_EVEN[fmt]))]
    rows += [("h-30", _size(h=30), (UNSUPPORTED, T_32)), ("w-30", _size(w=30), (UNSUPPORTED, T_32))]
    rows += [(f"null-plane-{i}", _item("planes", i), (ARG, T_NULL[fmt])) for i in range(PLANES[fmt])]
    for i in range(min(PLANES[fmt], 2)):
        rows += [(f"row-stride-{i}", _item("rows", i, -1), (ARG, T_STRIDES[fmt])), (f"frame-stride-{i}", _item("frames", i, -1), (ARG, T_STRIDES[fmt]))]
    return rows


def _both(*edits):
    def edit(c):
        for e in edits:
            e(c)
    return edit


# Two faults at once: the FIRST in the documented order is the one reported.
MULTI_FAULTS = [
    ("bgr-small-and-short-strided", BGR, _both(_size(h=30), _item("rows", 0, -1)), (UNSUPPORTED, T_32)),       # the minimum before the strides
    ("i420-mem-and-small", I420, _both(_size(w=30), _set(mem=2)), (ARG, T_MEM)),                                # mem before everything
]

# What the descriptor alone gets wrong (from_picture), before any of the above is looked at.
PICTURE_FAULTS = [
    ("struct-size-minus-8", NV12, _set(size_delta=-8), (ARG, t_size("picture"))),
    ("struct-size-plus-8", I420, _set(size_delta=8), (ARG, t_size("picture"))),
    ("format-3", NV12, _set(fmt=3), (ARG, "bad avd_picture.format")),
    ("rotate-minus-1", NV12, _set(rotate=-1), (ARG, "avd_picture.rotate must be 0 .. 3 quarter turns")),
    ("rotate-4", I420, _set(rotate=4), (ARG, "avd_picture.rotate must be 0 .. 3 quarter turns")),
    ("reserved-1", I420, _set(reserved=1), (ARG, "avd_picture.reserved must be 0")),
    ("bgr-rotate-1", BGR, _set(rotate=1), (UNSUPPORTED, "a turned BGR picture is not on the path: cv2 hands BGR over already rotated")),
    ("uv-row-strides-unequal", I420, lambda c: c["rows"].__setitem__(2, c["rows"][2] + 8), (ARG, "the U and V planes of an I420 picture share their strides")),
    ("uv-frame-strides-unequal", I420, lambda c: c["frames"].__setitem__(2, c["frames"][2] + 8), (ARG, "the U and V planes of an I420 picture share their strides")),
]


def constructors(fmt):
    """the ways a clip of this format can be made"""
    return ("direct", "picture") if fmt == I420 else ("direct", "public", "picture")


def edited(fmt, edit):
    c = copy.deepcopy(clip(fmt))
    edit(c)
    return c


# ---- the program ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(_lines):
    def run(cases):
        """cases: [(via, clip dict)] -> [dict(status, why, format, nspans, off, bytes, plane_off, total, copied)], the lists padded to three entries"""
        lines = []
        for via, c in cases:
            if via == "direct":
                lines.append(["D", c["fmt"], c["mem"], c["n"], c["h"], c["w"], *c["planes"], *c["rows"][:2], *c["frames"][:2]])
            elif via == "public":
                lines.append(["C", c["mem"], c["n"], c["h"], c["w"], *c["planes"][:2], *c["rows"][:2], *c["frames"][:2]])
            else:
                lines.append(["P", c["fmt"], c["mem"], c["n"], c["h"], c["w"], c["rotate"], c["reserved"], c["size_delta"], *c["planes"], *c["rows"], *c["frames"]])
        out = [parse(g) for g in _lines([" ".join(str(v) for v in l) for l in lines])]
        for g in out:
            for key in ("off", "bytes", "plane_off"):
                g[key] = (g[key] + [0, 0, 0])[:3]
        return out
    return run


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_every_fault_through_every_constructor(program):
    cases, want = [], []
    for fmt in (BGR, NV12, I420):
        for via in constructors(fmt):
            cases.append((via, clip(fmt)))
            want.append((f"{NAMES[fmt]}-{via}-valid", (OK, "")))
            for name, edit, expect in single_faults(fmt):
                if via == "public" and fmt == NV12 and name == "null-plane-1":
                    continue                                   # an avd_clip without uv IS a BGR clip (test_from_public_infers_the_format)
                cases.append((via, edited(fmt, edit)))
                want.append((f"{NAMES[fmt]}-{via}-{name}", expect))
    got = program(cases)
    for (tag, expect), g, (via, c) in zip(want, got, cases):
        assert (g["status"], g["why"]) == expect, (tag, g)
        assert g["format"] == c["fmt"], (tag, g)


def test_descriptor_faults_of_from_picture(program):
    got = program([("picture", edited(fmt, edit)) for _, fmt, edit, _ in PICTURE_FAULTS])
    for (name, _, _, expect), g in zip(PICTURE_FAULTS, got):
        assert (g["status"], g["why"]) == expect, (name, g)
    # a descriptor fault comes before anything check_clip looks at
    both = edited(I420, _both(_set(mem=2, reserved=1)))
    assert program([("picture", both)])[0]["why"] == "avd_picture.reserved must be 0"


def test_the_first_fault_in_the_documented_order_is_reported(program):
    for name, fmt, edit, expect in MULTI_FAULTS:
        for via, g in zip(constructors(fmt), program([(via, edited(fmt, edit)) for via in constructors(fmt)])):
            assert (g["status"], g["why"]) == expect, (name, via, g)
    # and the rest of the order, pairwise, on an NV12 clip: size range < even < 32 x 32 < null planes < strides
    order = [(_set(n=-1), T_GEOM), (_size(h=65), T_EVEN[NV12]), (_size(w=30), T_32), (_item("planes", 1), T_NULL[NV12]), (_item("rows", 0, -1), T_STRIDES[NV12])]
    pairs = [(a, b) for i, a in enumerate(order) for b in order[i + 1:]]
    got = program([("direct", edited(NV12, _both(b[0], a[0]))) for a, b in pairs])         # the later fault is applied first
    for (a, b), g in zip(pairs, got):
        assert g["why"] == a[1], (a[1], b[1], g)


def test_from_public_infers_the_format(program):
    nv, bg = clip(NV12), clip(BGR)
    no_uv = edited(NV12, _item("planes", 1))
    got = program([("public", nv), ("public", bg), ("public", no_uv)])
    assert (got[0]["format"], got[0]["status"]) == (NV12, OK)
    assert (got[1]["format"], got[1]["status"]) == (BGR, OK)
    # without uv the clip is BGR, and as BGR its luma strides are too small for three bytes per pixel
    assert (got[2]["format"], got[2]["status"], got[2]["why"]) == (BGR, ARG, T_STRIDES[BGR])


# ---- staging -------------------------------------------------------------------------------------------------------------------------------------
def _r256(v):
    return (v + 255) // 256 * 256


def _stage(c):
    """the staging plan of an accepted clip, from the rule"""
    zero = dict(nspans=0, off=[0, 0, 0], bytes=[0, 0, 0], plane_off=[0, 0, 0], total=0, copied=0)
    if c["mem"] != HOST or c["n"] <= 0:
        return zero
    fmt, n, h, w = c["fmt"], c["n"], c["h"], c["w"]
    span = lambda i, rows, row_bytes: c["frames"][i] * (n - 1) + c["rows"][i] * (rows - 1) + row_bytes
    if fmt == BGR:
        planes = [(c["planes"][0], span(0, h, 3 * w), 0)]
    else:
        cw = w // 2 if fmt == I420 else w
        planes = [(c["planes"][0], span(0, h, w), 0)] + [(c["planes"][i], span(1, h // 2, cw), i) for i in range(1, PLANES[fmt])]
    if fmt == I420:
        planes.sort(key=lambda p: p[0])
    spans, plane_off = [], [0, 0, 0]                       # span: [address, bytes, offset]
    for addr, length, i in planes:
        if fmt == I420 and spans and addr <= spans[-1][0] + spans[-1][1]:
            spans[-1][1] = max(spans[-1][1], addr - spans[-1][0] + length)
        else:
            spans.append([addr, length, _r256(spans[-1][2] + spans[-1][1]) if spans else 0])
        plane_off[i] = spans[-1][2] + addr - spans[-1][0]
    pad = [0] * (3 - len(spans))
    return dict(nspans=len(spans), off=[s[2] for s in spans] + pad, bytes=[s[1] for s in spans] + pad, plane_off=plane_off,
                total=_r256(spans[-1][2] + spans[-1][1]), copied=sum(s[1] for s in spans))


def test_staging_plans(program):
    n, h, w = 3, 34, 48
    picture = w * h * 3 // 2
    one_buffer = clip(I420, n, h, w, planes=(ADDR[0], ADDR[0] + w * h, ADDR[0] + w * h + (w // 2) * (h // 2)))     # Y, U, V of a frame adjacent
    one_buffer["frames"] = [picture] * 3
    separate = clip(I420, n, h, w, planes=(ADDR[2], ADDR[0], ADDR[1]))                                           # Y highest, then V, then U lowest
    touching = clip(I420, n, h, w, planes=(ADDR[0], ADDR[0] + n * w * h, ADDR[2]))                                # U starts where the Y planes end
    padded = clip(NV12, 2, 64, 80)
    padded["rows"], padded["frames"] = [96, 128, 0], [96 * 64 + 32, 128 * 32, 0]                                 # a decoder's pitch
    layouts = [("bgr", clip(BGR)), ("nv12", clip(NV12)), ("nv12-pitch", padded), ("i420-one-buffer", one_buffer), ("i420-separate", separate),
               ("i420-touching", touching), ("device", clip(I420, mem=DEVICE)), ("n-0", clip(NV12, n=0))]
    got = program([("direct", c) for _, c in layouts] + [("picture", c) for _, c in layouts])
    for (name, c), g in zip(layouts + layouts, got):
        assert g["status"] == OK, (name, g)
        assert {k: g[k] for k in ("nspans", "off", "bytes", "plane_off", "total", "copied")} == _stage(c), (name, g, _stage(c))
    by_name = {name: g for (name, _), g in zip(layouts, got)}
    # the same plans in plain numbers, where the rule's outcome is easy to state
    assert by_name["bgr"]["nspans"] == 1 and by_name["bgr"]["copied"] == by_name["bgr"]["total"] == 2 * 64 * 64 * 3
    g = by_name["nv12"]
    assert (g["nspans"], g["off"][:2], g["plane_off"][:2], g["copied"]) == (2, [0, 2 * 64 * 64], [0, 2 * 64 * 64], 2 * 64 * 64 * 3 // 2)
    g = by_name["i420-one-buffer"]                                             # one copy of the whole buffer, no byte twice
    assert (g["nspans"], g["copied"], g["plane_off"]) == (1, n * picture, [0, w * h, w * h + (w // 2) * (h // 2)])
    assert g["total"] == _r256(n * picture)
    g = by_name["i420-separate"]                                               # three copies, U first, then V, then Y
    ly, lc = n * w * h, n * (w // 2) * (h // 2)
    assert (g["nspans"], g["bytes"], g["copied"]) == (3, [lc, lc, ly], ly + 2 * lc)
    assert g["plane_off"] == [2 * _r256(lc), 0, _r256(lc)] and g["off"] == [0, _r256(lc), 2 * _r256(lc)]
    g = by_name["i420-touching"]
    assert (g["nspans"], g["bytes"], g["plane_off"]) == (2, [ly + lc, lc, 0], [0, ly, _r256(ly + lc)])
    for name in ("device", "n-0"):
        assert by_name[name]["nspans"] == by_name[name]["total"] == by_name[name]["copied"] == 0
