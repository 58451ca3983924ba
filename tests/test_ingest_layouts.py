"""The 13 ingest layouts are described once per side: include/avd.h (the values), csrc/avd_ingest_clip.h (kIngestLayouts, asked through
tests/ingest_check.cpp), the binding (avd_hip._lib.LAYOUTS) and the tests' own table (tests/ingest_host_kit.LAYOUTS).  Here the four are held
against each other, a value without a row is shown to be refused by both descriptors, the one vector-eligibility rule is asked for a strided
clip of every layout, and the exported symbol set is pinned (no layout ever added a function).  No GPU."""
import os
import re
import shutil
import subprocess

import avd_hip
from avd_hip import _lib
from tests.ingest_host_kit import ARG, BASE, DEVICE, FULL, LAYOUTS, OK, ROOT, frame_list, parse, picture, row_bytes, sub_shape, t_format
from tests.ingest_host_kit import program  # noqa: F401


def _header_values():
    hdr = open(os.path.join(ROOT, "include", "avd.h")).read()
    values = {name: int(v, 16) for name, v in re.findall(r"^#define AVD_FMT_(\w+)\s+(0x[0-9a-fA-F]+)", hdr, re.M)}
    values.update((name, int(v)) for name, v in re.findall(r"AVD_FMT_(\w+) = (\d+)", re.search(r"enum avd_format \{(.*?)\}", hdr).group(1)))
    return values


def test_header_table_binding_and_tests_agree_on_every_layout(program):
    h, w = 48, 64
    header = _header_values()
    assert header.pop("FULL_RANGE") == FULL == _lib.AVD_FMT_FULL_RANGE
    assert header == {l.name: l.value for l in LAYOUTS} and len(LAYOUTS) == 13
    a = parse(program(["A"])[0])
    assert a["rows"] == [l.value for l in LAYOUTS] == [l.value for l in _lib.LAYOUTS]
    assert a["AVD_FMT_FULL_RANGE"] == FULL
    rows = [parse(g) for g in program(["T %d %d %d" % (l.value, h, w) for l in LAYOUTS])]
    for l, row, b in zip(LAYOUTS, rows, _lib.LAYOUTS):
        assert a["AVD_FMT_" + l.name] == l.value == getattr(_lib, "AVD_FMT_" + l.name) == getattr(avd_hip, "AVD_FMT_" + l.name)
        assert (row["has_row"], row["value"], row["name"]) == (1, l.value, l.name) and (b.value, b.name) == (l.value, "AVD_FMT_" + l.name)
        assert (row["planes"], row["px"], row["sample"]) == (l.planes, l.px, l.sample) == (b.planes, b.px, b.item), l.name
        crows, cbytes = sub_shape(l.value, h, w)
        assert (row["sub_rows"], row["sub_row"]) == (crows, cbytes), l.name
        assert _lib._chroma_shape(b, h, w) == (crows, cbytes // l.sample), l.name
        # and what a descriptor of the layout carries through from_picture / from_frame_list
        p = parse(program([picture(l.value, h=h, w=w)])[0])
        assert (p["status"], p["format"], p["planes"], p["px"], p["sub_rows"], p["sub_row"]) == (OK, l.value, l.planes, l.px, crows, cbytes), l.name
    assert _lib._PACKED == {l.value: l.px for l in LAYOUTS if l.planes == 1}
    assert _lib._WIDE == tuple(l.value for l in LAYOUTS if l.sample == 2)


def test_a_value_without_a_row_is_refused_by_both_descriptors(program):
    rowless = [v for v in range(256) if v not in {l.value for l in LAYOUTS}]
    assert {0x14, 0x1F, 0x24, 0x2F, 0x32, 0xFF} <= set(rowless) and len(rowless) == 243
    for flag in (0, FULL):
        for g in program(["T %d 48 64" % v for v in rowless]):
            assert parse(g)["has_row"] == 0
        for v, g in zip(rowless, program([picture(v | flag) for v in rowless])):
            assert (parse(g)["status"], parse(g)["why"]) == (ARG, t_format("picture")), hex(v)
        for v, g in zip(rowless, program([frame_list(v | flag, [[BASE[0]], [BASE[1]], [BASE[2]]]) for v in rowless])):
            assert (parse(g)["status"], parse(g)["why"]) == (ARG, t_format("frame_list")), hex(v)


def test_the_vector_rule_of_a_strided_clip_is_the_one_of_a_list(program):
    """plane 0 and its strides on 16 bytes; the planes behind it on 8 where the table fills read 8 (the chroma planes of I420 and I422), else 16"""
    for l in LAYOUTS:
        align = 8 if l.name in ("I420", "I422") else 16
        rb = row_bytes(l.value, 64)
        crows = sub_shape(l.value, 48, 64)[0]
        fs = [rb[0] * 48, rb[1] * crows, rb[2] * crows]

        def vec(**kw):
            g = parse(program([picture(l.value, mem=DEVICE, **kw)])[0])
            assert g["status"] == OK, (l.name, kw, g)
            return g["vec"]
        assert vec() == 1, l.name
        assert vec(w=72, h=48) == 0, l.name
        rgbp = l.name == "RGBP"                                # all three planes share their strides: they move together
        for delta in (8, 16):
            assert vec(planes=(BASE[0] + delta,) + BASE[1:]) == (delta == 16), l.name
            rs0 = rb[0] + delta
            assert vec(rs=[rs0] * 3 if rgbp else [rs0, rb[1], rb[2]], fs=[rs0 * 48] * 3 if rgbp else [rs0 * 48, fs[1], fs[2]]) == (delta == 16), l.name
            for n in (2, 1):                                   # the frame stride counts whatever n is
                assert vec(n=n, fs=[fs[0] + delta] * 3 if rgbp else [fs[0] + delta, fs[1], fs[2]]) == (delta == 16), (l.name, n)
            want = delta % align == 0
            for p in range(1, l.planes):
                moved = list(BASE)
                moved[p] += delta
                assert vec(planes=tuple(moved)) == want, (l.name, p, delta)
            if l.planes > 1 and not rgbp:
                assert vec(rs=[rb[0], rb[1] + delta, rb[2] + delta], fs=[fs[0], (rb[1] + delta) * crows, (rb[2] + delta) * crows]) == want, l.name
                assert vec(fs=[fs[0], fs[1] + delta, fs[2] + delta]) == want, l.name
        # the same clip as a list of its frames: the same answer
        for delta in (0, 8, 16):
            addrs = [[BASE[p] + (delta if p else 0) + f * fs[p] for f in range(2)] for p in range(l.planes)]
            g = parse(program([frame_list(l.value, addrs, mem=DEVICE)])[0])
            moved = (BASE[0],) + tuple(b + delta for b in BASE[1:])
            assert g["given"] == vec(planes=moved), (l.name, delta)


def test_the_exported_symbol_set_is_unchanged():
    """layouts, never functions: what the headers declare is what the binding lists, and the library exports exactly that"""
    hdr = open(os.path.join(ROOT, "include", "avd.h")).read()
    own = open(os.path.join(ROOT, "include", "avd_frame_list.h")).read()
    assert set(re.findall(r"^\s*(?:int|void|int64_t|const char\*)\s+(avd_\w+)\s*\(", hdr, re.M)) == set(_lib.EXPORTS)
    assert set(re.findall(r"^int (avd_\w+)\(", own, re.M)) == set(_lib.LIST_EXPORTS)
    assert len(_lib.EXPORTS) == 43 and len(_lib.LIST_EXPORTS) == 3
    nm = shutil.which("nm")
    assert nm, "no nm"
    so = _lib.build()
    out = subprocess.run([nm, "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.search(r" T avd_\w+$", line)}
    assert exported == set(_lib.EXPORTS) | set(_lib.LIST_EXPORTS), exported ^ (set(_lib.EXPORTS) | set(_lib.LIST_EXPORTS))
    assert _lib.load().avd_abi_version() == 3
    assert callable(_lib.Context.ingest_format)
    assert callable(avd_hip.FrameAnalyzer.records_stream_i422)
    assert callable(avd_hip.FrameAnalyzer.records_stream_p010) and callable(avd_hip.FrameAnalyzer.records_stream_i010)
