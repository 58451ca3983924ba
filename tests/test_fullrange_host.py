"""Full-range 4:2:0 pictures (AVD_FMT_FULL_RANGE, ffmpeg's yuvj420p), the parts that need no GPU.

tests/yuv_tables_reference.py restates libswscale's table converter literally, with a range switch.  Here it is tied to the pinned converter
(limited range: bit for bit oracle/avd_oracle.c's, on content that enumerates the corner values), and its full-range tables are checked
against what the construction must give: the gray axis is the identity, the integers are the ones written out below, the table index
Y + offset spans [-226, 480] -- five entries lower and five higher than the limited window [-221, 475] the ingest kernels' tables were
once dimensioned for.  Then the binding's constant and struct, the .y4m range token, and the descriptor's refusals through a stand-alone
program (tests/ingest_check.cpp, built with the address and undefined-behaviour sanitizers by tests/ingest_host_kit.py, which also
holds the case writers, the answer reader and the texts every layout shares)."""
import ctypes
import os
import re

import numpy as np
import pytest

from avd_hip import _lib, sources
from tests import yuv_tables_reference as ref
from tests.ingest_host_kit import ARG, BGR, FULL, I420, NV12, OK, ROOT, T_MEM, UNSUPPORTED, parse, picture  # noqa: F401
from tests.ingest_host_kit import program as _lines  # noqa: F401

T_FORMAT = "bad avd_picture.format"
T_BGR_RANGE = "AVD_FMT_FULL_RANGE describes 4:2:0 samples: a BGR picture has no range"
T_ROTATE = "avd_picture.rotate must be 0 .. 3 quarter turns"
T_RESERVED = "avd_picture.reserved must be 0"


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def content():
    """50 x 38 (2 x 2 cells: 25 x 19 per frame, five frames of enumeration and one of random bytes) and 96 x 64"""
    return [ref.enum_planes(6, 38, 50, seed=1), ref.enum_planes(3, 64, 96, seed=2)]


def test_the_content_holds_every_enumerated_triple(content):
    want = {tuple(c) for c in ref.enum_cells()}
    assert len(want) == 13 ** 3
    for y, uv in content:
        u = np.repeat(np.repeat(uv[..., 0::2], 2, axis=1), 2, axis=2)
        v = np.repeat(np.repeat(uv[..., 1::2], 2, axis=1), 2, axis=2)
        seen = set(zip(y.ravel().tolist(), u.ravel().tolist(), v.ravel().tolist()))
        assert want <= seen
        # one whole 2 x 2 cell each: the first cell of the first frame is (0, 0, 0), four luma samples over one chroma pair
        assert not y[0, :2, :2].any() and not uv[0, 0, :2].any()


def test_limited_range_is_the_pinned_converter(oracle, content):
    for y, uv in content:
        assert np.array_equal(ref.nv12_to_bgr(y, uv, False), oracle.nv12_to_bgr(y, uv))
    pinned = oracle.yuv2rgb_consts()
    assert {k: ref.consts(False)[k] for k in pinned} == pinned
    assert ref.index_window(False) == (-221, 475)


def test_full_range_gray_axis_is_the_identity():
    y = np.arange(256, dtype=np.uint8).reshape(2, 128)
    bgr = ref.nv12_to_bgr(y, np.full((1, 128), 128, np.uint8), True)
    for ch in range(3):
        assert np.array_equal(bgr[..., ch], y), ch


def test_full_range_constants_and_index_window():
    assert ref.consts(True) == dict(cy=65536, crv=91881, cbu=116129, cgu=-22552, cgv=-46800, c0=32768, kr=-179, kb=-226, kg=137)
    assert ref.offset_ranges(True) == {"R": (-179, 178), "B": (-226, 225), "G": (-134, 137)}
    assert ref.index_window(True) == (-226, 480)
    # every coefficient fits the 24-bit multiply of the kernels with an 8-bit sample
    assert all(abs(ref.consts(fr)[k]) < 1 << 17 for fr in (False, True) for k in ("cy", "crv", "cbu", "cgu", "cgv"))


def test_full_range_arithmetic_form_equals_the_tables(content):
    """value = clip8((c0 + (Y + off) * cy) >> 16) with the derived integers -- the form the kernels evaluate -- is the table lookup, on
    the enumerated content, for both ranges"""
    for full in (False, True):
        k = ref.consts(full)
        for y, uv in content:
            Y = y.astype(np.int64)
            U = np.repeat(np.repeat(uv[..., 0::2], 2, axis=1), 2, axis=2).astype(np.int64)
            V = np.repeat(np.repeat(uv[..., 1::2], 2, axis=1), 2, axis=2).astype(np.int64)
            off = [((U * k["cbu"]) >> 16) + k["kb"], ((U * k["cgu"]) >> 16) + ((V * k["cgv"]) >> 16) + k["kg"], ((V * k["crv"]) >> 16) + k["kr"]]
            got = np.stack([np.clip((k["c0"] + (Y + o) * k["cy"]) >> 16, 0, 255) for o in off], -1).astype(np.uint8)
            assert np.array_equal(got, ref.nv12_to_bgr(y, uv, full)), full


def test_full_range_differs_from_limited(content):
    y, uv = content[1]
    lim, full = ref.nv12_to_bgr(y, uv, False), ref.nv12_to_bgr(y, uv, True)
    on_axis = np.repeat(np.repeat((uv[..., 0::2] == 128) & (uv[..., 1::2] == 128), 2, axis=1), 2, axis=2)
    assert on_axis.sum() >= 4 * 13 and np.array_equal(full[on_axis], np.repeat(y[on_axis][:, None], 3, axis=1))
    assert np.count_nonzero(lim != full) > lim.size // 2
    # blacks below 16 and whites above 235 survive in full range and are clipped away in limited range
    assert full[on_axis].min() == 0 and full[on_axis].max() == 255
    assert not lim[on_axis & (y <= 16)].any() and (lim[on_axis & (y >= 240)] == 255).all()


# ---- the binding ----------------------------------------------------------------------------------------------------------------------------
def test_flag_value_and_struct_size():
    assert _lib.AVD_FMT_FULL_RANGE == 0x100
    assert ctypes.sizeof(_lib.AvdPicture) == 104
    hdr = open(os.path.join(ROOT, "include", "avd.h")).read()
    assert re.search(r"#define AVD_FMT_FULL_RANGE 0x100\b", hdr)


# ---- .y4m ---------------------------------------------------------------------------------------------------------------------------------------
def test_y4m_range_token_round_trip(tmp_path):
    y, uv = ref.enum_planes(3, 64, 96, seed=3)
    plain, full = str(tmp_path / "plain.y4m"), str(tmp_path / "full.y4m")
    sources.write_y4m(plain, y, uv, fps=(25, 1))
    sources.write_y4m(full, y, uv, fps=(25, 1), full_range=True)
    head = lambda p: open(p, "rb").readline()
    assert head(plain) == b"YUV4MPEG2 W96 H64 F25:1 Ip A1:1 C420jpeg\n"                      # as it always was
    assert head(full) == b"YUV4MPEG2 W96 H64 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n"
    assert sources.FrameSource.full_range is False
    src = sources.Y4mSource(plain)
    assert src.full_range is False and src.frame_count == 3
    for planar in (False, True):
        src = sources.Y4mSource(full, planar=planar)
        assert src.full_range is True and src.rotate == 0 and (src.width, src.height, src.frame_count) == (96, 64, 3)
        first = next(iter(src.sampled(1)))
        assert np.array_equal(first[0], y[0])
        src.close()
    # with a rotation, and the LIMITED spelling
    both = str(tmp_path / "both.y4m")
    sources.write_y4m(both, y, uv, rotate=90, full_range=True)
    src = sources.Y4mSource(both)
    assert (src.full_range, src.rotate) == (True, 1)
    data = open(full, "rb").read()
    limited = str(tmp_path / "limited.y4m")
    open(limited, "wb").write(data.replace(b"XCOLORRANGE=FULL", b"XCOLORRANGE=LIMITED", 1))
    assert sources.Y4mSource(limited).full_range is False
    bad = str(tmp_path / "bad.y4m")
    open(bad, "wb").write(data.replace(b"XCOLORRANGE=FULL", b"XCOLORRANGE=JPEG", 1))
    with pytest.raises(ValueError, match="XCOLORRANGE"):
        sources.Y4mSource(bad)
    assert sources.open_source(bad) is None                # == capture not opened


# ---- the descriptor, host side ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(_lines):
    def run(cases):
        """cases: [(format, rotate, reserved, mem)] of an otherwise valid picture (2 frames of 64 x 64, tight strides) ->
        [(status, why, format, full_range, rotate)], the last three as the IngestClip carries them (zeros where from_picture refused)"""
        got = [parse(g) for g in _lines([picture(fmt, mem=mem, n=2, h=64, w=64, rotate=rotate, reserved=reserved) for fmt, rotate, reserved, mem in cases])]
        return [(g["status"], g["why"], g["format"], g["full"], g["rotate"]) for g in got]
    return run


def test_descriptor_range_flag(program):
    cases = [
        # accepted: the flag leaves the clip, the layout stays in `format`
        ((NV12 | FULL, 0, 0, 0), (OK, "", NV12, 1, 0)),
        ((I420 | FULL, 3, 0, 1), (OK, "", I420, 1, 3)),
        ((NV12, 0, 0, 0), (OK, "", NV12, 0, 0)),
        ((I420, 2, 0, 0), (OK, "", I420, 0, 2)),
        ((BGR, 0, 0, 0), (OK, "", BGR, 0, 0)),
        # refused
        ((BGR | FULL, 0, 0, 0), (ARG, T_BGR_RANGE, 0, 0, 0)),
        ((3 | FULL, 0, 0, 0), (ARG, T_FORMAT, 0, 0, 0)),
        ((3, 0, 0, 0), (ARG, T_FORMAT, 0, 0, 0)),
        ((NV12 | 0x200, 0, 0, 0), (ARG, T_FORMAT, 0, 0, 0)),
        ((NV12 | FULL | 0x200, 0, 0, 0), (ARG, T_FORMAT, 0, 0, 0)),
        ((I420 | 0x10000, 0, 0, 0), (ARG, T_FORMAT, 0, 0, 0)),
        ((I420 | FULL | (1 << 30), 0, 0, 0), (ARG, T_FORMAT, 0, 0, 0)),
        ((-1, 0, 0, 0), (ARG, T_FORMAT, 0, 0, 0)),
        ((NV12 | FULL | -0x80000000, 0, 0, 0), (ARG, T_FORMAT, 0, 0, 0)),
        # the order: format and range before rotate, before reserved, before anything check_clip looks at
        ((BGR | FULL, 4, 1, 2), (ARG, T_BGR_RANGE, 0, 0, 0)),
        ((BGR | FULL, 1, 0, 0), (ARG, T_BGR_RANGE, 0, 0, 0)),               # not "a turned BGR picture"
        ((NV12 | 0x200, -1, 1, 2), (ARG, T_FORMAT, 0, 0, 0)),
        ((NV12 | FULL, 4, 1, 2), (ARG, T_ROTATE, 0, 0, 0)),
        ((I420 | FULL, 0, 1, 2), (ARG, T_RESERVED, 0, 0, 0)),
        ((I420 | FULL, 0, 0, 2), (ARG, T_MEM, I420, 1, 0)),                 # check_clip's, on the clip from_picture made
    ]
    got = program([c for c, _ in cases])
    for (c, want), g in zip(cases, got):
        assert g == want, (c, g)
