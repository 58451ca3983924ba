"""Rotated decoder pictures, the host side: the C-ABI's descriptor family (avd_picture and its three entry points), the premise the
feature rests on -- the nearest-chroma conversion commutes with quarter turns of even-sized pictures, so "the call on the turned
planes" is also "the turned BGR frame" -- the test-data helper, the ``XAVD_ROTATE`` token of ``.y4m`` files and the binding's own
refusals.  No GPU is needed: the library is loaded, never given a context.  The kernels are checked in tests/test_gpu_rotate.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from avd_hip import _lib, sources, synth
from tests.test_nv12 import _planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICTURE_SYMBOLS = ("avd_preprocess_picture", "avd_analyze_pictures", "avd_analyze_pictures_async")
# every entry point of the library before the descriptor family (include/avd.h at ABI 3)
BEFORE = {
    "avd_abi_version", "avd_create", "avd_destroy", "avd_last_error", "avd_preprocess_bgr", "avd_farneback_pairs", "avd_analyze_frames",
    "avd_analyze_frames_async", "avd_synchronize", "avd_analyze_batch", "avd_analyze_batch_async", "avd_wait_stream",
    "avd_release_workspace", "avd_preprocess_nv12", "avd_analyze_frames_nv12", "avd_analyze_frames_nv12_async", "avd_preprocess_i420",
    "avd_analyze_frames_i420", "avd_analyze_frames_i420_async", "avd_vit_set_weights", "avd_vit_patch_embed", "avd_audio_features",
    "avd_layernorm", "avd_softmax", "avd_cnn_param_counts", "avd_cnn_set_weights", "avd_cnn_forward", "avd_cnn_conv", "avd_comm_unique_id",
    "avd_comm_init", "avd_allgather_records", "avd_allgather_last_records", "avd_timer_start", "avd_timer_stop", "avd_set_option",
    "avd_get_option", "avd_set_profiling", "avd_stage_ms", "avd_kernel_ms", "avd_debug_fetch",
}


def _header():
    return open(os.path.join(ROOT, "include", "avd.h")).read()


def test_the_library_the_header_and_the_binding_gain_exactly_the_three_entry_points():
    _lib.build()
    L = _lib.load()
    hdr = _header()
    declared = set(re.findall(r"^\s*(?:int|void|int64_t|const char\*)\s+(avd_\w+)\s*\(", hdr, re.M))
    assert declared - BEFORE == set(PICTURE_SYMBOLS) and BEFORE <= declared
    assert set(_lib.EXPORTS) - BEFORE == set(PICTURE_SYMBOLS) and BEFORE <= set(_lib.EXPORTS)
    for name in PICTURE_SYMBOLS:
        assert hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == (6 if name == "avd_preprocess_picture" else 4), name
    # ABI 3 stays, avd_clip keeps its layout, the strings earlier tests search for are still there
    assert L.avd_abi_version() == 3 and re.search(r"#define AVD_ABI_VERSION 3\b", hdr)
    fields = re.search(r"typedef struct avd_clip \{(.*?)\} avd_clip;", hdr, re.S).group(1)
    assert re.findall(r"\b(\w+)(?=[,;])", fields) == ["data", "uv", "mem", "n", "h", "w", "row_stride", "frame_stride", "uv_row_stride",
                                                       "uv_frame_stride"]
    assert ctypes.sizeof(_lib.AvdClip) == 64
    assert "5 i420_scalar, 6 i420_tables, 7 nv12_strip, 8 i420_strip" in hdr and '"ingest_rotate"' in hdr


def test_avd_picture_of_the_binding_is_the_header_struct():
    hdr = _header()
    fields = re.search(r"typedef struct avd_picture \{(.*?)\} avd_picture;", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"\b(\w+)(?:\[\d+\])?(?=[,;])", fields)
    assert names == ["struct_size", "format", "plane", "row_stride", "frame_stride", "mem", "n", "h", "w", "rotate", "reserved"]
    assert names == [f[0] for f in _lib.AvdPicture._fields_]
    # uint32 + int32, three pointers, 2 x 3 int64, six int32: no padding anywhere on an LP64 target
    assert ctypes.sizeof(_lib.AvdPicture) == 4 + 4 + 3 * 8 + 6 * 8 + 6 * 4 == 104
    assert _lib.AvdPicture.plane.offset == 8 and _lib.AvdPicture.row_stride.offset == 32 and _lib.AvdPicture.mem.offset == 80
    assert _lib.AvdPicture.rotate.offset == 96 and _lib.AvdPicture.reserved.offset == 100
    assert re.search(r"enum avd_format \{ AVD_FMT_BGR24 = 0, AVD_FMT_NV12 = 1, AVD_FMT_I420 = 2 \};", hdr)
    assert (_lib.AVD_FMT_BGR24, _lib.AVD_FMT_NV12, _lib.AVD_FMT_I420) == (0, 1, 2)


# ---- the premise ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
def test_the_conversion_commutes_with_quarter_turns(oracle, k):
    """swscale's nearest-chroma conversion of the turned planes IS the turned BGR frame (even sizes): np.rot90 of the oracle's BGR."""
    y, uv = _planes(2, 34, 48, seed=40 + k)
    ry, ruv = synth.rotate_planes((y, uv), k)
    assert ry.shape == ((2, 48, 34) if k & 1 else (2, 34, 48)) and ruv.shape == ((2, 24, 34) if k & 1 else (2, 17, 48))
    assert ry.flags.c_contiguous and ruv.flags.c_contiguous and ry.dtype == ruv.dtype == np.uint8
    assert np.array_equal(oracle.nv12_to_bgr(ry, ruv), np.rot90(oracle.nv12_to_bgr(y, uv), -k, axes=(1, 2)))
    # the definition, spelled out for the luma plane of a quarter turn: displayed[r][c] = stored[Hs-1-c][r] (k = 1), stored[c][Ws-1-r] (k = 3)
    if k == 1:
        assert ry[1, 5, 7] == y[1, 34 - 1 - 7, 5]
    if k == 3:
        assert ry[1, 5, 7] == y[1, 7, 48 - 1 - 5]


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_rotate_planes_round_trips_and_i420_agrees_with_nv12(k):
    y, uv = _planes(3, 34, 48, seed=50 + k)
    turned = synth.rotate_planes((y, uv), k)
    back = synth.rotate_planes(turned, (4 - k) % 4)
    assert np.array_equal(back[0], y) and np.array_equal(back[1], uv)
    planar = synth.rotate_planes(synth.nv12_to_i420(y, uv), k)
    assert len(planar) == 3 and all(p.flags.c_contiguous for p in planar)
    for a, b in zip(synth.i420_to_nv12(*planar), turned):
        assert np.array_equal(a, b)
    # one picture without the leading frame axis, as a source yields it
    one = synth.rotate_planes((y[1], uv[1]), k)
    assert np.array_equal(one[0], turned[0][1]) and np.array_equal(one[1], turned[1][1])
    one = synth.rotate_planes(tuple(p[1] for p in synth.nv12_to_i420(y, uv)), k)
    assert all(np.array_equal(a, b[1]) for a, b in zip(one, planar))


# ---- .y4m -----------------------------------------------------------------------------------------------------------------------------
def test_y4m_carries_the_rotation(tmp_path):
    y, uv = _planes(5, 34, 48, seed=9)
    path = str(tmp_path / "turned.y4m")
    sources.write_y4m(path, y, uv, fps=(25, 1), rotate=90)
    assert b" XAVD_ROTATE=90\n" in open(path, "rb").readline()
    for planar in (False, True):
        src = sources.open_source(path, planar=planar)
        assert isinstance(src, sources.Y4mSource) and src.rotate == 1
        assert (src.width, src.height, src.frame_count, src.fps) == (34, 48, 5, 25.0)        # the DISPLAYED picture: swapped
        got = list(src.sampled(2))
        assert len(got) == 3
        for planes, i in zip(got, (0, 2, 4)):                                                 # the STORED planes
            assert planes[0].shape == (34, 48) and np.array_equal(planes[0], y[i])
            if planar:
                assert np.array_equal(planes[1], uv[i][:, 0::2]) and np.array_equal(planes[2], uv[i][:, 1::2])
            else:
                assert np.array_equal(planes[1], uv[i])
        src.close()
    for deg, turns, size in ((180, 2, (48, 34)), (270, 3, (34, 48))):
        sources.write_y4m(path, y, uv, rotate=deg)
        src = sources.Y4mSource(path)
        assert src.rotate == turns and (src.width, src.height) == size
        src.close()
    # no token: no rotation, the file is byte for byte what it was before the token existed
    sources.write_y4m(path, y, uv, fps=(25, 1))
    assert open(path, "rb").readline() == b"YUV4MPEG2 W48 H34 F25:1 Ip A1:1 C420jpeg\n"
    src = sources.open_source(path)
    assert src.rotate == 0 and (src.width, src.height) == (48, 34)
    src.close()
    assert sources.FrameSource.rotate == 0 and sources.NpySource.rotate == 0
    # a value that is no quarter turn: the file does not open
    for bad in (45, 360, -90):
        sources.write_y4m(path, y, uv, rotate=bad)
        assert sources.open_source(path) is None
    head = open(path, "rb").read().replace(b"XAVD_ROTATE=-90", b"XAVD_ROTATE=left")
    open(path, "wb").write(head)
    assert sources.open_source(path) is None


# ---- the binding's own refusals ---------------------------------------------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def test_the_binding_refuses_without_touching_the_library():
    c = object.__new__(_lib.Context)                                   # no context, no device: the checks are the binding's own
    c._h, c._L = None, _NoLibrary()
    y, uv = _planes(2, 34, 48, seed=11)
    _, u, v = synth.nv12_to_i420(y, uv)
    rec = np.zeros(2, _lib.RECORD_DTYPE)
    for bad in (4, -1):
        for call in (lambda: c.preprocess_nv12(y, uv, rotate=bad), lambda: c.preprocess_i420(y, u, v, rotate=bad),
                     lambda: c.analyze_frames_nv12(y, uv, rotate=bad), lambda: c.analyze_frames_i420(y, u, v, rotate=bad),
                     lambda: c.analyze_frames_nv12_async(y, uv, rec, rotate=bad), lambda: c.analyze_frames_i420_async(y, u, v, rec, rotate=bad),
                     lambda: c.preprocess_picture((y, uv), bad), lambda: c.analyze_pictures([(y, u, v)], [bad])):
            with pytest.raises(ValueError, match="rotate must be 0, 1, 2 or 3"):
                call()
    import torch
    with pytest.raises(ValueError, match="all be numpy arrays or all torch tensors"):
        c.preprocess_i420(y, u, torch.from_numpy(v), rotate=1)
    with pytest.raises(ValueError, match="both planes must be numpy arrays or both torch tensors"):
        c.analyze_frames_nv12(y, torch.from_numpy(uv), rotate=3)
    wide = np.zeros((2, 17, 32), np.uint8)
    wide[..., :24] = v
    with pytest.raises(ValueError, match="same row and frame strides"):
        c.analyze_pictures([(y, u, wide[..., :24])], [2])
    with pytest.raises(ValueError, match="one rotation per clip"):
        c.analyze_pictures([(y, uv)], [1, 2])
    # what the binding hands over: the stored geometry, the rotation, the caller's header size
    p, n, keep = c._picture((y, u, v), 3)
    assert (p.struct_size, p.format, p.mem, p.n, p.h, p.w, p.rotate, p.reserved) == (104, _lib.AVD_FMT_I420, 0, 2, 34, 48, 3, 0) and n == 2
    assert list(p.plane) == [y.ctypes.data, u.ctypes.data, v.ctypes.data]
    assert list(p.row_stride) == [48, 24, 24] and list(p.frame_stride) == [34 * 48, 17 * 24, 17 * 24]
    p, n, keep = c._picture((y, uv), 1)
    assert (p.format, p.rotate) == (_lib.AVD_FMT_NV12, 1) and list(p.plane) == [y.ctypes.data, uv.ctypes.data, None]
    assert list(p.row_stride) == [48, 48, 0] and list(p.frame_stride) == [34 * 48, 17 * 48, 0]
    p, n, keep = c._picture(synth.random_frames(2, 40, 48, seed=3))
    assert (p.format, p.rotate, p.h, p.w) == (_lib.AVD_FMT_BGR24, 0, 40, 48) and list(p.row_stride) == [144, 0, 0]
