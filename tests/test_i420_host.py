"""Planar 4:2:0 (I420) input, the host side: the C-ABI's three new symbols, the planar ``.y4m`` source that hands out views of its memory
map, ``open_source``'s selection, the test-data helper and the binding's refusal of U and V planes with different strides.  No GPU is
needed: the library is loaded, never given a context.  The kernels are checked in tests/test_gpu_i420.py."""
import os
import re

import numpy as np
import pytest

from avd_hip import _lib, sources, synth
from tests.test_nv12 import _planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I420_SYMBOLS = ("avd_preprocess_i420", "avd_analyze_frames_i420", "avd_analyze_frames_i420_async")


def test_the_library_the_header_and_the_binding_gain_the_three_entry_points():
    _lib.build()
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "avd.h")).read()
    declared = set(re.findall(r"^\s*int\s+(avd_\w+)\s*\(", hdr, re.M))
    for name in I420_SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS and name in declared, name
        assert len(getattr(L, name).argtypes) == (16 if name == "avd_preprocess_i420" else 13), name
    assert L.avd_abi_version() == 3                                    # avd_clip and the records keep their layout
    assert re.search(r"#define AVD_ABI_VERSION 3\b", hdr)
    fields = re.search(r"typedef struct avd_clip \{(.*?)\} avd_clip;", hdr, re.S).group(1)
    assert re.findall(r"\b(\w+)(?=[,;])", fields) == ["data", "uv", "mem", "n", "h", "w", "row_stride", "frame_stride", "uv_row_stride",
                                                       "uv_frame_stride"]
    assert "5 i420_scalar, 6 i420_tables" in hdr and '"stage_bytes"' in hdr


def test_nv12_to_i420_round_trips():
    y, uv = _planes(3, 34, 48, seed=5)
    y2, u, v = synth.nv12_to_i420(y, uv)
    assert y2 is y and u.shape == v.shape == (3, 17, 24) and u.dtype == v.dtype == np.uint8
    assert u.flags.c_contiguous and v.flags.c_contiguous
    assert np.array_equal(u, uv[..., 0::2]) and np.array_equal(v, uv[..., 1::2])
    y3, uv3 = synth.i420_to_nv12(y2, u, v)
    assert np.array_equal(y3, y) and np.array_equal(uv3, uv)
    # one frame without the leading axis, as a source yields it
    _, u0, v0 = synth.nv12_to_i420(y[0], uv[0])
    assert np.array_equal(u0, u[0]) and np.array_equal(v0, v[0])


@pytest.fixture()
def y4m(tmp_path):
    y, uv = _planes(7, 34, 48, seed=9)
    path = str(tmp_path / "clip.y4m")
    sources.write_y4m(path, y, uv, fps=(25, 1))
    return path, y, uv


def test_planar_y4m_source_yields_views_of_the_map(y4m):
    path, y, uv = y4m
    nv = sources.Y4mSource(path)
    pl = sources.Y4mSource(path, planar=True)
    assert nv.surface == "nv12" and pl.surface == "i420"
    assert (pl.width, pl.height, pl.frame_count, pl.fps) == (48, 34, 7, 25.0)
    a, b = list(nv.sampled(3)), list(pl.sampled(3))                    # frames 0, 3, 6
    assert len(a) == len(b) == 3
    for (ny, nuv), planes, i in zip(a, b, (0, 3, 6)):
        assert len(planes) == 3
        py, pu, pv = planes
        assert py.shape == (34, 48) and pu.shape == pv.shape == (17, 24)
        assert np.array_equal(py, ny) and np.array_equal(py, y[i])
        assert np.array_equal(pu, nuv[:, 0::2]) and np.array_equal(pv, nuv[:, 1::2])
        assert np.array_equal(pu, uv[i][:, 0::2]) and np.array_equal(pv, uv[i][:, 1::2])
        for p in planes:                                               # no copy, no interleave: the planes ARE the file
            assert np.shares_memory(p, pl._map)
        # Y, U, V of a picture are adjacent in the file
        addr = [p.__array_interface__["data"][0] for p in planes]
        assert addr[1] - addr[0] == 34 * 48 and addr[2] - addr[1] == 17 * 24
    nv.close()
    pl.close()


def test_open_source_selects_the_surface(y4m, monkeypatch):
    path = y4m[0]
    monkeypatch.delenv("AVD_Y4M_SURFACE", raising=False)
    assert sources.open_source(path).surface == "nv12"                 # today's default stays
    assert sources.open_source(path, planar=True).surface == "i420"
    assert sources.open_source(path, planar=False).surface == "nv12"
    monkeypatch.setenv("AVD_Y4M_SURFACE", "i420")
    assert sources.open_source(path).surface == "i420"
    assert sources.open_source(path, planar=False).surface == "nv12"   # an explicit argument wins over the environment
    monkeypatch.setenv("AVD_Y4M_SURFACE", "nv12")
    assert sources.open_source(path).surface == "nv12"
    monkeypatch.setenv("AVD_Y4M_SURFACE", "planar")                    # anything but "i420"
    assert sources.open_source(path).surface == "nv12"
    assert isinstance(sources.open_source(path), sources.Y4mSource)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def test_the_binding_refuses_u_and_v_of_unequal_strides():
    c = object.__new__(_lib.Context)                                   # no context, no device: the check is the binding's own
    c._h, c._L = None, _NoLibrary()
    y, uv = _planes(2, 34, 48, seed=11)
    _, u, v = synth.nv12_to_i420(y, uv)
    wide = np.zeros((2, 17, 32), np.uint8)
    wide[..., :24] = v
    with pytest.raises(ValueError, match="same row and frame strides"):
        c._i420_ptrs(y, u, wide[..., :24])                             # V with a row pitch of 32, U of 24
    tall = np.zeros((2, 20, 24), np.uint8)
    tall[:, :17] = v
    with pytest.raises(ValueError, match="same row and frame strides"):
        c.preprocess_i420(y, u, tall[:, :17])                          # the same row pitch, another frame stride
    with pytest.raises(ValueError, match="chroma planes must be"):
        c.analyze_frames_i420(y, u, uv)
    import torch
    with pytest.raises(ValueError, match="all be numpy arrays or all torch tensors"):
        c._i420_ptrs(y, u, torch.from_numpy(v))
    # equal strides pass, strided views are handed over as they are
    pad_u, pad_v = np.zeros((2, 20, 32), np.uint8), np.zeros((2, 20, 32), np.uint8)
    pad_u[:, :17, :24], pad_v[:, :17, :24] = u, v
    out = c._i420_ptrs(y, pad_u[:, :17, :24], pad_v[:, :17, :24])
    assert out[:3] == (y.ctypes.data, pad_u.ctypes.data, pad_v.ctypes.data)
    assert out[3:11] == (_lib.AVD_MEM_HOST, 2, 34, 48, 48, 32, 34 * 48, 20 * 32)
