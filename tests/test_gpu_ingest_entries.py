"""Every public ingest entry point of the library behind the one argument check (csrc/avd_ingest_clip.h), and the one batch body behind every
avd_analyze_* entry.

1. The refusal table of tests/test_ingest_clip_host.py -- one row per fault, in the documented order of include/avd.h, plus the two-fault rows
   and the descriptor faults -- goes through EVERY C entry that takes the row's format, as raw ctypes calls: all of them return the row's
   status and leave the row's text in avd_last_error, and none of them launches anything ("ingest_plan" and "stage_bytes" stay what the valid
   call in front of the table left).
2. One batch of a BGR, an NV12 and a turned I420 clip of three geometries, the BGR clip in device memory one byte off a 16-byte boundary (the
   scalar kernel beside a table fill and a strip fill), through avd_analyze_pictures, avd_analyze_pictures_async + avd_synchronize and clip by
   clip through each format's own entry: byte-identical records, the same kernels."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import _lib, synth  # noqa: E402
from tests import test_ingest_clip_host as T  # noqa: E402
from tests.test_gpu_i420 import _device_view  # noqa: E402
from tests.test_nv12 import _planes  # noqa: E402

BGR, NV12, I420 = T.BGR, T.NV12, T.I420


# ---- 1: the refusal table ---------------------------------------------------------------------------------------------------------------------
def _ptr(v):
    return C.c_void_p(v) if v else None


def _leading(c):
    """the arguments of the format's own entry points up to the strides"""
    p, r, f = [_ptr(v) for v in c["planes"]], c["rows"], c["frames"]
    size = (c["mem"], c["n"], c["h"], c["w"])
    if c["fmt"] == BGR:
        return (p[0],) + size + (r[0], f[0])
    return tuple(p[:T.PLANES[c["fmt"]]]) + size + (r[0], r[1], f[0], f[1])


def _avd_clip(c):
    return _lib.AvdClip(c["planes"][0] or None, c["planes"][1] or None, c["mem"], c["n"], c["h"], c["w"], c["rows"][0], c["frames"][0], c["rows"][1],
                        c["frames"][1])


def _avd_picture(c):
    p = _lib.AvdPicture()
    p.struct_size, p.format, p.rotate, p.reserved = C.sizeof(_lib.AvdPicture) + c["size_delta"], c["fmt"], c["rotate"], c["reserved"]
    p.mem, p.n, p.h, p.w = c["mem"], c["n"], c["h"], c["w"]
    for i in range(3):
        p.plane[i], p.row_stride[i], p.frame_stride[i] = c["planes"][i] or None, c["rows"][i], c["frames"][i]
    return p


def _entries(L, fmt, descriptor_only=False):
    """-> [(name, call(H, clip dict, records pointer, small320 pointer) -> status)]: every C entry that takes a clip of this format"""
    own = {BGR: ("avd_preprocess_bgr", "avd_analyze_frames", "avd_analyze_frames_async"),
           NV12: ("avd_preprocess_nv12", "avd_analyze_frames_nv12", "avd_analyze_frames_nv12_async"),
           I420: ("avd_preprocess_i420", "avd_analyze_frames_i420", "avd_analyze_frames_i420_async")}[fmt]
    out = []
    if not descriptor_only:
        out.append((own[0], lambda H, c, rec, small: getattr(L, own[0])(H, *_leading(c), small, None, None, None)))
        for name in own[1:]:
            out.append((name, lambda H, c, rec, small, name=name: getattr(L, name)(H, *_leading(c), rec)))
        if fmt != I420:                                    # avd_clip holds BGR and NV12
            for name in ("avd_analyze_batch", "avd_analyze_batch_async"):
                out.append((name, lambda H, c, rec, small, name=name: getattr(L, name)(H, C.byref(_avd_clip(c)), 1, rec)))
    out.append(("avd_preprocess_picture", lambda H, c, rec, small: L.avd_preprocess_picture(H, C.byref(_avd_picture(c)), small, None, None, None)))
    for name in ("avd_analyze_pictures", "avd_analyze_pictures_async"):
        out.append((name, lambda H, c, rec, small, name=name: getattr(L, name)(H, C.byref(_avd_picture(c)), 1, rec)))
    return out


def refusal_rows():
    """-> [(tag, format, edit, (status, text), descriptor_only)]"""
    rows = []
    for fmt in (BGR, NV12, I420):
        rows += [(f"{T.NAMES[fmt]}-{name}", fmt, edit, expect, False) for name, edit, expect in T.single_faults(fmt)]
    rows += [(name, fmt, edit, expect, False) for name, fmt, edit, expect in T.MULTI_FAULTS]
    rows += [(name, fmt, edit, expect, True) for name, fmt, edit, expect in T.PICTURE_FAULTS]
    return rows


def run_refusal_table(ctx):
    """Every row through every entry -> [(tag, entry, status, text, (expected status, expected text))].  The planes are real host buffers of 2
    frames of 64 x 64, so a call that wrongly got past its check would read memory that exists."""
    y, uv = _planes(2, 64, 64, seed=5)
    _, u, v = synth.nv12_to_i420(y, uv)
    bgr = synth.random_frames(2, 64, 64, seed=6)
    real = {BGR: (bgr,), NV12: (y, uv), I420: (y, u, v)}
    rec = np.zeros(2, avd_hip.RECORD_DTYPE)
    small = np.empty((2, 320, 320), np.uint8)
    L, H = ctx._L, ctx._h
    results = []
    for tag, fmt, edit, expect, descriptor_only in refusal_rows():
        c = T.edited(fmt, edit)
        c["planes"] = [a.ctypes.data if p else 0 for a, p in zip(real[fmt], c["planes"])] + [0] * (3 - len(real[fmt]))
        for name, call in _entries(L, fmt, descriptor_only):
            if fmt == NV12 and tag == "nv12-null-plane-1" and name.startswith("avd_analyze_batch"):
                continue                                   # an avd_clip without uv is a BGR clip by the ABI-3 rule, not an NV12 clip with a fault
            status = call(H, c, rec.ctypes.data, small.ctypes.data)
            results.append((tag, name, status, L.avd_last_error(H).decode(), expect))
    return results


def test_every_entry_refuses_alike_and_launches_nothing(ctx):
    y, uv = _planes(2, 80, 96, seed=7)
    ctx.preprocess_nv12(y, uv)                             # the valid call in front of the table, of another geometry than the table's clips
    plan, staged = ctx.debug_fetch("ingest_plan", (8,), np.int32), ctx.stage_bytes()
    results = run_refusal_table(ctx)
    assert len({tag for tag, *_ in results}) == len(refusal_rows())
    wrong = []
    for tag, entry, status, text, expect in results:
        print(tag, entry, status, text)
        if (status, text) != expect:
            wrong.append((tag, entry, status, text, expect))
    assert not wrong, wrong
    assert np.array_equal(ctx.debug_fetch("ingest_plan", (8,), np.int32), plan) and ctx.stage_bytes() == staged      # nothing was launched or staged
    ctx.synchronize()                                      # and no asynchronous call is pending


# ---- 2: one batch of every format through the one body ---------------------------------------------------------------------------------------
P_KERNEL = 7
BGR_SCALAR, NV12_TABLES, I420_STRIP = 0, 4, 8


def _kernel(ctx):
    return int(ctx.debug_fetch("ingest_plan", (8,), np.int32)[P_KERNEL])


def test_a_mixed_batch_equals_its_clips_one_by_one(ctx):
    import torch
    bgr_host = synth.make_clip(3, 64, 80, seed=41, dup_every=2)
    view = _device_view(torch, bgr_host.reshape(3, 64, 240), (1, 0, False))               # device memory, base one byte off a 16-byte boundary
    bgr = view.as_strided((3, 64, 80, 3), (view.stride(0), view.stride(1), 3, 1), view.storage_offset())
    assert bgr.data_ptr() % 16 == 1
    nv = synth.bgr_to_nv12(synth.make_clip(2, 66, 96, seed=42, dup_every=0))
    p1 = synth.nv12_to_i420(*synth.bgr_to_nv12(synth.make_clip(4, 64, 64, seed=43, dup_every=3)))
    clips, turns, frames = [bgr, nv, p1], [0, 0, 1], [3, 2, 4]
    # clip by clip, each format's own entry (the turned clip: its own entry on the displayed planes, and the descriptor entry for its kernel)
    single, kernels = [], []
    single.append(ctx.analyze_frames(bgr))
    kernels.append(_kernel(ctx))
    assert single[0].tobytes() == ctx.analyze_frames(bgr_host).tobytes()
    single.append(ctx.analyze_frames_nv12(*nv))
    kernels.append(_kernel(ctx))
    single.append(ctx.analyze_pictures([p1], [1])[0])
    kernels.append(_kernel(ctx))
    assert single[2].tobytes() == ctx.analyze_frames_i420(*synth.rotate_planes(p1, 1)).tobytes()
    assert kernels == [BGR_SCALAR, NV12_TABLES, I420_STRIP], kernels
    assert [len(r) for r in single] == frames
    # the batch in its three rotations of the clip order: "ingest_plan" is the LAST clip's launch, so every clip is the last one once
    for first in range(3):
        order = [(first + i) % 3 for i in range(3)]
        want = np.concatenate([single[i] for i in order]).tobytes()
        got = ctx.analyze_pictures([clips[i] for i in order], [turns[i] for i in order])
        assert [len(r) for r in got] == [frames[i] for i in order]
        assert np.concatenate(got).tobytes() == want, order
        assert _kernel(ctx) == kernels[order[-1]], order
        rec = np.zeros(9, avd_hip.RECORD_DTYPE)
        keep, counts = ctx.analyze_pictures_async([clips[i] for i in order], rec, [turns[i] for i in order])
        ctx.synchronize()
        del keep
        assert counts == [frames[i] for i in order] and rec.tobytes() == want, order
        assert _kernel(ctx) == kernels[order[-1]], order
