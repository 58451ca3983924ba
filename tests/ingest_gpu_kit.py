"""What the ingest GPU tests share (test_gpu_ingest_plan, _i420, _rotate, _fullrange, _rgb, _yuv422, _yuv10): the fields of the "ingest_plan"
debug buffer and the one check of a launch's plan, the oracle's reference tuple and the one bit-for-bit comparison with it, a descriptor
written out by hand, the heights that give every kind of last band.  No tolerance anywhere.  Each test file keeps its own kernel ids, plans,
shapes and seeds; what stays local there (the mixed batches, the per-layout frame lists) differs by more than a parameter."""
import ctypes

import numpy as np

from avd_hip import _lib

# "ingest_plan" (include/avd.h): h, w, rows_per_band, nbands, pitch, NI, dynamic LDS bytes, kernel (enum IngestKernel, avd_internal.h)
P_H, P_W, P_ROWS, P_NBANDS, P_PITCH, P_NI, P_LDS, P_KERNEL = range(8)
GRAY_TABLES = 3 * 4 * 704                      # the three conversion tables behind the tile (table fills and the strip fill), limited range


def plan(ctx):
    return [int(v) for v in ctx.debug_fetch("ingest_plan", (8,), np.int32)]


def check_plan(ctx, h, w, kernel, rows, ni=0, lds=None, *, lds_behind_tile=0, fmt=None, rotate=None, full_range=None):
    """The launch that just ran on ctx: h, w the DISPLAYED picture, the kernel id and the rows per band the case was written for, the NI class.
    lds: the exact dynamic LDS bytes where the case knows them; the lower bound (rows + 2) * pitch (+ lds_behind_tile) holds always.
    fmt / rotate / full_range: what the launch recorded of the clip, where the case says what it must be."""
    p = plan(ctx)
    tag = (fmt, h, w, rotate, full_range, p)
    assert p[P_KERNEL] == kernel, tag
    assert p[P_ROWS] == rows, tag
    assert (p[P_H], p[P_W]) == (h, w) and p[P_NBANDS] == -(-h // rows), tag
    assert p[P_NI] == ni, tag
    assert p[P_PITCH] % 16 == 0 and p[P_PITCH] >= w + 17, tag            # 16 B left of pixel 0, the halo byte right of pixel w - 1
    assert p[P_LDS] >= (rows + 2) * p[P_PITCH] + lds_behind_tile, tag
    if lds is not None:
        assert p[P_LDS] == lds, tag
    if fmt is not None:
        assert ctx.ingest_format() == fmt, tag
    if rotate is not None:
        assert ctx.ingest_rotate() == rotate, tag
    if full_range is not None:
        assert ctx.ingest_range() == int(full_range), tag
    return p


def reference(oracle, bgr):
    """(small320, hash, lap_sum, lap_sumsq, area) of the oracle on BGR frames"""
    area = np.stack([oracle.resize_area(oracle.bgr2gray(f), 32, 32) for f in bgr])
    return tuple(oracle.preprocess_bgr(bgr)) + (area,)


def check_outputs(ctx, got, want, tag):
    """got = (small320, hash, lap_sum, lap_sumsq) of the preprocess call that just ran on ctx; want = reference(...)"""
    n = len(want[4])
    area = ctx.debug_fetch("area", (n, 32, 32), np.uint8)
    for name, a, b in zip(("lap_sum", "lap_sumsq", "area", "small320", "hash"), (got[2], got[3], area, got[0], got[1]),
                          (want[2], want[3], want[4], want[0], want[1])):
        assert np.array_equal(a, b), (tag, name, int(np.count_nonzero(np.asarray(a) != np.asarray(b))))


def same_records(a, b, tag):
    for key in ("lap_sum", "lap_sumsq", "ham", "flow_mean", "flow_var"):
        assert np.array_equal(a[key], b[key]), (tag, key, a[key].tolist(), b[key].tolist())


def raw_picture_at(ctx, fmt, planes, mem, n, h, w, rows, frames, rotate=0):
    """avd_preprocess_picture on a descriptor written out by hand: plane addresses and strides exactly as given"""
    p = _lib.AvdPicture()
    p.struct_size, p.format, p.mem, p.n, p.h, p.w, p.rotate, p.reserved = ctypes.sizeof(p), fmt, mem, n, h, w, rotate, 0
    for i, a in enumerate(planes):
        p.plane[i], p.row_stride[i], p.frame_stride[i] = a, rows[i], frames[i]
    return ctx._outputs_call("avd_preprocess_picture", (ctypes.byref(p),), n)


def raw_picture(ctx, fmt, views, n, h, w, rotate=0, rows=None):
    """the same from uint8 device views: plane addresses and BYTE strides exactly as they are (rows: other row strides than the views')"""
    return raw_picture_at(ctx, fmt, [t.data_ptr() for t in views], 1, n, h, w, rows or [t.stride(1) for t in views], [t.stride(0) for t in views], rotate)


def heights(rows):
    """The smallest frames (above the 32-row minimum) in which a plan of `rows` rows per band has a one-row last band, a two-row last
    band (plans of more than two rows) and a full one."""
    first = lambda rem: next(h for h in range(33, 33 + rows) if h % rows == rem % rows)
    return tuple(dict.fromkeys(first(rem) for rem in ((1, 2, 0) if rows > 2 else (1, 0))))


def heights_even(rows):
    """4:2:0 needs even heights: plans of an odd number of rows get a one-row and a full last band, even plans a two-row and a full one."""
    first = lambda rem: next(h for h in range(34, 34 + 2 * rows, 2) if h % rows == rem % rows)
    return tuple(dict.fromkeys(first(rem) for rem in ((1, 0) if rows % 2 else (2, 0))))


assert [heights(r) for r in (14, 13, 9, 7, 3, 2, 1)] == [(43, 44, 42), (40, 41, 39), (37, 38, 36), (36, 37, 35), (34, 35, 33), (33, 34), (33,)]
assert [heights_even(r) for r in (14, 9, 8, 7, 5, 3, 2, 1)] == [(44, 42), (46, 36), (34, 40), (36, 42), (36, 40), (34, 36), (34,), (34,)]
