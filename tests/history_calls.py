"""The call table, the histories and the comparison of tests/test_gpu_history.py (the controls that need no GPU: tests/test_history_host.py).

A context's workspace (csrc/avd_internal.h: Workspace) only ever grows, resets some members when another grows, allocates others when a
call first needs them, and keeps the tables of the last four geometries.  The session-scoped `ctx` of tests/conftest.py therefore reaches
most tests with buffers that an earlier test has grown and filled.  Here every public ingest / analysis call is a table entry
`call(c, content) -> {name: ndarray}` that also returns the avd_debug_fetch buffers that exist after it, its results as the FIRST call of a
fresh context are the reference, and the same entry after any history must give the same bytes.

Two kinds of debug-buffer elements are left out of the comparison, because no call defines them (csrc/avd_fbfast.hip, k_fb_fast; csrc/avd_capi.hip, k_records):
  * default mode, "flow1" .. "flow3" of a FLAGGED pair: the workgroups of the fast level kernels leave such a pair as soon as any of them
    has flagged it, and the exact re-run works at those levels in the other flow buffer of the level -- what "flow<L>" shows of the pair
    is whatever the abandoned launches wrote.  "flow0" of the pair is the re-run's result and IS compared, as are all levels of an
    unflagged pair and every level in exact mode;
  * the pair across a clip boundary of a batch: the Farneback stage computes it in vain, the record kernel ignores it and nothing re-runs it.
"""
import functools
import os
import re
import typing

import numpy as np

import avd_hip
from avd_hip import AvdError, Pixels, _lib, synth
from tests import yuv422_reference as y422
from tests.content_families import families, pink, smooth, u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, F32 = np.uint8, np.float32


# ---- content ---------------------------------------------------------------------------------------------------------------------------
def _bgr(gray):
    return np.ascontiguousarray(np.repeat(np.asarray(gray)[..., None], 3, axis=-1))


def _family_pair(name, seed):
    return families()[name](np.random.default_rng(seed))


def other_content(x):
    """the same shapes, strides and allocations with every byte inverted: what history "same shape, other content" runs before each entry"""
    if isinstance(x, np.ndarray):
        return (255 - x).astype(np.uint8)
    if isinstance(x, Pixels):
        return Pixels(other_content(x.data), x.fmt)
    if isinstance(x, (tuple, list)):
        return type(x)(other_content(v) for v in x)
    return x


# the four 320 x 320 frames of the avd_farneback_pairs entries (tests/content_families.py): a static scene but for one small patch
# (border-sign criterion), the cut from it to a ramp (unflagged), the ramp against itself rolled (solver criterion).  Three consecutive
# pairs share frames, so the pairs of three families do not fit into four frames: the cut stands where a smooth pair would.  Which pair
# meets which criterion is asserted on the device (test_gpu_history.py::test_the_farneback_frames_meet_each_criterion_once).
FB_FLAGGED = np.array([True, False, True])


@functools.lru_cache(maxsize=None)
def fb_frames():
    return np.stack(_family_pair("static_local_change", 401) + _family_pair("ramp_roll", 101))


@functools.lru_cache(maxsize=None)
def clip96():
    """5 x 96 x 128 BGR: smooth translation, frame 2 a duplicate of frame 1, frame 3 = frame 2 but for one patch (a flagged pair: border sign)"""
    f = smooth(np.random.default_rng(77), 3.0, size=480)
    cut = lambda oy, ox: u8(f[80 + oy:80 + oy + 96, 80 + ox:80 + ox + 128])
    s0, s1, s2 = cut(0, 0), cut(1, 2), cut(3, 5)
    patch = s1.copy()
    patch[40:46, 60:70] = np.clip(patch[40:46, 60:70].astype(int) + 50, 0, 255).astype(np.uint8)
    return _bgr(np.stack([s0, s1, s1, patch, s2]))


@functools.lru_cache(maxsize=None)
def clip48():
    """3 x 48 x 64 BGR, smooth content: the clip of the entry points the issue's list does not name (and its 4:2:0 forms)"""
    return synth.make_clip(3, 48, 64, seed=48, dup_every=0)


@functools.lru_cache(maxsize=None)
def big_clip():
    """134 x 64 x 96 BGR cycled from 8 base frames: a static background with a moving patch, every pair flagged (border sign) -- 133 pairs,
    more than the 128 the Farneback scratch holds at first"""
    bg = u8(pink(np.random.default_rng(5), 1.2, size=480)[100:164, 100:196])
    base = []
    for k in range(8):
        b = bg.copy()
        b[10 + 5 * k:16 + 5 * k, 8 + 9 * k:18 + 9 * k] = 255 - b[10 + 5 * k:16 + 5 * k, 8 + 9 * k:18 + 9 * k]
        base.append(b)
    return _bgr(np.stack(base)[np.arange(134) % 8])


@functools.lru_cache(maxsize=None)
def white1080():
    return np.full((3, 1080, 1920, 3), 255, np.uint8)


@functools.lru_cache(maxsize=None)
def long_clip():
    """140 x 64 x 96 BGR cycled from 8 smooth frames (history "options": its 139 pairs grow the Farneback scratch)"""
    return synth.make_clip(8, 64, 96, seed=31, dup_every=0)[np.arange(140) % 8]


def _planes420(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, h, w), dtype=U8), rng.integers(0, 256, (n, h // 2, w), dtype=U8)


def arrange_rgb(bgr, fmt):
    """BGR frames -> the same pixels as AVD_FMT_RGBP (channels first, R, G, B) or AVD_FMT_BGRA32 (seeded fourth byte)"""
    if fmt == _lib.AVD_FMT_RGBP:
        return np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2))
    alpha = np.random.default_rng(bgr.shape[1] * 31 + bgr.shape[2]).integers(0, 256, bgr.shape[:3] + (1,), dtype=U8)
    return np.concatenate([bgr, alpha], axis=-1)


# ---- what a call returns ---------------------------------------------------------------------------------------------------------------
def _pre_debug(c, n):
    return {"area": c.debug_fetch("area", (n, 32, 32), U8), "small": c.debug_fetch("small", (n, 320, 320), U8)}


def _fb_debug(c, n, keep0, keep_low, pyr0=False):
    """polyK, pyrK (pyr0 only where it exists) of n frames and flowK of the pairs keep0 (level 0) / keep_low (levels 1 .. 3): bool[n - 1]"""
    out = {}
    for k in range(4):
        s = 320 >> k
        out[f"poly{k}"] = c.debug_fetch(f"poly{k}", (n, s, s, 5), F32)
        if k > 0 or pyr0:
            out[f"pyr{k}"] = c.debug_fetch(f"pyr{k}", (n, s, s), F32)
        out[f"flow{k}"] = np.ascontiguousarray(c.debug_fetch(f"flow{k}", (n - 1, 2, s, s), F32)[keep0 if k == 0 else keep_low])
    return out


def _pre_out(c, got):
    small, hsh, s, q = got
    return {"small320": small, "hash": hsh, "lap_sum": s, "lap_sumsq": q, **_pre_debug(c, len(s))}


def _rec_out(c, recs, exact):
    """recs: the record arrays of the call's clips.  The Farneback buffers hold the concatenation of the clips."""
    rec = np.concatenate(recs)
    n = len(rec)
    inside = np.ones(n - 1, bool)                           # pair p = (frame p, frame p + 1) lies inside a clip
    inside[np.cumsum([len(r) for r in recs])[:-1] - 1] = False
    unflagged = rec["reserved"][1:] == 0
    return {"records": rec, "rerun_pairs": np.array([c.get_option("rerun_pairs")], np.int32), **_pre_debug(c, n),
            **_fb_debug(c, n, inside, inside if exact else inside & unflagged)}


class _Options:
    """set options for one call and put back what they were, whatever happens"""

    def __init__(self, c, **values):
        self.c, self.values, self.old = c, values, {}

    def __enter__(self):
        for k, v in self.values.items():
            self.old[k] = self.c.get_option(k)
            self.c.set_option(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            self.c.set_option(k, v)


class Entry(typing.NamedTuple):
    name: str
    symbols: frozenset          # the C entry points the call goes through
    kind: str                   # "pre": an avd_preprocess_* call; "fb": avd_farneback_pairs; "rec": an avd_analyze_* call
    exact: bool                 # the Farneback stage runs the exact kernels (fb_mode 0)
    inputs: typing.Callable     # () -> the call's input (content 0), built once
    run: typing.Callable        # (c, input) -> {name: ndarray}
    bgr: typing.Callable        # input -> the BGR clips the oracle sees, one per clip of the call (fb: None)

    def call(self, c, content=0):
        x = self.inputs()
        return self.run(c, x if content == 0 else _other_cached(self.name))


@functools.lru_cache(maxsize=None)
def _other_cached(name):
    return other_content(BY_NAME[name].inputs())


TABLE = []


def _add(name, symbols, kind, inputs, run, bgr=None, exact=False):
    TABLE.append(Entry(name, frozenset(symbols.split()), kind, exact, functools.lru_cache(maxsize=None)(inputs), run, bgr))


# -- avd_preprocess_bgr at one geometry of each BGR kernel (tests/test_gpu_parity.py::GEOMS) -----------------------------------------------
for _name, (_n, _h, _w) in (("preprocess_bgr_scalar", (2, 67, 101)), ("preprocess_bgr_vec16", (3, 48, 64)), ("preprocess_bgr_staged", (2, 45, 832))):
    _add(_name, "avd_preprocess_bgr", "pre", functools.partial(synth.random_frames, _n, _h, _w, seed=_h * 7 + _w),
         lambda c, x: _pre_out(c, c.preprocess_bgr(x)), lambda x: [x])

# -- one preprocess call of each other ingest family --------------------------------------------------------------------------------------
_add("preprocess_nv12", "avd_preprocess_nv12", "pre", lambda: _planes420(2, 48, 64, 112),
     lambda c, x: _pre_out(c, c.preprocess_nv12(*x)), lambda x: [("nv12", x, False)])
_add("preprocess_i420", "avd_preprocess_i420", "pre", lambda: synth.nv12_to_i420(*_planes420(2, 34, 48, 82)),
     lambda c, x: _pre_out(c, c.preprocess_i420(*x)), lambda x: [("nv12", synth.i420_to_nv12(*x), False)])
# stored 64 x 48, displayed after one quarter turn clockwise 48 x 64
_add("preprocess_i420_rotate1", "avd_preprocess_picture", "pre", lambda: synth.nv12_to_i420(*_planes420(2, 64, 48, 113)),
     lambda c, x: _pre_out(c, c.preprocess_i420(*x, rotate=1)), lambda x: [("nv12", synth.rotate_planes(synth.i420_to_nv12(*x), 1), False)])
_add("preprocess_i420_full_range", "avd_preprocess_picture", "pre", lambda: synth.nv12_to_i420(*_planes420(2, 48, 64, 114)),
     lambda c, x: _pre_out(c, c.preprocess_i420(*x, full_range=True)), lambda x: [("nv12", synth.i420_to_nv12(*x), True)])
for _name, _fmt in (("preprocess_yuyv", y422.YUYV422), ("preprocess_nv16", y422.NV16)):
    _add(_name, "avd_preprocess_picture", "pre", functools.partial(lambda fmt: Pixels(y422.pack(fmt, *y422.random_planes(2, 45, 64, 500 + fmt)), fmt), _fmt),
         lambda c, x: _pre_out(c, c.preprocess_picture(x)), lambda x: [y422.clip_to_bgr(x.fmt, x.data, False)])
for _name, _fmt in (("preprocess_rgbp", _lib.AVD_FMT_RGBP), ("preprocess_bgra", _lib.AVD_FMT_BGRA32)):
    _add(_name, "avd_preprocess_picture", "pre", functools.partial(lambda fmt: Pixels(arrange_rgb(synth.random_frames(2, 48, 64, seed=600 + fmt), fmt), fmt), _fmt),
         lambda c, x: _pre_out(c, c.preprocess_picture(x)),
         lambda x: [np.ascontiguousarray(x.data.transpose(0, 2, 3, 1)[..., ::-1] if x.fmt == _lib.AVD_FMT_RGBP else x.data[..., :3])])
# separately allocated frames: every frame an array of its own
_add("preprocess_frame_list", "avd_preprocess_frame_list", "pre", lambda: [np.array(f) for f in synth.random_frames(3, 67, 101, seed=700)],
     lambda c, x: _pre_out(c, c.preprocess_frame_list(x, _lib.AVD_FMT_BGR24)), lambda x: [np.stack(x)])


# -- avd_farneback_pairs on four 320 x 320 frames -----------------------------------------------------------------------------------------
def _fb_run(want_flow, exact, **options):
    def run(c, x):
        with _Options(c, **options):
            got = c.farneback_pairs(x, want_flow=want_flow)
            every = np.ones(len(x) - 1, bool)
            out = {"flow_mean": got[0], "flow_var": got[1], "rerun_pairs": np.array([c.get_option("rerun_pairs")], np.int32),
                   **_fb_debug(c, len(x), every, every if exact else ~FB_FLAGGED, pyr0=options.get("fb_fold_blur") == 0)}
            if want_flow:
                out["flow"] = got[2]
            return out
    return run


_add("farneback_default", "avd_farneback_pairs", "fb", fb_frames, _fb_run(False, False))
_add("farneback_default_flow", "avd_farneback_pairs", "fb", fb_frames, _fb_run(True, False))
_add("farneback_exact_fused", "avd_farneback_pairs", "fb", fb_frames, _fb_run(True, True, fb_mode=0, fb_fused=0xF), exact=True)
_add("farneback_exact_two_kernel_pyr0", "avd_farneback_pairs", "fb", fb_frames, _fb_run(True, True, fb_mode=0, fb_fused=0x0, fb_fold_blur=0), exact=True)


# -- the avd_analyze_* entry points ---------------------------------------------------------------------------------------------------------
def _async(c, n, submit):
    rec = np.zeros(n, avd_hip.RECORD_DTYPE)
    keep = submit(rec)
    c.synchronize()
    del keep
    return rec


def _exact(run):
    def wrapped(c, x):
        with _Options(c, fb_mode=0):
            return run(c, x)
    return wrapped


_add("analyze_frames_default", "avd_analyze_frames", "rec", clip96, lambda c, x: _rec_out(c, [c.analyze_frames(x)], False), lambda x: [x])
_add("analyze_frames_exact", "avd_analyze_frames", "rec", clip96, _exact(lambda c, x: _rec_out(c, [c.analyze_frames(x)], True)), lambda x: [x], exact=True)
_add("analyze_frames_async", "avd_analyze_frames_async", "rec", clip96,
     lambda c, x: _rec_out(c, [_async(c, len(x), lambda rec: c.analyze_frames_async(x, rec))], False), lambda x: [x])


def _nv12_of(bgr):
    return synth.bgr_to_nv12(bgr)


def _split(rec, clips_n):
    return list(np.split(rec, np.cumsum(clips_n)[:-1]))


# three clips, two geometries, the last one NV12
_batch_in = lambda: [clip48(), np.ascontiguousarray(clip96()[1:4]), _nv12_of(synth.make_clip(3, 48, 64, seed=49, dup_every=0))]
_batch_bgr = lambda x: [x[0], x[1], ("nv12", x[2], False)]
_add("analyze_batch", "avd_analyze_batch", "rec", _batch_in, lambda c, x: _rec_out(c, c.analyze_batch(x), False), _batch_bgr)
_add("analyze_batch_async", "avd_analyze_batch_async", "rec", _batch_in,
     lambda c, x: _rec_out(c, _split(_async(c, 9, lambda rec: c.analyze_batch_async(x, rec)), [3, 3, 3]), False), _batch_bgr)
# more geometries in ONE call than the context caches (kGeomCache = 4): the first pass over the clips evicts what it has just built
_five_in = lambda: [synth.random_frames(2, h, w, seed=h * 5 + w) for h, w in ((48, 64), (64, 48), (34, 48), (45, 64), (33, 40))]
_add("analyze_batch_five_geometries", "avd_analyze_batch", "rec", _five_in, lambda c, x: _rec_out(c, c.analyze_batch(x), False), lambda x: list(x))
# two formats, one rotation: I420 stored 64 x 48 and turned once, YUYV 45 x 64
_pic_in = lambda: [synth.nv12_to_i420(*synth.rotate_planes(_nv12_of(clip48()), 3)), Pixels(y422.pack(y422.YUYV422, *y422.random_planes(3, 45, 64, 801)), y422.YUYV422)]
_pic_bgr = lambda x: [("nv12", synth.rotate_planes(synth.i420_to_nv12(*x[0]), 1), False), y422.clip_to_bgr(x[1].fmt, x[1].data, False)]
_add("analyze_pictures", "avd_analyze_pictures", "rec", _pic_in, lambda c, x: _rec_out(c, c.analyze_pictures(x, [1, 0]), False), _pic_bgr)
_add("analyze_pictures_async", "avd_analyze_pictures_async", "rec", _pic_in,
     lambda c, x: _rec_out(c, _split(_async(c, 6, lambda rec: c.analyze_pictures_async(x, rec, [1, 0])), [3, 3]), False), _pic_bgr)
# the entry points that name their format, and the frame lists
_nv12_in = lambda: _nv12_of(clip48())
_i420_in = lambda: synth.nv12_to_i420(*_nv12_of(clip48()))
_add("analyze_frames_nv12", "avd_analyze_frames_nv12", "rec", _nv12_in, lambda c, x: _rec_out(c, [c.analyze_frames_nv12(*x)], False), lambda x: [("nv12", x, False)])
_add("analyze_frames_nv12_async", "avd_analyze_frames_nv12_async", "rec", _nv12_in,
     lambda c, x: _rec_out(c, [_async(c, 3, lambda rec: c.analyze_frames_nv12_async(*x, rec))], False), lambda x: [("nv12", x, False)])
_add("analyze_frames_i420", "avd_analyze_frames_i420", "rec", _i420_in, lambda c, x: _rec_out(c, [c.analyze_frames_i420(*x)], False),
     lambda x: [("nv12", synth.i420_to_nv12(*x), False)])
_add("analyze_frames_i420_async", "avd_analyze_frames_i420_async", "rec", _i420_in,
     lambda c, x: _rec_out(c, [_async(c, 3, lambda rec: c.analyze_frames_i420_async(*x, rec))], False), lambda x: [("nv12", synth.i420_to_nv12(*x), False)])
_lists_in = lambda: [([np.array(f) for f in clip48()], _lib.AVD_FMT_BGR24), ([np.array(f) for f in clip96()[1:4]], _lib.AVD_FMT_BGR24)]
_lists_bgr = lambda x: [np.stack(frames) for frames, _ in x]
_add("analyze_frame_lists", "avd_analyze_frame_lists", "rec", _lists_in, lambda c, x: _rec_out(c, c.analyze_frame_lists(x), False), _lists_bgr)
_add("analyze_frame_lists_async", "avd_analyze_frame_lists_async", "rec", _lists_in,
     lambda c, x: _rec_out(c, _split(_async(c, 6, lambda rec: c.analyze_frame_lists_async(x, rec)), [3, 3]), False), _lists_bgr)

BY_NAME = {e.name: e for e in TABLE}
assert len(BY_NAME) == len(TABLE)


def declared_entry_points():
    """the avd_preprocess_*, avd_analyze_* and avd_farneback_pairs symbols that include/avd.h declares, the header it includes (avd_frame_list.h)
    among them; parsed as tests/test_host_and_abi.py parses the header"""
    names = set()
    for header in ("avd.h", "avd_frame_list.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        names |= set(re.findall(r"^\s*(?:int|void|int64_t|const char\*)\s+(avd_\w+)\s*\(", text, re.M))
    return {n for n in names if n.startswith(("avd_preprocess_", "avd_analyze_")) or n == "avd_farneback_pairs"}


def oracle_bgr(oracle, spec):
    """one clip as entry.bgr describes it -> the BGR frames the oracle sees: an array, or ("nv12", (y, uv), full_range)"""
    if isinstance(spec, tuple):
        _, (y, uv), full = spec
        from tests import yuv_tables_reference as ytr
        return ytr.nv12_to_bgr(y, uv, True) if full else oracle.nv12_to_bgr(y, uv)
    return spec


# ---- the comparison ------------------------------------------------------------------------------------------------------------------------
def differences(got, want):
    """-> what differs between two results of a call, [] if nothing: the same names (a missing or an extra buffer is a difference), and per
    name the same dtype, shape and BYTES (NaN payloads and the sign of zero count)"""
    bad = [f"{k}: missing" for k in want if k not in got] + [f"{k}: not in the reference" for k in got if k not in want]
    for k in want:
        if k not in got:
            continue
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype != b.dtype or a.shape != b.shape:
            bad.append(f"{k}: {a.dtype}{list(a.shape)} against {b.dtype}{list(b.shape)}")
            continue
        x, y = a.reshape(-1).view(U8), b.reshape(-1).view(U8)
        if not np.array_equal(x, y):
            where = np.nonzero(x != y)[0]
            bad.append(f"{k}: {len(where)} of {len(x)} bytes differ, the first at byte {int(where[0])} (element {int(where[0]) // max(a.dtype.itemsize, 1)})")
    return bad


# ---- histories: functions of a context, made of public calls only ---------------------------------------------------------------------------
def bigger(c):
    """-> its own records (they, too, must not depend on what ran before)"""
    rec = c.analyze_frames(big_clip())                      # leaves d_fbflags, d_rlist, the re-run scratch and h_rec.reserved non-zero; fb_cap 133
    out = {"records": rec, "rerun_pairs": np.array([c.get_option("rerun_pairs")], np.int32)}
    out["white_records"] = c.analyze_frames(white1080())    # host memory: grows d_stage, d_rowbuf, d_lap_part
    frames = [np.array(f) for f in big_clip()[:24]]         # separately allocated: grows the table of plane pointers
    out["list_records"] = c.analyze_frame_lists([(frames, _lib.AVD_FMT_BGR24)])[0]
    return out


def entry_geometries(e):
    """(h, w) of the pictures the entry's ingest sees, as displayed (none for avd_farneback_pairs)"""
    out = []
    for spec in (e.bgr(e.inputs()) if e.bgr else []):
        frames = spec[1][0] if isinstance(spec, tuple) else spec
        out.append((int(frames.shape[1]), int(frames.shape[2])))
    return list(dict.fromkeys(out))


def table_geometries():
    """every geometry of the table, in the order of its first use: (67, 101), (48, 64), (45, 832), (34, 48), (45, 64), (96, 128), (64, 48), (33, 40)"""
    return list(dict.fromkeys(g for e in TABLE for g in entry_geometries(e)))


def _misaligned(n, h, w, seed):
    """BGR frames uint8[n, h, w, 3] whose first byte lies one byte past an allocation's start"""
    buf = np.empty(n * h * w * 3 + 1, U8)
    view = buf[1:].reshape(n, h, w, 3)
    view[...] = synth.random_frames(n, h, w, seed=seed)
    assert view.ctypes.data % 16 != 0
    return view


def geometries(c):
    """every table geometry transposed (more than four others: the geometry cache is evicted), and the same (h, w) from a misaligned buffer
    (the same cache entry, another kernel)"""
    for h, w in table_geometries():
        c.preprocess_bgr(synth.random_frames(2, w, h, seed=h + w))
    c.preprocess_bgr(synth.random_frames(2, 33, 40, seed=5))
    for h, w in table_geometries():
        c.preprocess_bgr(_misaligned(2, h, w, seed=h * w))


def formats_before(c, e):
    """run immediately before entry e: the other layouts of the entry's own (h, w) -- full-range NV12, I420 turned three times, UYVY (4:2:0 needs
    even sizes, 4:2:2 an even width) -- so that the entry finds its geometry's tables and buffers as another format's kernels left them"""
    for h, w in entry_geometries(e):
        if h % 2 == 0 and w % 2 == 0:
            c.preprocess_nv12(*_planes420(2, h, w, h + w), full_range=True)
            c.preprocess_i420(*synth.nv12_to_i420(*_planes420(2, w, h, h * w)), rotate=3)       # stored w x h, displayed h x w
        if w % 2 == 0:
            c.preprocess_picture(Pixels(y422.pack(y422.UYVY422, *y422.random_planes(2, h, w, h + 3 * w)), y422.UYVY422))


def options(c):
    """the two-kernel exact path with the dense flow and pyr0 allocates d_pyr[0], d_vs, d_vs0 and d_flow_il; the long clip's growth resets them"""
    with _Options(c, fb_mode=0, fb_fused=0, fb_fold_blur=0):
        c.farneback_pairs(fb_frames()[:3], want_flow=True)
    c.analyze_frames(long_clip())


def released(c):
    bigger(c)
    c.release_workspace()


@functools.lru_cache(maxsize=None)
def _extension_inputs():
    rng = np.random.default_rng(7)
    return dict(vit_w=(rng.standard_normal((768, 768)) * 0.02).astype(F32), vit_b=(rng.standard_normal(768) * 0.1).astype(F32),
                vit_frames=synth.random_frames(2, 224, 224, seed=19), ln_x=rng.standard_normal((5, 768)).astype(F32),
                ln_g=rng.standard_normal(768).astype(F32), ln_b=rng.standard_normal(768).astype(F32),
                sm_x=(rng.standard_normal((3, 1000)) * 4).astype(F32), conv_x=rng.standard_normal((1, 9, 7, 32)).astype(F32),
                conv_w=(rng.standard_normal((64, 3, 3, 32)) * 0.1).astype(F32), conv_b=rng.standard_normal(64).astype(F32),
                wav=(np.sin(np.arange(16000) * 0.05) * 0.3 + rng.standard_normal(16000) * 0.05).astype(F32))


def extensions(c):
    """ViT patch embedding of 2 frames, LayerNorm 5 x 768, softmax 3 x 1000, one convolution, one second of audio -> their results"""
    m = _extension_inputs()
    c.vit_set_weights(m["vit_w"], m["vit_b"])
    return {"vit_tokens": c.vit_patch_embed(m["vit_frames"])[0], "layernorm": c.layernorm(m["ln_x"], m["ln_g"], m["ln_b"])[0],
            "softmax": c.softmax(m["sm_x"])[0], "cnn_conv": c.cnn_conv(m["conv_x"], m["conv_w"], m["conv_b"]),
            "audio": c.audio_features(m["wav"], 8000)}


def refused(c):
    """calls that the argument checks refuse (ordinary error returns: nothing is launched)"""
    import pytest
    with pytest.raises(AvdError, match="status -4"):
        c.preprocess_bgr(np.zeros((1, 16, 16, 3), U8))                                   # below 32 x 32
    with pytest.raises(AvdError, match="status -4"):
        c.analyze_frames_nv12(np.zeros((2, 34, 35), U8), np.zeros((2, 17, 35), U8))      # an odd width of 4:2:0 input
    with pytest.raises(AvdError, match="status -4"):
        c.analyze_batch([clip48(), np.zeros((2, 16, 16, 3), U8)])                         # the last clip of a batch too small
    with pytest.raises(AvdError, match="status -1"):
        c.set_option("no_such_option", 1)


# run once on a fresh context, before the table
HISTORIES = {"bigger": bigger, "geometries": geometries, "options": options, "released": released, "extensions": extensions, "refused": refused}
# run immediately before every entry of the table
BEFORE_EACH = {"same shape, other content": lambda c, e: e.call(c, 1), "formats": formats_before}
