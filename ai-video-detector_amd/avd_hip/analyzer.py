"""FrameAnalyzer: decoded BGR frames -> HIP kernels -> per-frame records -> result dict.

This is the frames-level boundary of the hot path: everything the
reference does per sampled frame between ``cap.retrieve()`` and ``timeline_ai.append``
(reference app/analyzers/video.py:36-57), batched over all sampled frames of a clip.
"""
from __future__ import annotations

import logging

import collections
import contextlib
import itertools
import os
import threading
from typing import Iterable, Iterator, Optional, Tuple

import numpy as np

from . import _lib
from .timeline import records_to_result

class ContextPool:
    """Bounded pool of avd contexts for a threaded service.

    Reference api.py:133 runs the analyzer on ``asyncio.to_thread`` workers (up to 32 threads in the default
    executor) and a context is not re-entrant, so every request borrows one for its duration.  A context holds
    about 1.5 GB of HBM scratch after a 120-frame 1080p clip, so the pool is bounded: at most ``max_contexts``
    exist per device (further requests wait for one -- three or four clips in flight already saturate the GPU,
    DESIGN.md 4.5), and only ``keep_warm`` idle ones keep their workspace; the others give it back
    (``avd_release_workspace``) and re-reserve it on their next use.
    """

    def __init__(self, max_contexts: Optional[int] = None, keep_warm: Optional[int] = None):
        self.max_contexts = max(1, int(max_contexts if max_contexts is not None else os.getenv("AVD_MAX_CONTEXTS", "4")))
        self.keep_warm = max(0, int(keep_warm if keep_warm is not None else os.getenv("AVD_WARM_CONTEXTS", "2")))
        self._cv = threading.Condition()
        self._warm = {}            # device -> idle contexts that still hold their workspace, most recently used last
        self._cold = {}            # device -> idle contexts whose workspace was given back
        self._count = {}           # device -> contexts created

    @contextlib.contextmanager
    def borrow(self, device: int = 0):
        ctx = self._take(device)
        try:
            yield ctx
        except BaseException:
            # the request failed on this context: before it goes back to the MOST recently used end of the warm list -- the next request's
            # pick -- its stream is probed.  A device error is sticky on a HIP stream: such a context is closed and its slot given back (the
            # pool creates a fresh one); an ordinary error (bad argument, unreadable file) leaves a healthy context, which is reused.
            if self._healthy(ctx):
                self._give(device, ctx)
            else:
                self._drop(device, ctx, "the borrower's call failed and the context's stream reports an error")
            raise
        else:
            self._give(device, ctx)

    @staticmethod
    def _healthy(ctx) -> bool:
        try:
            ctx.synchronize()
            return True
        except Exception:
            return False

    def _drop(self, device, ctx, why):
        logging.getLogger("avd_hip").warning("context dropped from the pool: %s", why)
        try:
            ctx.close()
        except Exception:
            pass
        with self._cv:
            self._count[device] = max(0, self._count.get(device, 0) - 1)
            self._cv.notify()

    def _take(self, device):
        with self._cv:
            while True:
                warm, cold = self._warm.setdefault(device, []), self._cold.setdefault(device, [])
                if warm:
                    return warm.pop()                      # the most recently used one
                if cold:
                    return cold.pop()
                if self._count.get(device, 0) < self.max_contexts:
                    self._count[device] = self._count.get(device, 0) + 1
                    break
                self._cv.wait()
        try:
            return _lib.Context(device)
        except BaseException:
            with self._cv:
                self._count[device] -= 1
                self._cv.notify()
            raise

    def _give(self, device, ctx):
        trim = []
        with self._cv:
            warm = self._warm.setdefault(device, [])
            warm.append(ctx)
            while len(warm) > self.keep_warm:
                trim.append(warm.pop(0))                   # least recently used
            if warm:
                self._cv.notify()
        for c in trim:                                     # outside the lock: this synchronises the context's stream
            try:
                c.release_workspace()
            except Exception as exc:                       # must not mask the request's own result (or exception) ...
                # ... but a context whose stream reports an error (sticky after a fault) must not be handed to the next request: it is
                # logged, closed and its slot given back, so the pool creates a fresh one instead
                self._drop(device, c, "release_workspace failed: %r" % (exc,))
                continue
            with self._cv:
                self._cold.setdefault(device, []).append(c)
                self._cv.notify()

    def stats(self, device: int = 0):
        with self._cv:
            return {"created": self._count.get(device, 0), "warm": len(self._warm.get(device, [])),
                    "cold": len(self._cold.get(device, []))}

    def close(self):
        with self._cv:
            ctxs = [c for d in (self._warm, self._cold) for lst in d.values() for c in lst]
            self._warm.clear()
            self._cold.clear()
            self._count.clear()
        for c in ctxs:
            c.close()


_pool = ContextPool()


def default_pool() -> ContextPool:
    return _pool


class FrameAnalyzer:
    """Frames -> records on ONE context.  Pass ``ctx`` (tests, batch jobs) or borrow one from a pool
    (``with default_pool().borrow(device) as ctx: FrameAnalyzer(ctx=ctx)...``), which is what the drop-in
    ``app.analyzers.video.analyze`` does per request."""

    def __init__(self, device: int = 0, chunk: int = 64, ctx: Optional["_lib.Context"] = None, slot: int = 1, resident_carry: bool = False):
        """slot, resident_carry: the defaults of the records_stream* methods (see _stream_resident)"""
        self._own = ctx is None
        self.ctx = ctx or _lib.Context(device)
        self.chunk = max(2, int(chunk))
        self.resident_chunk = max(1, int(chunk))      # with the carry frame on the device a chunk of ONE frame has a predecessor too
        self.slot = int(slot)
        self.resident_carry = bool(resident_carry)

    def close(self):
        if self._own and self.ctx is not None:
            self.ctx.close()
        self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- whole stack resident (numpy host array or torch-ROCm tensor) ----------------------
    def records(self, frames) -> np.ndarray:
        return self.ctx.analyze_frames(frames)

    def analyze(self, frames, meta: dict) -> dict:
        """frames: uint8[N,H,W,3] BGR, the SAMPLED frames of one clip in order."""
        n, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        rec = self.records(frames) if n else np.zeros(0, _lib.RECORD_DTYPE)
        return records_to_result(rec, h * w, meta.get("width") or w, meta.get("height") or h,
                                 meta.get("fps") or 0.0, meta.get("duration") or 0.0)

    # -- several clips in one call (avd_analyze_batch): any mix of geometries; short clips fill the GPU together -------
    def records_many(self, clips) -> list:
        """clips: sequence of uint8[N,H,W,3] BGR stacks (or (y, uv) NV12 plane pairs) -> list of record arrays."""
        return self.ctx.analyze_batch(list(clips))

    def analyze_many(self, clips, metas) -> list:
        """The batched form of ``analyze``: one result dict per clip, identical to analysing them one by one."""
        clips = list(clips)
        out = []
        for frames, meta, rec in zip(clips, metas, self.records_many(clips)):
            y = frames[0] if isinstance(frames, tuple) else frames
            h, w = int(y.shape[1]), int(y.shape[2])
            out.append(records_to_result(rec, h * w, meta.get("width") or w, meta.get("height") or h,
                                         meta.get("fps") or 0.0, meta.get("duration") or 0.0))
        return out

    # -- streaming: bounded host memory, one-frame halo between chunks ----------------------
    def _stream(self, items, flush) -> np.ndarray:
        """items: frames or surfaces in order; flush(list of items) -> their records (the format's own call).  Chunks of self.chunk items, each
        analysed behind the last item of the chunk before it (the flow / hash predecessor), whose record is dropped."""
        def records(buf, carry):
            return flush(buf) if carry is None else flush([carry] + buf)[1:]

        out = []
        buf = []
        carry = None
        for it in items:
            buf.append(it)
            if len(buf) >= self.chunk:
                out.append(records(buf, carry))
                carry, buf = buf[-1], []
        if buf:
            out.append(records(buf, carry))
        return np.concatenate(out) if out else np.zeros(0, _lib.RECORD_DTYPE)

    def _stream_resident(self, items, submit, slot: int) -> np.ndarray:
        """The same stream with the carry frame RESIDENT: stream slot `slot` of the context (include/avd.h, option "stream_slot") keeps the last
        frame of every chunk on the device, so no chunk carries a prepended frame -- nothing is staged, ingested or hashed twice and the
        caller's frame is free once its chunk is drained.  submit(list of items, rec) enqueues one chunk (its records land in rec when the
        context is drained) and returns what the library reads; the next chunk is pulled from `items` -- decoded -- while that one runs."""
        ctx = self.ctx
        out = []
        ctx.stream_reset(slot)
        ctx.stream_slot(slot)
        try:
            it = iter(items)
            buf = list(itertools.islice(it, self.resident_chunk))
            while buf:
                rec = np.zeros(len(buf), _lib.RECORD_DTYPE)
                keep = submit(buf, rec)                    # the chunk's arrays stay referenced (buf, keep) until it is drained
                nxt = list(itertools.islice(it, self.resident_chunk))
                ctx.synchronize()
                out.append(rec)
                del keep
                buf = nxt
        finally:
            # an exception of the iterator finds a chunk in flight: buf, keep and rec are alive up to here, and it is drained first
            try:
                ctx.synchronize()
            finally:
                ctx.stream_slot(0)
        return np.concatenate(out) if out else np.zeros(0, _lib.RECORD_DTYPE)

    def _stream_list(self, items, fmt, rotate=0, full_range=False, slot=None, resident_carry=None) -> np.ndarray:
        """records_stream* behind their argument checks: the default stream (_stream), or with resident_carry the resident one"""
        if not (self.resident_carry if resident_carry is None else resident_carry):
            return self._stream(items, lambda chunk: self._flush_list(chunk, fmt, rotate, full_range))
        return self._stream_resident(items, lambda chunk, rec: self._submit_list(chunk, rec, fmt, rotate, full_range),
                                     self.slot if slot is None else int(slot))

    # A chunk goes to the library as a LIST of frames (avd_frame_list): every frame is staged from where the decoder left it, nothing is
    # stacked first.  The carry frame between chunks is simply the first entry of the next list.
    def _flush_list(self, items, fmt, rotate=0, full_range=False) -> np.ndarray:
        return self.ctx.analyze_frame_lists([(self._list_frames(items, fmt), fmt)], [rotate], [full_range])[0]

    def _submit_list(self, items, rec, fmt, rotate=0, full_range=False):
        """_flush_list without the wait: enqueue only (analyze_frame_lists_async); -> what the library reads until the context is drained"""
        return self.ctx.analyze_frame_lists_async([(self._list_frames(items, fmt), fmt)], rec, [rotate], [full_range])[0]

    @staticmethod
    def _list_frames(items, fmt) -> list:
        single = fmt in _lib._PACKED or fmt == _lib.AVD_FMT_RGBP          # one array per frame: interleaved [H,W,C], or channels first [3,H,W]
        lead = 1 if fmt == _lib.AVD_FMT_RGBP else 0                       # axes in front of the rows
        frames = [(np.asarray(it),) if single else tuple(np.asarray(p) for p in it) for it in items]
        # Frames go through as they lie -- row-padded decoder frames included -- while plane by plane their rows are dense and all frames share
        # one row stride, which is what a list takes.  Only a chunk that breaks that rule is copied (every plane to tight rows).
        tail = (_lib._PACKED[fmt], 1) if fmt in _lib._PACKED else (2 if fmt in _lib._WIDE else 1,)      # byte strides behind the rows
        agree = all(p.ndim == lead + len(tail) + 1 and p.strides[lead + 1:] == tail and p.strides[lead] == q.strides[lead]
                    for f in frames for p, q in zip(f, frames[0]))
        if not agree:
            frames = [tuple(np.ascontiguousarray(p) for p in f) for f in frames]
        if single:
            frames = [f[0] for f in frames]
        return frames

    # slot, resident_carry (every records_stream* method; None: the analyzer's): resident_carry keeps the frame between two chunks on the device,
    # in stream slot `slot` of the context, instead of prepending it to the next chunk (_stream_resident); the records are the same
    def records_stream(self, frames: Iterable[np.ndarray], fmt: int = _lib.AVD_FMT_BGR24, slot: Optional[int] = None,
                       resident_carry: Optional[bool] = None) -> np.ndarray:
        """fmt: the layout of the frames -- AVD_FMT_BGR24 (default) or AVD_FMT_RGB24 uint8[H,W,3], AVD_FMT_BGRA32 / AVD_FMT_RGBA32 uint8[H,W,4],
        AVD_FMT_RGBP uint8[3,H,W], AVD_FMT_YUYV422 / AVD_FMT_UYVY422 uint8[H,W,2] (limited range)."""
        if fmt not in _lib._PACKED and fmt != _lib.AVD_FMT_RGBP:
            raise ValueError(f"records_stream takes one array per frame: a packed layout or AVD_FMT_RGBP, got fmt {fmt!r}")
        return self._stream_list(frames, fmt, slot=slot, resident_carry=resident_carry)

    # -- the same for decoder surfaces: an iterable of (y uint8[H,W], uv uint8[H/2,W]) pairs ----------------
    # rotate: quarter turns clockwise from the stored pictures to the displayed one (a container's display rotation; include/avd.h, avd_picture)
    # full_range: the samples use 0 .. 255 (ffmpeg's J formats; AVD_FMT_FULL_RANGE)
    def records_stream_nv12(self, surfaces, rotate: int = 0, full_range: bool = False, slot: Optional[int] = None,
                            resident_carry: Optional[bool] = None) -> np.ndarray:
        return self._stream_list(surfaces, _lib.AVD_FMT_NV12, rotate, full_range, slot, resident_carry)

    # -- and for planar pictures (software decoders, .y4m): an iterable of (y uint8[H,W], u uint8[H/2,W/2], v uint8[H/2,W/2]) triples ----
    def records_stream_i420(self, surfaces, rotate: int = 0, full_range: bool = False, slot: Optional[int] = None,
                            resident_carry: Optional[bool] = None) -> np.ndarray:
        return self._stream_list(surfaces, _lib.AVD_FMT_I420, rotate, full_range, slot, resident_carry)

    # -- 4:2:2 planar pictures (MJPEG, a C422 .y4m): an iterable of (y uint8[H,W], u uint8[H,W/2], v uint8[H,W/2]) triples; H may be odd.
    # A turned 4:2:2 picture is not on the path: the library refuses rotate != 0 (include/avd.h)
    def records_stream_i422(self, surfaces, rotate: int = 0, full_range: bool = False, slot: Optional[int] = None,
                            resident_carry: Optional[bool] = None) -> np.ndarray:
        return self._stream_list(surfaces, _lib.AVD_FMT_I422, rotate, full_range, slot, resident_carry)

    # -- 10-bit 4:2:0 in 16-bit words (include/avd.h): P010 surfaces (VCN / rocDecode), an iterable of (y uint16[H,W], uv uint16[H/2,W]) pairs with
    # the 10 bits in the high bits; yuv420p10le pictures (libavcodec), (y uint16[H,W], u uint16[H/2,W/2], v likewise) triples with them in the low
    # bits.  The words are narrowed where the fused pass loads them: neither a stacked nor a narrowed copy exists anywhere
    def records_stream_p010(self, surfaces, rotate: int = 0, full_range: bool = False, slot: Optional[int] = None,
                            resident_carry: Optional[bool] = None) -> np.ndarray:
        return self._stream_list(surfaces, _lib.AVD_FMT_P010, rotate, full_range, slot, resident_carry)

    def records_stream_i010(self, surfaces, rotate: int = 0, full_range: bool = False, slot: Optional[int] = None,
                            resident_carry: Optional[bool] = None) -> np.ndarray:
        return self._stream_list(surfaces, _lib.AVD_FMT_I010, rotate, full_range, slot, resident_carry)


class StreamMux:
    """Several live streams on ONE context, one call per round: stream i is clip position i of every call and continues stream slot i + 1
    (include/avd.h, option "stream_map"), so a round of K short chunks costs one Farneback launch sequence instead of K -- calls of 1 to 8
    frames are bound by their launches, not by pixels.  The records of each stream are those of its frames analysed as
    one clip.

        mux = StreamMux(chunk=4)
        per_stream = mux.run([(decoder_a, AVD_FMT_NV12), (decoder_b, AVD_FMT_I420, 1), (camera, AVD_FMT_BGR24)])
    """

    MAX_STREAMS = 8                                   # the context's stream slots

    def __init__(self, ctx: Optional["_lib.Context"] = None, chunk: int = 8, device: int = 0, group: Optional[bool] = None):
        """group: option "ingest_group" (include/avd.h) for the rounds of run() -- True: the streams of a round that share a geometry, layout and
        alignment are ingested by one launch instead of one each; False: a launch per stream; None (default): whatever the context is set to,
        and no call is made for it.  The records are the same either way.  run() restores the context's value behind its drain."""
        self._own = ctx is None
        self.ctx = ctx or _lib.Context(device)
        self.chunk = max(1, int(chunk))
        self.group = None if group is None else bool(group)

    def close(self):
        if self._own and self.ctx is not None:
            self.ctx.close()
        self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def run(self, streams) -> list:
        """streams: up to eight (items, fmt[, rotate[, full_range]]) -- items an iterable of frames (a packed layout or AVD_FMT_RGBP: one array
        per frame) or of plane tuples, as the records_stream* methods of FrameAnalyzer take them.  -> one record array per stream.
        Each round pulls up to `chunk` items from every stream that still has some and submits them as ONE asynchronous call; the next round is
        pulled -- decoded -- while that one runs.  A stream with nothing to give keeps its position as an empty list.  The slots used are
        emptied first and the map is cleared at the end, also when an iterator raises (then after the round in flight has been drained)."""
        specs = []
        for s in streams:
            s = tuple(s)
            if not 2 <= len(s) <= 4:
                raise ValueError("a stream is (items, fmt[, rotate[, full_range]])")
            specs.append((iter(s[0]), s[1], s[2] if len(s) > 2 else 0, bool(s[3]) if len(s) > 3 else False))
        if len(specs) > self.MAX_STREAMS:
            raise ValueError(f"at most {self.MAX_STREAMS} streams: a context has {self.MAX_STREAMS} stream slots")
        if not specs:
            return []
        ctx = self.ctx
        fmts, rotates, ranges = [s[1] for s in specs], [s[2] for s in specs], [s[3] for s in specs]
        out = [[] for _ in specs]

        def pull():
            return [list(itertools.islice(s[0], self.chunk)) for s in specs]

        for i in range(len(specs)):
            ctx.stream_reset(i + 1)
        ctx.stream_map({i: i + 1 for i in range(len(specs))})
        group_was = None
        try:
            if self.group is not None:
                group_was = ctx.get_option("ingest_group")
                ctx.set_option("ingest_group", int(self.group))
            bufs = pull()
            while any(bufs):
                rec = np.zeros(sum(len(b) for b in bufs), _lib.RECORD_DTYPE)
                lists = [(FrameAnalyzer._list_frames(b, f), f) for b, f in zip(bufs, fmts)]
                keep = ctx.analyze_frame_lists_async(lists, rec, rotates, ranges)      # the round's arrays stay referenced (bufs, keep) until it is drained
                nxt = pull()
                ctx.synchronize()
                at = 0
                for o, b in zip(out, bufs):
                    if b:
                        o.append(rec[at:at + len(b)])
                    at += len(b)
                del keep
                bufs = nxt
        finally:
            # an exception of an iterator finds a round in flight: bufs, keep and rec are alive up to here, and it is drained first
            try:
                ctx.synchronize()
            finally:
                try:
                    if group_was is not None:
                        ctx.set_option("ingest_group", group_was)
                finally:
                    ctx.stream_map(None)
        return [np.concatenate(o) if o else np.zeros(0, _lib.RECORD_DTYPE) for o in out]


class ClipsInFlight:
    """Throughput mode for a service that analyses many clips on one GPU: up to ``depth`` clips are in
    flight, each on its own avd context (stream + workspace).  40 % of a clip's GPU time is launches that
    cannot fill the chip (the coarse Farneback levels, ~60 launch gaps, the host tail); other clips'
    bandwidth-bound kernels fill those holes: +18 % frames/s with 2, +24 % with 3 clips in flight (MI355X,
    1080p).  Results come back in submission order and are bit-identical to one-at-a-time analysis.

        runner = ClipsInFlight(device=0, depth=3)
        for tag, rec in runner.run((name, frames) for name, frames in clips):
            ...
    """

    def __init__(self, device: int = 0, depth: int = 3):
        self.ctxs = [_lib.Context(device) for _ in range(max(1, int(depth)))]
        self._pending = collections.deque()          # (slot, tag, records buffer, frames kept alive)
        self._free = collections.deque(range(len(self.ctxs)))

    @property
    def full(self) -> bool:
        return not self._free

    def submit(self, frames, tag=None) -> None:
        """Enqueue one clip (uint8[N,H,W,3] BGR, host numpy or torch-ROCm tensor) and return at once."""
        if self.full:
            raise RuntimeError("ClipsInFlight.submit: all contexts busy, drain() first")
        slot = self._free.popleft()
        rec = np.zeros(int(frames.shape[0]), _lib.RECORD_DTYPE)
        # `keep` is the buffer the kernels actually read (the input itself, or a contiguous copy of it): it must
        # stay allocated until the clip has been drained, or torch's caching allocator may hand it out again
        keep = self.ctxs[slot].analyze_frames_async(frames, rec)
        self._pending.append((slot, tag, rec, (frames, keep)))

    def submit_batch(self, clips, tag=None) -> None:
        """Enqueue SEVERAL clips as one call of one context (avd_analyze_batch_async): their Farneback pairs run as one
        launch sequence.  drain() returns (tag, [records of clip 0, records of clip 1, ...])."""
        if self.full:
            raise RuntimeError("ClipsInFlight.submit_batch: all contexts busy, drain() first")
        clips = list(clips)
        slot = self._free.popleft()
        total = sum(int((c[0] if isinstance(c, tuple) else c).shape[0]) for c in clips)
        rec = np.zeros(total, _lib.RECORD_DTYPE)
        keep, counts = self.ctxs[slot].analyze_batch_async(clips, rec)
        self._pending.append((slot, tag, (rec, counts), (clips, keep)))

    def drain(self) -> Tuple[object, np.ndarray]:
        """Wait for the OLDEST clip (or batch) in flight -> (tag, records)."""
        slot, tag, rec, _frames = self._pending.popleft()
        self.ctxs[slot].synchronize()
        self._free.append(slot)
        if isinstance(rec, tuple):
            rec, counts = rec
            return tag, (list(np.split(rec, np.cumsum(counts)[:-1])) if counts else [])
        return tag, rec

    def run(self, clips: Iterable[Tuple[object, object]]) -> Iterator[Tuple[object, np.ndarray]]:
        for tag, frames in clips:
            if self.full:
                yield self.drain()
            self.submit(frames, tag)
        while self._pending:
            yield self.drain()


def analyze_frames(frames, meta: Optional[dict] = None, device: int = 0) -> dict:
    """Convenience wrapper: the frames-level analogue of reference ``video.analyze``."""
    with default_pool().borrow(device) as ctx:
        return FrameAnalyzer(ctx=ctx).analyze(frames, meta or {})
