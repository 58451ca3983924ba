"""Stream slots without a GPU: the header's text (include/avd.h, options "stream_slot" / "stream_reset" / "stream_frames") and the streaming
logic of FrameAnalyzer with ``resident_carry`` (avd_hip/analyzer.py, _stream_resident), run against a context that only records its calls.

What the recording context pins:
  * with resident_carry no frame object reaches the library twice, and every chunk is submitted with analyze_frame_lists_async;
  * the slot is emptied and selected before the first chunk and slot 0 is restored afterwards -- also when the frame iterator raises,
    and then only after the chunk in flight has been drained;
  * the chunks hold the frames the default path's chunks hold (its prepended carry frame apart);
  * the default path makes exactly the calls it made before the parameters existed, and none of the stream helpers.
"""
import os
import re

import numpy as np
import pytest

from avd_hip import _lib
from avd_hip.analyzer import FrameAnalyzer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NV12 = _lib.AVD_FMT_NV12


# ---- the header -------------------------------------------------------------------------------------------------------------------------
def _options_block():
    text = open(os.path.join(ROOT, "include", "avd.h")).read()
    end = text.index("int avd_set_option(")
    return text[text.rindex("/*", 0, end):end]


def test_header_names_the_options_and_the_one_clip_rule():
    block = _options_block()
    for name in ('"stream_slot"', '"stream_reset"', '"stream_frames"'):
        assert name in block, name
    flat = re.sub(r"\s*\n \*\s*", " ", block)
    assert "stream_slot: one clip per call" in flat
    assert "more than one non-empty clip" in flat and "AVD_ERR_ARG" in flat
    assert "0 ... 8" in flat                                              # the accepted range of "stream_slot"
    assert "avd_release_workspace" in flat[flat.index('"stream_slot"'):]   # a slot is state, not scratch
    assert "read-only" in flat[flat.index('"stream_frames"') - 5:flat.index('"stream_frames"') + 40]


def test_header_declares_nothing_new():
    """the feature goes through avd_set_option / avd_get_option: no exported function and no ABI step"""
    text = open(os.path.join(ROOT, "include", "avd.h")).read()
    assert not re.search(r"\bavd_\w*stream_(slot|reset|frames)\w*\s*\(", text)
    assert re.search(r"#define\s+AVD_ABI_VERSION\s+3\b", text)


def test_binding_has_the_helpers():
    for name in ("stream_slot", "stream_reset", "stream_frames"):
        assert callable(getattr(_lib.Context, name))


# ---- the streaming logic ------------------------------------------------------------------------------------------------------------------
class Recorder:
    """what FrameAnalyzer needs of a Context; every call is appended to .calls, list calls with the identities of the frames' planes"""

    def __init__(self):
        self.calls = []
        self.pending = None
        self.slot = 0

    @staticmethod
    def _ids(lists):
        (frames, fmt), = lists
        return [tuple(id(p) for p in f) for f in frames]

    def stream_reset(self, slot=0):
        self.calls.append(("reset", slot))

    def stream_slot(self, slot=0):
        self.calls.append(("slot", slot))
        self.slot = slot

    def analyze_frame_lists(self, lists, rotates=None, full_ranges=None):
        ids = self._ids(lists)
        self.calls.append(("blocking", ids, self.slot))
        rec = np.zeros(len(ids), _lib.RECORD_DTYPE)
        rec["ham"] = np.arange(len(ids))
        return [rec]

    def analyze_frame_lists_async(self, lists, rec, rotates=None, full_ranges=None):
        assert self.pending is None, "a chunk was submitted while another one was in flight"
        ids = self._ids(lists)
        assert len(rec) == len(ids)
        self.calls.append(("async", ids, self.slot))
        self.pending = rec
        return [lists[0][0]], [len(ids)]

    def synchronize(self):
        self.calls.append(("sync",))
        if self.pending is not None:
            self.pending["ham"] = 7
            self.pending = None


def surfaces(n, h=4, w=6):
    return [(np.full((h, w), i, np.uint8), np.full((h // 2, w), 128, np.uint8)) for i in range(n)]


def planes_of(items):
    return [tuple(id(p) for p in it) for it in items]


@pytest.mark.parametrize("n,chunk", [(7, 3), (7, 2), (6, 3), (1, 5), (0, 4), (9, 64)])
def test_resident_passes_every_frame_once(n, chunk):
    items = surfaces(n)
    r = Recorder()
    rec = FrameAnalyzer(ctx=r, chunk=chunk).records_stream_nv12(iter(items), resident_carry=True)
    assert len(rec) == n and (rec["ham"] == 7).all()                          # every record came out of a drained chunk
    sent = [i for c in r.calls if c[0] == "async" for i in c[1]]
    assert sent == planes_of(items)                                          # every frame once, in order: none twice
    assert not [c for c in r.calls if c[0] == "blocking"]
    assert all(c[2] == 1 for c in r.calls if c[0] == "async")                # with the default slot selected
    # reset, then select, then the chunks; slot 0 last
    assert r.calls[:2] == [("reset", 1), ("slot", 1)]
    assert r.calls[-1] == ("slot", 0)
    kinds = [c[0] for c in r.calls[2:-1]]
    assert "reset" not in kinds and "slot" not in kinds
    # each chunk is drained before the next one is submitted
    for a, b in zip(kinds, kinds[1:]):
        assert not (a == "async" and b == "async")


@pytest.mark.parametrize("n,chunk", [(7, 3), (7, 2), (6, 3), (5, 5), (9, 4)])
def test_chunk_sizes_are_the_default_paths(n, chunk):
    items = surfaces(n)
    d, r = Recorder(), Recorder()
    FrameAnalyzer(ctx=d, chunk=chunk).records_stream_nv12(iter(items))
    FrameAnalyzer(ctx=r, chunk=chunk).records_stream_nv12(iter(items), resident_carry=True)
    default = [c[1] for c in d.calls if c[0] == "blocking"]
    own = [ids if k == 0 else ids[1:] for k, ids in enumerate(default)]      # behind the first chunk every list begins with the carry frame
    assert [c[1] for c in r.calls if c[0] == "async"] == own


def test_default_path_calls_are_unchanged():
    items = surfaces(7)
    p = planes_of(items)
    want = [("blocking", p[0:3], 0), ("blocking", p[2:6], 0), ("blocking", p[5:7], 0)]
    for kwargs in ({}, {"resident_carry": False}, {"slot": 3}):
        d = Recorder()
        rec = FrameAnalyzer(ctx=d, chunk=3).records_stream_nv12(iter(items), **kwargs)
        assert d.calls == want, kwargs                                       # no stream helper, no asynchronous call, no synchronize
        assert len(rec) == 7
    d = Recorder()
    FrameAnalyzer(ctx=d, chunk=3, slot=2, resident_carry=False).records_stream_nv12(iter(items))
    assert d.calls == want


def test_slot_and_default_come_from_the_analyzer_or_the_call():
    items = surfaces(3)
    r = Recorder()
    FrameAnalyzer(ctx=r, chunk=2, slot=4, resident_carry=True).records_stream_nv12(iter(items))
    assert r.calls[:2] == [("reset", 4), ("slot", 4)] and r.calls[-1] == ("slot", 0)
    r = Recorder()
    FrameAnalyzer(ctx=r, chunk=2, slot=4, resident_carry=True).records_stream_nv12(iter(items), slot=6)
    assert r.calls[:2] == [("reset", 6), ("slot", 6)]
    r = Recorder()
    FrameAnalyzer(ctx=r, chunk=2, resident_carry=True).records_stream_nv12(iter(items), resident_carry=False)
    assert [c[0] for c in r.calls] == ["blocking", "blocking"]


def test_one_frame_chunks_with_resident_carry():
    """chunk = 1 is a live stream's call; the default path keeps its minimum of two"""
    items = surfaces(3)
    r = Recorder()
    FrameAnalyzer(ctx=r, chunk=1).records_stream_nv12(iter(items), resident_carry=True)
    assert [len(c[1]) for c in r.calls if c[0] == "async"] == [1, 1, 1]


def test_slot_zero_is_restored_after_an_exception_in_the_iterator():
    items = surfaces(5)

    def broken():
        yield from items[:4]
        raise OSError("decoder failed")

    r = Recorder()
    with pytest.raises(OSError, match="decoder failed"):
        FrameAnalyzer(ctx=r, chunk=3).records_stream_nv12(broken(), resident_carry=True)
    assert r.calls[:2] == [("reset", 1), ("slot", 1)]
    assert r.calls[-1] == ("slot", 0)
    # the first chunk was in flight while the iterator raised: it is drained before slot 0 is selected
    assert [c[0] for c in r.calls[2:]] == ["async", "sync", "slot"]
    assert r.pending is None


@pytest.mark.parametrize("method,fmt,make", [
    ("records_stream", _lib.AVD_FMT_BGR24, lambda i: np.full((4, 6, 3), i, np.uint8)),
    ("records_stream_i420", _lib.AVD_FMT_I420, lambda i: (np.full((4, 6), i, np.uint8), np.zeros((2, 3), np.uint8), np.zeros((2, 3), np.uint8))),
    ("records_stream_i422", _lib.AVD_FMT_I422, lambda i: (np.full((4, 6), i, np.uint8), np.zeros((4, 3), np.uint8), np.zeros((4, 3), np.uint8))),
    ("records_stream_p010", _lib.AVD_FMT_P010, lambda i: (np.full((4, 6), i, np.uint16), np.zeros((2, 6), np.uint16))),
    ("records_stream_i010", _lib.AVD_FMT_I010, lambda i: (np.full((4, 6), i, np.uint16), np.zeros((2, 3), np.uint16), np.zeros((2, 3), np.uint16))),
])
def test_every_stream_method_takes_the_parameters(method, fmt, make):
    items = [make(i) for i in range(5)]
    r = Recorder()
    rec = getattr(FrameAnalyzer(ctx=r, chunk=2), method)(iter(items), slot=2, resident_carry=True)
    assert len(rec) == 5
    assert [len(c[1]) for c in r.calls if c[0] == "async"] == [2, 2, 1]
    assert r.calls[:2] == [("reset", 2), ("slot", 2)] and r.calls[-1] == ("slot", 0)


def test_dropin_reads_the_environment(monkeypatch):
    """app.analyzers.video.analyze: AVD_STREAM_CARRY=resident turns resident_carry on, unset leaves the analyzer's arguments as they were"""
    import contextlib
    from app.analyzers import video
    from avd_hip import analyzer as A

    made = []

    class Source:
        fps, width, height, frame_count, surface = 2.0, 6, 4, 3, "nv12"

        def sampled(self, step):
            return iter(surfaces(3))

        def close(self):
            pass

    class Pool:
        @contextlib.contextmanager
        def borrow(self, device):
            yield Recorder()

    class Analyzer(FrameAnalyzer):
        def __init__(self, **kw):
            made.append({k: v for k, v in kw.items() if k != "ctx"})
            super().__init__(**kw)

    monkeypatch.setattr(video._sources, "open_source", lambda path: Source())
    monkeypatch.setattr(A, "default_pool", lambda: Pool())
    monkeypatch.setattr(A, "FrameAnalyzer", Analyzer)
    monkeypatch.delenv("AVD_STREAM_CARRY", raising=False)
    video.analyze("x.y4m", {})
    monkeypatch.setenv("AVD_STREAM_CARRY", "resident")
    video.analyze("x.y4m", {})
    assert made == [{"chunk": 64}, {"chunk": 64, "resident_carry": True}]
