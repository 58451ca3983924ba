"""Option "stream_map" without a GPU: the header's text (include/avd.h), the binding's helpers, and avd_hip.StreamMux run against a context
that only records its calls (in the manner of tests/test_stream_host.py's Recorder).

What the recording context pins of StreamMux.run:
  * the slots used are emptied and position i is mapped to slot i + 1 before the first round;
  * one analyze_frame_lists_async per round, every position present, a finished stream as an empty list;
  * no plane object reaches the library twice;
  * the map is cleared after the drain -- also when an iterator raises, and then only after the round in flight has been drained;
  * streams of unequal length come back with the right lengths.
"""
import os
import re

import numpy as np
import pytest

import avd_hip
from avd_hip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NV12, I420, BGR = _lib.AVD_FMT_NV12, _lib.AVD_FMT_I420, _lib.AVD_FMT_BGR24


# ---- the header -------------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "avd.h")).read()


def _flat(block):
    return re.sub(r"\s*\n \*\s*", " ", block)


def _options_block():
    text = _header()
    end = text.index("int avd_set_option(")
    return _flat(text[text.rindex("/*", 0, end):end])


def test_header_names_the_option_its_encoding_and_its_refusals():
    flat = _options_block()
    at = flat.index('"stream_map":')                               # the option's own paragraph
    assert at > flat.index('"stream_frames"')                      # the new text stands behind the old
    rest = flat[at:]
    assert "(position << 4) | slot" in rest and "0 ... 63" in rest and "0 ... 8" in rest
    assert "-1 clears" in rest and "number of mapped positions" in rest
    assert 'begins "stream_map:"' in rest and "AVD_ERR_ARG" in rest
    assert "already mapped at another position" in rest
    assert 'while "stream_slot" is not 0' in rest
    assert "never hold at once" in rest
    assert "Positions >= 64 cannot be mapped" in rest
    assert "ONE launch" in rest
    assert "avd_preprocess_*" in rest and "avd_farneback_pairs" in rest
    # the sentence test_stream_host.py looks for is only added to
    assert "serves up to eight streams in turn" in flat


def test_header_names_the_debug_buffers_and_the_allgather_rule():
    text = _header()
    end = text.index("int64_t avd_debug_fetch(")
    fetch = _flat(text[text.rindex("/*", 0, end):end])
    assert '"stream_state" int32[8][2]' in fetch and '"stream_call" int32[4]' in fetch
    end = text.index("int avd_allgather_last_records(")
    gather = _flat(text[text.rindex("/*", 0, end):end])
    assert "AVD_ERR_UNSUPPORTED" in gather and '"stream_map"' in gather and "not compacted on the device" in gather
    rest = _options_block()
    assert "avd_allgather_last_records is refused" in rest and "AVD_ERR_UNSUPPORTED" in rest


def test_no_new_export_and_no_abi_step():
    text = _header()
    assert len(_lib.EXPORTS) == 43
    assert re.search(r"#define\s+AVD_ABI_VERSION\s+3\b", text)
    assert not re.search(r"\bavd_\w*stream_(map|state|call)\w*\s*\(", text)


def test_binding_has_the_helpers():
    for name in ("stream_map", "stream_state", "stream_call"):
        assert callable(getattr(_lib.Context, name))
    assert avd_hip.StreamMux is avd_hip.analyzer.StreamMux


class OptionLog:
    """a Context without a device: set_option is recorded"""

    def __init__(self, refuse=None):
        self.sets, self.refuse = [], refuse

    def set_option(self, name, value):
        self.sets.append((name, value))
        if value == self.refuse:
            raise _lib.AvdError("stream_map: refused")

    stream_map = _lib.Context.stream_map


def test_stream_map_helper_encodes_and_clears():
    c = OptionLog()
    c.stream_map({0: 2, 5: 1, 63: 8})
    assert c.sets == [("stream_map", -1), ("stream_map", 2), ("stream_map", (5 << 4) | 1), ("stream_map", (63 << 4) | 8)]
    for empty in (None, {}):
        c = OptionLog()
        c.stream_map(empty)
        assert c.sets == [("stream_map", -1)]
    for bad in ({64: 1}, {0: 0}, {0: 9}, {-1: 1}):
        c = OptionLog()
        with pytest.raises(ValueError, match="stream_map"):
            c.stream_map(bad)
        assert c.sets[-1] == ("stream_map", -1) and all(v == -1 for _, v in c.sets)
    c = OptionLog(refuse=(1 << 4) | 3)
    with pytest.raises(_lib.AvdError):
        c.stream_map({0: 1, 1: 3})
    assert c.sets == [("stream_map", -1), ("stream_map", 1), ("stream_map", (1 << 4) | 3), ("stream_map", -1)]      # a refused entry leaves no half map


# ---- StreamMux ------------------------------------------------------------------------------------------------------------------------------
class Recorder:
    """what StreamMux needs of a Context; every call is appended to .calls, list calls with the identities of the frames' planes per position"""

    def __init__(self):
        self.calls = []
        self.pending = None
        self.map = {}

    def stream_reset(self, slot=0):
        self.calls.append(("reset", slot))

    def stream_map(self, mapping=None):
        self.map = dict(mapping or {})
        self.calls.append(("map", dict(self.map)))

    def stream_slot(self, slot=0):
        raise AssertionError("StreamMux chooses slots through the map")

    def analyze_frame_lists(self, lists, rotates=None, full_ranges=None):
        raise AssertionError("StreamMux submits asynchronous calls only")

    def analyze_frame_lists_async(self, lists, rec, rotates=None, full_ranges=None):
        assert self.pending is None, "a round was submitted while another one was in flight"
        ids = [[tuple(id(p) for p in (f if isinstance(f, tuple) else (f,))) for f in frames] for frames, fmt in lists]
        assert len(rec) == sum(len(i) for i in ids)
        self.calls.append(("async", ids, [fmt for _, fmt in lists], list(rotates), list(full_ranges), dict(self.map)))
        self.pending = (rec, [len(i) for i in ids])
        return [frames for frames, _ in lists], [len(i) for i in ids]

    def synchronize(self):
        self.calls.append(("sync",))
        if self.pending is not None:
            rec, counts = self.pending
            rec["ham"] = np.repeat(np.arange(len(counts)), counts)          # every record names the position it was submitted at
            rec["lap_sum"] = 7
            self.pending = None


def surfaces(n, tag, h=4, w=6):
    return [(np.full((h, w), tag + i, np.uint8), np.full((h // 2, w), 128, np.uint8)) for i in range(n)]


def planes_of(items):
    return [tuple(id(p) for p in it) for it in items]


@pytest.mark.parametrize("lengths,chunk", [((7, 3, 5), 3), ((1, 1, 1, 1, 1, 1, 1, 1), 1), ((4, 0, 9), 4), ((5,), 8), ((2, 6), 2)])
def test_rounds_positions_and_lengths(lengths, chunk):
    items = [surfaces(n, 10 * i) for i, n in enumerate(lengths)]
    r = Recorder()
    out = avd_hip.StreamMux(ctx=r, chunk=chunk).run([(iter(it), NV12) for it in items])
    k = len(lengths)
    # the right lengths, every record out of a drained round and from its own position
    assert [len(o) for o in out] == list(lengths)
    for i, o in enumerate(out):
        assert o.dtype == _lib.RECORD_DTYPE and (o["lap_sum"] == 7).all() and (o["ham"] == i).all()
    # the slots are emptied and mapped before the first round; the map is cleared last
    assert r.calls[:k] == [("reset", i + 1) for i in range(k)]
    assert r.calls[k] == ("map", {i: i + 1 for i in range(k)})
    assert r.calls[-1] == ("map", {})
    body = r.calls[k + 1:-1]
    assert not [c for c in body if c[0] in ("reset", "map")]
    rounds = [c for c in body if c[0] == "async"]
    assert len(rounds) == max(-(-n // chunk) for n in lengths)              # one call per round
    for a, b in zip(body, body[1:]):
        assert not (a[0] == "async" and b[0] == "async")                    # each round is drained before the next one is submitted
    for rnd, c in enumerate(rounds):
        assert len(c[1]) == k and c[2] == [NV12] * k                        # every position present, in order
        assert c[5] == {i: i + 1 for i in range(k)}                         # submitted under the map
        for i, n in enumerate(lengths):
            assert c[1][i] == planes_of(items[i][rnd * chunk:(rnd + 1) * chunk])      # a finished stream: an empty list
    # no plane object is passed twice
    sent = [p for c in rounds for ids in c[1] for f in ids for p in f]
    assert len(sent) == len(set(sent)) == 2 * sum(lengths)


def test_formats_rotations_and_ranges_keep_their_positions():
    bgr = [np.full((4, 6, 3), i, np.uint8) for i in range(3)]
    i420 = [(np.full((4, 6), i, np.uint8), np.zeros((2, 3), np.uint8), np.zeros((2, 3), np.uint8)) for i in range(2)]
    r = Recorder()
    out = avd_hip.StreamMux(ctx=r, chunk=2).run([(bgr, BGR), (iter(i420), I420, 1), (surfaces(4, 0), NV12, 0, True)])
    assert [len(o) for o in out] == [3, 2, 4]
    for c in (c for c in r.calls if c[0] == "async"):
        assert c[2] == [BGR, I420, NV12] and c[3] == [0, 1, 0] and c[4] == [False, False, True]


def test_no_stream_no_call_and_too_many_streams():
    r = Recorder()
    assert avd_hip.StreamMux(ctx=r).run([]) == []
    assert r.calls == []
    with pytest.raises(ValueError, match="at most 8"):
        avd_hip.StreamMux(ctx=r).run([([], NV12)] * 9)
    with pytest.raises(ValueError):
        avd_hip.StreamMux(ctx=r).run([([],)])
    assert r.calls == []
    # streams that never give a frame: mapped, no round, cleared
    out = avd_hip.StreamMux(ctx=r).run([([], NV12), ([], NV12)])
    assert [len(o) for o in out] == [0, 0]
    assert [c[0] for c in r.calls] == ["reset", "reset", "map", "sync", "map"]


def test_the_map_is_cleared_after_an_exception_and_after_the_drain():
    good = surfaces(6, 0)
    bad_items = surfaces(4, 50)

    def broken():
        yield from bad_items
        raise OSError("decoder failed")

    r = Recorder()
    with pytest.raises(OSError, match="decoder failed"):
        avd_hip.StreamMux(ctx=r, chunk=3).run([(iter(good), NV12), (broken(), NV12)])
    # round 0 was in flight while the second stream's iterator raised: it is drained before the map is cleared
    assert [c[0] for c in r.calls] == ["reset", "reset", "map", "async", "sync", "map"]
    assert r.calls[-1] == ("map", {})
    assert r.pending is None


def test_frame_analyzer_knows_nothing_of_the_map():
    """the existing streaming paths make the calls they made (tests/test_stream_host.py pins them against its own recorder): none of them maps"""
    r = Recorder()
    r.stream_slot = lambda slot=0: r.calls.append(("slot", slot))
    r.analyze_frame_lists_async = lambda lists, rec, rotates=None, full_ranges=None: (r.calls.append(("async1", len(lists))), ([lists[0][0]], [len(rec)]))[1]
    avd_hip.FrameAnalyzer(ctx=r, chunk=2).records_stream_nv12(iter(surfaces(3, 0)), resident_carry=True)
    assert [c[0] for c in r.calls] == ["reset", "slot", "async1", "sync", "async1", "sync", "sync", "slot"]
    assert not [c for c in r.calls if c[0] == "map"]
