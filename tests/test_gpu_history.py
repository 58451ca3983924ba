"""A call's result must not depend on what its context ran before (the table, the histories and the comparison: tests/history_calls.py).

Nearly every other GPU test runs on the session-scoped `ctx`, whose workspace an earlier test has already grown and filled: a buffer reserved
too small passes there because it is big enough already, an element a kernel forgets to write because it still holds a plausible value.
Every context here is the test's own.

1. The reference of a table entry is the entry run as the FIRST call of a fresh context.  It is anchored once: preprocess outputs bit for
   bit to the oracle on the BGR frames of the format's pinned definition; exact-mode flows, statistics and records bit for bit to
   oracle.farneback / flow_stats; the default mode under the guarantee of include/avd.h with the checker of tests/holdout_families.py
   (flagged pairs bit for bit, the others rel 1e-6), its dense flow within the 1e-5 px of tests/test_gpu_fbfast.py.
2. Per history: a fresh context runs the history, then the whole table in order and again in reverse; every returned array -- results and
   avd_debug_fetch buffers -- equals the reference BYTE for byte.
3. The Farneback chunk boundary against the oracle: 515 frames of 320 x 320 are 514 pairs, more than the 512 the scratch ever holds
   (kFbChunkMax, csrc/avd_capi.hip), so the call runs as two chunks -- shown by the scratch, which afterwards holds the SECOND chunk: its
   first two flows are those of pairs 512 and 513.

No history has produced a mismatch so far.  That the comparison bites was checked once with a record kernel that left `reserved` unwritten
when it was zero and a dense-flow copy-out that ignored the chunk base: 24 of the tests here failed, the references against the oracle among
them.  On one MI355X a history takes 0.2 - 0.4 s (684 (entry, buffer) comparisons each; "grow in the middle" 804 in 0.6 s), a boundary
case 0.02 - 0.06 s, the file 7 s; every history prints its count and time (pytest -s).
"""
import hashlib
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from tests import history_calls as T  # noqa: E402
from tests import holdout_families as HF  # noqa: E402
from tests.content_families import families  # noqa: E402
from tests.test_host_and_abi import _records_from_oracle  # noqa: E402

U32 = np.uint32


class Refs:
    """each call as the first call of a fresh context, computed once and left unchanged"""

    def __init__(self):
        self._entry, self._other = {}, {}

    def entry(self, name):
        if name not in self._entry:
            with avd_hip.Context(0) as c:
                self._entry[name] = T.BY_NAME[name].call(c)
        return self._entry[name]

    def history(self, name):
        """what the histories that return something return on a fresh context"""
        if name not in self._other:
            with avd_hip.Context(0) as c:
                self._other[name] = T.HISTORIES[name](c)
        return self._other[name]


@pytest.fixture(scope="module")
def refs():
    return Refs()


_oracle_records = {}


def _want_records(oracle, bgr):
    key = hashlib.sha1(np.ascontiguousarray(bgr).tobytes()).hexdigest()
    if key not in _oracle_records:
        _oracle_records[key] = _records_from_oracle(oracle, bgr)
    return _oracle_records[key]


def _bits(a):
    return np.ascontiguousarray(a).view(U32)


@pytest.fixture(scope="module")
def fb_oracle(oracle):
    """the oracle on the four Farneback frames: the three flows, their statistics, and pyramid / polynomial expansion per level and frame"""
    f = T.fb_frames()
    flows = [oracle.farneback(f[p], f[p + 1]) for p in range(3)]
    stats = [oracle.flow_stats(x) for x in flows]
    ks = {0: (3, 0.0), 1: (3, 0.5), 2: (9, 1.5), 3: (19, 3.5)}           # tests/test_gpu_parity.py::test_farneback_stages_bit_exact
    pyr, poly = {}, {}
    for k in range(4):
        s = 320 >> k
        pyr[k] = np.stack([oracle.resize_linear_f32(oracle.gaussian_blur(x.astype(np.float32), *ks[k]), s, s) for x in f])
        poly[k] = np.stack([oracle.poly_exp(p) for p in pyr[k]])
    return flows, np.array([s[0] for s in stats], np.float32), np.array([s[1] for s in stats], np.float32), pyr, poly


# ---- 1: the references are right ---------------------------------------------------------------------------------------------------------
def test_the_farneback_frames_meet_each_criterion_once():
    """avd_frame_record.reserved of the four frames as a clip: the border-sign criterion, no flag, the solver's criterion"""
    with avd_hip.Context(0) as c:
        res = c.analyze_frames(T._bgr(T.fb_frames()))["reserved"][1:]
    assert np.array_equal(res != 0, T.FB_FLAGGED), [hex(int(v)) for v in res]
    assert res[0] & 0xF0 and res[2] & 0x0F and res[1] == 0, [hex(int(v)) for v in res]


@pytest.mark.parametrize("name", [e.name for e in T.TABLE if e.kind == "pre"])
def test_fresh_preprocess_equals_the_oracle(refs, oracle, name):
    e, ref = T.BY_NAME[name], refs.entry(name)
    (spec,) = e.bgr(e.inputs())
    bgr = T.oracle_bgr(oracle, spec)
    small, hsh, s, q = oracle.preprocess_bgr(bgr)
    area = np.stack([oracle.resize_area(oracle.bgr2gray(f), 32, 32) for f in bgr])
    want = {"small320": small, "hash": hsh, "lap_sum": s, "lap_sumsq": q, "area": area, "small": small}
    assert T.differences(ref, want) == []


@pytest.mark.parametrize("name", [e.name for e in T.TABLE if e.kind == "fb"])
def test_fresh_farneback_equals_the_oracle(refs, fb_oracle, name):
    e, ref = T.BY_NAME[name], refs.entry(name)
    flows, xm, xv, pyr, poly = fb_oracle
    for k in range(4):                                     # pyramid and polynomial expansion do not depend on the mode
        assert np.array_equal(_bits(ref[f"poly{k}"]), _bits(poly[k])), k
        if f"pyr{k}" in ref:
            assert np.array_equal(_bits(ref[f"pyr{k}"]), _bits(pyr[k])), k
    assert ("pyr0" in ref) == name.endswith("pyr0")
    planar = np.stack([x.transpose(2, 0, 1) for x in flows])
    if e.exact:
        assert ref["rerun_pairs"][0] == 0
        assert np.array_equal(_bits(ref["flow_mean"]), _bits(xm)) and np.array_equal(_bits(ref["flow_var"]), _bits(xv))
        assert np.array_equal(_bits(ref["flow"]), _bits(np.stack(flows)))
        assert np.array_equal(_bits(ref["flow0"]), _bits(planar))
    else:
        assert ref["rerun_pairs"][0] == int(T.FB_FLAGGED.sum())
        assert HF.check(ref["flow_mean"], ref["flow_var"], xm, xv, T.FB_FLAGGED) == []
        for p in range(3):                                 # the level-0 scratch holds the re-run's flow of a flagged pair
            for got in ([ref["flow"][p]] if "flow" in ref else []) + [ref["flow0"][p].transpose(1, 2, 0)]:
                if T.FB_FLAGGED[p]:
                    assert np.array_equal(_bits(got), _bits(flows[p])), p
                else:
                    assert float(np.abs(got - flows[p]).max()) <= HF.FLOW_TOL, p


@pytest.mark.parametrize("name", [e.name for e in T.TABLE if e.kind == "rec"])
def test_fresh_records_equal_the_oracle(refs, oracle, name):
    e, ref = T.BY_NAME[name], refs.entry(name)
    want = np.concatenate([_want_records(oracle, T.oracle_bgr(oracle, spec)) for spec in e.bgr(e.inputs())])
    got = ref["records"]
    assert ref["rerun_pairs"][0] == np.count_nonzero(got["reserved"])
    if e.exact:
        assert got.tobytes() == want.tobytes()             # `reserved` is 0 in exact mode, as in the oracle's records
    else:
        for key in ("lap_sum", "lap_sumsq", "ham"):
            assert np.array_equal(got[key], want[key]), key
        first = want["ham"] == -1
        assert not got["flow_mean"][first].any() and not got["flow_var"][first].any() and not got["reserved"][first].any()
        assert HF.check(got["flow_mean"][~first], got["flow_var"][~first], want["flow_mean"][~first], want["flow_var"][~first],
                        got["reserved"][~first] != 0) == []
    if name.startswith("analyze_frames_") and e.inputs() is T.clip96():
        assert got["ham"][2] == 0                          # the duplicated frame
        assert np.array_equal(got["reserved"] != 0, [False, False, False, not e.exact, False])      # one flagged pair, default mode only


# ---- 2: histories -------------------------------------------------------------------------------------------------------------------------
def _check(refs, c, e, where, before=None):
    if before:
        before(c, e)
    got = e.call(c)
    bad = T.differences(got, refs.entry(e.name))
    assert not bad, (where, e.name, bad)
    return len(got)


def _table_both_ways(refs, c, where, before=None):
    return sum(_check(refs, c, e, (where, direction), before)
               for direction, order in (("in order", T.TABLE), ("reversed", T.TABLE[::-1])) for e in order)


@pytest.mark.parametrize("name", list(T.HISTORIES) + list(T.BEFORE_EACH) + ["grow in the middle"])
def test_history(refs, name):
    for e in T.TABLE:                                      # the references first: no reference context is alive beside a history's
        refs.entry(e.name)
    t0 = time.perf_counter()
    if name == "grow in the middle":
        # entry, then the growth, then the entry again -- each on a context of its own, or only the first entry would see a growth
        want_big = refs.history("bigger")
        t0 = time.perf_counter()
        count = 0
        for e in T.TABLE:
            with avd_hip.Context(0) as c:
                count += _check(refs, c, e, "before the growth")
                bad = T.differences(T.bigger(c), want_big)
                assert not bad, ("the growing call itself", e.name, bad)
                count += len(want_big) + _check(refs, c, e, "after the growth")
    else:
        with avd_hip.Context(0) as c:
            if name in T.HISTORIES:
                T.HISTORIES[name](c)
            count = _table_both_ways(refs, c, name, T.BEFORE_EACH.get(name))
    print(f"\n[history] {name}: {count} (entry, buffer) comparisons, {time.perf_counter() - t0:.2f} s")


def test_the_extensions_after_a_bigger_call(refs):
    """the converse of history "extensions": the five extension calls after the growing calls give what they give on a fresh context"""
    want = refs.history("extensions")
    with avd_hip.Context(0) as c:
        T.bigger(c)
        assert T.differences(T.extensions(c), want) == []
        c.release_workspace()                              # the uploaded weights are state and stay
        assert T.differences(T.extensions(c), want) == []


# ---- 3: the Farneback chunk boundary against the oracle ---------------------------------------------------------------------------------
N_LONG = 515                 # 514 pairs > 512: two chunks, pairs 0 .. 511 and 512, 513
FLAGGED_TYPES = (3,)         # the stripes pair: asserted below on both sides of the boundary


class Boundary:
    """515 frames of 320 x 320 cycled from six base frames with stride 1: pair p is of type p % 6 -- 0 a smooth translation, 1 a bit-identical
    pair, 2 the cut to stripes, 3 stripes against themselves shifted (solver criterion), 4 the cut to white noise, 5 the cut back"""

    def __init__(self, oracle):
        fam = families()
        sa, sb = fam["smooth_shift"](np.random.default_rng(201))
        ta, tb = fam["stripes"](np.random.default_rng(301))
        self.base = np.stack([sa, sb, sb.copy(), ta, tb, np.random.default_rng(9).integers(0, 256, (320, 320), dtype=np.uint8)])
        self.idx = np.arange(N_LONG) % 6
        self.type = self.idx[:-1]
        self.frames = self.base[self.idx]
        self.clip = T._bgr(self.frames)
        self.flows = [oracle.farneback(self.base[t], self.base[(t + 1) % 6]) for t in range(6)]
        stats = [oracle.flow_stats(f) for f in self.flows]
        self.mean = np.array([s[0] for s in stats], np.float32)[self.type]
        self.var = np.array([s[1] for s in stats], np.float32)[self.type]
        small, hsh, s, q = oracle.preprocess_bgr(T._bgr(self.base))
        assert np.array_equal(small, self.base)
        want = np.zeros(N_LONG, avd_hip.RECORD_DTYPE)      # the oracle's records (reserved 0)
        want["lap_sum"], want["lap_sumsq"] = s[self.idx], q[self.idx]
        want["flow_mean"][1:], want["flow_var"][1:] = self.mean, self.var
        want["ham"][0] = -1
        want["ham"][1:] = np.array([int(np.sum(hsh[t] ^ hsh[(t + 1) % 6])) for t in range(6)])[self.type]
        self.records = want
        self.flagged = np.isin(self.type, FLAGGED_TYPES)

    def resident_chunk(self, c, exact, pairs=(512, 513)):
        """the scratch holds the call's LAST chunk: its first flows are those of `pairs` -- 512 and 513 after the 515 frames, not 0 and 1"""
        got = c.debug_fetch("flow0", (len(pairs), 2, 320, 320), np.float32)
        for i, p in enumerate(pairs):
            want = self.flows[self.type[p]].transpose(2, 0, 1)
            assert p == i or not np.array_equal(self.flows[self.type[p]], self.flows[self.type[i]])   # told apart from the first chunk's pairs
            if exact or self.flagged[p]:
                assert np.array_equal(_bits(got[i]), _bits(want)), p
            else:
                assert float(np.abs(got[i] - want).max()) <= HF.FLOW_TOL, p

    def check_default(self, rec):
        """the records of the clip's first len(rec) frames in default mode against the oracle's: the guarantee of include/avd.h, and the flag
        words by pair type"""
        want = self.records[:len(rec)]
        for key in ("lap_sum", "lap_sumsq", "ham"):
            assert np.array_equal(rec[key], want[key]), key
        assert rec["flow_mean"][0] == 0 and rec["flow_var"][0] == 0 and rec["reserved"][0] == 0
        fl = rec["reserved"][1:] != 0
        assert np.array_equal(fl, self.flagged[:len(rec) - 1]), np.nonzero(fl != self.flagged[:len(rec) - 1])[0][:8]
        assert HF.check(rec["flow_mean"][1:], rec["flow_var"][1:], want["flow_mean"][1:], want["flow_var"][1:], fl) == []


@pytest.fixture(scope="module")
def boundary(oracle):
    return Boundary(oracle)


@pytest.mark.parametrize("n,resident", [(515, (512, 513)), (514, (512,)), (513, (0, 1))], ids=["515-two-pairs-beyond", "514-one-pair-beyond", "513-one-full-chunk"])
def test_boundary_farneback_pairs_exact(boundary, n, resident):
    """the issue's 515 frames, and the two sizes next to the split: a second chunk of a single pair, and exactly the 512 pairs one chunk holds"""
    b = boundary
    with avd_hip.Context(0) as c:
        c.set_option("fb_mode", 0)
        fm, fv, flow = c.farneback_pairs(b.frames[:n], want_flow=True)
        b.resident_chunk(c, exact=True, pairs=resident)
    assert len(fm) == n - 1
    assert np.array_equal(_bits(fm), _bits(b.mean[:n - 1])) and np.array_equal(_bits(fv), _bits(b.var[:n - 1]))
    for p in range(n - 5, n - 1):                          # 515 frames: flows 510 .. 513
        assert np.array_equal(_bits(flow[p]), _bits(b.flows[b.type[p]])), p


def test_boundary_analyze_frames_exact(boundary):
    b = boundary
    with avd_hip.Context(0) as c:
        c.set_option("fb_mode", 0)
        c.set_profiling(True)
        rec = c.analyze_frames(b.clip)
        assert c.kernel_ms()["pyramid"] > 0                 # the region was recorded; the proof of the split is the resident second chunk
        b.resident_chunk(c, exact=True)
    assert rec["ham"][0] == -1
    assert rec[510:].tobytes() == b.records[510:].tobytes()
    assert rec.tobytes() == b.records.tobytes()            # all of them: equal pair types give equal records on both sides of pair 512


@pytest.mark.parametrize("how", ["blocking", "async"])
def test_boundary_analyze_frames_default(boundary, how):
    b = boundary
    with avd_hip.Context(0) as c:
        assert c.get_option("fb_mode") == 1 and c.get_option("fb_rerun") == 1
        if how == "blocking":
            rec = c.analyze_frames(b.clip)
        else:
            rec = np.zeros(N_LONG, avd_hip.RECORD_DTYPE)
            keep = c.analyze_frames_async(b.clip, rec)
            c.synchronize()
            del keep
        assert c.get_option("rerun_pairs") == int(b.flagged.sum())
        b.resident_chunk(c, exact=False)
    assert b.flagged[507] and rec["reserved"][508] != 0   # a flagged pair in the first chunk, next to the boundary ...
    assert b.flagged[513] and rec["reserved"][514] != 0   # ... and one in the second
    b.check_default(rec)


@pytest.mark.parametrize("mode", [1, 0], ids=["default", "exact"])
def test_boundary_batch_with_a_clip_boundary_on_frame_513(boundary, mode):
    """the pair the Farneback stage computes in vain across the two clips is pair 512, the first of the second chunk"""
    b = boundary
    clips = [b.clip[:513], b.clip[513:]]
    with avd_hip.Context(0) as c:
        c.set_option("fb_mode", mode)
        got = c.analyze_batch(clips)
    with avd_hip.Context(0) as c:
        c.set_option("fb_mode", mode)
        single = [c.analyze_frames(k) for k in clips]
    for g, s in zip(got, single):
        assert g.tobytes() == s.tobytes()
    # and through the single calls the oracle's: the second clip starts on base frame 513 % 6 = 3, its one pair is of type 3
    want_tail = np.zeros(2, avd_hip.RECORD_DTYPE)
    want_tail[:] = b.records[513:]
    want_tail["ham"][0], want_tail["flow_mean"][0], want_tail["flow_var"][0] = -1, 0, 0
    if mode == 0:
        assert single[0].tobytes() == b.records[:513].tobytes() and single[1].tobytes() == want_tail.tobytes()
    else:
        b.check_default(single[0])
        t = single[1]
        assert t["reserved"][0] == 0 and t["reserved"][1] != 0 and t["ham"].tolist() == want_tail["ham"].tolist()
        assert np.array_equal(t["lap_sum"], want_tail["lap_sum"]) and np.array_equal(t["lap_sumsq"], want_tail["lap_sumsq"])
        assert HF.check(t["flow_mean"][1:], t["flow_var"][1:], want_tail["flow_mean"][1:], want_tail["flow_var"][1:], t["reserved"][1:] != 0) == []
