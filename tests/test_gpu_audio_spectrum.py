"""The audio analyzer's spectrum, bin by bin, on both transform paths (csrc/avd_audio.hip; debug buffers "audio_plan" / "audio_xw" / "audio_mag").

tests/test_audio.py sees the five audio kernels through four sums per window, on one speech-like kind of signal.  Two of those sums do
not change when bins are permuted.  Here every bin of every window is compared with numpy:

    ref = |np.fft.rfft(float64(seg) * np.hanning(L))| + 1e-9          |audio_mag[k] - ref[k]| <= 1e-12 * sum|xw|

The bound is derived, not tuned: a direct double sum of L <= 8192 terms errs by at most L * 2^-53 * sum|xw| = 9.1e-13 * sum|xw|; table
rounding and hypot add a few units of 2^-53; the 80 x 100 path sums fewer terms.  A mis-indexed bin or twiddle errs at the scale of the
bins themselves, nine orders of magnitude above it.  On the CPU a float64 direct DFT differs from pocketfft by at most 5.2e-16 * sum|xw|
on these families (L = 8000, 8192, 7999, 1001, 6).  Worst |audio_mag - ref| / sum|xw| observed on an MI355X over all cases of this file:

    80 x 100 path (k_audio_fft_a / _b):   6.8e-16   (the Nyquist bin of a tone on bin 4000)
    direct path   (k_audio_dft):          4.8e-15   (bin 0 of the constant, win = 8192)

(the module prints both when it finishes: run with -s).

The record fields are bounded from the same per-bin tolerance (tol_bin = 1e-12 * sum|xw|): sum_mag and sum_fmag by nbins * tol_bin + 1e-12 |ref|,
sum_log by the logarithm's conditioning at the reference's own magnitudes, sum_k tol_bin / ref[k] + 1e-12 * sum|log ref|.  Signals carry a
white-noise floor (sigma 1e-3) so that this bound stays below 1e-3 absolute; the roll-off index is exact because the reference's running sum
clears the cutoff by more than the sums can err.  Both input conditions are asserted from the reference alone, before the GPU value is read.

"audio_xw" against float64(seg) * np.hanning(L), element by element: relative 4 * 2^-52, which covers the one rounding of the product and no
more.  It holds because the library's tables and np.hanning form the factor by the same expression, 0.5 + 0.5 cos(.), with cosines that return
the same bits (glibc's cos and numpy's agree on every argument of these tables).  A cosine that differed in its last place would move the factor
by 2^-53 ABSOLUTE, which at the ends of a window, where cos is close to -1 and the sum cancels, is about 1e-9 relative for L = 8000: the check
would then fail without the kernel being wrong, and its message says when that is the case (|difference| <= 2^-52 |seg|)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FFT_WIN = 8000                    # the window length that takes the 80 x 100 path (full windows only)
MAX_WIN = 8192
TOL = 1e-12                       # per bin, in units of sum|xw|
EPS_XW = 4 * 2.0 ** -52

FLOORED = ("noise", "tone_on_bin", "tone_off_bin", "nyquist", "impulse", "chirp", "dc")
UNFLOORED = ("silence", "tone_alone")
FAMILIES = FLOORED + UNFLOORED

_worst = {"fft": (0.0, None), "direct": (0.0, None)}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for path, (ratio, where) in _worst.items():
        print(f"\nworst |audio_mag - ref| / sum|xw| on the {path} path: {ratio:.3e} at {where} (bound {TOL:g})")


# ---- signals ------------------------------------------------------------------------------------
def tone_bin(L):
    """the bin the on-bin tone of an L-sample window sits on"""
    return max(1, L // 5) if L >= 4 else 0


def window_signal(family, L, rng):
    """One window of L samples, float64 before clipping; frequencies are relative to L, so every window length gets its own on-bin tone."""
    i = np.arange(L)
    k0 = tone_bin(L)
    ph = 6.28 * rng.random()
    if family == "noise":
        x = 0.3 * rng.standard_normal(L)
    elif family in ("tone_on_bin", "tone_alone"):
        x = 0.5 * np.sin(2 * np.pi * k0 * i / L + ph)
    elif family == "tone_off_bin":
        x = 0.5 * np.sin(2 * np.pi * (k0 + 0.37) * i / L + ph)
    elif family == "nyquist":
        x = 0.5 * (1.0 - 2.0 * (i & 1))
    elif family == "impulse":
        x = np.zeros(L)
        x[L // 3] = 0.9
    elif family == "chirp":
        x = 0.5 * np.sin(2 * np.pi * (0.02 * i + (0.4 - 0.02) * i * i / (2.0 * L)) + ph)      # 0.02 ... 0.4 cycles per sample
    elif family == "dc":
        x = np.full(L, 0.25)
    elif family == "silence":
        x = np.zeros(L)
    else:
        raise KeyError(family)
    if family in FLOORED:
        x = x + 1e-3 * rng.standard_normal(L)
    return x


@functools.lru_cache(maxsize=None)
def clip_of(family, win, n, seed=0):
    rng = np.random.default_rng([FAMILIES.index(family), win, n, seed])
    parts = [window_signal(family, min(win, n - s), rng) for s in range(0, n, win)]
    wav = np.clip(np.concatenate(parts), -1.0, 1.0).astype(np.float32)
    wav.setflags(write=False)
    return wav


# ---- the reference: numpy alone -------------------------------------------------------------------
def expected_plan(win, n):
    nwin = -(-n // win)
    last = n - (nwin - 1) * win
    nfull = (nwin if last == win else nwin - 1) if win == FFT_WIN else 0
    return (nwin, win, last, nfull)


def window_reference(seg):
    """-> dict of everything one window is compared with, plus the input-validity conditions, from numpy alone."""
    L = len(seg)
    xw = seg.astype(np.float64) * np.hanning(L)
    ref = np.abs(np.fft.rfft(xw)) + 1e-9
    nb = len(ref)
    assert nb == L // 2 + 1
    s_abs = float(np.sum(np.abs(xw)))
    tol_bin = TOL * s_abs
    total = float(np.sum(ref))
    run = np.cumsum(ref)                                   # sequential, as audio.py:52-58 adds
    hit = np.nonzero(run >= 0.85 * total)[0]
    idx = int(hit[0]) if len(hit) else 0
    slack = nb * tol_bin + 1e-12 * total                   # how far the library's running sum and cutoff may be from these
    roll_ok = len(hit) > 0 and run[idx] - 0.85 * total > slack and (idx == 0 or 0.85 * total - run[idx - 1] > slack)
    # the indices the roll-off may take when the sums are off by `slack`: one, unless the running sum meets the cutoff at a bin
    roll_set = tuple(int(k) for k in np.nonzero((run >= 0.85 * total - slack) & (np.concatenate([[-np.inf], run[:-1]]) < 0.85 * total + slack))[0])
    assert idx in roll_set and (not roll_ok or roll_set == (idx,))
    return {
        "roll_set": roll_set, "L": L, "nb": nb, "xw": xw, "ref": ref, "s_abs": s_abs, "tol_bin": tol_bin,
        "zero_cross": int(np.abs(np.diff(np.sign(seg))).sum()),
        "sumsq": float(np.sum((seg ** 2).astype(np.float64))),            # float32 squares (audio.py:44), double sum
        "sum_mag": total,
        "sum_fmag": float(np.sum(np.linspace(0.0, 1.0, nb) * ref)),
        "sum_log": float(np.sum(np.log(ref))),
        "log_bound": float(np.sum(tol_bin / ref) + 1e-12 * np.sum(np.abs(np.log(ref)))),
        "rolloff_index": idx, "roll_ok": bool(roll_ok),
    }


@functools.lru_cache(maxsize=None)
def clip_reference(family, win, n, seed=0):
    wav = clip_of(family, win, n, seed)
    return tuple(window_reference(wav[s:s + win]) for s in range(0, n, win))


def assert_inputs_valid(family, refs):
    """The conditions under which sum_log and rolloff_index pin the kernels; no look at a GPU value."""
    for w, r in enumerate(refs):
        if family in FLOORED:
            assert r["roll_ok"], f"{family} window {w}: the reference's running sum passes the 85 % cutoff too closely for an exact index: change the seed"
            assert r["log_bound"] <= 1e-3, f"{family} window {w}: sum_log is conditioned no better than {r['log_bound']:.2e}: change the seed"


# ---- the comparison -----------------------------------------------------------------------------
def check_bins(ctx, wav, win, refs, where):
    """(a): the plan, audio_xw and every bin of audio_mag of the call just made on ctx."""
    n = len(wav)
    plan = ctx.audio_plan()
    assert plan == expected_plan(win, n), where
    nfull = plan[3]
    xw, mag = ctx.audio_xw(), ctx.audio_mag()
    assert xw.shape == (plan[0], win) and mag.shape == (plan[0], win // 2 + 1)
    for w, r in enumerate(refs):
        L, nb = r["L"], r["nb"]
        bad = np.nonzero(np.abs(xw[w, :L] - r["xw"]) > EPS_XW * np.abs(r["xw"]))[0]
        if len(bad):
            seg = np.abs(wav[w * win:w * win + L].astype(np.float64))
            libm = bool(np.all(np.abs(xw[w, :L] - r["xw"]) <= 2.0 ** -52 * seg))
            raise AssertionError(f"{where} window {w}: audio_xw[{bad[0]}] = {xw[w, bad[0]]!r}, numpy {r['xw'][bad[0]]!r}"
                                 + (": every difference is within 2^-52 |seg|, the mark of a host cosine that differs from numpy's in the last place "
                                    "(module docstring), not of the kernel" if libm else ""))
        err = np.abs(mag[w, :nb] - r["ref"])
        k = int(np.argmax(err))
        path = "fft" if w < nfull else "direct"
        if r["s_abs"] > 0:
            ratio = float(err[k]) / r["s_abs"]
            if ratio > _worst[path][0]:
                _worst[path] = (ratio, f"{where} window {w} bin {k}")
        assert err[k] <= r["tol_bin"], (f"{where} window {w} ({path} path, L = {L}): bin {k} is {mag[w, k]!r}, numpy {r['ref'][k]!r}: "
                                        f"off by {err[k]:.3e} = {err[k] / max(r['s_abs'], 1e-300):.3e} sum|xw|, bound {TOL:g}")
    return mag


def check_fields(rec, family, refs, where):
    """(d): every field of the records."""
    assert len(rec) == len(refs)
    for w, (g, r) in enumerate(zip(rec, refs)):
        at = f"{where} window {w}"
        assert (g["length"], g["nbins"], g["zero_cross"]) == (r["L"], r["nb"], r["zero_cross"]), at
        np.testing.assert_allclose(g["sumsq"], r["sumsq"], rtol=1e-12, atol=0, err_msg=at)
        slack = r["nb"] * r["tol_bin"]
        assert abs(g["sum_mag"] - r["sum_mag"]) <= slack + 1e-12 * abs(r["sum_mag"]), (at, g["sum_mag"], r["sum_mag"])
        assert abs(g["sum_fmag"] - r["sum_fmag"]) <= slack + 1e-12 * abs(r["sum_fmag"]), (at, g["sum_fmag"], r["sum_fmag"])
        if family in FLOORED:
            assert abs(g["sum_log"] - r["sum_log"]) <= r["log_bound"], (at, g["sum_log"], r["sum_log"], r["log_bound"])
        elif family == "silence":                          # every bin is the 1e-9 floor itself
            np.testing.assert_allclose(g["sum_log"], r["sum_log"], rtol=1e-12, atol=0, err_msg=at)
        # the tone without a floor: its empty bins are rounding noise in the reference itself, sum_log is not compared
        # silence has no seed to change: 4000 bins of exactly 1e-9 reach 85 % of their sum AT a bin (3400 of them), a tie that the last
        # place of the total decides.  There, and only there, the index is one of the two that the tie admits
        if family in FLOORED:
            assert g["rolloff_index"] == r["rolloff_index"], (at, g["rolloff_index"], r["rolloff_index"])
        else:
            assert len(r["roll_set"]) <= 2 and g["rolloff_index"] in r["roll_set"], (at, g["rolloff_index"], r["roll_set"])


def run_case(ctx, family, win, n, seed=0):
    wav, refs = clip_of(family, win, n, seed), clip_reference(family, win, n, seed)
    where = f"{family} win={win} n={n}"
    assert_inputs_valid(family, refs)
    rec = ctx.audio_features(wav, win)
    check_bins(ctx, wav, win, refs, where)
    check_fields(rec, family, refs, where)
    return rec


# ---- (a), (d): families x lengths ---------------------------------------------------------------
LENGTHS = (
    [(FFT_WIN, 2 * FFT_WIN)]                                                             # 80 x 100 path, two full windows
    + [(w, 2 * w) for w in (8192, 8190, 7999, 1001, 1002, 6, 5, 4, 3, 2, 1)]             # direct path, full windows
    + [(FFT_WIN, FFT_WIN + t) for t in (1, 2, 3, 5, 4161, 4162, 4163, 7999)]             # direct path, short last window under 8000
    + [(MAX_WIN, MAX_WIN + 8000)]                                                        # ... under 8192
    + [(1002, 3 * 1002)]                                                                 # an exact multiple of win
    + [(FFT_WIN, 3000)]                                                                  # shorter than win
)


def test_every_length_class_is_listed():
    plans = {(w, n): expected_plan(w, n) for w, n in LENGTHS}
    assert plans[(FFT_WIN, 2 * FFT_WIN)] == (2, 8000, 8000, 2)
    assert all(p[3] == 0 for (w, n), p in plans.items() if w != FFT_WIN)
    assert all(plans[(FFT_WIN, FFT_WIN + t)] == (2, 8000, t, 1) for t in (1, 2, 3, 5, 4161, 4162, 4163, 7999))
    assert plans[(MAX_WIN, MAX_WIN + 8000)] == (2, 8192, 8000, 0) and plans[(FFT_WIN, 3000)] == (1, 8000, 3000, 0)
    assert {p[2] % 4 for p in plans.values()} == {0, 1, 2, 3}


@pytest.mark.parametrize("win,n", LENGTHS)
@pytest.mark.parametrize("family", FAMILIES)
def test_bins_and_fields(ctx, family, win, n):
    run_case(ctx, family, win, n)


# ---- (b): where a bin lands on the 80 x 100 path ------------------------------------------------
@pytest.mark.parametrize("k0", [1, 79, 80, 81, 99, 100, 159, 160, 2000, 3999, 4000])
def test_tone_lands_on_its_bin_on_the_fft_path(ctx, k0):
    """The seams of k = k1 + 80 k2 and of the quarter-period switch at table index 2000."""
    rng = np.random.default_rng([7, k0])
    i = np.arange(FFT_WIN)
    parts = []
    for _ in range(2):
        # bin 4000 is the alternation itself; a sine there would sample its own zeros
        tone = 0.5 * np.cos(np.pi * i) if k0 == 4000 else 0.5 * np.sin(2 * np.pi * k0 * i / FFT_WIN + 6.28 * rng.random())
        parts.append(tone + 1e-3 * rng.standard_normal(FFT_WIN))
    wav = np.clip(np.concatenate(parts), -1, 1).astype(np.float32)
    refs = tuple(window_reference(wav[s:s + FFT_WIN]) for s in (0, FFT_WIN))
    assert all(int(np.argmax(r["ref"])) == k0 for r in refs)
    assert_inputs_valid("tone_on_bin", refs)
    rec = ctx.audio_features(wav, FFT_WIN)
    assert ctx.audio_plan() == (2, FFT_WIN, FFT_WIN, 2)
    got = [int(np.argmax(m)) for m in ctx.audio_mag()]
    assert got == [k0, k0], f"a tone on bin {k0} came out on bins {got}"
    check_bins(ctx, wav, FFT_WIN, refs, f"tone k0={k0}")
    check_fields(rec, "tone_on_bin", refs, f"tone k0={k0}")


# ---- (c): the same samples through both paths ---------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_both_paths_agree_on_the_same_samples(ctx, family):
    wav = clip_of(family, FFT_WIN, FFT_WIN)
    s_abs = clip_reference(family, FFT_WIN, FFT_WIN)[0]["s_abs"]
    fast = ctx.audio_features(wav, FFT_WIN)
    assert ctx.audio_plan() == (1, FFT_WIN, FFT_WIN, 1)
    m_fast = ctx.audio_mag()[0]
    direct = ctx.audio_features(wav, MAX_WIN)
    assert ctx.audio_plan() == (1, MAX_WIN, FFT_WIN, 0)
    m_direct = ctx.audio_mag()[0, :FFT_WIN // 2 + 1]
    err = np.abs(m_fast - m_direct)
    k = int(np.argmax(err))
    assert err[k] <= 2 * TOL * s_abs, f"{family}: bin {k}: 80 x 100 path {m_fast[k]!r}, direct path {m_direct[k]!r}"
    for f in ("zero_cross", "length", "rolloff_index", "nbins"):
        assert fast[f][0] == direct[f][0], f
    assert fast["sumsq"][0] == direct["sumsq"][0]


# ---- (e): the time-domain pass ------------------------------------------------------------------
@pytest.mark.parametrize("win", [FFT_WIN, 1001])
def test_zero_crossings_and_energy_at_signed_zeros_and_seams(ctx, win):
    """np.sign is 0 for both zeros: +x, 0.0, -0.0, -x is two crossings of one each, a run of zeros between opposite signs the same two.
    Sample i is compared with i + 1 by the lane that owns i, 256 lanes to a stride: 255|256 and 511|512 are pairs that straddle two
    strides.  The pair across a window boundary belongs to no window."""
    rng = np.random.default_rng(win)
    n = 2 * win + 300
    x = rng.choice(np.array([-0.7, -0.3, -0.0, 0.0, 0.2, 0.9], np.float32), n).astype(np.float32)
    for base in (0, win, 2 * win):
        x[base + 8:base + 12] = (0.5, 0.0, -0.0, -0.5)
        x[base + 20] = 0.25
        x[base + 21:base + 40] = 0.0
        x[base + 30:base + 35] = -0.0
        x[base + 40] = -0.25
        x[base + 250:base + 256] = 0.4                       # 255|256
        x[base + 256:base + 262] = -0.4
    for base in (0, win):
        x[base + 500:base + 512] = -0.6                      # 511|512
        x[base + 512:base + 520] = 0.6
    x[win - 1], x[win] = 0.8, -0.8                            # across the boundary of windows 0 and 1: counted by neither
    x[2 * win - 1], x[2 * win] = -0.0, 0.8
    rec = ctx.audio_features(x, win)
    assert ctx.audio_plan() == expected_plan(win, n)
    want = [int(np.abs(np.diff(np.sign(x[s:s + win]))).sum()) for s in range(0, n, win)]
    assert np.signbit(x).sum() > (x < 0).sum() and (x == 0).sum() > 100           # -0.0 is in there
    assert int(np.abs(np.diff(np.sign(x))).sum()) == sum(want) + 2 + 1           # the whole clip has the two boundary pairs more
    assert rec["zero_cross"].tolist() == want
    assert rec["length"].tolist() == [win, win, 300]
    for w, s in enumerate(range(0, n, win)):
        np.testing.assert_allclose(rec["sumsq"][w], np.sum((x[s:s + win] ** 2).astype(np.float64)), rtol=1e-12, atol=0)


# ---- (f): the table cache, keyed on (win, last) -------------------------------------------------
def test_tables_follow_win_and_last_over_a_run_of_calls():
    """One context, fifteen calls: win changes alone, last changes alone, both, neither, an earlier pair returns, the workspace is
    released in the middle.  A fresh context given the same call is the reference: byte for byte."""
    import avd_hip
    calls = [(8000, 16000), (8000, 16000),          # neither changes
             (8000, 12161),                         # last only
             (1001, 1001 + 4161),                   # win only (last stays 4161)
             (1002, 2500),                          # both
             (8000, 12161),                         # back to an earlier pair
             (8192, 8192 + 8000),
             (8000, 8000),                          # win == last == the last window of the call before
             "release",
             (8000, 8000),                          # the same pair after the release: the tables are gone and must be rebuilt
             (8000, 8003), (8000, 8002),            # last only, both without a quarter period
             (6, 20), (5, 20), (1001, 5162),
             (8000, 16000)]
    wav = clip_of("noise", 8192, 2 * 8192)
    with avd_hip.Context(0) as c:
        for step, call in enumerate(calls):
            if call == "release":
                c.release_workspace()
                with pytest.raises(avd_hip.AvdError):
                    c.audio_mag()                   # no stale buffer after the release
                continue
            win, n = call
            got = c.audio_features(wav[:n], win)
            got_mag = c.audio_mag()
            with avd_hip.Context(0) as fresh:
                want = fresh.audio_features(wav[:n], win)
                want_mag = fresh.audio_mag()
            assert got.tobytes() == want.tobytes(), f"call {step} {call}"
            nwin, _, last, _ = c.audio_plan()
            assert (nwin, last) == expected_plan(win, n)[::2]
            assert got_mag[:-1].tobytes() == want_mag[:-1].tobytes(), f"call {step} {call}"
            assert got_mag[-1, :last // 2 + 1].tobytes() == want_mag[-1, :last // 2 + 1].tobytes(), f"call {step} {call}"
    assert sum(1 for c in calls if c != "release") >= 12


# ---- (g): input forms, refusals, a wide grid ----------------------------------------------------
def test_plan_is_refused_before_the_first_call():
    import avd_hip
    with avd_hip.Context(0) as c:
        for fetch in (c.audio_plan, c.audio_xw, c.audio_mag):
            with pytest.raises(avd_hip.AvdError, match="no avd_audio_features call"):
                fetch()
        with pytest.raises(avd_hip.AvdError, match="unknown debug buffer"):
            c.debug_fetch("audio_", (1,), np.int32)
        assert len(c.audio_features(np.zeros(0, np.float32), 8000)) == 0          # nothing to do is not a call either
        with pytest.raises(avd_hip.AvdError, match="no avd_audio_features call"):
            c.audio_plan()


def test_device_strided_and_float64_input_give_the_same_records(ctx):
    import torch
    wav = clip_of("chirp", FFT_WIN, FFT_WIN + 4163)
    want = ctx.audio_features(wav, FFT_WIN).tobytes()
    dev = torch.from_numpy(np.array(wav)).cuda()
    assert ctx.audio_features(dev, FFT_WIN).tobytes() == want
    assert ctx.audio_plan() == (2, FFT_WIN, 4163, 1)
    wide = np.zeros((len(wav), 3), np.float32)
    wide[:, 1] = wav
    view = wide[:, 1]
    assert not view.flags["C_CONTIGUOUS"]
    assert ctx.audio_features(view, FFT_WIN).tobytes() == want
    assert ctx.audio_features(wav.astype(np.float64), FFT_WIN).tobytes() == want
    assert ctx.audio_features(torch.from_numpy(np.array(wav)), FFT_WIN).tobytes() == want       # a host tensor


def test_refused_calls_leave_the_context_usable(ctx):
    import ctypes
    import avd_hip
    from avd_hip._lib import AUDIO_WINDOW_DTYPE, AVD_MEM_HOST
    wav = clip_of("noise", 1001, 2 * 1001)
    want = run_case(ctx, "noise", 1001, 2 * 1001).tobytes()
    plan = ctx.audio_plan()
    for bad_win in (0, -1, 8193):
        with pytest.raises(avd_hip.AvdError, match="1..8192"):
            ctx.audio_features(wav, bad_win)
        with pytest.raises(avd_hip.AvdError, match="1..8192"):
            ctx.audio_features(np.zeros(0, np.float32), bad_win)
    with pytest.raises(ValueError):
        ctx.audio_features(np.zeros((4, 500), np.float32), 1001)
    small = np.zeros(1, AUDIO_WINDOW_DTYPE)                # room for one record, the call needs two
    rc = ctx._L.avd_audio_features(ctx._h, ctypes.c_void_p(wav.ctypes.data), AVD_MEM_HOST, len(wav), 1001, ctypes.c_void_p(small.ctypes.data), 1)
    assert rc != 0 and small.tobytes() == bytes(small.nbytes)
    assert len(ctx.audio_features(np.zeros(0, np.float32), 1001)) == 0
    assert ctx.audio_plan() == plan                                # none of these was a call
    assert run_case(ctx, "noise", 1001, 2 * 1001).tobytes() == want


def test_three_hundred_windows_in_one_call(ctx):
    """The widest grid of the file: 300 workgroups in every kernel of the direct path."""
    rec = run_case(ctx, "noise", 64, 300 * 64)
    assert len(rec) == 300 and ctx.audio_plan() == (300, 64, 64, 0)
