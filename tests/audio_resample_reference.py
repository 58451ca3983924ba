"""The conversion rule of options "audio_rate" / "audio_channels" (include/avd.h), restated in numpy from its text: int64 throughout after the
first step, nothing taken from the C++.  The tests compare the library's filter banks, its converted tracks and its plan with this file."""
import functools
import math

import numpy as np

OUT_RATE = 16000
RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)


def ratio(rate):
    """-> (U, D, T); T = 0 at 16000, which has no filter"""
    assert rate in RATES, rate
    g = math.gcd(rate, OUT_RATE)
    U, D = OUT_RATE // g, rate // g
    if rate == OUT_RATE:
        return U, D, 0
    f = min(1.0, 0.97 * U / D)
    return U, D, 2 * math.ceil(16 / f)


@functools.lru_cache(maxsize=None)
def bank(rate):
    """-> (q int64[U, T], the unrounded entries float64[U, T]) of step 3"""
    U, D, T = ratio(rate)
    if T == 0:
        return np.zeros((U, 0), np.int64), np.zeros((U, 0))
    f = min(1.0, 0.97 * U / D)
    phi = np.arange(U, dtype=np.float64)[:, None]
    k = np.arange(T, dtype=np.float64)[None, :]
    x = (k - T // 2 + 1) - phi / U
    t = f * x
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0.0, 1.0, np.sin(np.pi * t) / (np.pi * t))
    a = 1.0 - (2.0 * x / T) ** 2
    h = np.where(a < 0.0, 0.0, f * sinc * np.i0(9.0 * np.sqrt(np.maximum(a, 0.0))) / np.i0(9.0))
    v = h / h.sum(axis=1, keepdims=True) * 32768.0
    q = np.rint(v).astype(np.int64)
    for p in range(U):
        q[p, int(np.argmax(h[p]))] += 32768 - q[p].sum()          # argmax: the lowest k on a tie
    q.setflags(write=False)
    return q, v


def narrow(samples):
    """step 1 -> int64"""
    samples = np.asarray(samples)
    if samples.dtype == np.int16:
        return samples.astype(np.int64)
    assert samples.dtype == np.float32, samples.dtype
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(samples.astype(np.float64) * 32768.0)          # exact product; rint: ties to even
    v = np.where(np.isnan(v), 0.0, np.clip(v, -32768.0, 32767.0))
    return v.astype(np.int64)


def downmix(wav):
    """steps 1 and 2: [n] or [n, 1] or [n, 2] -> mono int64[n]"""
    s = narrow(wav)
    if s.ndim == 1:
        return s
    assert s.ndim == 2 and s.shape[1] in (1, 2), s.shape
    return s[:, 0] if s.shape[1] == 1 else (s[:, 0] + s[:, 1] + 1) >> 1       # >> on int64: floor


def n_out(n, rate):
    U, D, _ = ratio(rate)
    return -(-n * U // D)


def convert(wav, rate, first=0, count=None):
    """the whole rule for ONE track -> int16[count] output samples first ... first + count - 1 (default: all of them)"""
    U, D, T = ratio(rate)
    mono = downmix(wav)
    n = len(mono)
    total = n_out(n, rate)
    if count is None:
        count = total - first
    assert 0 <= first and first + count <= total
    m = np.arange(first, first + count, dtype=np.int64)
    if T == 0:
        return mono[m].astype(np.int16)
    q, _ = bank(rate)
    i0, ph = (m * D) // U, (m * D) % U
    acc = np.zeros(count, np.int64)
    for k in range(T):
        i = i0 - T // 2 + 1 + k
        inside = (i >= 0) & (i < n)
        acc += q[ph, k] * np.where(inside, mono[np.clip(i, 0, n - 1)], 0)
    return np.clip((acc + 16384) >> 15, -32768, 32767).astype(np.int16)


def convert_many(tracks, rate):
    """-> (the converted buffer: every track converted alone, side by side; int32[tracks, 2] first output sample and count)"""
    outs = [convert(t, rate) for t in tracks]
    counts = np.array([len(o) for o in outs], np.int64)
    firsts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return np.concatenate(outs), np.stack([firsts, counts], axis=1).astype(np.int32)


def tiles(n, rate, tile_out):
    """the tile table of ONE track of n frames that begins at frame 0: [(first frame of the span, first output, outputs, phase)], python ints"""
    U, D, T = ratio(rate)
    out = []
    for m0 in range(0, n_out(n, rate), tile_out):
        out.append(((m0 * D) // U - (T // 2 - 1 if T else 0), m0, min(tile_out, n_out(n, rate) - m0), (m0 * D) % U))
    return out
