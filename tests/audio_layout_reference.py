"""The downmix rule of option "audio_layout" (include/avd.h), restated in numpy from its text: M = (sum_c w_c s_c + 16384) >> 15 with Q15 weights
derived from the gains, on int64.  Narrowing and the filter bank are tests/audio_resample_reference.py's.  Nothing is taken from the C++."""
import math

import numpy as np

from tests import audio_resample_reference as ref

PLANAR = 0x100
# FFmpeg's / WAVE's native orders; the id is the channel count
CHANNELS = {1: ("FC",), 2: ("FL", "FR"), 6: ("FL", "FR", "FC", "LFE", "BL", "BR"), 8: ("FL", "FR", "FC", "LFE", "BL", "BR", "SL", "SR")}
GAINS = {"FC": 1.0, "FL": math.sqrt(0.5), "FR": math.sqrt(0.5), "BL": 0.5, "BR": 0.5, "SL": 0.5, "SR": 0.5, "LFE": 0.0}
# the table as the issue and the header write it out
TABLE = {1: (32768,), 2: (16384, 16384), 6: (6786, 6786, 9598, 0, 4799, 4799), 8: (5249, 5249, 7422, 0, 3712, 3712, 3712, 3712)}


def derive(layout):
    """w_c = rint(g_c / sum g * 32768); 32768 - sum w goes to the channel with the largest g, the lowest index on a tie"""
    g = [GAINS[name] for name in CHANNELS[layout]]
    total = sum(g)
    w = [int(np.rint(x / total * 32768.0)) for x in g]
    w[g.index(max(g))] += 32768 - sum(w)
    return tuple(w)


WEIGHTS = {layout: derive(layout) for layout in CHANNELS}
assert WEIGHTS == TABLE, (WEIGHTS, TABLE)


def mix(frames, layout):
    """frames int[n, c], narrowed already -> int16[n]: the formula.  The shift is arithmetic (int64 >>: floor); no clamp is needed."""
    frames = np.asarray(frames).astype(np.int64)
    assert frames.ndim == 2 and frames.shape[1] == layout, (frames.shape, layout)
    acc = frames @ np.array(WEIGHTS[layout], np.int64)
    m = (acc + 16384) >> 15
    assert m.size == 0 or (-32768 <= m.min() and m.max() <= 32767)
    return m.astype(np.int16)


def frames_of(wav, layout, planar):
    """a track as the call takes it -- [n, c] interleaved or [c, n] planar -> [n, c]"""
    wav = np.asarray(wav)
    if wav.ndim == 1:
        wav = wav[None, :] if planar else wav[:, None]
    return wav.T if planar else wav


def convert(wav, rate, layout, planar=False):
    """the whole rule for ONE track -> int16 output samples: narrow per sample, mix, then the filter of the existing restatement (which takes a
    mono int16 track as it is: its own steps 1 and 2 are the identity there)"""
    frames = frames_of(wav, layout, planar)
    assert frames.shape[1] == layout, (frames.shape, layout)
    return ref.convert(mix(ref.narrow(np.ascontiguousarray(frames)), layout), rate)
