"""Host side of the audio analyzer: waveform loading and the scalar tail of reference
``app/analyzers/audio.py``.

The per-window loop (audio.py:40-61: RMS, zero crossings, Hann window, rFFT magnitudes, flatness / roll-off / centroid) runs
in the HIP kernels behind ``avd_audio_features`` for all windows of the file at once; what is left is O(windows) float64
numpy -- percentile, variances, tts_like, timeline (audio.py:63-110) -- kept on the host so that the reductions are the
very calls the reference makes.  There is no CPU fallback for the spectral part."""
from __future__ import annotations

import os
import shutil
import subprocess
import tempfile
import wave

import numpy as np

SAMPLE_RATE = 16000          # audio.py:10: ffmpeg -ac 1 -ar 16000


def read_wav_pcm(path: str):
    """-> (float32 samples of channel 0 scaled like soundfile's dtype='float32', sample rate); PCM 8/16/32-bit WAV."""
    with wave.open(path, "rb") as w:
        nch, width, sr, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    if width == 2:
        a = np.frombuffer(raw, "<i2").astype(np.float32) / np.float32(32768.0)
    elif width == 4:
        a = (np.frombuffer(raw, "<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    elif width == 1:
        a = (np.frombuffer(raw, np.uint8).astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    else:
        raise RuntimeError("soundfile_read_failed")
    if nch > 1:
        a = a.reshape(-1, nch)[:, 0]          # audio.py:34: first channel
    return np.ascontiguousarray(a), int(sr)


def read_wav_native(path: str):
    """read_wav_pcm's sibling: a 16-bit file gives the int16 samples of channel 0 UNTOUCHED (half the bytes; the analyzer takes them as
    float32(s) * 2^-15 on the device, bit for bit what read_wav_pcm's division gives), every other width what read_wav_pcm returns."""
    with wave.open(path, "rb") as w:
        nch, width, sr, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n) if width == 2 else None
    if raw is None:
        return read_wav_pcm(path)
    a = np.frombuffer(raw, "<i2").astype(np.int16, copy=False)
    if nch > 1:
        a = a.reshape(-1, nch)[:, 0]          # audio.py:34: first channel
    return np.ascontiguousarray(a), int(sr)


RESAMPLE_RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)   # option "audio_rate" (include/avd.h)


def read_wav_frames(path: str):
    """-> (all channels untouched as [n, channels] -- int16 for a 16-bit file, float32 scaled like read_wav_pcm for 8 / 32 bit --, sample rate):
    what analyze_decoded takes."""
    with wave.open(path, "rb") as w:
        nch, width, sr, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    return _frames_of(raw, width, nch), int(sr)


def _frames_of(raw: bytes, width: int, nch: int) -> np.ndarray:
    """the bytes readframes() returned as [n, channels]: int16 for a 16-bit file, float32 scaled like read_wav_pcm for 8 / 32 bit"""
    if width == 2:
        a = np.frombuffer(raw, "<i2").astype(np.int16, copy=False)
    elif width == 4:
        a = (np.frombuffer(raw, "<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    elif width == 1:
        a = (np.frombuffer(raw, np.uint8).astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    else:
        raise RuntimeError("soundfile_read_failed")
    return np.ascontiguousarray(a.reshape(-1, nch))


def wav_info(path: str):
    """-> (channels, bytes per sample, rate, frames) of a PCM .wav"""
    with wave.open(path, "rb") as w:
        return w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()


def read_wav_chunks(path: str, chunk: int):
    """read_wav_frames in pieces: yields [<= chunk, channels] arrays read with readframes(chunk) -- what analyze_decoded_chunks takes, which
    holds a piece back until its successor shows that it was not the last: two pieces of the file are in host memory at most, never the file."""
    with wave.open(path, "rb") as w:
        nch, width = w.getnchannels(), w.getsampwidth()
        while True:
            raw = w.readframes(int(chunk))
            if not raw:
                return
            yield _frames_of(raw, width, nch)


def extract_wav_16k(path: str, native: bool = False):
    """audio.py:7-20: ffmpeg -> 16 kHz mono wav -> float32 (native: the int16 samples of the 16-bit file ffmpeg writes, as read_wav_native
    hands them over).  Without ffmpeg (this image has none) a file that already IS a 16 kHz PCM wav is read directly; anything else fails the
    way the reference fails when ffmpeg does."""
    read = read_wav_native if native else read_wav_pcm
    if shutil.which("ffmpeg"):
        tmp = tempfile.NamedTemporaryFile(delete=False, suffix=".wav")
        tmp.close()
        try:
            proc = subprocess.run(["ffmpeg", "-y", "-i", path, "-ac", "1", "-ar", str(SAMPLE_RATE), "-f", "wav", tmp.name],
                                  stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            if proc.returncode != 0:
                raise RuntimeError("ffmpeg_convert_failed")
            try:
                return read(tmp.name)
            except Exception:
                raise RuntimeError("soundfile_read_failed")
        finally:
            try:
                os.unlink(tmp.name)
            except OSError:
                pass
    try:
        wav, sr = read(path)
    except Exception:
        raise RuntimeError("ffmpeg_convert_failed")
    if sr != SAMPLE_RATE:
        raise RuntimeError("ffmpeg_convert_failed")          # resampling is ffmpeg's job
    return wav, sr


def window_values(rec: np.ndarray) -> dict:
    """avd_audio_window records -> the five per-window lists of audio.py:38-61 (python floats)."""
    n = rec["length"].astype(np.float64)
    nb = rec["nbins"].astype(np.float64)
    rms = np.sqrt(rec["sumsq"] / n)
    # np.mean over a float32 array divides in float32 (audio.py:45), then / 2.0
    with np.errstate(invalid="ignore", divide="ignore"):
        zcr = (rec["zero_cross"].astype(np.float32) / (rec["length"] - 1).astype(np.float32)).astype(np.float64) / 2.0
    flat = np.exp(rec["sum_log"] / nb) / (rec["sum_mag"] / nb)
    roll = rec["rolloff_index"].astype(np.float64) / np.maximum(1.0, nb)
    sc = rec["sum_fmag"] / rec["sum_mag"]
    return {k: [float(x) for x in v] for k, v in (("rms", rms), ("zcr", zcr), ("flat", flat), ("roll", roll), ("sc", sc))}


def _norm01(x):
    x = np.asarray(x, dtype=float)
    if x.size == 0:
        return np.zeros(1)
    lo, hi = float(np.min(x)), float(np.max(x))
    return (x - lo) / (hi - lo + 1e-9)


def features_to_result(values: dict, dur: float) -> dict:
    """The tail of audio.py (63-110): same numpy calls, same order."""
    arr = {k: (np.array(v) if v else np.zeros(1)) for k, v in values.items()}
    rms, zcr, flat, roll, sc = arr["rms"], arr["zcr"], arr["flat"], arr["roll"], arr["sc"]
    speech_ratio = float(np.mean(rms >= np.percentile(rms, 60)))
    flat_mean = float(np.mean(flat))
    sc_var, roll_var, zcr_var = float(np.var(sc)), float(np.var(roll)), float(np.var(zcr))
    tts_base = 0.7 * flat_mean + 0.15 * (1.0 / (1e-6 + zcr_var)) + 0.15 * (1.0 / (1e-6 + roll_var))
    tts_like = float(np.clip(tts_base * (1.0 / (1.0 + 5.0 * (sc_var + roll_var + zcr_var))), 0.0, 1.0))
    if sc_var + roll_var + zcr_var > 0.005:                  # "cap del TTS" when the variability is not negligible
        tts_like = float(min(tts_like, 0.90))
    dzcr = np.diff(np.concatenate([[zcr[0]], zcr]))
    droll = np.diff(np.concatenate([[roll[0]], roll]))
    line = np.clip(0.5 * _norm01(flat) + 0.3 * (1.0 - _norm01(dzcr ** 2)) + 0.2 * (1.0 - _norm01(np.abs(droll))), 0.0, 1.0).tolist()
    tlen = int(max(1, round(dur)))
    line = line + [line[-1] if line else 0.5] * (tlen - len(line)) if len(line) < tlen else line[:tlen]
    return {"scores": {"speech_ratio": speech_ratio, "tts_like": tts_like},
            "flags_audio": {"speech_ratio": speech_ratio, "tts_like": tts_like, "rms_var": float(np.var(rms)),
                            "zcr_var": zcr_var, "roll_var": roll_var, "sc_var": sc_var},
            "timeline": line}


def _mono(wav):
    """the first channel (audio.py:34); int16 PCM stays int16, everything else becomes float32"""
    wav = np.asarray(wav)
    if wav.ndim > 1:
        wav = wav[:, 0]
    return np.ascontiguousarray(wav, np.int16 if wav.dtype == np.int16 else np.float32)


def _win_of(sr: int) -> int:
    return max(1, int(sr * 0.5)) if sr else 1


def analyze_wave(wav: np.ndarray, sr: int, ctx) -> dict:
    """audio.py:33-110 for a decoded waveform (float32, or 16-bit PCM as int16), spectral features on the GPU."""
    wav = _mono(wav)
    dur = len(wav) / sr if sr > 0 else 0.0
    rec = ctx.audio_features(wav, _win_of(sr))
    return features_to_result(window_values(rec), dur)


def analyze_waves(waves, ctx) -> list:
    """[(wav, sr), ...] -> the list of analyze_wave's results, in input order.  Tracks of one window length (that is, one sample rate) and one
    sample type share calls (Context.audio_features_many: up to 64 tracks per call), so that short tracks fill the chip together."""
    waves = [(_mono(w), sr) for w, sr in waves]
    groups = {}
    for i, (w, sr) in enumerate(waves):
        groups.setdefault((_win_of(sr), w.dtype == np.int16), []).append(i)
    results = [None] * len(waves)
    for (win, _), members in groups.items():
        recs = ctx.audio_features_many([waves[i][0] for i in members], win)
        for i, rec in zip(members, recs):
            w, sr = waves[i]
            results[i] = features_to_result(window_values(rec), len(w) / sr if sr > 0 else 0.0)
    return results


def _decoded(wav):
    """a decoded track as [n, c]: int16 PCM stays int16, everything else becomes float32"""
    wav = np.asarray(wav)
    if wav.ndim == 1:
        wav = wav[:, None]
    if wav.ndim != 2 or wav.shape[1] not in (1, 2):
        raise ValueError("a decoded track is [n] or [n, c] with c = 1 or 2 (other layouts and planar samples: layout=, planar=)")
    return np.ascontiguousarray(wav, np.int16 if wav.dtype == np.int16 else np.float32)


# option "audio_layout" (include/avd.h): the Q15 downmix weights of each layout, in FFmpeg's native channel order -- the id is the channel count
LAYOUT_WEIGHTS = {
    1: (32768,),
    2: (16384, 16384),
    6: (6786, 6786, 9598, 0, 4799, 4799),                       # FL FR FC LFE BL BR
    8: (5249, 5249, 7422, 0, 3712, 3712, 3712, 3712),           # FL FR FC LFE BL BR SL SR
}


def layout_of(channels: int) -> int:
    """the "audio_layout" id of a track of ``channels`` channels in FFmpeg's native order: 1, 2, 6 (5.1) or 8 (7.1)"""
    if channels not in LAYOUT_WEIGHTS:
        raise ValueError("no layout of %r channels: 1 (mono), 2 (stereo), 6 (5.1) or 8 (7.1)" % (channels,))
    return int(channels)


def _decoded_layout(wav, layout: int, planar: bool):
    """a decoded track with a layout: interleaved [n, layout] (dense), or planar [layout, n] AS IT LIES -- a column slice of a wider array keeps
    its strides, which the call passes on; int16 PCM stays int16, everything else becomes float32"""
    layout_of(layout)
    wav = np.asarray(wav)
    wav = wav if wav.dtype == np.int16 or wav.dtype == np.float32 else wav.astype(np.float32)
    if wav.ndim == 1 and layout == 1:
        wav = wav[None, :] if planar else wav[:, None]
    if wav.ndim != 2 or wav.shape[0 if planar else 1] != layout:
        raise ValueError("a decoded track of layout %d is %s" % (layout, "[%d, n]" % layout if planar else "[n, %d]" % layout))
    return wav if planar else np.ascontiguousarray(wav)


def _layout_tools(layout, planar: bool):
    """-> (prepare, frames of a prepared chunk, keywords for the Context's calls); layout None: the helpers as they were"""
    if layout is None:
        if planar:
            raise ValueError("planar needs layout")
        return _decoded, len, {}
    layout = int(layout)
    return (lambda w: _decoded_layout(w, layout, planar)), (lambda w: int(w.shape[1 if planar else 0])), {"layout": layout, "planar": bool(planar)}


def _converted_duration(n: int, sr: int, ctx) -> float:
    return ctx.audio_converted_length(n, sr) / SAMPLE_RATE


def analyze_decoded(wav: np.ndarray, sr: int, ctx, layout=None, planar: bool = False) -> dict:
    """audio.py:7-110 for a track as its decoder produced it -- [n] or [n, c], c = 1 or 2, int16 or float32, at one of RESAMPLE_RATES: what the
    reference's ffmpeg line does (downmix, 16 kHz, 16 bit) happens on the device in front of the analyzer (Context.audio_features, rate=sr).

    layout (1, 2, 6 or 8: see layout_of) names the channel layout; the track is then [n, layout], or with planar=True [layout, n] as planar
    decoders (AAC, Opus, MP3 ...) hand it over, and is downmixed on the device by LAYOUT_WEIGHTS."""
    prepare, frames, kw = _layout_tools(layout, planar)
    wav = prepare(wav)
    rec = ctx.audio_features(wav, _win_of(SAMPLE_RATE), rate=int(sr), **kw)
    return features_to_result(window_values(rec), _converted_duration(frames(wav), int(sr), ctx))


def analyze_decoded_many(waves, ctx, layout=None, planar: bool = False) -> list:
    """[(wav, sr), ...] -> the list of analyze_decoded's results, in input order.  Tracks of one rate, one channel count and one sample type share
    calls (Context.audio_features_many: up to 64 tracks per call).  layout / planar: as for analyze_decoded, the same for every track."""
    prepare, frames, kw = _layout_tools(layout, planar)
    waves = [(prepare(w), int(sr)) for w, sr in waves]
    groups = {}
    for i, (w, sr) in enumerate(waves):
        groups.setdefault((sr, w.shape[0 if planar else 1], w.dtype == np.int16), []).append(i)
    results = [None] * len(waves)
    for (sr, _, _), members in groups.items():
        recs = ctx.audio_features_many([waves[i][0] for i in members], _win_of(SAMPLE_RATE), rate=sr, **kw)
        for i, rec in zip(members, recs):
            results[i] = features_to_result(window_values(rec), _converted_duration(frames(waves[i][0]), sr, ctx))
    return results


def _chunk_records(chunks, ctx, slot: int, prepare, win: int, rate=None, frames_of=len, **kw):
    """The decode loop read -> analyze -> drop: every chunk goes to the device once, as it comes, and only the LAST one is marked as the end of
    the track (so a chunk is held until its successor shows that it was not the last).  -> (records of the whole track, frames seen)"""
    recs, frames, held = [], 0, None
    ctx.set_option("audio_slot_reset", int(slot))            # the helper owns the slot for the length of the track
    try:
        for chunk in chunks:
            chunk = prepare(chunk)
            if held is not None:
                recs.append(ctx.audio_features(held, win, rate=rate, slot=slot, **kw))
                frames += frames_of(held)
            held = chunk
        if held is not None:
            recs.append(ctx.audio_features(held, win, rate=rate, slot=slot, last=True, **kw))
            frames += frames_of(held)
    except BaseException:
        ctx.set_option("audio_slot_reset", int(slot))        # half a track is of no use to the next one
        raise
    if not recs:
        return ctx.audio_features(np.zeros(0, np.float32), win), 0
    return np.concatenate(recs), frames


def analyze_wave_chunks(chunks, sr: int, ctx, slot: int = 1) -> dict:
    """analyze_wave for a 16 kHz track that arrives in pieces: an iterator of [n] or [n, c] arrays (one sample type throughout), continued on
    the device in audio slot ``slot`` (Context.audio_features, slot=...).  -> what analyze_wave gives for the concatenation, in bounded memory."""
    rec, n = _chunk_records(chunks, ctx, slot, _mono, _win_of(sr))
    return features_to_result(window_values(rec), n / sr if sr > 0 else 0.0)


def analyze_decoded_chunks(chunks, sr: int, ctx, slot: int = 1, layout=None, planar: bool = False) -> dict:
    """analyze_decoded for a track that arrives as its decoder's packets: an iterator of [n] or [n, c] arrays at rate ``sr`` (one channel count and
    one sample type throughout).  -> what analyze_decoded gives for the concatenation; the duration is ceil(N U / D) / 16000 of the N frames seen.
    layout / planar: as for analyze_decoded; planar packets are [layout, n]."""
    prepare, frames, kw = _layout_tools(layout, planar)
    rec, n = _chunk_records(chunks, ctx, slot, prepare, _win_of(SAMPLE_RATE), int(sr), frames, **kw)
    return features_to_result(window_values(rec), _converted_duration(n, int(sr), ctx))


MAX_STREAMS = 8              # the audio slots (option "audio_slot"; Context.AUDIO_SLOTS)


def _stream_records(streams, ctx, prepare, win: int, rate=None, frames_of=len, **kw):
    """K <= 8 tracks that arrive in pieces side by side: stream k is continued in audio slot k + 1, and every ROUND -- one piece of each stream that
    still gives something -- is ONE call (Context.audio_features_mapped: one gather, converter, analyzer and save launch however many streams).
    A piece is held until its stream's next one shows that it was not the last, so a stream ends in the round that carries its last piece; one
    that gave nothing at all is the empty track.  Empty pieces are skipped.  The helper owns slots 1 ... K: they are emptied first and, whatever
    happens, at the end.  -> [(records of the whole track, frames seen)] per stream"""
    its = [iter(s) for s in streams]
    if len(its) > MAX_STREAMS:
        raise ValueError("at most %d streams side by side (the audio slots)" % MAX_STREAMS)

    def pull(it):
        for chunk in it:
            chunk = prepare(chunk)
            if frames_of(chunk):
                return chunk
        return None

    recs, frames = [[] for _ in its], [0] * len(its)
    try:
        for k in range(len(its)):
            ctx.set_option("audio_slot_reset", k + 1)
        held = [pull(it) for it in its]
        while any(h is not None for h in held):
            ahead = [pull(it) if h is not None else None for it, h in zip(its, held)]
            members = [k for k, h in enumerate(held) if h is not None]
            got = ctx.audio_features_mapped([held[k] for k in members], [k + 1 for k in members], [ahead[k] is None for k in members], win, rate=rate, **kw)
            for k, rec in zip(members, got):
                recs[k].append(rec)
                frames[k] += frames_of(held[k])
            held = ahead
    finally:
        for k in range(len(its)):
            ctx.set_option("audio_slot_reset", k + 1)        # half a track is of no use to the next one; a finished one has left its slot empty
    empty = None
    out = []
    for k in range(len(its)):
        if recs[k]:
            out.append((np.concatenate(recs[k]), frames[k]))
        else:
            empty = ctx.audio_features(np.zeros(0, np.float32), win) if empty is None else empty
            out.append((empty, 0))
    return out


def analyze_wave_streams(streams, sr: int, ctx) -> list:
    """analyze_wave_chunks for up to eight 16 kHz tracks that arrive in pieces side by side (live streams): an iterable of pieces per stream, one
    sample type throughout.  One call per round of pieces.  -> per stream what analyze_wave gives for its concatenation."""
    return [features_to_result(window_values(rec), n / sr if sr > 0 else 0.0) for rec, n in _stream_records(streams, ctx, _mono, _win_of(sr))]


def analyze_decoded_streams(streams, sr: int, ctx, layout=None, planar: bool = False) -> list:
    """analyze_decoded_chunks for up to eight tracks that arrive as their decoders' packets side by side, all at rate ``sr`` with one channel count
    and one sample type.  One call per round of packets.  -> per stream what analyze_decoded gives for its concatenation.
    layout / planar: as for analyze_decoded, the same for every stream."""
    prepare, frames, kw = _layout_tools(layout, planar)
    return [features_to_result(window_values(rec), _converted_duration(n, int(sr), ctx))
            for rec, n in _stream_records(streams, ctx, prepare, _win_of(SAMPLE_RATE), int(sr), frames, **kw)]
