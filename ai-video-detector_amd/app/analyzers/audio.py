"""MI355X drop-in for reference ``app/analyzers/audio.py`` -- same name, signature, result.

``analyze(path, meta)`` keeps the reference's contract (audio.py:29-122): it never raises -- any failure (no ffmpeg, an
unreadable file, a HIP error) becomes ``{"scores": {}, "flags_audio": {"error": str(e)}, "timeline": [0.5] * tlen}``
exactly as the reference's own ``except`` does (audio.py:111-118).  The per-window spectral features run in the HIP
kernels behind the C-ABI (``avd_audio_features``); there is no CPU fallback for them.

``AVD_AUDIO_RESAMPLE=1``: a PCM ``.wav`` at one of the converter's rates (``avd_hip.audio.RESAMPLE_RATES``) is read as it is, every channel, and
what the reference's ffmpeg line does (downmix, 16 kHz, 16 bit) happens on the device (``analyze_decoded``); no ffmpeg runs.  Any other file takes
the usual way.  Unset, nothing changes.

``AVD_AUDIO_CHUNK=<frames>`` (read only with ``AVD_AUDIO_RESAMPLE=1``): such a file is read with ``readframes(<frames>)`` in a loop and continued on the
device in an audio slot (``analyze_decoded_chunks``): the result of the whole-file read, in memory bounded by one piece.  Unset, nothing changes.

``AVD_AUDIO_LAYOUT=1`` (read only with ``AVD_AUDIO_RESAMPLE=1``): a 6- or 8-channel PCM ``.wav`` (5.1 / 7.1 in WAVE's native channel order) is taken as
well and downmixed on the device by the layout's weights (``analyze_decoded(..., layout=channels)``).  Unset, nothing changes."""
from __future__ import annotations

import os

from avd_hip import analyzer as _analyzer
from avd_hip import audio as _audio


def _channel_counts() -> tuple:
    """the channel counts the AVD_AUDIO_RESAMPLE path takes: one or two, and with AVD_AUDIO_LAYOUT=1 also six (5.1) and eight (7.1)"""
    return (1, 2, 6, 8) if os.getenv("AVD_AUDIO_LAYOUT", "0") == "1" else (1, 2)


def _layout_kw(channels: int) -> dict:
    """one or two channels go the way they always went; 5.1 / 7.1 name their layout"""
    return {"layout": _audio.layout_of(channels)} if channels > 2 else {}


def _read_decoded(path: str):
    """-> (frames, rate) of a PCM .wav the converter takes (a channel count of _channel_counts(), a supported rate), else None"""
    try:
        frames, sr = _audio.read_wav_frames(path)
    except Exception:          # noqa: BLE001 -- not a PCM .wav: ffmpeg's job
        return None
    return (frames, sr) if sr in _audio.RESAMPLE_RATES and frames.shape[1] in _channel_counts() and len(frames) else None


def _chunk_frames() -> int:
    """AVD_AUDIO_CHUNK: frames per readframes() of the AVD_AUDIO_RESAMPLE path; unset, empty, not a number or below 1: the file is read whole"""
    try:
        return max(0, int(os.getenv("AVD_AUDIO_CHUNK", "0") or 0))
    except ValueError:
        return 0


def _chunked_rate(path: str):
    """-> (rate, channels) of a PCM .wav the converter takes in pieces (the same files _read_decoded accepts), else None"""
    try:
        nch, width, sr, n = _audio.wav_info(path)
    except Exception:          # noqa: BLE001 -- not a PCM .wav: ffmpeg's job
        return None
    return (sr, nch) if sr in _audio.RESAMPLE_RATES and nch in _channel_counts() and width in (1, 2, 4) and n else None


def analyze(path: str, meta: dict):
    try:
        resample = os.getenv("AVD_AUDIO_RESAMPLE", "0") == "1"
        chunk = _chunk_frames() if resample else 0
        rate = _chunked_rate(path) if chunk else None
        if rate:
            # the bounded-memory decode loop: read -> analyze -> drop, the track continued on the device in an audio slot
            with _analyzer.default_pool().borrow(int(os.getenv("AVD_DEVICE", "0"))) as ctx:
                return _audio.analyze_decoded_chunks(_audio.read_wav_chunks(path, chunk), rate[0], ctx, **_layout_kw(rate[1]))
        if resample:
            decoded = _read_decoded(path)
            if decoded is not None:
                with _analyzer.default_pool().borrow(int(os.getenv("AVD_DEVICE", "0"))) as ctx:
                    return _audio.analyze_decoded(decoded[0], decoded[1], ctx, **_layout_kw(decoded[0].shape[1]))
        wav, sr = _audio.extract_wav_16k(path, native=True)      # a 16-bit file: its int16 samples as they are, converted on the device
        with _analyzer.default_pool().borrow(int(os.getenv("AVD_DEVICE", "0"))) as ctx:
            return _audio.analyze_wave(wav, sr, ctx)
    except Exception as e:          # noqa: BLE001 -- the reference swallows everything here (audio.py:111)
        tlen = int(max(1, round(meta.get("duration") or 0.0)))
        return {"scores": {}, "flags_audio": {"error": str(e)}, "timeline": [0.5] * tlen}
