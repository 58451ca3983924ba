#!/usr/bin/env python3
"""Golden vectors for the audio analyzer from the REFERENCE's own code (build container only).

    python tests/golden/make_audio_golden.py        # writes tests/golden/audio_golden.json

reference app/analyzers/audio.py cannot run as it stands: it imports ``soundfile`` (absent) and shells out to ``ffmpeg``
(absent) to obtain the 16 kHz mono waveform (audio.py:7-20).  Everything AFTER that point -- the per-window features and
the scalar tail, audio.py:33-110 -- is plain numpy and is exactly what the build accelerates.  So this script loads the
reference module BY FILE PATH with
  * a placeholder ``soundfile`` entry in sys.modules (an empty module object, only so that the import statement succeeds;
    no function of it is ever called), and
  * ``_extract_wav_16k`` replaced by a function that returns a seeded synthetic waveform (oracle.audio_oracle.synth_wave,
    oracle.audio_oracle.named_wave),
and calls the reference's own ``analyze``.  No arithmetic of the reference is replaced.  Inputs are stored as seeds or names
(the generators are deterministic numpy), outputs verbatim.  Nothing of the reference's source is copied.  A case is kept only
if its speech ratio cannot flip on a last-place difference of an rms (check_speech_ratio_is_well_conditioned), and a
regeneration must reproduce every case already in the file."""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("AVD_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
from oracle import audio_oracle  # noqa: E402

CASES = [(0, 6.0), (1, 9.25), (2, 3.0), (3, 0.5), (4, 0.26), (5, 12.0), (6, 1.0001), (7, 4.49)]   # (seed, seconds)


def check_speech_ratio_is_well_conditioned(case):
    """speech_ratio counts windows whose rms reaches the 60th percentile.  The reference averages float32 squares where the library
    sums them in double (rms equal to ~1e-7 relative), so a case pins the count only if no comparison can flip: two windows' rms are
    bitwise equal or more than 1e-5 relative apart, and no rms is within 1e-5 relative of the threshold unless it IS the threshold.
    The reference module has no per-window function (its loop is the body of ``analyze``) and does not return rms, so the rms values
    come from oracle.audio_oracle.window_features, the same numpy expression on the same samples.  What ties them to the reference here is
    only that the speech ratio they give equals the one ``analyze`` has just returned (asserted below); that the restatement's other
    outputs equal the reference's is tests/test_audio.py::test_oracle_equals_the_reference_outputs."""
    wav = audio_oracle.synth_wave(case["seconds"], case["seed"]) if "seed" in case else audio_oracle.named_wave(case["named"])
    rms = np.array(audio_oracle.window_features(wav, 16000)["rms"])
    assert float(np.mean(rms >= np.percentile(rms, 60))) == case["out"]["scores"]["speech_ratio"]
    far = lambda a, b: a == b or abs(a - b) > 1e-5 * max(abs(a), abs(b))
    thr = float(np.percentile(rms, 60))
    for i, a in enumerate(rms):
        assert far(a, thr), (case.get("seed", case.get("named")), "rms", i, a, "threshold", thr)
        for j in range(i):
            assert far(a, rms[j]), (case.get("seed", case.get("named")), "rms", i, a, j, rms[j])


def main():
    sys.modules.setdefault("soundfile", types.ModuleType("soundfile"))       # placeholder, never called
    spec = importlib.util.spec_from_file_location("ref_audio", os.path.join(REF, "app", "analyzers", "audio.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = []
    for seed, seconds in CASES:
        wav = audio_oracle.synth_wave(seconds, seed)
        ref._extract_wav_16k = lambda path, w=wav: (None, w, 16000)           # I/O only
        res = ref.analyze("synthetic.wav", {"duration": seconds})
        assert "error" not in res["flags_audio"], res
        out.append({"seed": seed, "seconds": seconds, "samples": int(len(wav)), "out": res})
    # named waveforms (oracle.audio_oracle.named_wave).  Silence and a constant: degenerate windows (log of the 1e-9 floor, zero
    # variance).  The others: noise, a tone on a bin and between bins, an impulse train, a chirp, and last windows of every kind
    for name in audio_oracle.NAMED_WAVES:
        wav = audio_oracle.named_wave(name)
        ref._extract_wav_16k = lambda path, w=wav: (None, w, 16000)
        res = ref.analyze("synthetic.wav", {"duration": 2.0 if name in ("silence", "dc") else len(wav) / 16000})
        assert "error" not in res["flags_audio"], res
        out.append({"named": name, "samples": int(len(wav)), "out": res})
    for case in out:
        check_speech_ratio_is_well_conditioned(case)
    ref._extract_wav_16k = lambda path: (_ for _ in ()).throw(RuntimeError("ffmpeg_convert_failed"))
    out.append({"named": "extract_fails", "meta_duration": 3.4, "out": ref.analyze("x.mp4", {"duration": 3.4})})
    path = os.path.join(HERE, "audio_golden.json")
    if os.path.exists(path):                                 # a regeneration adds cases, it never changes one
        old = {json.dumps({k: v for k, v in c.items() if k != "out"}, sort_keys=True): c["out"] for c in json.load(open(path))["cases"]}
        new = {json.dumps({k: v for k, v in c.items() if k != "out"}, sort_keys=True): c["out"] for c in out}
        for key, res in old.items():
            assert new.get(key) == res, ("an existing case changed", key)
    json.dump({"generator": "tests/golden/make_audio_golden.py", "numpy": np.__version__, "cases": out}, open(path, "w"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
