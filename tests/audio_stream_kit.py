"""tests/audio_stream_check.cpp built with the address and undefined-behaviour sanitizers and run as its own process, in the way
tests/audio_resample_kit.py builds audio_resample_check.cpp: once per pytest process, nothing loaded into Python, nothing preloaded.

Three programs come out of the one source: one over csrc/avd_audio_stream.h as it is, and one over each of two mutated copies of it (the
controls).  A copy is the header's text with ONE expression replaced -- the replacement must find its place, so a control cannot silently become
a copy of the original."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ai-video-detector_amd", "csrc")
HEADER = os.path.join(CSRC, "avd_audio_stream.h")

MUTATIONS = {
    # the T/2 hold-back dropped: outputs are formed whose last taps have not arrived yet
    "no_holdback": ("const long long usable = last ? n_frames : std::max<long long>(0, n_frames - r.T / 2);", "const long long usable = last ? n_frames : n_frames + 0;"),
    # the history one frame short: the first new output's first tap is gone
    "short_history": ("r.T > 0 ? r.T - 1 : 0", "r.T > 1 ? r.T - 2 : 0"),
}


def mutated_header(which):
    with open(HEADER) as f:
        text = f.read()
    old, new = MUTATIONS[which]
    assert text.count(old) == 1, ("csrc/avd_audio_stream.h no longer reads as the control expects", old, text.count(old))
    return text.replace(old, new)


@functools.lru_cache(maxsize=None)
def executables():
    """-> {None: the program over the library's header, 'no_holdback': ..., 'short_history': ...}"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    where = tempfile.mkdtemp(prefix="audio_stream_check")
    atexit.register(shutil.rmtree, where, True)
    headers = {None: HEADER}
    for which in MUTATIONS:
        headers[which] = os.path.join(where, "avd_audio_stream_%s.h" % which)
        with open(headers[which], "w") as f:
            f.write(mutated_header(which))
    jobs, exes = [], {}
    for which, header in headers.items():
        exes[which] = os.path.join(where, "audio_stream_check_%s" % (which or "library"))
        # -I: a mutated copy lies elsewhere and still includes "avd_audio_resample.h"
        jobs.append([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                     '-DAUDIO_STREAM_HEADER="%s"' % header, "-o", exes[which], os.path.join(ROOT, "tests", "audio_stream_check.cpp")])
    running = [subprocess.Popen(j, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for j in jobs]
    for j, p in zip(jobs, running):
        out = p.communicate()[0]
        assert p.returncode == 0, (" ".join(j), out)
    return exes


def run(*args, mutated=None):
    """-> (status, stdout); anything on stderr (a sanitizer report) fails the caller"""
    r = subprocess.run([executables()[mutated], *[str(a) for a in args]], capture_output=True, text=True)
    assert not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.returncode, r.stdout


def outputs_after(rate, frames, last=False):
    """M of the rule as the header computes it (rate 0: an unconverted track)"""
    status, out = run("m", rate, frames, int(bool(last)))
    assert status == 0, (status, out)
    return int(out)


def plan(rate, win, before, n, last=False, mutated=None):
    """-> {'refused', 'm_before', 'm_after', 'held_before', 'held_after', 'hist_before', 'hist_after', 'windows', 'analysed', 'tile_out', 'ntiles',
    'tiles': [(in0, out0, count, phase)] (first and last beyond 64)}"""
    status, out = run("plan", rate, win, before, n, int(bool(last)), mutated=mutated)
    assert status == 0, (status, out)
    lines = out.splitlines()
    head = lines[0].split()
    got = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    got["tiles"] = [tuple(int(x) for x in v.split(":")) for v in lines[1].split()[1:]]
    return got
