"""tests/audio_resample_check.cpp built with the address and undefined-behaviour sanitizers and run as its own process, in the way
tests/audio_plan_kit.py builds audio_plan_check.cpp: once per pytest process, nothing loaded into Python, nothing preloaded.

Three programs come out of the one source: one over csrc/avd_audio_resample.h as it is, and one over each of two mutated copies of it (the
controls).  A copy is the header's text with ONE expression replaced -- the replacement must find its place, so a control cannot silently become
a copy of the original."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "ai-video-detector_amd", "csrc", "avd_audio_resample.h")

MUTATIONS = {
    # the tile base m0 * D formed in 32 bits (unsigned arithmetic: it wraps, it is not undefined)
    "base32": ("const long long base = m0 * (long long)r.D;", "const long long base = (long long)(int)((unsigned)m0 * (unsigned)r.D);"),
    # floor instead of ceil: a track's last, partial output is dropped
    "floor": ("const long long count = ((end - begin) * r.U + r.D - 1) / r.D;", "const long long count = std::max<long long>(1, (end - begin) * r.U / r.D);"),
}


def mutated_header(which):
    with open(HEADER) as f:
        text = f.read()
    old, new = MUTATIONS[which]
    assert text.count(old) == 1, ("csrc/avd_audio_resample.h no longer reads as the control expects", old, text.count(old))
    return text.replace(old, new)


@functools.lru_cache(maxsize=None)
def executables():
    """-> {None: the program over the library's header, 'base32': ..., 'floor': ...}"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    where = tempfile.mkdtemp(prefix="audio_resample_check")
    atexit.register(shutil.rmtree, where, True)
    headers = {None: HEADER}
    for which in MUTATIONS:
        headers[which] = os.path.join(where, "avd_audio_resample_%s.h" % which)
        with open(headers[which], "w") as f:
            f.write(mutated_header(which))
    jobs, exes = [], {}
    for which, header in headers.items():
        exes[which] = os.path.join(where, "audio_resample_check_%s" % (which or "library"))
        jobs.append([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                     '-DAUDIO_RESAMPLE_HEADER="%s"' % header, "-o", exes[which], os.path.join(ROOT, "tests", "audio_resample_check.cpp")])
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


@functools.lru_cache(maxsize=None)
def taps(rate):
    """-> (U, D, T, outputs per tile, int64[U, T]) as the header builds them"""
    status, out = run("taps", rate)
    assert status == 0, (status, out[:200])
    lines = out.splitlines()
    U, D, T, tile_out = (int(v) for v in lines[0].split())
    q = np.array([[int(v) for v in line.split()] for line in lines[1:]], np.int64).reshape(U, T)
    return U, D, T, tile_out, q


def plan(rate, n, cuts=(), mutated=None):
    """-> {'refused', 'tile_out', 'n_out', 'ntiles', 'tracks': [(first, count)], 'tiles': [(in0, out0, count, phase)] (first and last beyond 64)}"""
    status, out = run("plan", rate, n, *cuts, mutated=mutated)
    assert status == 0, (status, out)
    lines = out.splitlines()
    head = lines[0].split()
    got = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    for line in lines[1:]:
        name, *vals = line.split()
        got[name] = [tuple(int(x) for x in v.split(":")) for v in vals]
    return got
