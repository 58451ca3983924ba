"""tests/audio_plan_check.cpp built with the address and undefined-behaviour sanitizers and run as its own process, in the way tests/tables_kit.py
builds tables_check.cpp: once per pytest process, nothing loaded into Python, nothing preloaded.

Two programs come out of the one source: one over csrc/avd_audio_plan.h as it is, and one over a mutated copy of it (the control).  The copy is
the header's text with ONE expression replaced -- the replacement must find its place, so the control cannot silently become a copy of the
original."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "ai-video-detector_amd", "csrc", "avd_audio_plan.h")

# windows counted from the buffer's start instead of the track's: a window ends at the next multiple of win of the BUFFER
MUTATION = ("const long long stop = std::min(end, s + (long long)win);", "const long long stop = std::min(end, (s / win + 1) * (long long)win);")


def mutated_header():
    with open(HEADER) as f:
        text = f.read()
    old, new = MUTATION
    assert text.count(old) == 1, ("csrc/avd_audio_plan.h no longer reads as the control expects", old, text.count(old))
    return text.replace(old, new)


@functools.lru_cache(maxsize=None)
def executables():
    """-> (the program over the library's header, the program over the mutated header)"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    where = tempfile.mkdtemp(prefix="audio_plan_check")
    atexit.register(shutil.rmtree, where, True)
    mutant = os.path.join(where, "avd_audio_plan_mutated.h")
    with open(mutant, "w") as f:
        f.write(mutated_header())
    jobs, exes = [], []
    for name, header in (("audio_plan_check", HEADER), ("audio_plan_check_mutated", mutant)):
        exe = os.path.join(where, name)
        exes.append(exe)
        jobs.append([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                     '-DAUDIO_PLAN_HEADER="%s"' % header, "-o", exe, os.path.join(ROOT, "tests", "audio_plan_check.cpp")])
    running = [subprocess.Popen(j, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for j in jobs]
    for j, p in zip(jobs, running):
        out = p.communicate()[0]
        assert p.returncode == 0, (" ".join(j), out)
    return tuple(exes)


def run(*args, mutated=False):
    """-> (status, stdout); anything on stderr (a sanitizer report) fails the caller"""
    r = subprocess.run([executables()[1 if mutated else 0], *[str(a) for a in args]], capture_output=True, text=True)
    assert not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.returncode, r.stdout


def plan(n, win, cuts=(), max_windows=1 << 24, mutated=False):
    """-> {'refused': ..., 'nwin': ..., 'tracks': [(first, count, last)], 'windows': [(off, len, tab)], 'lengths': [...]} of one call"""
    status, out = run(n, win, max_windows, *cuts, mutated=mutated)
    assert status == 0, (status, out)
    lines = out.splitlines()
    head = lines[0].split()
    got = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    for line in lines[1:]:
        name, *vals = line.split()
        got[name] = [int(v) for v in vals] if name == "lengths" else [tuple(int(x) for x in v.split(":")) for v in vals]
    return got
