"""tests/audio_map_check.cpp built with the address and undefined-behaviour sanitizers and run as its own process, in the way
tests/audio_stream_kit.py builds audio_stream_check.cpp: once per pytest process, nothing loaded into Python, nothing preloaded.

Three programs come out of the one source: one over csrc/avd_audio_map.h as it is, and one over each of two mutated copies of it (the
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
HEADER = os.path.join(CSRC, "avd_audio_map.h")

MUTATIONS = {
    # a track's windows run over its held remainder into the next region
    "windows_overrun": ("append_windows(p.windows, tr.region, c.analysed);", "append_windows(p.windows, tr.region, c.analysed + c.held_after + kRegionAlign);"),
    # a track is handed the neighbouring track's history: the row's slot is where the call path takes the history's address from
    "neighbour_history": ("c.hist_before, tr.slot});", "c.hist_before, p.tracks[(size_t)((t + 1) % nentries)].slot});"),
}


def mutated_header(which):
    with open(HEADER) as f:
        text = f.read()
    old, new = MUTATIONS[which]
    assert text.count(old) == 1, ("csrc/avd_audio_map.h no longer reads as the control expects", old, text.count(old))
    return text.replace(old, new)


@functools.lru_cache(maxsize=None)
def executables():
    """-> {None: the program over the library's header, 'windows_overrun': ..., 'neighbour_history': ...}"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    where = tempfile.mkdtemp(prefix="audio_map_check")
    atexit.register(shutil.rmtree, where, True)
    headers = {None: HEADER}
    for which in MUTATIONS:
        headers[which] = os.path.join(where, "avd_audio_map_%s.h" % which)
        with open(headers[which], "w") as f:
            f.write(mutated_header(which))
    jobs, exes = [], {}
    for which, header in headers.items():
        exes[which] = os.path.join(where, "audio_map_check_%s" % (which or "library"))
        # -I: a mutated copy lies elsewhere and still includes the three audio headers
        jobs.append([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                     '-DAUDIO_MAP_HEADER="%s"' % header, "-o", exes[which], os.path.join(ROOT, "tests", "audio_map_check.cpp")])
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


def plan(rate, win, n, cuts, entries, frames=(), max_windows=1 << 24, mutated=None):
    """One call as the header plans it.  frames: what audio slots 1 ... hold (frames absorbed; the rest follows from the rule).
    -> {'refused', 'total', 'records', 'fresh', 'continued', 'tiles', 'gather', 'saves', 'tracks': [{'slot', 'last', 'begin', 'n', 'region', 'held',
    'fresh', 'first', 'count', 'held_after'}]}"""
    def text(values):
        return ",".join(str(int(v)) for v in values) or "-"
    status, out = run("plan", rate, win, n, text(cuts), text(entries), text(frames), max_windows, mutated=mutated)
    assert status == 0, (status, out)
    lines = out.splitlines()
    head = lines[0].split()
    got = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    got["tracks"] = []
    for line in lines[1:]:
        f = line.split()[1:]
        got["tracks"].append({f[i]: int(f[i + 1]) for i in range(0, len(f), 2)})
    return got
