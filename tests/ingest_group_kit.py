"""tests/ingest_group_check.cpp built with the address and undefined-behaviour sanitizers and run as its own process, in the way
tests/test_stream_plan_host.py builds stream_plan_check.cpp: once per pytest process, nothing loaded into Python, nothing preloaded."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "ai-video-detector_amd", "csrc", "avd_ingest_group.h")

# the three keys of the check program: 96 x 64 BGR dense rows, the same with padded rows, 100 x 66 NV12 -- h, nbands of each
KEY_H, KEY_NBANDS = (64, 64, 66), (5, 5, 5)
LAP_SLOTS = 8


@functools.lru_cache(maxsize=None)
def executable():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    where = tempfile.mkdtemp(prefix="ingest_group_check")
    atexit.register(shutil.rmtree, where, True)
    exe = os.path.join(where, "ingest_group_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "ingest_group_check.cpp")], check=True)
    return exe


def run(*args):
    """-> (status, stdout); anything on stderr (a sanitizer report, a failed property) fails the caller"""
    r = subprocess.run([executable(), *[str(a) for a in args]], capture_output=True, text=True)
    assert not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.returncode, r.stdout


def plan(*clips, bound=None):
    """clips: (key 0 .. 2, n, f0) -> [{'grouped', 'frames', 'rowbuf', 'lappart', 'members': [...], 'out': [...]}, ...], (rowbuf total, lappart total)"""
    status, out = run(*("%d:%d:%d" % c for c in clips), *(["bound=%d" % bound] if bound is not None else []))
    assert status == 0, (status, out)
    groups, total = [], None
    for line in out.splitlines():
        w = line.split()
        if w[0] == "total":
            total = (int(w[2]), int(w[4]))
            continue
        m, o = w.index("members"), w.index("out")
        groups.append({"grouped": int(w[2]), "frames": int(w[4]), "rowbuf": int(w[6]), "lappart": int(w[8]),
                       "members": [int(v) for v in w[m + 1:o]], "out": [int(v) for v in w[o + 1:]]})
    return groups, total
