"""tests/audio_layout_check.cpp built with the address and undefined-behaviour sanitizers and run as its own process, in the way
tests/audio_resample_kit.py builds audio_resample_check.cpp: once per pytest process, nothing loaded into Python, nothing preloaded."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "ai-video-detector_amd", "csrc", "avd_audio_resample.h")


@functools.lru_cache(maxsize=None)
def executable():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    where = tempfile.mkdtemp(prefix="audio_layout_check")
    atexit.register(shutil.rmtree, where, True)
    exe = os.path.join(where, "audio_layout_check")
    job = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "audio_layout_check.cpp")]
    p = subprocess.run(job, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, (" ".join(job), p.stdout)
    return exe


def run(*args):
    """-> (status, stdout); anything on stderr (a sanitizer report) fails the caller"""
    r = subprocess.run([executable(), *[str(a) for a in args]], capture_output=True, text=True)
    assert not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.returncode, r.stdout


def weights(layout):
    """-> (channels, [eight weights]) as the header derives them"""
    status, out = run("weights", layout)
    assert status == 0, (status, out)
    vals = [int(v) for v in out.split()]
    return vals[0], vals[1:]


def lds(rate):
    """-> (bytes of a layout launch, bytes of today's stereo launch, max_span) of the rate"""
    status, out = run("lds", rate)
    assert status == 0, (status, out)
    return tuple(int(v) for v in out.split())
