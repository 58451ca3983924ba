"""The layout plan of a call that continues stream slots (csrc/avd_stream_plan.h), without a GPU.

tests/stream_plan_check.cpp is a stand-alone program: it is compiled here from the header with AddressSanitizer and UBSan and RUN AS A PROGRAM
(nothing is loaded into Python and nothing is preloaded).  Without arguments it enumerates every call of up to four clips with n in
{0, 1, 2, 3} and the three slot states (unmapped, mapped and empty, mapped and filled) -- 1 + 12 + 12^2 + 12^3 + 12^4 = 22 621 calls -- and
checks the properties of the layout rule (include/avd.h, option "stream_map"); with "n:state" arguments it prints one call's plan, which
the tests below compare with layouts written out by hand.
"""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNMAPPED, EMPTY, FILLED = 0, 1, 2


@functools.lru_cache(maxsize=None)
def _executable():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    where = tempfile.mkdtemp(prefix="stream_plan_check")
    atexit.register(shutil.rmtree, where, True)
    exe = os.path.join(where, "stream_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "stream_plan_check.cpp")], check=True)
    return exe


def _run(*args):
    r = subprocess.run([_executable(), *args], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout, r.stderr)      # a sanitizer report ends the program with a non-zero status
    return r.stdout


def plan(*clips):
    """clips: (n, state) -> {'total': ..., 'f0': [...], 'carry': [...], 'clipstart': [...], 'runs': [(first, count), ...]}"""
    lines = _run(*("%d:%d" % c for c in clips)).splitlines()
    head = lines[0].split()
    out = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    for line in lines[1:]:
        name, *vals = line.split()
        out[name] = [tuple(int(x) for x in v.split("+")) for v in vals] if name == "runs" else [int(v) for v in vals]
    return out


def test_the_header_is_plain_host_code():
    """like avd_ingest_clip.h: the standard library only, so that a stand-alone program can include it"""
    text = open(os.path.join(ROOT, "ai-video-detector_amd", "csrc", "avd_stream_plan.h")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


def test_every_call_of_up_to_four_clips():
    out = _run()
    assert out.strip() == "stream plan: 22621 calls checked, 0 failures", out


def test_the_three_stream_layout():
    # [carry_a][a a][carry_b][b][c c]: two continued clips and a new one
    p = plan((2, FILLED), (1, FILLED), (2, UNMAPPED))
    assert p["total"] == 7 and p["own"] == 5 and p["carries"] == 2 and p["segments"] == 3
    assert p["f0"] == [1, 4, 5] and p["carry"] == [0, 3, -1]
    assert p["clipstart"] == [1, 0, 0, 1, 0, 1, 0]
    assert p["runs"] == [(1, 2), (4, 3)]                       # b's frame and c's frames are neighbours: one run


def test_no_filled_slot_is_the_batch_layout():
    p = plan((3, EMPTY), (0, FILLED), (2, UNMAPPED), (1, EMPTY))      # an empty clip restores nothing, whatever its slot holds
    assert p["total"] == 6 and p["carries"] == 0
    assert p["f0"] == [0, 3, 3, 5] and p["carry"] == [-1] * 4
    assert p["clipstart"] == [1, 0, 0, 1, 0, 1]
    assert p["runs"] == [(0, 6)]


def test_a_single_continued_clip_is_the_single_slot_layout():
    p = plan((0, UNMAPPED), (3, FILLED), (0, UNMAPPED))
    assert p["total"] == 4 and p["f0"][1] == 1 and p["carry"] == [-1, 0, -1] and p["segments"] == 1
    assert p["clipstart"] == [1, 0, 0, 0]
    assert p["runs"] == [(1, 3)]


def test_eight_one_frame_clips():
    p = plan(*[(1, FILLED)] * 8)
    assert p["total"] == 16 and p["clipstart"] == [1, 0] * 8
    assert p["runs"] == [(2 * i + 1, 1) for i in range(8)]


def test_a_call_without_frames():
    p = plan((0, FILLED), (0, EMPTY))
    assert p["total"] == 0 and p["runs"] == [] and p["clipstart"] == []


@pytest.mark.parametrize("bad", ["x", "1"])
def test_dump_mode_refuses_what_it_cannot_read(bad):
    r = subprocess.run([_executable(), bad], capture_output=True, text=True)
    assert r.returncode == 2
