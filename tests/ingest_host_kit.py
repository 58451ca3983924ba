"""What the ingest host tests share (test_*_host.py; no GPU, no library): tests/ingest_check.cpp built ONCE per pytest process with the address and
undefined-behaviour sanitizers and run as its own process, the writers of its case lines, the one reader of its `key=value` answers, the tests'
own table of the 13 layouts, the status constants and the refusal texts that every layout shares.  Each test file keeps its tables of cases."""
import atexit
import collections
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

from avd_hip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED = 0, -1, -4
HOST, DEVICE = 0, 1
FULL = 0x100
BASE = (0x10000000, 0x20000000, 0x30000000)              # stand-ins for plane pointers: the header never reads through them

# The interface table of include/avd.h, written out: planes 1 and 2 have h // ydiv rows of w // xdiv samples of `sample` bytes.
Layout = collections.namedtuple("Layout", "value name planes px sample ydiv xdiv")
LAYOUTS = (
    Layout(0x00, "BGR24", 1, 3, 1, 1, 1), Layout(0x01, "NV12", 2, 1, 1, 2, 1), Layout(0x02, "I420", 3, 1, 1, 2, 2),
    Layout(0x10, "RGB24", 1, 3, 1, 1, 1), Layout(0x11, "BGRA32", 1, 4, 1, 1, 1), Layout(0x12, "RGBA32", 1, 4, 1, 1, 1), Layout(0x13, "RGBP", 3, 1, 1, 1, 1),
    Layout(0x20, "YUYV422", 1, 2, 1, 1, 1), Layout(0x21, "UYVY422", 1, 2, 1, 1, 1), Layout(0x22, "I422", 3, 1, 1, 1, 2), Layout(0x23, "NV16", 2, 1, 1, 1, 1),
    Layout(0x30, "P010", 2, 2, 2, 2, 1), Layout(0x31, "I010", 3, 2, 2, 2, 2),
)
BY_VALUE = {l.value: l for l in LAYOUTS}
PLANES = {l.value: l.planes for l in LAYOUTS}
PX = {l.value: l.px for l in LAYOUTS}
BGR, NV12, I420 = 0, 1, 2

T_MEM = "mem must be AVD_MEM_HOST or AVD_MEM_DEVICE"
T_GEOM = "bad frame geometry"
T_SMALL = "frame smaller than 32x32: INTER_AREA upscaling is not on the path"
T_NULL_ARRAY = "null plane array of a frame list"
T_NULL_ENTRY = "null plane pointer in a frame list"
T_ODD = "16-bit samples need 2-byte aligned planes and strides"


def t_size(kind):
    return "avd_%s.struct_size is not sizeof(avd_%s)" % (kind, kind)


def t_format(kind):
    return "bad avd_%s.format" % kind


def t_rotate(kind):
    return "avd_%s.rotate must be 0 .. 3 quarter turns" % kind


def t_reserved(kind):
    return "avd_%s.reserved must be 0" % kind


def r256(v):
    return (v + 255) // 256 * 256


# ---- the program ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _executable():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    where = tempfile.mkdtemp(prefix="ingest_check")
    atexit.register(shutil.rmtree, where, True)
    exe = os.path.join(where, "ingest_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "ingest_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def program():
    """-> run(lines): one answer line per case line"""
    exe = _executable()

    def run(lines):
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr)       # a sanitizer report ends the program with a non-zero status
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


@pytest.fixture()
def binding():
    return object.__new__(_lib.Context)                       # no context, no device: what is checked is the binding's own


_TEXT, _LISTS = ("why", "name"), ("off", "bytes", "plane_off", "list_offsets", "rows")


def parse(line):
    """an answer line -> {key: int, [int] or text}; a field the reader does not know is simply there"""
    out = {}
    for field in line.split("|"):
        key, value = field.split("=", 1)
        out[key] = value if key in _TEXT else [int(v) for v in value.split(",") if v] if key in _LISTS else int(value)
    return out


# ---- the case lines ------------------------------------------------------------------------------------------------------------------------
def sub_shape(fmt, h, w):
    """-> (rows, bytes of a row) of planes 1 and 2; a value without a row: as a full-size 8-bit plane"""
    l = BY_VALUE.get(fmt & 0xFF)
    return (h // l.ydiv, w // l.xdiv * l.sample) if l else (h, w)


def row_bytes(fmt, w):
    """bytes of a row of planes 0, 1, 2"""
    c = sub_shape(fmt, 0, w)[1]
    return [w * PX.get(fmt & 0xFF, 1), c, c]


def picture(fmt, mem=HOST, n=2, h=48, w=64, rotate=0, reserved=0, planes=BASE, rs=None, fs=None, size_delta=0):
    """-> the P line of a valid picture of layout fmt (low byte), with whatever the keywords change"""
    rs = row_bytes(fmt, w) if rs is None else list(rs)
    crows = sub_shape(fmt, h, w)[0]
    fs = [rs[0] * h, rs[1] * crows, rs[2] * crows] if fs is None else list(fs)
    return " ".join(str(v) for v in ["P", fmt, mem, n, h, w, rotate, reserved, size_delta, *planes, *rs, *fs])


def frame_list(fmt, addrs, mem=HOST, h=48, w=64, rotate=0, reserved=0, rs=None, null_arrays=0, size_delta=0, n=None):
    """addrs: [plane][frame] addresses (missing planes: zeros) -> the L line"""
    n = len(addrs[0]) if n is None else n
    m = max(n, 0)
    rs = row_bytes(fmt, w) if rs is None else list(rs)
    flat = [a for p in range(3) for a in ((list(addrs[p]) if p < len(addrs) else []) + [0] * m)[:m]]
    return " ".join(str(v) for v in ["L", fmt, mem, n, h, w, rotate, reserved, size_delta, *rs, null_arrays, *flat])


def list_addrs(fmt, n=2, step=0x100000):
    return [[BASE[p] + f * step for f in range(n)] for p in range(PLANES[fmt])]
