"""What the two table tests share (test_tables_host.py: no GPU, no library; test_gpu_geometry_sweep.py): the sizes at which cv2's own double
arithmetic flips a decision, and tests/tables_check.cpp built ONCE per pytest process with the address and undefined-behaviour sanitizers
and run as its own process, in the way tests/ingest_host_kit.py builds ingest_check.cpp.

The program links csrc/avd_tables.cpp four times: as it is, and three mutated copies (the controls).  A copy is the source text with ONE
expression replaced -- every replacement must find its place, so a control cannot silently become a copy of the original -- compiled with
its external names renamed, so that all four builders live in one program."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ai-video-detector_amd", "csrc")
ORACLE = os.path.join(ROOT, "oracle")

SIZE_MIN, SIZE_MAX = 32, 16384
FIRST_FLIPS = [1568, 2976, 3136, 3168, 3296, 3360, 3424, 3744, 3936, 5952, 6272]


def flip_sizes(dst=32):
    """The sizes s that dst divides at which cv2's `scale = 1. / ((double)dst / s)` is not s / dst (the classic 1 / (1 / 49.) != 49): there
    |scale - iscale| >= DBL_EPSILON, and INTER_AREA leaves its integer path although the scale "is" an integer.  Python's floats are the
    same IEEE doubles, and this is the same expression."""
    return [s for s in range(dst, SIZE_MAX + 1, dst) if 1. / (float(dst) / s) != s // dst]


# (text of csrc/avd_tables.cpp, its replacement, occurrences) per control
MUTATIONS = {
    # scale = (double)src / dst instead of cv2's reciprocal of a reciprocal
    1: [("1. / ((double)dst / src)", "((double)src / dst)", 1),
        ("1. / ((double)dst_w / src_w)", "((double)src_w / dst_w)", 1), ("1. / ((double)dst_h / src_h)", "((double)src_h / dst_h)", 1)],
    # half-up instead of half-even in to_q11
    2: [("int i = round_half_even(v * 2048.f);", "int i = (int)std::floor(v * 2048.f + 0.5f);", 1)],
    # the smallest share of a source sample that still counts as a tap
    3: [("> 1e-3)", "> 1e-2)", 2)],
}
EXTERNALS = ("build_linear_tab", "build_area_tab", "build_band_dy", "build_fb_consts", "build_yuv_consts", "yuv_index_window")


def mutated_source(which):
    with open(os.path.join(CSRC, "avd_tables.cpp")) as f:
        text = f.read()
    for old, new, count in MUTATIONS[which]:
        assert text.count(old) == count, ("csrc/avd_tables.cpp no longer reads as control %d expects" % which, old, text.count(old))
        text = text.replace(old, new)
    return text


@functools.lru_cache(maxsize=None)
def executable():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cxx and cc, "no host compiler"
    where = tempfile.mkdtemp(prefix="tables_check")
    atexit.register(shutil.rmtree, where, True)
    # frame pointers: the address sanitizer records a stack at every allocation, and area_axis allocates per cell; with them that walk is short
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    # csrc/Makefile's floating-point flags for the library's file, oracle/Makefile's for the oracle's
    cxxflags = ["-std=c++17", "-O2", "-g", "-Wall", "-ffp-contract=off", "-fno-fast-math", *sanitize, "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-D__HIP_PLATFORM_AMD__",     # avd_internal.h includes the HIP runtime's header
                "-I" + CSRC, "-I" + ORACLE]
    cflags = ["-std=gnu11", "-O2", "-g", "-ffp-contract=off", "-fno-fast-math", "-fno-unsafe-math-optimizations", "-Wall", "-Wextra",
              "-Wno-unused-parameter", *sanitize]
    jobs = [[cxx, *cxxflags, "-Wextra", "-Werror", "-c", os.path.join(ROOT, "tests", "tables_check.cpp"), "-o", os.path.join(where, "check.o")],
            [cxx, *cxxflags, "-c", os.path.join(CSRC, "avd_tables.cpp"), "-o", os.path.join(where, "tables.o")],
            [cc, *cflags, "-c", os.path.join(ORACLE, "avd_oracle.c"), "-o", os.path.join(where, "oracle.o")]]
    for which in MUTATIONS:
        src = os.path.join(where, "tables_m%d.cpp" % which)
        with open(src, "w") as f:
            f.write(mutated_source(which))
        jobs.append([cxx, *cxxflags, *["-D%s=%s_m%d" % (name, name, which) for name in EXTERNALS], "-c", src, "-o", os.path.join(where, "tables_m%d.o" % which)])
    running = [subprocess.Popen(j, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for j in jobs]
    for j, p in zip(jobs, running):
        out = p.communicate()[0]
        assert p.returncode == 0, (" ".join(j), out)
    exe = os.path.join(where, "tables_check")
    subprocess.run([cxx, *sanitize, "-o", exe, *[j[-1] for j in jobs], "-lm"], check=True)
    return exe


def run(*args):
    """-> {key: text} of the program's answer lines; a non-zero exit status, anything on stderr or a FAIL line fails the caller"""
    r = subprocess.run([executable(), *[str(a) for a in args]], capture_output=True, text=True)
    failed = [l for l in r.stdout.splitlines() if l.startswith("FAIL")]
    assert r.returncode == 0 and not r.stderr and not failed, (r.returncode, r.stderr[-2000:], failed[:10])
    return dict(l.split("=", 1) for l in r.stdout.splitlines())


def image_differences(which, image, area_shape=(32, 32)):
    """builder `which` (0: the library's own) on a 2-D uint8 image -> (bytes of the 320 x 320 INTER_LINEAR image, bytes of the INTER_AREA
    image of area_shape) that differ from the oracle's"""
    h, w = image.shape
    with tempfile.NamedTemporaryFile(suffix=".gray") as f:
        f.write(image.tobytes())
        f.flush()
        out = run("image", which, h, w, area_shape[0], area_shape[1], f.name)
    return int(out["linear_differs"]), int(out["area_differs"])
