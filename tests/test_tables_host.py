"""The host-built resampling tables (csrc/avd_tables.cpp, and band_dy as build_geom forms it) at EVERY frame size the API accepts, without a GPU
and without the library: tests/tables_check.cpp, built with the address and undefined-behaviour sanitizers (tests/tables_kit.py) and run as
child processes.  Nothing is loaded into Python.

a. Invariants of the tables for every s in 32 .. 16384 on each axis (and band_dy for every number of rows per band, 1 .. 14).
b. The tables APPLIED, by a plain restatement of what the kernels are documented to do with them, against the oracle's resizes byte for
   byte: 32 x s and s x 32 for 4 934 sizes s (all up to 4400, every multiple of 32 and of 320, every 64th above 4400, the ends), the 121 class
   crossings, five other destinations.  No tolerance.
Controls: three mutated copies of the builder, each of which the program must report as different from the oracle -- at images and with
counts that were found with the ORACLE alone, mutated the same way, so that they are properties of the reference.

Measured where this was written (8 CPUs, the sweep in four parts side by side): 5 s to build the program, 27 s of wall time for the sweep,
76 s of CPU time in all parts together -- 20 s of it without the sanitizers, most of that in the oracle's own float chains."""
import os
import subprocess

import numpy as np
import pytest

from tests import tables_kit as K


@pytest.fixture(scope="module")
def sweep():
    """the whole sweep, in parts that run side by side: the answers of all parts"""
    exe = K.executable()
    parts = max(1, min(4, os.cpu_count() or 1))
    running = [subprocess.Popen([exe, "full", "64", str(p), str(parts)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for p in range(parts)]
    answers = []
    for p in running:
        out, err = p.communicate()
        failed = [l for l in out.splitlines() if l.startswith("FAIL")]
        assert p.returncode == 0 and not err and not failed, (p.returncode, err[-2000:], failed[:10])     # a sanitizer report ends a part with a non-zero status
        answers.append(dict(l.split("=", 1) for l in out.splitlines()))
    total = lambda key: sum(int(a[key]) for a in answers)
    listed = lambda key: sorted(int(v) for a in answers for v in a[key].split(",") if v)
    seconds = sum(float(a["invariants_seconds"]) + float(a["comparisons_seconds"]) for a in answers)
    print("tables_check: %d parts, %.0f s of CPU time in all" % (parts, seconds))
    return total, listed


def test_invariants_and_oracle_at_every_size(sweep):
    total, _ = sweep
    assert total("failures") == 0
    # 4369 sizes up to 4400, 375 multiples of 32 above, 187 more every 64th, 16383, 15679, 15681 (every multiple of 320 is one of 32)
    assert total("compared_sizes") == 4934
    assert total("compared_geometries") == 2 * 4934 - 1 + 100                    # 32 x 32 once; the crossings that are no axis sweep


def test_flip_sizes(sweep):
    """`fast` is set exactly for the 512 multiples of 32 minus the sizes at which cv2's reciprocal of a reciprocal is not the quotient (the
    program FAILs otherwise); the list the program computes from cv2's expression is the one the GPU sweep visits."""
    total, listed = sweep
    flips = listed("flip32")
    assert flips == K.flip_sizes(32)
    assert len(flips) == 62 and flips[:11] == K.FIRST_FLIPS == [1568, 2976, 3136, 3168, 3296, 3360, 3424, 3744, 3936, 5952, 6272]
    assert total("flip_sizes") == 62 and total("fast_sizes") == 512 - 62
    # the 320-px resize: one such size, and the exact 2 x 2 that cv2 reroutes from INTER_LINEAR to INTER_AREA
    assert listed("flip320") == K.flip_sizes(320) == [15680]
    assert listed("reroute320") == [640]


def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def test_the_library_builder_passes_where_the_controls_fail():
    for image, area in ((_noise(1, 32, 3136), (32, 32)), (_noise(1, 3136, 32), (32, 32)), (_noise(1, 32, 201), (32, 200)), (_noise(1, 201, 32), (200, 32))):
        assert K.image_differences(0, image, area) == (0, 0), image.shape


@pytest.mark.parametrize("h,w,flipped", [(32, 3136, True), (3136, 32, True), (32, 5952, True), (32, 1568, False), (32, 3104, False)])
def test_control_scale_as_quotient(oracle, h, w, flipped):
    """scale = (double)src / dst instead of cv2's 1. / ((double)dst / src): the flip sizes take the integer path.  What that path gives is
    written out here (box sums times 1.f / area, half-even) and compared with the oracle ALONE first: 8, 3 and 3 cells differ, none at 1568
    (a flip size where the two paths happen to agree on this image) and none at 3104 (no flip size)."""
    image = _noise(1, h, w)
    sums = image.astype(np.int64).reshape(32, h // 32, 32, w // 32).sum(axis=(1, 3))
    integer_path = np.rint(sums.astype(np.float32) * (np.float32(1) / np.float32((h // 32) * (w // 32)))).astype(np.uint8)
    want = int(np.count_nonzero(integer_path != oracle.resize_area(image, 32, 32)))
    assert (want > 0) == flipped and want == {(32, 3136): 8, (3136, 32): 3, (32, 5952): 3}.get((h, w), 0)
    assert K.image_differences(1, image)[1] == want


@pytest.mark.parametrize("seed,h,w,want", [(1, 32, 3136, 1724), (1, 3136, 32, 1752), (2, 32, 4099, 1990), (2, 4099, 32, 1877), (4, 32, 2500, 0)])
def test_control_q11_half_up(seed, h, w, want):
    """to_q11 rounding half up: a weight is an exact half of 1 / 2048 only where the float source coordinate has 12 fraction bits left,
    from 2048 px on.  want: bytes of the 320 x 320 image that the oracle with half-up in its own sat_short_f changes (none at 2500 px)."""
    assert K.image_differences(2, _noise(seed, h, w))[0] == want


@pytest.mark.parametrize("h,w,area,want", [(32, 201, (32, 200), 53), (201, 32, (200, 32), 61), (203, 407, (200, 400), 1366), (32, 3136, (32, 32), 0)])
def test_control_tap_threshold(h, w, area, want):
    """1e-2 for 1e-3 in area_axis.  With 32 cells the share of a source sample in a cell is a multiple of 1 / 32 (or a rounding error of
    one), never between 1e-3 and 1e-2: the control cannot show there, at any size (the last case).  It shows with 200 cells over 201 samples,
    where the shares are multiples of 1 / 200.  want: cells that the oracle with 1e-2 in its own area_tab changes."""
    assert K.image_differences(3, _noise(1, h, w), area)[1] == want
