"""The fused ingest at the frame sizes that matter to the host-built tables: every width and every height up to 4400 (one axis at a time),
the sizes at which cv2's double arithmetic flips INTER_AREA off its integer path, the table classes crossed in two dimensions, the
resolutions people upload, and the geometry cache cycled past its four entries.

Everything is compared with the CPU oracle BIT FOR BIT through tests/ingest_gpu_kit.py: small320, the hash, both Laplacian moments and
the "area" cells.  There is no tolerance in this file.  Every case reads "ingest_plan" back and asserts its h and w.  The content is
white noise seeded from (h, w): it keeps the area cells near the hash threshold and every rounding boundary in reach.

tests/test_tables_host.py checks the same tables at every size without a GPU; a size that passes there and fails here is a kernel defect."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from avd_hip import synth  # noqa: E402
from tests.ingest_gpu_kit import P_H, P_W, check_outputs, plan, reference  # noqa: E402
from tests.tables_kit import FIRST_FLIPS, flip_sizes  # noqa: E402
from tests.test_nv12 import _planes  # noqa: E402


def _seed(h, w):
    return h * 100003 + w


def _bgr_case(ctx, oracle, n, h, w):
    frames = synth.random_frames(n, h, w, seed=_seed(h, w))
    got = ctx.preprocess_bgr(frames)
    assert (plan(ctx)[P_H], plan(ctx)[P_W]) == (h, w), (h, w, plan(ctx))
    check_outputs(ctx, got, reference(oracle, frames), (h, w))


# ---- axis sweeps: 32 x w for every w, h x 32 for every h -------------------------------------------------------------------------------
# Runs of 256 consecutive sizes per test; every call misses the four-entry geometry cache, so a run is 256 evictions and rebuilds as well.
SWEEP_LAST, RUN = 4400, 256
RUNS = [(a, min(a + RUN - 1, SWEEP_LAST)) for a in range(32, SWEEP_LAST + 1, RUN)]
assert len(RUNS) == 18 and RUNS[0] == (32, 287) and RUNS[-1] == (4384, 4400)


def _run(ctx, oracle, first, last, shape):
    failed = []
    for s in range(first, last + 1):
        try:
            _bgr_case(ctx, oracle, 1, *shape(s))
        except AssertionError as e:                     # the SIZE fails, not the run: go on and name every one
            failed.append((shape(s), str(e)[:200]))
    assert not failed, (len(failed), failed[:8])


@pytest.mark.parametrize("first,last", RUNS, ids=["w%d-%d" % r for r in RUNS])
def test_every_width(ctx, oracle, first, last):
    _run(ctx, oracle, first, last, lambda s: (32, s))


@pytest.mark.parametrize("first,last", RUNS, ids=["h%d-%d" % r for r in RUNS])
def test_every_height(ctx, oracle, first, last):
    _run(ctx, oracle, first, last, lambda s: (s, 32))


# ---- the flip sizes: a general-path table with count == iscale, begin % iscale == 0 and one weight missing -----------------------------
FLIPS = flip_sizes(32)          # tests/test_tables_host.py: the list the table program computes from cv2's expression is this one
FLIPS_AND_320 = sorted(set(FLIPS) | set(flip_sizes(320)))


def test_flip_list():
    assert len(FLIPS) == 62 and FLIPS[:11] == FIRST_FLIPS and flip_sizes(320) == [15680] and 15680 in FLIPS and len(FLIPS_AND_320) == 62


@pytest.mark.parametrize("s", FLIPS_AND_320)
def test_flip_size_as_width(ctx, oracle, s):
    _bgr_case(ctx, oracle, 1, 32, s)


@pytest.mark.parametrize("s", FLIPS_AND_320)
def test_flip_size_as_height(ctx, oracle, s):
    _bgr_case(ctx, oracle, 1, s, 32)


# ---- class crossings: fast x fast, fast x general, flip x fast, uniform4 x general, the 2 x 2 reroute, up on one axis and down on the other ----
CROSS = (32, 64, 96, 128, 256, 320, 333, 640, 641, 1568, 3136)


@pytest.mark.parametrize("h", CROSS)
@pytest.mark.parametrize("w", CROSS)
def test_class_crossing(ctx, oracle, h, w):
    _bgr_case(ctx, oracle, 2, h, w)


# ---- the resolutions people upload ------------------------------------------------------------------------------------------------------
LANDSCAPE = [(144, 176), (288, 352), (240, 320), (360, 480), (480, 640), (480, 720), (576, 720), (480, 848), (480, 854), (540, 960), (576, 1024),
             (600, 800), (768, 1024), (720, 960), (768, 1366), (900, 1600), (1080, 1440), (1088, 1920), (1080, 2048), (1200, 1920), (1440, 2560),
             (1440, 3440), (1600, 2560), (2160, 4096), (2880, 5120), (4320, 7680)]
PORTRAIT_AND_SQUARE = [(640, 360), (854, 480), (1280, 720), (1920, 1080), (3840, 2160), (2340, 1080), (2400, 1080), (2532, 1170), (1792, 828),
                       (2778, 1284), (720, 720), (1080, 1080)]
RESOLUTIONS = LANDSCAPE + PORTRAIT_AND_SQUARE
assert len(RESOLUTIONS) == 38 and all(h % 2 == 0 and w % 2 == 0 for h, w in RESOLUTIONS)
_ids = ["%dx%d" % (w, h) for h, w in RESOLUTIONS]


@pytest.mark.parametrize("h,w", RESOLUTIONS, ids=_ids)
def test_resolution_bgr(ctx, oracle, h, w):
    _bgr_case(ctx, oracle, 1, h, w)


def _yuv_case(ctx, oracle, h, w, i420):
    y, uv = _planes(1, h, w, seed=_seed(h, w) + 1)
    got = ctx.preprocess_i420(*synth.nv12_to_i420(y, uv)) if i420 else ctx.preprocess_nv12(y, uv)
    assert (plan(ctx)[P_H], plan(ctx)[P_W]) == (h, w), (h, w, plan(ctx))
    check_outputs(ctx, got, reference(oracle, oracle.nv12_to_bgr(y, uv)), (h, w, "i420" if i420 else "nv12"))


@pytest.mark.parametrize("h,w", RESOLUTIONS, ids=_ids)
def test_resolution_nv12(ctx, oracle, h, w):
    _yuv_case(ctx, oracle, h, w, False)


@pytest.mark.parametrize("h,w", RESOLUTIONS[:25] + RESOLUTIONS[26:], ids=_ids[:25] + _ids[26:])       # the 8K frame: BGR and NV12 only
def test_resolution_i420(ctx, oracle, h, w):
    _yuv_case(ctx, oracle, h, w, True)


# ---- the geometry cache: five geometries in turn through four entries ------------------------------------------------------------------
def test_cache_cycling(ctx, oracle):
    """Least-recently-used eviction with one geometry more than entries: every visit rebuilds tables in the entry of the geometry that is
    needed next.  Two pairs share a width or a height.  Every visit gives the bytes of the first, and the first the oracle's."""
    cycle = [(480, 854), (480, 848), (854, 480), (576, 720), (768, 1366)]
    frames = {g: synth.random_frames(1, *g, seed=_seed(*g)) for g in cycle}
    first = {}
    for visit in range(3):
        for g in cycle:
            got = ctx.preprocess_bgr(frames[g])
            assert (plan(ctx)[P_H], plan(ctx)[P_W]) == g, (visit, g)
            got = tuple(got) + (ctx.debug_fetch("area", (1, 32, 32), np.uint8),)
            if visit == 0:
                check_outputs(ctx, got[:4], reference(oracle, frames[g]), g)
                first[g] = got
            for name, a, b in zip(("small320", "hash", "lap_sum", "lap_sumsq", "area"), got, first[g]):
                assert np.array_equal(a, b), (visit, g, name)
