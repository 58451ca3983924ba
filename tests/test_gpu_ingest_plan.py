"""The ingest kernels (avd_preprocess.hip) over every class of the band plan and every alignment the launcher tells apart.

The generic kernel k_preprocess and the staged kernel k_preprocess_vec (NI row chunks per lane) are written once and templated on a
fill policy per layout; which fill runs and how many rows a band has follow from the width alone (band_plan) and from the 16-byte alignment of the input
(launch_preprocess).  Every case here names the kernel and the rows per band it was written for and reads both back from the
"ingest_plan" debug buffer, so a sweep that silently took another kernel fails instead of passing.

Everything is compared with the CPU oracle BIT FOR BIT: small320, hash, lap_sum, lap_sumsq and the "area" debug buffer.  There
is no tolerance in this file.

The expected kernels and row counts are literals, taken from the plan as avd_preprocess.hip documents it: a band has 14 rows
while (rows + 2) tile rows fit 48 KiB of LDS (w up to about 3040), then 13, 12, ... down to 1 (3 rows from w = 8161, 2 from
9793, 1 from 12257); the staged kernel holds NI = 3 / 4 / 6 / 8 / 9 row chunks per lane for w <= 672 / 1024 / 1360 / 2048 /
4096 and has 7-row bands above 2048.  They are not recomputed here by a copy of band_plan."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from avd_hip import synth  # noqa: E402
from tests.ingest_gpu_kit import P_KERNEL, P_NBANDS, check_outputs, reference  # noqa: E402
from tests.ingest_gpu_kit import check_plan as _check_plan  # noqa: E402
from tests.ingest_gpu_kit import heights as _heights  # noqa: E402
from tests.ingest_gpu_kit import heights_even as _heights_nv12  # noqa: E402
from tests.ingest_gpu_kit import plan as _plan  # noqa: E402
from tests.test_nv12 import _planes  # noqa: E402

# enum IngestKernel (avd_internal.h) and the layout of "ingest_plan" (include/avd.h)
BGR_SCALAR, BGR_VEC16, BGR_STAGED, NV12_SCALAR, NV12_TABLES = range(5)
KERNEL_NAMES = ("bgr_scalar", "bgr_vec16", "bgr_staged", "nv12_scalar", "nv12_tables")


def _check_outputs(ctx, oracle, got, ref_bgr, tag):
    """got = (small320, hash, lap_sum, lap_sumsq) of the call that just ran on ctx; ref_bgr = the frames the oracle sees."""
    check_outputs(ctx, got, reference(oracle, ref_bgr), tag)


def _expand(table, heights):
    out = []
    for kernel, ni, widths, rows in table:
        rows = rows if isinstance(rows, tuple) else (rows,) * len(widths)
        for w, r in zip(widths, rows):
            out += [pytest.param(kernel, ni, w, r, h, id=f"{KERNEL_NAMES[kernel]}-ni{ni}-w{w}-r{r}-h{h}") for h in heights(r)]
    return out


def test_ingest_plan_needs_a_launch():
    import avd_hip
    with avd_hip.Context(0) as c:
        with pytest.raises(avd_hip.AvdError, match="ingest_plan"):
            c.debug_fetch("ingest_plan", (8,), np.int32)
        with pytest.raises(avd_hip.AvdError, match="unknown debug buffer"):
            c.debug_fetch("ingest_plans", (8,), np.int32)


# ---- (a) BGR, contiguous host frames: every plan class x the last-band heights -------------------------------------------------
# kernel, NI, widths, rows per band.  Staged: w = 32 has 128 tile rows per pass (more than the tile: surplus lanes re-read the last
# row), 48 has 85 (chunks does not divide 256: one idle lane), 256 has exactly the tile's 16, 272 one short of it (15), 4096 one
# chunk per lane; the other widths sit on either side of each NI boundary.
BGR_PLANS = [
    (BGR_STAGED, 3, (32, 48, 256, 272, 592, 672), 14),
    (BGR_STAGED, 4, (688, 1024), 14),
    (BGR_STAGED, 6, (1040, 1360), 14),
    (BGR_STAGED, 8, (1376, 2048), 14),
    (BGR_STAGED, 9, (2064, 4096), 7),
    (BGR_VEC16, 0, (4112, 4448, 4896, 5440, 6128, 6992, 8176, 9808, 12272, 16384), (9, 8, 7, 6, 5, 4, 3, 2, 1, 1)),
    (BGR_SCALAR, 0, (3041, 3473, 4881, 6977, 8161, 9793, 12257, 16383), (13, 11, 7, 4, 3, 2, 1, 1)),
    (BGR_SCALAR, 0, (12258, 12259), 1),         # the ragged-quad mask (w & 3) on one-row bands
    (BGR_SCALAR, 0, (9794, 9795), 2),           # and on two-row bands: the peeled boundary rows with an empty interior loop
]


@pytest.mark.parametrize("kernel,ni,w,rows,h", _expand(BGR_PLANS, _heights))
def test_bgr_plan_classes(ctx, oracle, kernel, ni, w, rows, h):
    frames = synth.random_frames(2, h, w, seed=h * 7 + w)
    got = ctx.preprocess_bgr(frames)
    _check_plan(ctx, h, w, kernel, rows, ni)
    _check_outputs(ctx, oracle, got, frames, (h, w))


def test_bgr_tall_and_thin(ctx, oracle):
    """16384 x 32: 1171 bands of one frame, k_hash sums 4 684 partial moment slots, the area_fast cells hold 512 x 1 pixels."""
    frames = synth.random_frames(1, 16384, 32, seed=16384)
    got = ctx.preprocess_bgr(frames)
    _check_plan(ctx, 16384, 32, BGR_STAGED, 14, 3)
    assert _plan(ctx)[P_NBANDS] == 1171
    _check_outputs(ctx, oracle, got, frames, (16384, 32))


# ---- (b) NV12, contiguous host planes -------------------------------------------------------------------------------------------
# With an odd number of rows per band a band starts on an odd row, so the chroma row it shares with the row above is split
# across two workgroups of the table fill.
NV12_PLANS = [
    (NV12_TABLES, 0, (48, 2064, 4112, 4448, 6128, 8176, 9808, 12272, 16384), (14, 7, 9, 8, 5, 3, 2, 1, 1)),
    (NV12_SCALAR, 0, (34, 1922, 8190, 12274, 16382), (14, 14, 3, 1, 1)),
]


@pytest.mark.parametrize("kernel,ni,w,rows,h", _expand(NV12_PLANS, _heights_nv12))
def test_nv12_plan_classes(ctx, oracle, kernel, ni, w, rows, h):
    y, uv = _planes(2, h, w, seed=h + w)
    got = ctx.preprocess_nv12(y, uv)
    # the widest table launch asks for more than 48 KiB of dynamic LDS: 3 tile rows of 16416 B + the three conversion tables
    lds = 57696 if (kernel, w) == (NV12_TABLES, 16384) else None          # 3 * 16416 + 3 * 4 * 704
    _check_plan(ctx, h, w, kernel, rows, ni, lds)
    _check_outputs(ctx, oracle, got, oracle.nv12_to_bgr(y, uv), (h, w))


# ---- (c) alignment dispatch: device tensors viewed out of a larger flat buffer ----------------------------------------------------
# launch_preprocess takes the vector kernels only if base pointer, row stride and frame stride of every plane are multiples of 16.
# view name -> (base offset, row padding, make the frame stride odd) for the Y / BGR plane and the same for the UV plane
VIEWS = {
    "base+3": ((3, 16, False), (0, 16, False)),
    "row_stride%16=8": ((0, 8, False), (0, 16, False)),
    "frame_stride_odd": ((0, 16, True), (0, 16, False)),
    "aligned_padded": ((32, 16, False), (48, 16, False)),
    "uv_base+2": ((0, 16, False), (2, 16, False)),
    "uv_row_stride%16=8": ((0, 16, False), (0, 8, False)),
}
# image -> (kind, n, h, w, rows per band, kernel when everything is aligned, its NI)
IMAGES = {
    "bgr45x832": ("bgr", 2, 45, 832, 14, BGR_STAGED, 4),
    "bgr44x2064": ("bgr", 2, 44, 2064, 7, BGR_STAGED, 9),
    "nv12_46x2064": ("nv12", 2, 46, 2064, 7, NV12_TABLES, 0),
}
ALIGN_CASES = [(img, view) for img, spec in IMAGES.items() for view in VIEWS if spec[0] == "nv12" or not view.startswith("uv_")]


def _device_view(torch, host, plane_spec):
    """host uint8[n, rows, row_bytes...] -> a device view with the same values: base pointer = a 16-byte boundary + offset, row stride =
    row bytes + pad, frame stride = the next multiple of 16 that holds the rows (+ 1 if odd is asked for)."""
    offset, pad, odd = plane_spec
    n, rows = host.shape[:2]
    row_bytes = int(np.prod(host.shape[2:]))
    rs = row_bytes + pad
    fs = (rs * rows + 15) // 16 * 16 + (1 if odd else 0)
    flat = torch.empty(16 + offset + n * fs + 16, dtype=torch.uint8, device="cuda:0")
    offset += -flat.data_ptr() % 16
    tail = (3, 1) if host.ndim == 4 else (1,)
    # laid out on the host and uploaded as one flat copy: no strided copy kernel of torch's is needed
    staged = np.zeros(flat.numel(), np.uint8)
    np.lib.stride_tricks.as_strided(staged[offset:], host.shape, (fs, rs) + tail)[...] = host
    flat.copy_(torch.from_numpy(staged))
    view = flat.as_strided(tuple(host.shape), (fs, rs) + tail, offset)
    assert (view.data_ptr() - plane_spec[0]) % 16 == 0 and view.stride(1) % 16 == pad % 16 and view.stride(0) % 16 == (1 if odd else 0)
    return view


@pytest.fixture(scope="module")
def align_inputs(oracle):
    """The three images and their oracle results, formed once and left unchanged."""
    out = {}
    for name, (kind, n, h, w, rows, kernel, ni) in IMAGES.items():
        if kind == "bgr":
            planes = (synth.random_frames(n, h, w, seed=h * 7 + w),)
            bgr = planes[0]
        else:
            planes = _planes(n, h, w, seed=h + w)
            bgr = oracle.nv12_to_bgr(*planes)
        out[name] = (planes, oracle.preprocess_bgr(bgr), reference(oracle, bgr)[4])
    return out


@pytest.mark.parametrize("image,view", ALIGN_CASES, ids=[f"{i}-{v}" for i, v in ALIGN_CASES])
def test_alignment_dispatch(ctx, align_inputs, image, view):
    """Every view of an image equals the oracle (so they equal each other), and only the fully aligned one runs a vector kernel."""
    torch = pytest.importorskip("torch")
    kind, n, h, w, rows, kernel, ni = IMAGES[image]
    planes, want, o_area = align_inputs[image]
    views = [_device_view(torch, p, spec) for p, spec in zip(planes, VIEWS[view])]
    got = ctx.preprocess_bgr(views[0]) if kind == "bgr" else ctx.preprocess_nv12(*views)
    if view == "aligned_padded":
        _check_plan(ctx, h, w, kernel, rows, ni)
    else:
        _check_plan(ctx, h, w, BGR_SCALAR if kind == "bgr" else NV12_SCALAR, rows, 0)
    area = ctx.debug_fetch("area", (n, 32, 32), np.uint8)
    for name, a, b in zip(("small320", "hash", "lap_sum", "lap_sumsq", "area"), got + (area,), want + (o_area,)):
        assert np.array_equal(a, b), (image, view, name)


# ---- (d) seeded sweep over the vector paths -----------------------------------------------------------------------------------------
def _sweep_draws():
    rng = np.random.default_rng(2064)
    return [(int(rng.integers(1, 4)), int(rng.integers(32, 121)), 16 * int(rng.integers(2, 261))) for _ in range(24)]


@pytest.mark.parametrize("n,h,w", _sweep_draws())
def test_vector_paths_random_geometries(ctx, oracle, n, h, w):
    """Widths that are multiples of 16 (the existing random sweep draws none): the staged kernel up to 4096 px, the generic kernel's 16-byte
    fill above, and the NV12 table fill on the draws of even height."""
    frames = synth.random_frames(n, h, w, seed=h * 1000 + w)
    got = ctx.preprocess_bgr(frames)
    assert _plan(ctx)[P_KERNEL] == (BGR_STAGED if w <= 4096 else BGR_VEC16), (h, w)
    _check_outputs(ctx, oracle, got, frames, ("bgr", n, h, w))
    if h % 2 == 0:
        y, uv = _planes(n, h, w, seed=h * 1000 + w + 1)
        got = ctx.preprocess_nv12(y, uv)
        assert _plan(ctx)[P_KERNEL] == NV12_TABLES, (h, w)
        _check_outputs(ctx, oracle, got, oracle.nv12_to_bgr(y, uv), ("nv12", n, h, w))


# ---- (e) extreme content on narrow bands ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,kernel,rows", [(33, 12272, BGR_VEC16, 1), (34, 9808, BGR_VEC16, 2), (35, 8161, BGR_SCALAR, 3)])
def test_extreme_values_on_narrow_bands(ctx, oracle, h, w, kernel, rows):
    """All-0 / all-255 / checkerboard / inverse checkerboard where every band (or all but the last) has 1, 2 or 3 rows: the largest
    Laplacian magnitude at every pixel through the one-row branch and the peeled boundary rows of band_phases.
    Known answer of a checkerboard: |lap| = 1020 everywhere, with the sign of the pixel's parity -- so lap_sumsq = 1020^2 h w and
    lap_sum = 0 when h w is even; 35 x 8161 has one more pixel of even parity (value 0 in the checkerboard, lap = +1020) than of
    odd parity, so there lap_sum = +1020 and, for the inverse, -1020."""
    chk = ((np.add.outer(np.arange(h), np.arange(w)) & 1) * 255).astype(np.uint8)
    frames = np.stack([np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8),
                       np.repeat(chk[..., None], 3, axis=2), np.repeat((255 - chk)[..., None], 3, axis=2)])
    got = ctx.preprocess_bgr(frames)
    _check_plan(ctx, h, w, kernel, rows)
    _check_outputs(ctx, oracle, got, frames, (h, w))
    lap_sum, lap_sumsq = got[2], got[3]
    odd = (h * w) & 1
    assert lap_sum.tolist() == [0, 0, 1020 * odd, -1020 * odd]
    assert lap_sumsq.tolist() == [0, 0, 1020 * 1020 * h * w, 1020 * 1020 * h * w]


# ---- (f) batch offsets across very different plans ---------------------------------------------------------------------------------
def test_batch_offsets_across_plans(ctx):
    """One avd_analyze_batch over clips whose slices of the row-partial and moment-partial buffers differ by orders of magnitude
    (33 one-row bands of 12272 px, 5 bands of 101 px, 6 bands of NV12, 4 bands of 32 px): rowbuf_off / lappart_off of every clip.
    Moments, Hamming distances and the flow fields equal one-at-a-time analysis, twice (the second call re-uses every table)."""
    items = [synth.random_frames(2, 33, 12272, seed=1), synth.random_frames(2, 67, 101, seed=2), _planes(2, 46, 4112, seed=3),
             synth.random_frames(2, 43, 32, seed=4)]
    want, want_flow = [], []
    for x in items:
        want.append(ctx.analyze_frames_nv12(*x) if isinstance(x, tuple) else ctx.analyze_frames(x))
        want_flow.append(ctx.debug_fetch("flow0", (1, 2, 320, 320), np.float32))
    for rep in range(2):
        got = ctx.analyze_batch(items)
        flow = ctx.debug_fetch("flow0", (7, 2, 320, 320), np.float32)       # 8 frames: pairs 1, 3, 5 straddle two clips and are ignored
        for i, (a, b) in enumerate(zip(got, want)):
            for key in ("lap_sum", "lap_sumsq", "ham", "flow_mean", "flow_var"):
                assert np.array_equal(a[key], b[key]), (rep, i, key, a[key].tolist(), b[key].tolist())
            assert np.array_equal(flow[2 * i], want_flow[i][0]), (rep, i, "flow0")
