"""The polynomial expansion with its three moment rows kept in LDS as one 16-byte quad {t0, t1, t1, t2} per column.

The horizontal pass of k_polyexp_all reads a column's quad with one 128-bit LDS read and forms its float sums, differences and products
as two-component operations; every half of such an operation is the IEEE single operation of the scalar form on the same operands, and
the order of every accumulation is unchanged, so nothing may change by a bit -- not even the sign of a zero.  Every comparison here is
on the uint32 views of the float32 buffers poly0 .. poly3 against the CPU oracle's pyramid + polynomial expansion (the oracle calls of
tests/test_gpu_parity.py), through the Farneback entry point on 320 x 320 gray frames, with fb_fold_blur 1 and 0.

Frame counts 2, 3 and 9: with 3 frames no scale's workgroup count (60, 30, 15, 15: the 160- and 80-px scales walk bands of 16 rows as the
320-px scale does) is a multiple of eight, so the padded, idle workgroups of the XCD remap are exercised; 9 frames span more than one
remap period.  Content: constants, ramps, noise, single 255 pixels at the
corners, at the seam of the 16-row walk (15/16), at the wave seam (63/64) and mid-frame, a period-2 checkerboard; every kind is frame 0 of
one two-frame call with a different kind as frame 1.
"""
import numpy as np
import pytest

S = 320
KS = {0: (3, 0.0), 1: (3, 0.5), 2: (9, 1.5), 3: (19, 3.5)}
WGS_PER_FRAME = (20, 10, 5, 5)     # k_polyexp_all: bands of 16 rows at 320 / 160 / 80 px, steps of 8 rows at 40 px
PIXELS = [(0, 0), (0, 319), (319, 0), (319, 319), (15, 63), (16, 64), (159, 160)]


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    """float32 arrays of one shape whose bit patterns agree everywhere (-0.0 is not +0.0, and a NaN equals only itself bit for bit)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != np.float32 or want.dtype != np.float32 or got.shape != want.shape:
        return False
    return bool(np.array_equal(_u32(got), _u32(want)))


def _kinds():
    """name -> uint8[320, 320]"""
    yy, xx = np.mgrid[0:S, 0:S]
    k = {
        "zero": np.zeros((S, S), np.uint8),
        "full": np.full((S, S), 255, np.uint8),
        "hramp": (xx * 255 // (S - 1)).astype(np.uint8),
        "vramp": (yy * 255 // (S - 1)).astype(np.uint8),
        "noise": np.random.default_rng(20).integers(0, 256, (S, S), dtype=np.uint8),
        "checker": (((xx + yy) & 1) * 255).astype(np.uint8),
    }
    for (y, x) in PIXELS:
        p = np.zeros((S, S), np.uint8)
        p[y, x] = 255
        k[f"pixel_{y}_{x}"] = p
    return k


KINDS = _kinds()
NAMES = list(KINDS)


@pytest.fixture(scope="module")
def want(oracle):
    """kind -> [the oracle's expansion at the four scales], computed once and never written to"""
    out = {}
    for name, img in KINDS.items():
        per = []
        for k in range(4):
            wl = S >> k
            pyr = oracle.resize_linear_f32(oracle.gaussian_blur(img.astype(np.float32), *KS[k]), wl, wl)
            p = np.ascontiguousarray(oracle.poly_exp(pyr), dtype=np.float32)
            p.setflags(write=False)
            per.append(p)
        out[name] = per
    return out


@pytest.fixture(scope="module")
def dev():
    import avd_hip
    avd_hip.build()
    with avd_hip.Context(0) as c:
        yield c


def _check(dev, want, names):
    frames = np.stack([KINDS[n] for n in names])
    n = len(names)
    assert dev.get_option("fb_fold_blur") == 1
    try:
        for fold in (1, 0):
            dev.set_option("fb_fold_blur", fold)
            dev.farneback_pairs(frames)
            for k in range(4):
                wl = S >> k
                got = dev.debug_fetch(f"poly{k}", (n, wl, wl, 5), np.float32)
                for f, name in enumerate(names):
                    if not same_bits(got[f], want[name][k]):
                        bad = np.argwhere(_u32(got[f]) != _u32(want[name][k]))
                        raise AssertionError(f"fold_blur {fold}, scale {k}, frame {f} ({name}) of {n}: {len(bad)} words differ, first at "
                                             f"{tuple(bad[0])}: {got[f][tuple(bad[0])]!r} against {want[name][k][tuple(bad[0])]!r}")
    finally:
        dev.set_option("fb_fold_blur", 1)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_each_kind_as_frame_0(dev, want, i):
    """two frames: the kind and, as frame 1, the next kind of the list (a different one)"""
    _check(dev, want, [NAMES[i], NAMES[(i + 1) % len(NAMES)]])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 9])
def test_idle_workgroups_and_remap_periods(dev, want, n):
    """3 frames: 60 / 30 / 15 / 15 workgroups per scale, none a multiple of eight; 9 frames: more than one remap period at every scale"""
    for k, per_frame in enumerate(WGS_PER_FRAME):
        assert (3 * per_frame) % 8 != 0 and 9 * per_frame > 8, k
    pick = ["noise", "checker", "pixel_16_64", "hramp", "pixel_319_319", "vramp", "full", "pixel_15_63", "pixel_0_0"][:n]
    _check(dev, want, pick)


def test_signed_zeros_of_the_constants(want):
    """b2, b4, b6 start at +0 and sum signed zeros on constant frames: what the oracle leaves there is what the comparison must pin"""
    for name in ("zero", "full", "checker"):
        zeros = sum(int((_u32(p) << 1 == 0).sum()) for p in want[name])
        neg = sum(int((_u32(p) == 0x80000000).sum()) for p in want[name])
        print(f"[polyexp_quads] {name}: {zeros} zeros in the oracle's expansion, {neg} of them -0.0")
        if name != "checker" and zeros == 0:
            print(f"[polyexp_quads] {name}: the oracle produces no zero; the case is a plain equality case")
    const_zeros = sum(int((_u32(p) << 1 == 0).sum()) for n in ("zero", "full") for p in want[n])
    if const_zeros:
        # a zero's sign is part of the pattern compared: flipping one must be seen (second control below does it on a +0.0)
        p = next(p for n in ("zero", "full") for p in want[n] if (_u32(p) << 1 == 0).any())
        q = p.copy()
        idx = tuple(np.argwhere(_u32(q) << 1 == 0)[0])
        q.view(np.uint32)[idx] ^= np.uint32(0x80000000)
        assert not same_bits(q, p)


def test_control_one_ulp_is_rejected():
    a = np.random.default_rng(1).standard_normal((40, 40, 5)).astype(np.float32)
    assert same_bits(a.copy(), a)
    b = a.copy()
    b.view(np.uint32)[17, 23, 2] += np.uint32(1)
    assert b[17, 23, 2] != a[17, 23, 2] and np.allclose(a, b, rtol=1e-6, atol=0)
    assert not same_bits(b, a)


def test_control_negative_zero_is_rejected():
    a = np.random.default_rng(2).standard_normal((40, 40, 5)).astype(np.float32)
    a[5, 6, 1] = 0.0
    b = a.copy()
    b[5, 6, 1] = -0.0
    assert np.array_equal(a, b)                           # equal as numbers ...
    assert not same_bits(b, a)                            # ... but not the same result
