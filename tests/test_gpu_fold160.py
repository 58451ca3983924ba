"""The 160-px level's initial flow formed inside its first launch (option fb_fold_up160), and the pyramid kernel's item loops.

In the one-strip shape of the 160-px level (fb_wide160 = 1, or 2 with another call in flight) the chain wave of the first launch resizes
the 80-px level's flow itself, as the 320-px level's has done since round 3, and k_flow_up<160> is not launched.  The resize is
flow_up_chunk's arithmetic in its operation order, so nothing may change by a bit: every comparison here is on uint32 views.  The shapes
are chosen by pair count (every level works on 320 x 320 frames whatever the input): 2 pairs = one XCD group, 9 pairs = one more than a
multiple of 8 (pairs per XCD 2, idle tail workgroups).  Each set holds a bit-identical pair (exempt from the border-sign criterion) and a
pair of the stripes family, which a coarse level flags: with the re-run on, its workgroups leave the 160-px launch behind the extra
barrier of the resizing path.

The pyramid kernel (k_pyramid_all) lost the index work of its item loops, not a floating-point operation: its three scales equal the
oracle's pyramid, on noise and on a frame whose last column and row carry a hard edge (the reflected taps).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.content_families import families as _families  # noqa: E402

COARSE = 0xCC        # avd_frame_record.reserved: bits 2, 3 (solver criterion) and 6, 7 (border-sign criterion) = the 80- and 40-px levels


STRIPES_SEED = 160


def _frames(n):
    """n frames uint8[320, 320] that end in a stripes pair and its second frame again; n = 10 puts a smooth, a noise and a pink pair, the cuts
    between them and a bit-identical pink pair (pair 5) in front."""
    fam = _families()
    rng = np.random.default_rng(STRIPES_SEED)
    sa, sb = fam["stripes"](rng)
    tail = [sa, sb, sb.copy()]
    if n == 3:
        return np.stack(tail)
    a0, a1 = fam["smooth_shift"](rng)
    w0, w1 = fam["white_noise"](rng)
    p0, p1 = fam["pink_shift"](rng)
    return np.stack([a0, a1, w0, w1, p0, p1, p1.copy()] + tail)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(c, frames, wide, fold, rerun):
    """-> (flow_mean, flow_var, final flow, 160-px flow, pairs re-run, shape used) of one farneback_pairs call"""
    c.set_option("fb_wide160", wide)
    c.set_option("fb_fold_up160", fold)
    c.set_option("fb_rerun", rerun)
    fm, fv, flow = c.farneback_pairs(frames, want_flow=True)
    lvl1 = c.debug_fetch("flow1", (len(frames) - 1, 2, 160, 160), np.float32)
    return fm, fv, flow, lvl1, c.get_option("rerun_pairs"), c.get_option("fb_wide160_used")


@pytest.fixture(scope="module")
def flagged():
    """(n, wide) -> the reserved mask of every pair of _frames(n) (non-zero: flagged and re-run), from one records call in that shape"""
    import avd_hip
    out = {}
    with avd_hip.Context(0) as c:
        for n in (3, 10):
            for wide in (0, 1):
                c.set_option("fb_wide160", wide)
                rec = c.analyze_frames(np.repeat(_frames(n)[..., None], 3, axis=3))
                out[n, wide] = rec["reserved"][1:].copy()
    return out


@pytest.mark.parametrize("n", [3, 10])
@pytest.mark.parametrize("wide", [1, 0])
def test_fold_changes_no_bit(flagged, n, wide):
    """Cases (a) and (b): fb_wide160 = 1 (one strip: the fold is active) and 0 (two strips: the option changes nothing).  Option on against off:
    the 160-px flow, the final flow and both statistics, with the re-run off (every workgroup runs to the end: all pairs compared at 160 px)
    and on (the stripes pair's workgroups leave early; at 160 px the pairs that were not re-run are compared -- a flagged pair's level buffers
    are not written by the fast kernels)."""
    import avd_hip
    frames = _frames(n)
    res = flagged[n, wide]
    stripes = n - 3                                       # the pair (sa, sb)
    print(f"[fold160] n={n} reserved masks {[hex(int(v)) for v in res]}")
    assert res[stripes] & COARSE, hex(int(res[stripes]))  # flagged at the 80- or 40-px level: its workgroups skip the 160-px launches
    if n == 10:
        assert res[5] == 0 and np.array_equal(frames[5], frames[6])      # a bit-identical pair that runs all launches
    with avd_hip.Context(0) as c:
        assert c.get_option("fb_fold_up160") == 1 and c.get_option("fb_fold_up") == 5
        for rerun in (0, 1):
            off = _run(c, frames, wide, 0, rerun)
            on = _run(c, frames, wide, 1, rerun)
            assert off[5] == on[5] == wide
            assert off[4] == on[4] == (int((res != 0).sum()) if rerun else 0)
            keep = res == 0 if rerun else np.ones(n - 1, bool)
            assert np.array_equal(_u32(on[3])[keep], _u32(off[3])[keep]), (wide, rerun)
            assert np.array_equal(_u32(on[2]), _u32(off[2])), (wide, rerun)
            assert np.array_equal(_u32(on[0]), _u32(off[0])) and np.array_equal(_u32(on[1]), _u32(off[1])), (wide, rerun)


def test_fold_is_what_runs():
    """With the fold active the call has no k_flow_up<160> region (avd_kernel_ms); with the option off, or with two strips per pair, it has one."""
    import avd_hip
    clip = np.repeat(_frames(10)[..., None], 3, axis=3)
    with avd_hip.Context(0) as c:
        c.set_profiling(True)
        seen = {}
        for wide, fold in ((1, 1), (1, 0), (0, 1)):
            c.set_option("fb_wide160", wide)
            c.set_option("fb_fold_up160", fold)
            c.analyze_frames(clip)
            seen[wide, fold] = c.kernel_ms()
        print("[fold160] flow_up160 / level160 ms:", {k: (v["flow_up160"], v["level160"]) for k, v in seen.items()})
        assert seen[1, 1]["flow_up160"] == 0 and seen[1, 1]["level160"] > 0
        assert seen[1, 0]["flow_up160"] > 0 and seen[0, 1]["flow_up160"] > 0


def test_shape_is_decided_once_per_call():
    """Case (c): fb_wide160 = 2 and a call pending on another context: the call takes the one-strip shape (and with it the fold); its records
    equal those of fb_wide160 = 1."""
    import avd_hip
    clip = np.repeat(_frames(10)[..., None], 3, axis=3)
    with avd_hip.Context(0) as a, avd_hip.Context(0) as b:
        assert b.get_option("fb_wide160") == 2
        b.set_option("fb_wide160", 1)
        want = b.analyze_frames(clip)
        assert b.get_option("fb_wide160_used") == 1
        b.set_option("fb_wide160", 2)
        rec = np.zeros(len(clip), avd_hip.RECORD_DTYPE)
        keep = a.analyze_frames_async(clip, rec)               # enqueued, not drained
        shared = b.analyze_frames(clip)
        assert b.get_option("fb_wide160_used") == 1
        a.synchronize()
        del keep
        assert shared.tobytes() == want.tobytes()
        assert (want["reserved"][1:] != 0).any()


def test_pyramid_equals_the_oracle(oracle):
    """Case (d): pyr1 .. pyr3 of three frames -- noise, a hard edge in the last column and row, smooth content -- equal the oracle's
    GaussianBlur + INTER_LINEAR decimation; and pyr0, which the kernel writes with fb_fold_blur off."""
    import avd_hip
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, (320, 320), dtype=np.uint8)
    edge = np.full((320, 320), 30, np.uint8)
    edge[:, -1] = 255
    edge[-1, :] = 255
    edge[0, :] = 200
    edge[:, 0] = 0
    smooth = _families()["smooth_shift"](rng)[0]
    small = np.stack([noise, edge, smooth])
    ks = {0: (3, 0.0), 1: (3, 0.5), 2: (9, 1.5), 3: (19, 3.5)}
    with avd_hip.Context(0) as c:
        for fold_blur in (1, 0):
            c.set_option("fb_fold_blur", fold_blur)
            c.farneback_pairs(small)
            for k in range(0 if not fold_blur else 1, 4):
                wl = 320 >> k
                got = c.debug_fetch(f"pyr{k}", (3, wl, wl), np.float32)
                for f in range(3):
                    want = oracle.resize_linear_f32(oracle.gaussian_blur(small[f].astype(np.float32), *ks[k]), wl, wl)
                    assert np.array_equal(got[f], want), (fold_blur, k, f)
