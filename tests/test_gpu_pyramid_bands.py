"""The pyramid kernel (k_pyramid_all) in bands: a workgroup walks eight output rows of the 80- and 40-px scales in two steps of four and takes the
row-filtered source rows both steps read over from the first; a lane of the row pass forms both columns of a pair, a lane of the column pass reads
its two columns once.  Not a floating-point operation changed, so every comparison here is on uint32 views:

  * pyr1 .. pyr3 (and pyr0 with fb_fold_blur off) of 2, 3 and 9 frames against the oracle's GaussianBlur + INTER_LINEAR decimation -- nine frames make
    the workgroup counts per scale (5 / 10 / 20 per frame) no multiples of eight.  Content: seeded noise; all 255 and all 0 (a tap applied twice or
    dropped); a frame whose first and last two rows and columns differ from the interior (the reflected border at every band's edge); a ramp whose rows
    are all distinct (a row taken over from the wrong place, or read before it is written);
  * a batch of two clips leaves the levels the clips give alone;
  * the pair-identity words ("pairdiff", one per pair and 160-px tile): a single differing byte anywhere is seen, at the corners, mid-frame and in the
    row on either side of every boundary between tiles (multiples of 16 source rows, which are also all band and step boundaries of the 80- and 40-px
    scales: multiples of 32 / 16 and 64 / 32), and only the tiles whose rows hold the byte report it;
  * nothing downstream moved: the default mode against fb_mode = exact, and the re-run counter under AVD_FB_RERUN.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = {0: (3, 0.0), 1: (3, 0.5), 2: (9, 1.5), 3: (19, 3.5)}
TILES = 20                                                # 160-px tiles per frame: 16 source rows each, and one row above and below


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _content():
    """nine frames uint8[320, 320]"""
    rng = np.random.default_rng(2024)
    noise = rng.integers(0, 256, (4, 320, 320), dtype=np.uint8)
    white, black = np.full((320, 320), 255, np.uint8), np.zeros((320, 320), np.uint8)
    border = np.full((320, 320), 90, np.uint8)
    border[:2, :], border[-2:, :], border[:, :2], border[:, -2:] = 250, 5, 170, 33
    border[0, :], border[-1, :], border[:, 0], border[:, -1] = 10, 240, 60, 200
    r, x = np.arange(320)[:, None], np.arange(320)[None, :]
    ramp = ((r * 5 + x * (1 + (r >> 6))) & 255).astype(np.uint8)
    assert len(np.unique(ramp, axis=0)) == 320            # every row differs from every other
    return np.stack([ramp, border, white, black, noise[0], noise[1], border.T.copy(), noise[2], ramp[::-1].copy()])


SETS = {2: [0, 1], 3: [2, 3, 4], 9: list(range(9))}      # frames of _content() per clip length


@pytest.fixture(scope="module")
def frames():
    return _content()


@pytest.fixture(scope="module")
def want(oracle, frames):
    """level -> float32[9, wl, wl]: the oracle's pyramid of the nine frames, computed once"""
    out = {}
    for k, (ksize, sigma) in KS.items():
        wl = 320 >> k
        out[k] = np.stack([oracle.resize_linear_f32(oracle.gaussian_blur(f.astype(np.float32), ksize, sigma), wl, wl) for f in frames])
        out[k].setflags(write=False)
    return out


@pytest.mark.parametrize("fold_blur", [1, 0])
@pytest.mark.parametrize("n", [2, 3, 9])
def test_pyramid_bit_identical(frames, want, n, fold_blur):
    import avd_hip
    sel = SETS[n]
    with avd_hip.Context(0) as c:
        c.set_option("fb_fold_blur", fold_blur)
        c.farneback_pairs(frames[sel])
        for k in range(1 if fold_blur else 0, 4):
            wl = 320 >> k
            got = c.debug_fetch(f"pyr{k}", (n, wl, wl), np.float32)
            for i, f in enumerate(sel):
                bad = np.argwhere(_u32(got[i]) != _u32(want[k][f]))
                assert bad.size == 0, (n, fold_blur, k, f, len(bad), bad[:4].tolist())


def test_batch_leaves_the_same_levels(frames):
    import avd_hip
    clips = [np.repeat(frames[:4][..., None], 3, axis=3), np.repeat(frames[4:][..., None], 3, axis=3)]
    with avd_hip.Context(0) as c:
        alone = []
        for clip in clips:
            c.analyze_frames(clip)
            alone.append({k: c.debug_fetch(f"pyr{k}", (len(clip), 320 >> k, 320 >> k), np.float32) for k in (1, 2, 3)})
        recs = c.analyze_batch(clips)
        assert [len(r) for r in recs] == [4, 5]
        for k in (1, 2, 3):
            got = c.debug_fetch(f"pyr{k}", (9, 320 >> k, 320 >> k), np.float32)       # the buffers hold the concatenation of the clips
            assert np.array_equal(_u32(got), _u32(np.concatenate([a[k] for a in alone]))), k


def _identity_clip(frames, row, col):
    """frame 1 == frame 0, frame 2 differs from frame 1 in the one byte (row, col), frame 3 is other content"""
    a = frames[4]
    b = a.copy()
    b[row, col] ^= 0x10
    return np.stack([a, a.copy(), b, frames[5]])


BOUNDARY_ROWS = [r for t in range(1, TILES) for r in (16 * t - 1, 16 * t)]
PLACES = [(0, 0), (0, 319), (319, 0), (319, 319), (160, 157)] + [(r, (r * 37) % 320) for r in BOUNDARY_ROWS]


def test_pair_identity_sees_one_byte(frames):
    import avd_hip
    assert len(PLACES) == 5 + 2 * (TILES - 1)
    with avd_hip.Context(0) as c:
        for row, col in PLACES:
            clip = _identity_clip(frames, row, col)
            assert np.count_nonzero(clip[2] != clip[1]) == 1 and np.array_equal(clip[1], clip[0])
            c.farneback_pairs(clip)
            pd = c.debug_fetch("pairdiff", (3, TILES), np.int32)
            for p in range(3):
                assert bool(pd[p].any()) == (not np.array_equal(clip[p], clip[p + 1])), (row, col, p, pd[p].tolist())
            # tile t reads source rows 16 t - 1 .. 16 t + 16 (reflected at the frame's edge: no further row)
            tiles = [t for t in range(TILES) if 16 * t - 1 <= row <= 16 * t + 16]
            assert np.nonzero(pd[1])[0].tolist() == tiles, (row, col, pd[1].tolist())
            assert pd[2].all()


def _records_equal_exact(default, exact, clip):
    """the records of the default mode against exact mode's: every field but `reserved` (the default mode's flag word, which exact mode does not
    have), the two flow statistics on their bits -> the default mode's records"""
    got, ref = default.analyze_frames(clip), exact.analyze_frames(clip)
    for name in got.dtype.names:
        if name == "reserved":
            continue
        a, b = got[name], ref[name]
        if a.dtype.kind == "f":
            a, b = _u32(a.astype(np.float32)), _u32(b.astype(np.float32))
        print(f"[pyramid bands] {name}: {int(np.count_nonzero(a != b))} of {a.size} differ; flag words {[hex(int(v)) for v in got['reserved']]}")
        assert np.array_equal(a, b), name
    return got


def test_nothing_else_moved(frames, monkeypatch):
    import avd_hip
    rng = np.random.default_rng(9)
    noise9 = rng.integers(0, 256, (9, 320, 320), dtype=np.uint8)
    clips = [np.repeat(_identity_clip(frames, 160, 157)[..., None], 3, axis=3), np.repeat(noise9[..., None], 3, axis=3)]
    monkeypatch.setenv("AVD_FB_RERUN", "1")
    with avd_hip.Context(0) as c, avd_hip.Context(0) as x:
        assert c.get_option("fb_mode") == 1 and c.get_option("fb_rerun") == 1
        x.set_option("fb_mode", 0)
        flagged = []
        for clip in clips:
            rec = _records_equal_exact(c, x, clip)
            flagged.append(int(np.count_nonzero(rec["reserved"])))
            assert c.get_option("rerun_pairs") == flagged[-1]
            if clip is clips[0]:
                assert rec["reserved"][1] == 0                                   # a pair of bit-identical frames is never flagged
    monkeypatch.setenv("AVD_FB_RERUN", "0")
    with avd_hip.Context(0) as c:
        assert c.get_option("fb_rerun") == 0
        for clip in clips:
            rec = c.analyze_frames(clip)
            assert not rec["reserved"].any() and c.get_option("rerun_pairs") == 0
