"""The hold-out content of tests/holdout_families.py and its checker, on the CPU (no GPU): every family keeps its interface, is a pure function of its
seed, and has the pinned bytes tests/test_gpu_holdout.py finds again on frames composed on the device; the CPU oracle (reference site:
cv2.calcOpticalFlowFarneback, app/analyzers/video.py:45) gives a finite flow on them; and the checker that referees the default Farneback mode rejects
what it has to reject.
"""
import hashlib

import numpy as np
import pytest
import torch

from tests import holdout_families as H
from tests.content_families import families

NAMES = ("pan_right", "pan_down", "pan_left_up", "subpixel_pan", "pan_coarse_edge", "halves", "blocks8", "banding", "comb", "ticker", "dark_noise",
         "blend", "rot_checker", "near_periodic", "static_rb_border", "near_duplicate")


@pytest.fixture(scope="module")
def pairs():
    """name -> the first eight test pairs of the family, uint8[8, 2, 320, 320] on torch-CPU (composed once)"""
    fam = H.holdout_families()
    return {name: make(H.bank(), H.seeds_for_tests(j, 8), "cpu") for j, (name, make) in enumerate(fam.items())}


def test_the_sixteen_families_and_no_soak_name():
    fam = H.holdout_families()
    assert tuple(fam) == NAMES
    assert not set(fam) & set(families()) and H.CUT_BETWEEN not in fam and H.CUT_BETWEEN not in families()
    assert set(H.MOSTLY_UNFLAGGED) <= set(fam) and set(H.PINNED_SHA256) == set(fam)
    assert max(H.seeds_for_tests(len(fam) - 1, 512)) < H.FUZZ_SEED_MIN                 # the one-off fuzz draws other seeds


def test_bank_is_integer_and_pinned():
    b = H.bank()
    assert b.fields.dtype == np.uint8 and b.fields.shape == (H.NF + 2, 480, 480) and H.NF >= 24
    assert b.noise.dtype == np.int16 and b.noise.shape == (16, 320, 320) and int(b.noise.min()) == -2 and int(b.noise.max()) == 2
    assert b.wave.dtype == np.uint8 and b.wave.shape == (1024,)
    assert hashlib.sha256(b.fields.tobytes() + b.noise.tobytes() + b.wave.tobytes()).hexdigest() == H.BANK_SHA256
    assert min(float(f.std()) for f in b.fields) > 20                                   # no field came out flat


@pytest.mark.parametrize("name", NAMES)
def test_family_shape_purity_and_pinned_bytes(pairs, name):
    g = pairs[name]
    assert g.shape == (8, 2, 320, 320) and g.dtype == torch.uint8 and g.device.type == "cpu"
    j = NAMES.index(name)
    make = H.holdout_families()[name]
    seeds = H.seeds_for_tests(j, 8)
    again = make(H.bank(), seeds[2:5], "cpu")                       # another call, another batch: the same bytes per seed
    assert torch.equal(again, g[2:5])
    assert not torch.equal(g[0], g[1])                              # and the seed matters
    assert (H.pair_sha256(g[0]), H.pair_sha256(g[1])) == H.PINNED_SHA256[name]
    for k in range(8):                                              # no bit-identical pair (near_duplicate: exactly one pixel differs)
        ndiff = int((g[k, 0] != g[k, 1]).sum())
        assert (ndiff == 1) if name == "near_duplicate" else (ndiff >= 1), (name, seeds[k], ndiff)
    if name == "dark_noise":
        assert int(g.max()) == 3


def test_near_duplicate_reaches_every_ballot_word():
    """the one differing pixel is drawn from the four corners, (1, 0), the centre and every one of the 20 row tiles (16 source rows) of the 160-px scale"""
    g = H.holdout_families()["near_duplicate"](H.bank(), H.seeds_for_tests(15, 512), "cpu")
    where = (g[:, 0] != g[:, 1]).flatten(1).nonzero()
    assert where.shape[0] == 512
    pos = {(int(i) // 320, int(i) % 320) for i in where[:, 1]}
    assert set(H.NEAR_DUP_FIXED) <= pos
    assert {y // 16 for y, x in pos - set(H.NEAR_DUP_FIXED)} == set(range(20))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_flow_is_finite(oracle, pairs, name):
    for k in range(2):
        a, b = pairs[name][k].numpy()
        flow = oracle.farneback(a, b)
        assert flow.shape == (320, 320, 2) and np.isfinite(flow).all(), (name, k)
        m, v = oracle.flow_stats(flow)
        assert np.isfinite(m) and np.isfinite(v) and m >= 0 and v >= 0


# ---- the checker's controls ---------------------------------------------------------------------------------------------------------------------
def _f32(*v):
    return np.array(v, np.float32)


def test_checker_accepts_what_is_inside_the_guarantee():
    xm, xv = _f32(0.0, 1.0, 3.5, 250.0, 1e-3), _f32(0.0, 2.0, 0.25, 4000.0, 1e-5)
    none, every = np.zeros(5, bool), np.ones(5, bool)
    assert H.check(xm, xv, xm, xv, none) == [] and H.check(xm, xv, xm, xv, every) == []
    fm = (xm.astype(np.float64) * (1 + 5e-7)).astype(np.float32)                      # unflagged, rel 5e-7 on both statistics
    fv = (xv.astype(np.float64) * (1 - 5e-7)).astype(np.float32)
    assert not np.array_equal(fm, xm) and H.check(fm, fv, xm, xv, none) == []
    assert H.check(_f32(5e-8), _f32(0.0), _f32(0.0), _f32(9e-8), _f32(0).astype(bool)) == []   # inside abs 1e-7 of a zero statistic


def test_checker_rejects_one_ulp_on_a_flagged_pair():
    xm, xv = _f32(1.0, 3.5, 0.0), _f32(2.0, 0.25, 0.0)
    for which in range(2):
        for p in range(3):
            fm, fv = xm.copy(), xv.copy()
            (fm, fv)[which][p] = np.nextafter((xm, xv)[which][p], np.float32(np.inf))
            bad = H.check(fm, fv, xm, xv, np.ones(3, bool))
            assert [(b[0], b[1]) for b in bad] == [(p, "flagged pair not bit-identical")], (which, p, bad)
            if p < 2:
                assert H.check(fm, fv, xm, xv, np.zeros(3, bool)) == []               # one ulp is inside an unflagged pair's tolerance
    assert H.check(_f32(-0.0), _f32(0.0), _f32(0.0), _f32(0.0), np.ones(1, bool)) != []   # bit for bit: not even the sign of zero


def test_checker_rejects_rel_2e_6_unflagged():
    xm, xv = _f32(1.0, 3.5, 250.0), _f32(2.0, 0.25, 4000.0)
    none = np.zeros(3, bool)
    fm = (xm.astype(np.float64) * (1 + 2e-6)).astype(np.float32)
    bad = H.check(fm, xv, xm, xv, none)
    assert {b[0] for b in bad} == {0, 1, 2} and all("flow_mean" in b[1] or "ai_susp" in b[1] for b in bad)
    fv = (xv.astype(np.float64) * (1 - 2e-6)).astype(np.float32)
    bad = H.check(xm, fv, xm, xv, none)
    assert [(b[0], b[1]) for b in bad] == [(p, "unflagged pair out of tolerance: flow_var") for p in range(3)]
    assert H.check(fm, fv, xm, xv, np.ones(3, bool)) != []                             # and a flagged pair all the more


def test_checker_rejects_the_ai_susp_bound_and_nan():
    # |delta flow_mean| above 1e-6 * max(1, |m|): at m = 0.05 a difference of 2e-6, at m = 40 one of 5e-5
    for m, dm in ((0.05, 2e-6), (40.0, 5e-5)):
        bad = H.check(_f32(m + dm), _f32(1.0), _f32(m), _f32(1.0), np.zeros(1, bool))
        assert (0, "unflagged pair out of tolerance: ai_susp") in [(b[0], b[1]) for b in bad], (m, bad)
    for flagged in (False, True):
        for slot in range(4):
            v = [_f32(1.0, 2.0) for _ in range(4)]
            v[slot][1] = np.nan
            bad = H.check(*v, np.array([flagged, flagged]))
            assert [(b[0], b[1]) for b in bad] == [(1, "not finite")], (flagged, slot, bad)
        bad = H.check(_f32(np.inf), _f32(1.0), _f32(np.inf), _f32(1.0), np.array([flagged]))
        assert [(b[0], b[1]) for b in bad] == [(0, "not finite")]


def test_committed_fuzz_findings_are_family_and_seed():
    """tests/golden/holdout_fuzz_<family>_<seed>.npz: the two violators the one-off fuzz found on the MI355X, as they were written there -- a rebuild on
    torch-CPU from the family name and the seed alone gives the same bytes (the reproducibility rule at work)"""
    import glob
    import os
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "holdout_fuzz_*.npz")))
    assert len(files) == 2
    for f in files:
        name, seed = os.path.basename(f)[len("holdout_fuzz_"):-len(".npz")].rsplit("_", 1)
        assert int(seed) >= H.FUZZ_SEED_MIN
        z = np.load(f)
        g = H.holdout_families()[name](H.bank(), [int(seed)], "cpu")[0].numpy()
        assert np.array_equal(g[0], z["prev"]) and np.array_equal(g[1], z["next"]), f
