"""The patch-embed GEMM's cross-tile stream (k_gemm_bf16_nt_persistent, csrc/avd_vit.hip) with two and with three tiles per workgroup.

The kernel is persistent: grid = min(CUs rounded down to 8, tiles rounded up to 8), a workgroup walks tiles lw, lw + grid, ..., and the
ring of LDS-DMA half stages runs on across tile boundaries.  Everything hand-counted lives in that crossing -- the `!first` waits that add
the previous tile's epilogue stores to vmcnt (2 P + STORES, another STORES for f32 and for bf16 tokens), the refill that takes half stages
0-2 of the NEXT tile while the current one is multiplied, the late waves' epilogue inside step 0 of the next tile, the `!more` waits at the
end of the stream -- and with 256 CUs none of it runs below 112 frames; the other tests of the GEMM use at most 9.

Sizes come from the device (the launcher's grid rule restated in `stream_sizes`), on 256 CUs:
  S2      112 frames, 258 tiles on 256 workgroups: two workgroups get a second tile, both in the padded last row block
  S2full  128 frames, 294 tiles: M a multiple of 256, no row of the last tile masked
  S3      279 frames, 642 tiles: about half the workgroups run a middle tile (first == false and more == true at once) and a third one
Every test asserts tiles > g (S3: > 2 g) before it launches and prints n, tiles and grid.

Per size, four launches on the same inputs (f32 / bf16 tokens x gemm_waves 8 / 16) into a device tensor with a guard frame behind it:
  (a) bit identity with the same frames computed in chunks of one tile per workgroup (the path tests/test_vit.py validates);
  (b) f32 tokens against the float64 product of the bf16-rounded operands within the float32 accumulation bound
      768 * 2^-24 * (|A| @ |Wq|^T) + 2^-23 |ref| + 1e-30 per element (derived, and at most test_vit's 1e-3 + 1e-3 |ref| on these inputs);
      bf16 tokens within |f32 token| * 2^-8 of the f32 tokens of the same launch shape;
  (c) one-hot weights at S3: tokens == patchify_reference(frames)[:, perm], exactly;
  (d) the GEMM enqueued again on the resident patches (timing_reps = 2) gives the bits of timing_reps = 0;
  (e) a fresh context through 2 frames, S2, 2 frames, 5 frames (the rows that pad the last tile then hold the long call's stale patches):
      each call bit-identical to the same call on another fresh context.
CPU controls (not marked gpu) corrupt a CPU result the way a wrong stream would and show that the checkers of (b) and (c) reject it.

What these results pin and what they cannot: built with the late waves' zero_acc() after a crossing removed, (a), (b) and (c) fail at every
size (S2: 32768 elements of tile 256 and 257, S3: 12.6 M).  Built with the `!first` waits one half stage too permissive (3 P + STORES), and
even with no wait at all in the three steps after a crossing (vmcnt(63)), every test here still passed on an MI355X: a half stage is issued
three steps before it is read and lands long before its wait on an otherwise idle device.  So the addressing of the crossing (which tile
the refill takes, where the late epilogue stores, what is cleared, what is masked) is checked by value; the wait counts themselves are run
but remain an argument from the issue order, written next to them in the kernel.

Measured on an MI355X (256 CUs): (a) held bit for bit in all four launch shapes at every size; worst |got - ref| / bound of (b), the same
for gemm_waves 8 and 16: S2 0.0028, S2full 0.0032, S3 0.0028 (float32 numpy in the kernel's order of half stages: 0.0013 at 3 frames).
"""
import functools

import numpy as np
import pytest

from avd_hip import _lib, synth
from tests.test_vit import patchify_reference

BM = BN = 256                                            # the GEMM's tile
DIM, TOK = 768, 196
PERM = (np.arange(DIM) * 7 + 3) % DIM
SENTINEL16 = 0x7FA5                                      # a bf16 NaN with a payload no rounding produces


# ---- the launcher's grid rule (launch_gemm_bf16_nt) ------------------------------------------------------------------------------------
def grid_rule(cus, n):
    """-> (g, tiles, grid) of a call with n frames on a device of `cus` compute units."""
    g = max(8, cus // 8 * 8)
    tiles = -(-TOK * n // BM) * (DIM // BN)
    return g, tiles, min(g, -(-tiles // 8) * 8)


def stream_sizes(cus):
    """-> {"one": the largest n with one tile per workgroup, "S2", "S2full", "S3": frame counts}."""
    g = grid_rule(cus, 1)[0]
    tiles = lambda n: grid_rule(cus, n)[1]
    s2 = next(n for n in range(1, 1 << 20) if tiles(n) > g)
    s2full = next(n for n in range(64, 1 << 20, 64) if tiles(n) > g)
    s3 = next(n for n in range(1, 1 << 20) if 2 * tiles(n) >= 5 * g)
    return {"one": s2 - 1, "S2": s2, "S2full": s2full, "S3": s3}


def tiles_of_workgroup(lw, tiles, grid):
    return list(range(lw, tiles, grid))


def test_grid_rule_on_256_cus():
    s = stream_sizes(256)
    assert s == {"one": 111, "S2": 112, "S2full": 128, "S3": 279}
    assert grid_rule(256, 111) == (256, 255, 256) and grid_rule(256, 112) == (256, 258, 256) and grid_rule(256, 279) == (256, 642, 256)
    assert grid_rule(256, 9) == (256, 21, 24)                                    # the largest earlier test of the GEMM: one tile each
    assert (TOK * 128) % BM == 0 and grid_rule(256, 128)[1] == 294
    # S2: workgroups 0 and 1 get tiles 256 and 257, row block 85 of 86, which has 192 valid rows
    assert tiles_of_workgroup(0, 258, 256) == [0, 256] and tiles_of_workgroup(1, 258, 256) == [1, 257] and tiles_of_workgroup(2, 258, 256) == [2]
    assert 256 // 3 == 85 and TOK * 112 - 85 * BM == 192
    # S3: 130 workgroups run three tiles, the other 126 two
    assert sum(len(tiles_of_workgroup(lw, 642, 256)) == 3 for lw in range(256)) == 130
    for cus in (8, 64, 80, 228, 304):                                            # partitioned or other devices: the rule still yields >= 2 / >= 3
        s, g = stream_sizes(cus), grid_rule(cus, 1)[0]
        assert grid_rule(cus, s["one"])[1] <= g < grid_rule(cus, s["S2"])[1] and g < grid_rule(cus, s["S2full"])[1]
        assert grid_rule(cus, s["S3"])[1] > 2 * g and (TOK * s["S2full"]) % BM == 0


# ---- inputs, references, checkers --------------------------------------------------------------------------------------------------------
def seeded_weights(seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((DIM, DIM)) * 0.02).astype(np.float32), (rng.standard_normal(DIM) * 0.1).astype(np.float32)


def bf16_round(w):
    return _lib.bf16_bits_to_f32(_lib.f32_to_bf16_bits(np.ascontiguousarray(w, np.float32)))


def float64_reference(a, weight, bias):
    """a: patchify_reference(frames).  -> (ref, bound): the float64 product of the bf16-rounded operands plus bias, and the float32
    accumulation bound gamma_K sum|a||b| (K = 768 products, unit roundoff 2^-24) plus the rounding of the bias add."""
    a = a.astype(np.float64)
    wq = bf16_round(weight).astype(np.float64)
    ref = a @ wq.T + (0.0 if bias is None else bias.astype(np.float64))
    bound = DIM * 2.0 ** -24 * (np.abs(a) @ np.abs(wq).T) + 2.0 ** -23 * np.abs(ref) + 1e-30
    return ref, bound


def within_bound(got, ref, bound):
    """The checker of (b).  -> (ok, worst |got - ref| / bound); an unwritten (NaN) element fails."""
    err = np.abs(got.astype(np.float64) - ref)
    ok = bool(np.all(err <= bound))                                              # NaN <= x is False
    with np.errstate(invalid="ignore"):
        ratio = err / bound
    return ok, float(np.inf if np.isnan(ratio).any() else ratio.max())


def onehot_ok(got, a):
    """The checker of (c): with W[j, PERM[j]] = 1 and no bias every token is one input value."""
    return bool(np.array_equal(got, a[:, PERM]))


def onehot_weight():
    w = np.zeros((DIM, DIM), np.float32)
    w[np.arange(DIM), PERM] = 1.0
    return w


# ---- CPU controls: what a wrong stream would produce, and that the checkers see it --------------------------------------------------------
CONTROL_CUS = 8                                          # a device of 8 CUs: S2 = 3 frames, 9 tiles on 8 workgroups -- small enough for the CPU


@functools.lru_cache(maxsize=None)
def control_case():
    n = stream_sizes(CONTROL_CUS)["S2"]
    g, tiles, grid = grid_rule(CONTROL_CUS, n)
    assert (n, g, tiles, grid) == (3, 8, 9, 8)
    first, second = tiles_of_workgroup(0, tiles, grid)                           # workgroup 0: tile 0, then tile 8 in the padded last row block
    a = patchify_reference(synth.random_frames(n, 224, 224, seed=21))
    weight, bias = seeded_weights(22)
    ref, bound = float64_reference(a, weight, bias)
    m = a.shape[0]

    def box(tile):                                                               # rows (clipped to M) and columns of a tile
        r0, c0 = tile // (DIM // BN) * BM, tile % (DIM // BN) * BN
        return slice(r0, min(r0 + BM, m)), slice(c0, c0 + BN)
    return dict(a=a, weight=weight, bias=bias, ref=ref, bound=bound, first=box(first), second=box(second), m=m)


def float32_stream(a, weight, bias):
    """The kernel's arithmetic in float32 numpy: 24 half stages of 32 k accumulated in turn, then the bias."""
    wq = bf16_round(weight)
    acc = np.zeros((a.shape[0], DIM), np.float32)
    for k in range(0, DIM, 32):
        acc += a[:, k:k + 32] @ wq[:, k:k + 32].T
    return acc + (np.float32(0) if bias is None else bias)


def test_control_unmodified_results_pass():
    c = control_case()
    assert np.all(c["bound"] <= 1e-3 + 1e-3 * np.abs(c["ref"]))                  # never weaker than test_vit's tolerance
    ok, ratio = within_bound(c["ref"].astype(np.float32), c["ref"], c["bound"])
    assert ok and ratio < 1
    got = float32_stream(c["a"], c["weight"], c["bias"])                         # float32 in the kernel's order of half stages
    ok, ratio = within_bound(got, c["ref"], c["bound"])
    print(f"control: float32 accumulation over 24 half stages is {ratio:.4f} of the bound")
    assert got.dtype == np.float32 and ok and ratio < 1
    assert onehot_ok(float32_stream(c["a"], onehot_weight(), None), c["a"])


def _stale_first_half_stage(c, weight):
    """The second tile's half stage 0 (k = 0 .. 31) read before it landed: the ring slot still holds the same rows and columns of the
    workgroup's first tile.  -> the float64 difference to add to the second tile."""
    (r1, c1), (r2, c2) = c["first"], c["second"]
    rows = r2.stop - r2.start
    a, wq = c["a"].astype(np.float64), bf16_round(weight).astype(np.float64)
    stale = a[r1.start:r1.start + rows, :32] @ wq[c1, :32].T
    right = a[r2, :32] @ wq[c2, :32].T
    return stale - right


def test_control_second_tile_reads_the_first_tiles_half_stage():
    c = control_case()
    r2, c2 = c["second"]
    wrong = c["ref"].copy()
    wrong[r2, c2] += _stale_first_half_stage(c, c["weight"])
    assert not within_bound(wrong.astype(np.float32), c["ref"], c["bound"])[0]
    # ... and the one-hot check sees it: whole columns of the tile whose PERM falls in k < 32 change
    right = float32_stream(c["a"], onehot_weight(), None)
    wrong = right.copy()
    wrong[r2, c2] += _stale_first_half_stage(c, onehot_weight()).astype(np.float32)
    assert onehot_ok(right, c["a"]) and not onehot_ok(wrong, c["a"])
    others = np.ones(wrong.shape, bool)
    others[r2, c2] = False
    assert np.array_equal(wrong[others], right[others])


def test_control_second_tile_starts_from_the_first_tiles_accumulators():
    c = control_case()
    (r1, c1), (r2, c2) = c["first"], c["second"]
    rows = r2.stop - r2.start
    wrong = c["ref"].copy()
    wrong[r2, c2] += c["ref"][r1.start:r1.start + rows, c1] - c["bias"][c1].astype(np.float64)      # zero_acc() skipped
    assert not within_bound(wrong.astype(np.float32), c["ref"], c["bound"])[0]
    a = c["a"]
    right = float32_stream(a, onehot_weight(), None)
    wrong = right.copy()
    wrong[r2, c2] += right[r1.start:r1.start + rows, c1]
    assert not onehot_ok(wrong, a)


def test_control_tile_of_the_last_row_block_left_unwritten():
    c = control_case()
    r2, c2 = c["second"]
    assert r2.stop == c["m"] and r2.stop - r2.start < BM                         # the padded row block
    wrong = c["ref"].astype(np.float32)
    wrong[r2, c2] = np.nan                                                       # the output's fill
    ok, ratio = within_bound(wrong, c["ref"], c["bound"])
    assert not ok and ratio == np.inf
    right = float32_stream(c["a"], onehot_weight(), None)
    right[r2, c2] = np.nan
    assert not onehot_ok(right, c["a"])
    # one element is enough for either checker
    one = c["ref"].astype(np.float32)
    one[c["m"] - 1, DIM - 1] = np.nan
    assert not within_bound(one, c["ref"], c["bound"])[0]


# ---- the GPU tests ------------------------------------------------------------------------------------------------------------------------
class Case:
    """Frames of one size, shared by the tests of this module; the CPU references are formed once, on first use."""

    def __init__(self, name, cus):
        sizes = stream_sizes(cus)
        self.name, self.cus, self.n, self.one = name, cus, sizes[name], sizes["one"]
        self.g, self.tiles, self.grid = grid_rule(cus, self.n)
        self.frames = synth.random_frames(self.n, 224, 224, seed=40 + self.n)
        self.weight, self.bias = seeded_weights(41 + self.n)

    def announce(self, what):
        print(f"\n{self.name} {what}: n = {self.n} frames, M = {self.n * TOK}, tiles = {self.tiles}, grid = {self.grid} "
              f"({self.tiles / self.grid:.2f} tiles per workgroup)")
        assert self.tiles > (2 * self.g if self.name == "S3" else self.g) and self.grid == self.g
        assert grid_rule(self.cus, self.one)[1] <= self.g                        # the chunks of (a): one tile per workgroup

    @functools.cached_property
    def device_frames(self):
        import torch
        return torch.from_numpy(self.frames).to("cuda:0")

    @functools.cached_property
    def a(self):
        return patchify_reference(self.frames)

    @functools.cached_property
    def reference(self):
        ref, bound = float64_reference(self.a, self.weight, self.bias)
        assert np.all(bound <= 1e-3 + 1e-3 * np.abs(ref)), "the derived bound must never be the weaker one"
        return ref, bound


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)        # the HIP property avd_create stores


@pytest.fixture(scope="module")
def case(request, cus):
    return Case(request.param, cus)


def _guarded(n, bf16):
    """-> (whole [n + 1, 196, 768] tensor filled with the sentinel, its contiguous [:n] view)."""
    import torch
    if bf16:
        whole = torch.empty((n + 1, TOK, DIM), dtype=torch.bfloat16, device="cuda:0")
        whole.view(torch.int16).fill_(SENTINEL16)
    else:
        whole = torch.full((n + 1, TOK, DIM), float("nan"), dtype=torch.float32, device="cuda:0")
    return whole, whole[:n]


def _bits(t):
    import torch
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)     # the uint16 / uint32 bits; torch compares the signed views


def _sentinels(t):
    import torch
    return (_bits(t) == SENTINEL16) if t.dtype == torch.bfloat16 else torch.isnan(t)


def _embed_guarded(ctx, frames, bf16, step=None, timing_reps=0):
    """One call (step None) or calls of `step` frames each into one guarded tensor.  -> the [n] view; asserts the guard frame untouched
    and no sentinel left inside."""
    n = frames.shape[0]
    whole, out = _guarded(n, bf16)
    for s in range(0, n, step or n):
        e = min(n, s + (step or n))
        ctx.vit_patch_embed(frames[s:e], out=out[s:e], bf16=bf16, timing_reps=timing_reps)
    assert bool(_sentinels(whole[n]).all()), "written past row M"
    left = int(_sentinels(out).sum())
    assert left == 0, f"{left} elements never written"
    return out


def _same_bits(x, y):
    import torch
    return bool(torch.equal(_bits(x), _bits(y)))


def _mismatch(x, y):
    d = (_bits(x) != _bits(y)).reshape(-1, DIM)
    rows = d.any(dim=1).nonzero().flatten()
    return f"{int(d.sum())} elements differ in {rows.numel()} rows, first rows {rows[:8].tolist()} (tiles are 256 x 256)"


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["S2", "S2full", "S3"], indirect=True)
def test_stream_against_single_tile_calls_and_float64(ctx, case):
    """(a) and (b) for the four launch shapes."""
    case.announce("(a)+(b)")
    ref, bound = case.reference
    frames = case.device_frames
    ctx.vit_set_weights(case.weight, case.bias)
    assert ctx.get_option("gemm_waves") == 8
    worst = {}
    try:
        for waves in (8, 16):
            ctx.set_option("gemm_waves", waves)
            tok32 = None
            for bf16 in (False, True):
                long = _embed_guarded(ctx, frames, bf16)
                chunks = _embed_guarded(ctx, frames, bf16, step=case.one)       # every workgroup has one tile
                assert _same_bits(long, chunks), f"{case.name} waves {waves} bf16 {bf16}: " + _mismatch(long, chunks)
                if not bf16:
                    ok, worst[waves] = within_bound(long.cpu().numpy().reshape(-1, DIM), ref, bound)
                    print(f"{case.name} gemm_waves {waves}: worst |got - ref| / bound = {worst[waves]:.4f}")
                    assert ok, (case.name, waves, worst[waves])
                    tok32 = long.double()
                else:                                                            # one rounding of the same product to bf16
                    assert bool(((long.double() - tok32).abs() <= tok32.abs() * 2.0 ** -8 + 1e-30).all()), (case.name, waves)
    finally:
        ctx.set_option("gemm_waves", 8)
    print(f"{case.name}: n = {case.n}, tiles = {case.tiles}, grid = {case.grid}, worst error / bound = {max(worst.values()):.4f}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["S3"], indirect=True)
def test_stream_one_hot_weights(ctx, case):
    """(c): every token is a single product, so a half stage read early or late changes whole 32-column groups exactly."""
    case.announce("(c)")
    ctx.vit_set_weights(onehot_weight(), None)
    try:
        for waves in (8, 16):
            ctx.set_option("gemm_waves", waves)
            got = _embed_guarded(ctx, case.device_frames, False).cpu().numpy().reshape(-1, DIM)
            assert onehot_ok(got, case.a), (waves, int((got != case.a[:, PERM]).sum()))
    finally:
        ctx.set_option("gemm_waves", 8)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["S2"], indirect=True)
def test_stream_relaunched_on_resident_patches(ctx, case):
    """(d): timing_reps = 2 enqueues the GEMM twice more on the same stream, on the patches and into the tokens of the first launch."""
    case.announce("(d)")
    ctx.vit_set_weights(case.weight, case.bias)
    for bf16 in (False, True):
        once = _embed_guarded(ctx, case.device_frames, bf16)
        again = _embed_guarded(ctx, case.device_frames, bf16, timing_reps=2)
        assert _same_bits(once, again), f"bf16 {bf16}: " + _mismatch(once, again)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["S2"], indirect=True)
def test_stream_buffer_history(case):
    """(e): after the long call the rows that pad a short call's last tile hold stale patches instead of zeros; they reach masked output
    rows only."""
    import avd_hip
    case.announce("(e)")
    calls = [synth.random_frames(2, 224, 224, seed=51), case.frames, synth.random_frames(2, 224, 224, seed=51),
             synth.random_frames(5, 224, 224, seed=52)]
    with avd_hip.Context(0) as c:
        c.vit_set_weights(case.weight, case.bias)
        history = [c.vit_patch_embed(f)[0] for f in calls]
    assert np.array_equal(history[0].view(np.uint32), history[2].view(np.uint32))
    for i, f in enumerate(calls):
        with avd_hip.Context(0) as fresh:
            fresh.vit_set_weights(case.weight, case.bias)
            alone, _ = fresh.vit_patch_embed(f)
        assert np.isfinite(alone).all() and np.array_equal(history[i].view(np.uint32), alone.view(np.uint32)), f"call {i}: {f.shape[0]} frames"
