"""Hold-out content for the DEFAULT Farneback mode (fast level kernels + exact re-run of the pairs they flag): sixteen families that did not
exist when the four thresholds of csrc/avd_fb_device.h (kCondMax, kFlowMax, kTinyFlow, kJumpMin / kJumpMinZero) were derived on the 28 families
of tests/content_families.py -- the out-of-sample counterpart of that file.  Several of them aim at the one place where cv2's warp is
discontinuous and the fast kernels have no guard: FarnebackUpdateMatrices takes its "inside" branch iff floor(x + dx) < w - 1 and floor(y + dy) <
h - 1, so an integer pan to the right or downwards puts the warped coordinate of an interior pixel exactly on the last column / row.

Test infrastructure: used by tests/test_holdout_host.py, tests/test_gpu_holdout.py and tools/fuzz_fast_vs_exact.py.

REPRODUCIBILITY RULE.  A pair is a pure function of (bank, family, seed), the same bytes on torch-CPU and torch-ROCm:
  * the bank of base fields is built once on the host, in INTEGER numpy arithmetic from a fixed seed (box-blurred integer noise: no FFT, no
    libm, nothing a different CPU could round differently), and stored as uint8 / int16;
  * all randomness is integer parameters drawn on the host from numpy.random.default_rng(seed);
  * all pixel work is batched torch integer arithmetic on the device: crops, integer-weight blends (w * f + (256 - w) * g + 128) >> 8,
    sub-pixel pans with weights in sixteenths, table look-ups, comparisons.  No device RNG, no float anywhere.
That is what lets a violator found on the GPU be rebuilt on the CPU from its family name and seed alone.

Interface: holdout_families() -> {name: make}, make(bank, seeds, device) -> torch uint8[K, 2, 320, 320] on `device` (K = len(seeds)); bank() ->
the Bank; check() the one tolerance checker; run_default_and_exact() the one referee procedure.
"""
import math

import numpy as np
import torch

S = 320
F = 480                       # side of a bank field
M = 80                        # a crop's origin is (M + oy, M + ox); |oy|, |ox| <= 78 keeps crops (and the + 1 of a sub-pixel pan) inside
BANK_SEED = 0x40D0
TEST_SEED0 = 500_000          # seeds of the committed tests: seeds_for_tests(); the one-off fuzz takes its seeds from 10 ** 7 upwards (tools/fuzz_fast_vs_exact.py)
FUZZ_SEED_MIN = 10_000_000

# the soak draws sigma from {2.35, 2.5, 3, 4, 5, 6, 12} and beta from [0.8, 1.6]; three passes of a box of odd width w have sigma = sqrt((w * w - 1) / 4)
SMOOTH_BOX = (3, 7, 9, 15, 19, 27)                  # sigma 1.4, 3.5, 4.5, 7.5, 9.5, 13.5
# "pink": octaves of box-blurred noise (widths PINK_BOX, each brought to the same variance), weighted by small integers: spectral slopes of about
PINK_WEIGHTS = ((16, 11, 8, 6, 4, 3),               # beta 0.5
                (16, 13, 10, 8, 7, 5),              # beta 0.7
                (4, 6, 10, 16, 26, 42),             # beta 1.7
                (2, 4, 8, 15, 29, 56),              # beta 1.9
                (1, 2, 5, 12, 28, 64),              # beta 2.2
                (8, 8, 8, 8, 8, 8))                 # beta 1.0 on the octaves, white below the first
PINK_BOX = (1, 3, 5, 9, 17, 33)
PER_PRESET = 3
NF = (len(SMOOTH_BOX) + len(PINK_WEIGHTS)) * PER_PRESET    # 36 smooth / pink fields; then the text-like and the block field
TEXT, BLOCK = NF, NF + 1


# ---- the bank: integer numpy on the host ---------------------------------------------------------------------------------------------------
def _box(a, w):
    """periodic box SUM of odd width w along both axes (int64, exact)"""
    h = w // 2
    if h == 0:
        return a
    for ax in (0, 1):
        a = np.moveaxis(a, ax, 0)
        p = np.concatenate([a[-h:], a, a[:h]])
        c = np.concatenate([np.zeros((1,) + a.shape[1:], np.int64), np.cumsum(p, axis=0)])
        a = np.moveaxis(c[w:] - c[:-w], 0, ax)
    return a


def _blur3(a, w):
    for _ in range(3):
        a = _box(a, w)
    return a


def _stretch(f):
    """integer field -> 0 .. 255 over its full range"""
    lo, hi = int(f.min()), int(f.max())
    return ((f - lo) * 255 // max(hi - lo, 1)).astype(np.uint8)


def _standardise(f):
    """integer field -> clip(128 + 45 * (f - mean) / std), in integers"""
    n = f.size
    mean = int(f.sum()) // n
    d = f - mean
    std = max(math.isqrt(int((d * d).sum()) // n), 1)
    return np.clip(128 + (d * 45 + (std >> 1)) // std, 0, 255).astype(np.uint8)


class Bank:
    """fields uint8[NF + 2, 480, 480] (smooth, pink, text-like, 8 x 8 blocks), noise int16[16, 320, 320] in -2 .. 2, wave uint8[1024] (one period of
    a parabolic sine, 7 .. 247)."""

    def __init__(self):
        rng = np.random.default_rng(BANK_SEED)
        fields = np.empty((NF + 2, F, F), np.uint8)
        k = 0
        for w in SMOOTH_BOX:
            for _ in range(PER_PRESET):
                fields[k] = _stretch(_blur3(rng.integers(0, 256, (F, F)).astype(np.int64), w))
                k += 1
        octaves = []                                                # PER_PRESET sets of noise octaves, each octave brought to the same variance
        for _ in range(PER_PRESET):
            bs = [_blur3(rng.integers(-128, 128, (F, F)).astype(np.int64), w) // w ** 3 for w in PINK_BOX]
            octaves.append([b * 4096 // max(math.isqrt(int((b * b).sum()) // b.size), 1) for b in bs])
        for weights in PINK_WEIGHTS:
            for octs in octaves:
                fields[k] = _standardise(sum(b * wt for b, wt in zip(octs, weights)))
                k += 1
        text = np.full((F, F), 235, np.uint8)                       # lines of dark strokes on a light page
        for line in range(6, F - 12, 14):
            x = int(rng.integers(0, 12))
            while x < F - 12:
                ww, hh = int(rng.integers(2, 10)), int(rng.integers(3, 10))
                if rng.integers(0, 6):
                    text[line + 9 - hh:line + 9, x:x + ww] = int(rng.integers(0, 80))
                x += ww + int(rng.integers(1, 5))
        fields[TEXT] = text
        fields[BLOCK] = np.kron(rng.integers(0, 256, (F // 8, F // 8)).astype(np.uint8), np.ones((8, 8), np.uint8))
        self.fields = fields
        self.noise = rng.integers(-2, 3, (16, S, S)).astype(np.int16)
        t = np.arange(512, dtype=np.int64)
        half = (120 * 4 * t * (512 - t)) // (512 * 512)
        self.wave = np.concatenate([127 + half, 127 - half]).astype(np.uint8)
        self._on = {}

    def on(self, device):
        """the bank as torch tensors on `device` (cached)"""
        key = str(device)
        if key not in self._on:
            self._on[key] = {"fields": torch.from_numpy(self.fields).to(device), "noise": torch.from_numpy(self.noise).to(device),
                             "wave": torch.from_numpy(self.wave).to(device), "ar": torch.arange(S, dtype=torch.int64, device=device)}
        return self._on[key]


_BANK = None


def bank():
    global _BANK
    if _BANK is None:
        _BANK = Bank()
    return _BANK


# ---- batched integer pixel work (torch; every argument but `t` is an int64 tensor [K] on the device) ------------------------------------------
def _crop(t, fi, oy, ox):
    ys = (M + oy)[:, None] + t["ar"]
    xs = (M + ox)[:, None] + t["ar"]
    return t["fields"][fi[:, None, None], ys[:, :, None], xs[:, None, :]].to(torch.int32)


def _subpix(t, fi, oy16, ox16):
    """a crop at an origin given in sixteenths of a pixel: bilinear with integer weights, (.. + 128) >> 8"""
    oy, fy, ox, fx = oy16 >> 4, (oy16 & 15)[:, None, None], ox16 >> 4, (ox16 & 15)[:, None, None]
    a, b, c, d = _crop(t, fi, oy, ox), _crop(t, fi, oy, ox + 1), _crop(t, fi, oy + 1, ox), _crop(t, fi, oy + 1, ox + 1)
    return ((16 - fx) * (16 - fy) * a + fx * (16 - fy) * b + (16 - fx) * fy * c + fx * fy * d + 128) >> 8


def _blend(w, f, g):
    w = w[:, None, None]
    return (w * f + (256 - w) * g + 128) >> 8


def _noise(t, ni, lim=1):
    return t["noise"][ni].to(torch.int32).clamp(-lim, lim)


def _yx(t):
    return t["ar"][None, :, None], t["ar"][None, None, :]


def _rect(t, y0, x0, hh, ww):
    y, x = _yx(t)
    y0, x0, hh, ww = (v[:, None, None] for v in (y0, x0, hh, ww))
    return (y >= y0) & (y < y0 + hh) & (x >= x0) & (x < x0 + ww)


def _blockavg(a):
    k = a.shape[0]
    m = (a.reshape(k, S // 8, 8, S // 8, 8).sum((2, 4)) + 32) >> 6
    return m[:, :, None, :, None].expand(k, S // 8, 8, S // 8, 8).reshape(k, S, S)


def _base(rng):
    return [int(rng.integers(0, NF)), int(rng.integers(-40, 41)), int(rng.integers(-40, 41))]


def _nonzero2(rng, lim):
    """two integers in -lim .. lim, not both zero"""
    while True:
        a, b = (int(v) for v in rng.integers(-lim, lim + 1, 2))
        if a or b:
            return [a, b]


def _rot(rng):
    """an integer rotation (c, s) with c * c + s * s ~ 1024 ** 2, any angle"""
    s = int(rng.integers(-1024, 1025))
    c = math.isqrt(1024 * 1024 - s * s) * (1 if rng.integers(0, 2) else -1)
    return [c, s]


def _family(draw, compose):
    def make(bank, seeds, device="cpu"):
        P = np.array([draw(np.random.default_rng(int(s))) for s in seeds], np.int64).reshape(len(seeds), -1)
        t = bank.on(device)
        a, b = compose(t, *[torch.from_numpy(np.ascontiguousarray(P[:, j])).to(device) for j in range(P.shape[1])])
        return torch.stack([a.clamp(0, 255).to(torch.uint8), b.clamp(0, 255).to(torch.uint8)], 1)
    return make


NEAR_DUP_FIXED = ((0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1), (1, 0), (S // 2, S // 2))   # then one pixel in each of the 20 row tiles (16 source rows each)


def holdout_families():
    """name -> make(bank, seeds, device) -> torch uint8[K, 2, 320, 320]"""
    fam = {}

    # 1 .. 3: integer pans.  Content moving right by d: next(x) = prev(x - d); the flow dx = +d aims x + dx at column 319 from column 319 - d
    fam["pan_right"] = _family(lambda r: _base(r) + [int(r.integers(1, 9))],
                               lambda t, f, oy, ox, d: (_crop(t, f, oy, ox), _crop(t, f, oy, ox - d)))
    fam["pan_down"] = _family(lambda r: _base(r) + [int(r.integers(1, 9))],
                              lambda t, f, oy, ox, d: (_crop(t, f, oy, ox), _crop(t, f, oy - d, ox)))
    fam["pan_left_up"] = _family(lambda r: _base(r) + [int(r.integers(1, 9)), int(r.integers(1, 9))],
                                 lambda t, f, oy, ox, dy, dx: (_crop(t, f, oy, ox), _crop(t, f, oy + dy, ox + dx)))

    # 4: pans in sixteenths of a pixel, up to 4 px either way
    fam["subpixel_pan"] = _family(lambda r: _base(r) + _nonzero2(r, 64),
                                  lambda t, f, oy, ox, dy, dx: (_crop(t, f, oy, ox), _subpix(t, f, 16 * oy + dy, 16 * ox + dx)))

    # 5: pans of 2, 4, 8, 16 px right / down / both: 1, 2, 4, 8 px or a half at the 160-, 80- and 40-px levels, whose up-sampled flow aims at their last column / row
    def coarse(r):
        d, way = int(r.choice([2, 4, 8, 16])), int(r.integers(0, 3))
        return _base(r) + [d * (way != 0), d * (way != 1)]
    fam["pan_coarse_edge"] = _family(coarse, lambda t, f, oy, ox, dy, dx: (_crop(t, f, oy, ox), _crop(t, f, oy - dy, ox - dx)))

    # 6: two fields side by side (or one above the other), moving differently
    def halves(r):
        f2 = int(r.integers(0, NF))
        return _base(r) + [f2] + _nonzero2(r, 4) + _nonzero2(r, 4) + [int(r.integers(80, 241)), int(r.integers(0, 2))]

    def halves_c(t, f, oy, ox, f2, dy1, dx1, dy2, dx2, cut, vert):
        y, x = _yx(t)
        m = torch.where(vert[:, None, None] != 0, y >= cut[:, None, None], x >= cut[:, None, None])
        a = torch.where(m, _crop(t, f2, ox, oy), _crop(t, f, oy, ox))           # the second field at the transposed origin: other content even where f2 == f
        return a, torch.where(m, _crop(t, f2, ox - dy2, oy - dx2), _crop(t, f, oy - dy1, ox - dx1))
    fam["halves"] = _family(halves, halves_c)

    # 7: moving content under a fixed 8 x 8 block grid: each frame blended with its own block averages (heavy compression)
    def blocks8_c(t, f, oy, ox, dy, dx, w):
        a, b = _crop(t, f, oy, ox), _crop(t, f, oy - dy, ox - dx)
        return _blend(w, _blockavg(a), a), _blend(w, _blockavg(b), b)
    fam["blocks8"] = _family(lambda r: _base(r) + _nonzero2(r, 3) + [int(r.integers(64, 225))], blocks8_c)

    # 8: a quantised gradient at any angle with +-1 dither, sliding by a few pixels
    def banding(r):
        while True:
            ay, ax = (int(v) for v in r.integers(-160, 161, 2))              # grey levels per 256 px
            if abs(ay) + abs(ax) >= 32:
                break
        n1 = int(r.integers(0, 16))
        return [ay, ax, int(r.integers(4, 25)), int(r.integers(0, 64)), n1, (n1 + 1 + int(r.integers(0, 15))) % 16] + _nonzero2(r, 6)

    def banding_c(t, ay, ax, q, off, n1, n2, sy, sx):
        y, x = _yx(t)
        ay, ax, q, off, sy, sx = (v[:, None, None] for v in (ay, ax, q, off, sy, sx))

        def frame(yy, xx, ni):
            lvl = (128 + off + ((ay * (yy - 160) + ax * (xx - 160)) >> 8)).clamp(0, 255)
            return (torch.div(lvl, q, rounding_mode="floor") * q + _noise(t, ni)).to(torch.int32)
        return frame(y, x, n1), frame(y - sy, x - sx, n2)
    fam["banding"] = _family(banding, banding_c)

    # 9: interlace comb: even rows from field time t, odd rows from t + 1
    def comb_c(t, f, oy, ox, dy, dx):
        even = (t["ar"] & 1)[None, :, None] == 0
        f0, f1, f2 = _crop(t, f, oy, ox), _crop(t, f, oy - dy, ox - dx), _crop(t, f, oy - 2 * dy, ox - 2 * dx)
        return torch.where(even, f0, f1), torch.where(even, f1, f2)
    fam["comb"] = _family(lambda r: _base(r) + [int(r.integers(-3, 4)), int(r.integers(1, 7)) * (1 if r.integers(0, 2) else -1)], comb_c)

    # 10: a band of text scrolling to the left over a bit-identical background
    def ticker(r):
        bh = int(r.integers(16, 49))
        return _base(r) + [int(r.integers(150, S - 4 - bh)), bh, int(r.integers(-40, 41)), int(r.integers(-40, 33)), int(r.integers(1, 9))]

    def ticker_c(t, f, oy, ox, y0, bh, ty, tx, d):
        bg = _crop(t, f, oy, ox)
        zero = torch.zeros_like(y0)
        band = _rect(t, y0, zero, bh, zero + S)
        txt = torch.full_like(f, TEXT)
        return torch.where(band, _crop(t, txt, ty, tx), bg), torch.where(band, _crop(t, txt, ty, tx + d), bg)
    fam["ticker"] = _family(ticker, ticker_c)

    # 11: values 0 .. 3: a dark scene's two bits plus fresh +-1 noise, panning slightly
    def dark(r):
        n1 = int(r.integers(0, 16))
        return _base(r) + [int(r.integers(-2, 3)), int(r.integers(-2, 3)), n1, (n1 + 1 + int(r.integers(0, 15))) % 16]
    fam["dark_noise"] = _family(dark, lambda t, f, oy, ox, dy, dx, n1, n2: (((_crop(t, f, oy, ox) >> 6) + _noise(t, n1)).clamp(0, 3),
                                                                             ((_crop(t, f, oy - dy, ox - dx) >> 6) + _noise(t, n2)).clamp(0, 3)))

    # 12: two steps of a cross-fade between two fields
    def blend(r):
        w1 = int(r.integers(0, 257))
        step = int(r.integers(8, 65))
        w2 = w1 + step if w1 + step <= 256 else w1 - step
        return _base(r) + [(int(r.integers(1, NF))), int(r.integers(-40, 41)), int(r.integers(-40, 41)), w1, w2]

    def blend_c(t, f, oy, ox, df, gy, gx, w1, w2):
        a, g = _crop(t, f, oy, ox), _crop(t, (f + df) % NF, gy, gx)
        return _blend(w1, a, g), _blend(w2, a, g)
    fam["blend"] = _family(blend, blend_c)

    # 13: a rotated checkerboard, cell 5 .. 23 px, shifted by 1/4 .. 4 px in sixteenths
    def rot_checker(r):
        lo = int(r.integers(0, 101))
        sh = [int(r.integers(4, 65)) * (1 if r.integers(0, 2) else -1) for _ in range(2)]
        return _rot(r) + [int(r.integers(5, 24)), int(r.integers(0, 1 << 20)), int(r.integers(0, 1 << 20)), lo, int(r.integers(lo + 60, 256))] + sh

    def rot_checker_c(t, c, s, cell, ou, ov, lo, hi, sy, sx):
        y, x = _yx(t)
        c, s, cell, ou, ov, lo, hi, sy, sx = (v[:, None, None] for v in (c, s, cell, ou, ov, lo, hi, sy, sx))

        def frame(y16, x16):                                                  # coordinates in sixteenths of a pixel; u, v in 1 / 16384 px
            u, v = c * x16 + s * y16 + ou * 16, c * y16 - s * x16 + ov * 16
            bit = (torch.div(u, cell * 16384, rounding_mode="floor") + torch.div(v, cell * 16384, rounding_mode="floor")) & 1
            return (lo + bit * (hi - lo)).to(torch.int32)
        return frame(16 * y, 16 * x), frame(16 * y - sy, 16 * x - sx)
    fam["rot_checker"] = _family(rot_checker, rot_checker_c)

    # 14: two waves of the table, periods P (6 .. 40 px, in sixteenths) and 1.01 P, along any direction; shifted by up to 3 px
    def near_periodic(r):
        return _rot(r) + [int(r.integers(96, 641)), int(r.integers(0, 1 << 16)), int(r.integers(0, 1 << 16))] + _nonzero2(r, 48)

    def near_periodic_c(t, c, s, p16, ph1, ph2, sy, sx):
        y, x = _yx(t)
        c, s, p16, ph1, ph2, sy, sx = (v[:, None, None] for v in (c, s, p16, ph1, ph2, sy, sx))
        st1 = torch.div(1 << 26, p16, rounding_mode="floor")                  # 2 ** 16 of phase (65536 = one period) per 1 / 1024 px
        st2 = torch.div(st1 * 100, 101, rounding_mode="floor")                # the second wave's period is 1 % longer

        def frame(y16, x16):
            u = (c * x16 + s * y16) >> 4                                      # distance along the direction in 1 / 1024 px
            i1 = ((((u * st1) >> 16) + ph1) >> 6) & 1023
            i2 = ((((u * st2) >> 16) + ph2) >> 6) & 1023
            return ((t["wave"][i1].to(torch.int32) + t["wave"][i2].to(torch.int32) + 1) >> 1)
        return frame(16 * y, 16 * x), frame(16 * y - sy, 16 * x - sx)
    fam["near_periodic"] = _family(near_periodic, near_periodic_c)

    # 15: a static flat picture with a textured right / bottom border (the last 20 columns and rows) and one changed patch inside
    def static_rb(r):
        return _base(r) + [int(r.integers(20, 270)), int(r.integers(20, 270)), int(r.integers(1, 12)), int(r.integers(1, 12)),
                           int(r.integers(1, 61)) * (1 if r.integers(0, 2) else -1)]

    def static_rb_c(t, f, oy, ox, y0, x0, hh, ww, delta):
        y, x = _yx(t)
        a = torch.where((y >= S - 20) | (x >= S - 20), _crop(t, f, oy, ox), torch.full((1, 1, 1), 128, dtype=torch.int32, device=f.device))
        return a, torch.where(_rect(t, y0, x0, hh, ww), a + delta[:, None, None], a)
    fam["static_rb_border"] = _family(static_rb, static_rb_c)

    # 16: frame t + 1 is frame t except for ONE pixel: a corner, (1, 0), the centre, or a pixel in one of the 20 row tiles of the pyramid kernel's
    # 160-px scale (16 source rows each), whose "frames differ" words the fast level kernels ballot over
    def near_dup(r):
        k = int(r.integers(0, len(NEAR_DUP_FIXED) + 20))
        yy, xx = int(r.integers(0, 16)), int(r.integers(0, S))
        y, x = NEAR_DUP_FIXED[k] if k < len(NEAR_DUP_FIXED) else (16 * (k - len(NEAR_DUP_FIXED)) + yy, xx)
        return _base(r) + [y, x, int(r.integers(1, 256))]

    def near_dup_c(t, f, oy, ox, y0, x0, m):
        a = _crop(t, f, oy, ox)
        one = torch.ones_like(y0)
        return a, torch.where(_rect(t, y0, x0, one, one), a ^ m[:, None, None].to(torch.int32), a)
    fam["near_duplicate"] = _family(near_dup, near_dup_c)

    return fam


CUT_BETWEEN = "cut_between"      # the seventeenth row: the pairs (2k + 1, 2k + 2) between two pairs of a family, scene cuts between unrelated content
# families in which at least three quarters of the pairs must stay UNFLAGGED (the CPU model of the fast arithmetic flagged none of their counterparts):
# otherwise the fast kernels are not what is being tested
MOSTLY_UNFLAGGED = ("pan_right", "pan_down", "pan_left_up", "subpixel_pan", "halves", "blocks8", "comb", "dark_noise", "blend")


def seeds_for_tests(family_index, n):
    """the committed tests' seeds of a family: the first two are the pinned-hash pairs"""
    return [TEST_SEED0 + 100_003 * family_index + i for i in range(n)]


def pair_sha256(pair):
    """SHA-256 of one pair, uint8[2, 320, 320] (torch on any device, or numpy)"""
    import hashlib
    a = pair.cpu().numpy() if hasattr(pair, "cpu") else np.asarray(pair)
    assert a.shape == (2, S, S) and a.dtype == np.uint8
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the checker: the default mode's stated guarantee, pair by pair --------------------------------------------------------------------------
REL, ABS = 1e-6, 1e-7            # tests/test_gpu_soak.py: pytest.approx(rel=1e-6, abs=1e-7) on flow_mean and flow_var, i.e. |delta| <= max(rel * |exact|, abs)
MEAN_TOL = 1e-6                  # and |delta flow_mean| <= 1e-6 * max(1, |m|)  (|delta ai_susp| at tex -> infinity)
FLOW_TOL = 1e-5                  # px, dense flow of an unflagged pair (tests/test_gpu_fbfast.py)


def check(fm, fv, xm, xv, flagged):
    """fm, fv: the default mode's flow_mean / flow_var (float32[n]); xm, xv: the referee's (exact mode or oracle); flagged: bool[n], the pair was
    re-run exactly.  -> list of violations (pair index, kind, default's value, referee's value); empty = the guarantee holds:
      every value finite; a flagged pair equal to the referee BIT FOR BIT; an unflagged pair within rel 1e-6 / abs 1e-7 on both statistics and
      |delta flow_mean| <= 1e-6 * max(1, |m|)."""
    fm, fv, xm, xv = (np.ascontiguousarray(v, np.float32) for v in (fm, fv, xm, xv))
    flagged = np.asarray(flagged, bool)
    assert fm.shape == fv.shape == xm.shape == xv.shape == flagged.shape and fm.ndim == 1
    bad = []
    finite = np.isfinite(fm) & np.isfinite(fv) & np.isfinite(xm) & np.isfinite(xv)
    same = (fm.view(np.uint32) == xm.view(np.uint32)) & (fv.view(np.uint32) == xv.view(np.uint32))
    d = {k: (f.astype(np.float64), x.astype(np.float64)) for k, f, x in (("flow_mean", fm, xm), ("flow_var", fv, xv))}
    with np.errstate(invalid="ignore"):
        out = {k: np.abs(f - x) > np.maximum(REL * np.abs(x), ABS) for k, (f, x) in d.items()}
        f, x = d["flow_mean"]
        out["ai_susp"] = np.abs(f - x) > MEAN_TOL * np.maximum(1.0, np.abs(x))
    for p in range(len(fm)):
        if not finite[p]:
            bad.append((p, "not finite", (float(fm[p]), float(fv[p])), (float(xm[p]), float(xv[p]))))
        elif flagged[p]:
            if not same[p]:
                bad.append((p, "flagged pair not bit-identical", (float(fm[p]), float(fv[p])), (float(xm[p]), float(xv[p]))))
        else:
            for k in ("flow_mean", "flow_var", "ai_susp"):
                if out[k][p]:
                    src = d["flow_mean" if k == "ai_susp" else k]
                    bad.append((p, f"unflagged pair out of tolerance: {k}", float(src[0][p]), float(src[1][p])))
    return bad


# ---- the referee procedure: default mode against exact mode, both on the GPU ------------------------------------------------------------------
def run_default_and_exact(default, exact, G):
    """G: uint8[n, 320, 320] frames (torch on the device, or numpy); default / exact: two contexts, library defaults and fb_mode = 0.
    -> dict: fm, fv (default, avd_farneback_pairs), xm, xv (exact), reserved int[n - 1] (the flag word of each pair, from the records of
    avd_analyze_frames on the same frames as three equal channels), rerun_pairs of either call, rec_mean / rec_var (the records' statistics)."""
    assert default.get_option("fb_mode") == 1 and default.get_option("fb_rerun") == 1          # the library defaults
    assert exact.get_option("fb_mode") == 0
    fm, fv = default.farneback_pairs(G)
    rerun_pairs_call = default.get_option("rerun_pairs")
    if hasattr(G, "expand"):
        G3 = G[..., None].expand(-1, -1, -1, 3).contiguous()
    else:
        G3 = np.repeat(G[..., None], 3, axis=3)
    rec = default.analyze_frames(G3)
    rerun_records_call = default.get_option("rerun_pairs")
    xm, xv = exact.farneback_pairs(G)
    return {"fm": fm, "fv": fv, "xm": xm, "xv": xv, "reserved": rec["reserved"][1:].astype(np.int64), "rec_mean": rec["flow_mean"][1:].copy(),
            "rec_var": rec["flow_var"][1:].copy(), "rerun_pairs_call": rerun_pairs_call, "rerun_records_call": rerun_records_call}


def summarise(r, sel=None):
    """the figures of a report line for the pairs `sel` (a slice or index array; default all) of a run_default_and_exact result ->
    dict(pairs, flagged, solver, border, differ, max_dmean)"""
    sel = slice(None) if sel is None else sel
    res = r["reserved"][sel]
    fm, fv, xm, xv = (np.ascontiguousarray(r[k][sel], np.float32) for k in ("fm", "fv", "xm", "xv"))
    differ = (fm.view(np.uint32) != xm.view(np.uint32)) | (fv.view(np.uint32) != xv.view(np.uint32))
    dm = np.abs(fm.astype(np.float64) - xm.astype(np.float64))
    return {"pairs": int(len(res)), "flagged": int(np.count_nonzero(res)), "solver": int(np.count_nonzero(res & 0x0F)),
            "border": int(np.count_nonzero(res & 0xF0)), "differ": int(np.count_nonzero(differ)),
            "max_dmean": float(np.nanmax(dm)) if len(dm) else 0.0}


# ---- pinned bytes: SHA-256 of the bank and of the first two test pairs of every family (seeds_for_tests(j, 2)).  tests/test_holdout_host.py checks them on
# torch-CPU, tests/test_gpu_holdout.py on frames composed on the device
BANK_SHA256 = "61460a63277453481c461de8de604f094da050222b9223ec63f0d0a51e5b6d7d"
PINNED_SHA256 = {
    "pan_right": ("8148327308ba4b851025db883bd3e9fe1d20094a7bb68d1aa1a35b0a381369d5",
                 "d56b27ae2c809bc659fe6ec518cb07b70d010e6c475fe4992e9d884c0c7b7b78"),
    "pan_down": ("698a1b60abb2e68615b8ea8aae93f60554f33e6e2ed59676d86966f2c1650995",
                "d9f7d9bf551080170cedd473e310360d525cb464836226bce3fe2d3bc9f6e204"),
    "pan_left_up": ("2ccf255f5b0246bbf98c8a26533f9a5e4b2c8e547177d00b3dc038bfc623523b",
                   "26999e2706e99bf7e087fec63a307ac40f8c9cda5e176283d3ecdc932a348ff5"),
    "subpixel_pan": ("9151b548472311241d73a6ece8d56575284b222a3fb02e33bce020edbff6765d",
                    "159ba9c5f00e2f02a42bce071460e632214d77f1b31c2bd415e18d842948c160"),
    "pan_coarse_edge": ("53c5d7a506d1b02e56ab98a50842f13ea234156bfd22a61ee4990299ba5b4141",
                       "d8b40230f164ca205deff49399793ebe741874b9d23103397cf7371db4f32cf6"),
    "halves": ("5b86a5743c7bdce093b4ea2da517e78090be2004ab8be9a7c19f28e7f9142455",
              "dc11645a53f79547d8db8e648fe9f6323a64ddaf1b17631f96d08aa11ab1a042"),
    "blocks8": ("9c2bfdc5acdfd40c5ae7620f686c238af55bdbb295148d403ada536ec1edbbc9",
               "bc779cb0dd3b09be64b4b7c4dd22013e338d15057ad83c0b6de97446eb558103"),
    "banding": ("7f92558cad763a7de485fc10068332c41610fbbe33637a3c4d010a81115611cf",
               "7dfaa00e9df385e45a1d3885b2d0176aebfe2af611e495208603e942164d371d"),
    "comb": ("74e86fcc82f96fad40fac3caa8a92a6a0136a23b5193378f48d86ff5a55ac485",
            "16d18915c1c1749f63f77502b7511b120a06a5610f04ce00bab780064a31d565"),
    "ticker": ("efc2a97c38d7d9072618ec033c226ba35f04a96546624d5d79a1fd415569d7e7",
              "662cb6628662444f475fa8377ae8a97f7a7b50fe15d21a6fcda18faca8a15aa5"),
    "dark_noise": ("689c270a345f358a4de344e6e5c6da330abac539ae39eb49c2be985d935b4b89",
                  "d40fdc66f8a2d84d5b0f7d0c7e4d985c813355960c04451727d5173f2484e73f"),
    "blend": ("ea556c4c39438a3a7be05e6de9969d4a7e8a16a87a54400c9e2c82154532a66a",
             "8ae425b22f30ee57296c3ca88101fef45093fe6bb484f8ace32aff7184973c34"),
    "rot_checker": ("4ac083e9b8e25f79a5717c8a19ba0988e8a5c588dc5f6978c052bb98c90c0836",
                   "3953081578df43d07d7d26a40af0ce60b7a464aed0eabf6b530cf136705f1d7d"),
    "near_periodic": ("eff8c728807504519953c4e00b2368b3985b8a76e298b643d91fca24ef9b35d2",
                     "ef99ea1216581d739a0b054ba0ea62050eb86f022d93713ee07ca0ded3197c7b"),
    "static_rb_border": ("a840018d723b2c85d4b0a447dd6c9dd485e668302030adf8151154d5843c91c8",
                        "c50606b33cad49e5803744f6248c3041e52f78bf46314c7d4416f4b8c0f95c3e"),
    "near_duplicate": ("2c6215d1b4d228f7c259f503af3367b517a6c5e8bb08c7e0ba6489bf9a45820d",
                      "71f7d55b6359ba33255d51d5dfa1dae8921e67bf2732331ed42238c18ef6f290"),
}
