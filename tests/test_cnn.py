"""ResNet-50-style CNN forward on the matrix cores -- a build-defined extension with NO
reference counterpart (the reference has no learned model).  Its oracle is a float32 restatement on
the CPU (torch.nn.functional on the host, plumbing only): the same bf16-rounded weights, every activation rounded to bf16
where the HIP path stores it, accumulation in float32.  Tolerances (stated here; north_star's 1e-4 is for the reference's
own outputs): one layer -- the two float32 accumulation orders can land on opposite sides of a bf16 rounding boundary, so
|error| <= 2^-7 |ref| + 2e-3 (one bf16 ulp); the whole network (53 layers of such roundings) -- logits within 0.8 % of the
largest |logit| (budget derived in test_forward_against_float32, with a negative control: a missing residual in the last
block is 5x outside it) and a correlation above 0.9999.

The forward is also checked STAGE BY STAGE (option "cnn_tap", debug buffers "cnn_tap" / "cnn_plan"): each stage alone against a CPU reference
computed from the GPU's own taps of its producers, so a stage's tolerance is that of one layer.  Input image and max pool: bit for bit.  Each of
the 53 convolutions: the per-layer tolerance above on every element, more than 98 % of the elements bit-identical.  Pooled features:
|err| <= 64 * 2^-24 * ref (a sequential float32 sum of 49 non-negative terms and one multiply).  Logits: |err| <= 64 * 2^-24 * (|pooled| @ |W|.T + |b|)
(32 FMAs per lane, six shuffle adds, the bias).  Recorded on an MI355X (two 360 x 640 frames, seeded_parameters(0); "[cnn-stages]" lines of
-m gpu -s): over the 53 convolutions the worst |err| / tolerance is 0.803 (conv 27, 512 -> 1024 1x1 / 2; the stem 0.678) -- a single bf16 ulp
where the two accumulation orders round apart -- and the smallest bit-identical share 0.99986 (conv 47, 2048 -> 512 1x1); pooled features 0.024
of their bound, logits 0.005 of theirs.  CPU negative controls restate five kernel bugs that the end-to-end comparison cannot see (a stem that pads by
replication or drops kernel column 6, a wrapped right-border tap, an unstored tail tile, a dropped bias channel): the stage criterion rejects each."""
import numpy as np
import pytest

from avd_hip import _lib, synth

torch = pytest.importorskip("torch")
F = torch.nn.functional

DEPTH = (3, 4, 6, 3)


def topology(roles=False):
    """[(cin, cout, ksize, stride)] in the order of avd_cnn_set_weights, without the final linear layer."""
    convs, role = [(3, 64, 7, 2)], ["stem"]
    cin = 64
    for st, depth in enumerate(DEPTH):
        mid, out = 64 << st, (64 << st) * 4
        for b in range(depth):
            s = 2 if (b == 0 and st > 0) else 1
            convs += [(cin, mid, 1, 1), (mid, mid, 3, s), (mid, out, 1, 1)]
            role += ["reduce", "spatial", "expand"]
            if b == 0:
                convs.append((cin, out, 1, s))
                role.append("shortcut")
            cin = out
    return (convs, role) if roles else convs


def seeded_parameters(seed=0):
    """He-style random weights (the third convolution of a block and the shortcut damped so that the residual sums stay
    bounded without batch norm), small biases; returns flat float32 arrays in the documented order."""
    rng = np.random.default_rng(seed)
    ws, bs = [], []
    convs, role = topology(roles=True)
    for (cin, cout, k, s), what in zip(convs, role):
        fan = cin * k * k
        std = np.sqrt(2.0 / fan) * (0.5 if what in ("expand", "shortcut") else 1.0)
        ws.append((rng.standard_normal((cout, k, k, cin)) * std).astype(np.float32).ravel())
        bs.append((rng.standard_normal(cout) * 0.05).astype(np.float32))
    ws.append((rng.standard_normal((1000, 2048)) * np.sqrt(1.0 / 2048)).astype(np.float32).ravel())
    bs.append((rng.standard_normal(1000) * 0.05).astype(np.float32))
    return np.concatenate(ws), np.concatenate(bs)


def bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)          # round to nearest even, as the kernels do


def conv_preactivation(x_nhwc, w, bias, stride, padding=None):
    """float32 NHWC x and [cout][k][k][cin] w, both rounded to bf16 first -> the float32 sums + bias, NCHW (torch)."""
    x = bf16(torch.from_numpy(np.ascontiguousarray(x_nhwc))).permute(0, 3, 1, 2)
    wt = bf16(torch.from_numpy(np.ascontiguousarray(w))).permute(0, 3, 1, 2)
    return F.conv2d(x, wt, torch.from_numpy(bias), stride=stride, padding=w.shape[1] // 2 if padding is None else padding)


def conv_finish(y, relu, residual=None):
    """+ residual (NHWC, rounded to bf16 first), ReLU, rounded to bf16 -> float32 NHWC (numpy)."""
    if residual is not None:
        y = y + bf16(torch.from_numpy(np.ascontiguousarray(residual))).permute(0, 3, 1, 2)
    if relu:
        y = torch.relu(y)
    return bf16(y).permute(0, 2, 3, 1).contiguous().numpy()


def conv_reference(x_nhwc, w, bias, stride, relu, residual=None):
    """float32 NHWC in / out; x, w, residual are rounded to bf16 first; output rounded to bf16."""
    return conv_finish(conv_preactivation(x_nhwc, w, bias, stride), relu, residual)


def input_reference(frames):
    """uint8 BGR [N,H,W,3] -> float32 (bf16-rounded) [N,3,224,224] RGB, the arithmetic of the patch-embed input."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("_vit_reference", os.path.join(os.path.dirname(__file__), "test_vit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    patchify_reference = mod.patchify_reference
    n = frames.shape[0]
    a = patchify_reference(frames).reshape(n, 14, 14, 3, 16, 16)              # [n, gy, gx, c, py, px]
    return np.ascontiguousarray(a.transpose(0, 3, 1, 4, 2, 5).reshape(n, 3, 224, 224))


def forward_reference(frames, weights, biases, break_last_residual=False):
    """break_last_residual: a deliberately WRONG network (the last block forgets its residual) -- the negative control of
    the end-to-end test: its logits must differ from the right ones by far more than the test's tolerance."""
    convs = topology()
    wo = bo = 0
    params = []
    for cin, cout, k, s in convs:
        w = torch.from_numpy(weights[wo:wo + cout * k * k * cin].reshape(cout, k, k, cin))
        params.append((bf16(w).permute(0, 3, 1, 2).contiguous(), torch.from_numpy(biases[bo:bo + cout]), k, s))
        wo += cout * k * k * cin
        bo += cout
    wfc = bf16(torch.from_numpy(weights[wo:wo + 1000 * 2048].reshape(1000, 2048)))
    bfc = torch.from_numpy(biases[bo:bo + 1000])

    def conv(x, i, relu=True, res=None):
        w, b, k, s = params[i]
        y = F.conv2d(x, w, b, stride=s, padding=k // 2)
        if res is not None:
            y = y + res
        return bf16(torch.relu(y) if relu else y)

    x = torch.from_numpy(input_reference(frames))
    x = conv(x, 0)
    x = F.max_pool2d(x, 3, 2, 1)
    li = 1
    for st, depth in enumerate(DEPTH):
        for b in range(depth):
            a1 = conv(x, li)
            a2 = conv(a1, li + 1)
            res = conv(x, li + 3, relu=False) if b == 0 else x
            if break_last_residual and st == len(DEPTH) - 1 and b == depth - 1:
                res = None
            x = conv(a2, li + 2, res=res)
            li += 4 if b == 0 else 3
    pooled = x.mean(dim=(2, 3))
    return (pooled @ wfc.t() + bfc).numpy()


def test_parameter_counts_match_the_documented_topology():
    nw, nb = _lib.Context.cnn_param_counts()
    convs = topology()
    assert len(convs) == 53
    assert nw == sum(co * k * k * ci for ci, co, k, s in convs) + 1000 * 2048 == 25_502_912
    assert nb == sum(co for ci, co, k, s in convs) + 1000
    w, b = seeded_parameters(1)
    assert w.size == nw and b.size == nb


CONV_CASES = [
    # n, h, w, cin, cout, k, stride, relu, residual
    (1, 8, 8, 64, 64, 1, 1, True, False),            # K = 64: two half stages, one tile, 64-channel body
    (2, 14, 14, 64, 128, 3, 1, True, False),         # 3x3 with padding, 128-channel body, 392 rows (tail tile)
    (1, 20, 20, 128, 256, 1, 1, False, True),        # residual without ReLU, 256-channel body
    (2, 16, 16, 128, 128, 3, 2, True, False),        # stride 2 on the 3x3
    (1, 14, 14, 256, 512, 1, 2, False, False),       # strided 1x1 (projection shortcut), two column tiles
    (3, 7, 7, 512, 2048, 1, 1, True, True),          # last stage: 147 rows, eight column tiles, residual + ReLU
    (1, 28, 28, 160, 64, 1, 1, True, False),         # the stem's im2col shape: K = 160 (five half stages)
    (1, 9, 11, 96, 192, 3, 1, True, False),          # odd geometry, channel counts that are not powers of two
    (1, 8, 8, 32, 64, 1, 1, True, False),            # one half stage: a ring of one slot
    (1, 8, 8, 96, 128, 1, 1, False, False),          # three half stages
    (1, 1, 1, 32, 64, 3, 1, True, False),            # a single pixel: eight of nine taps on the zero page
    (5, 3, 3, 32, 64, 3, 1, True, True),             # tiny frames: neighbouring frames adjoin in the pixel index and a tap must not cross
    (1, 33, 31, 256, 512, 3, 2, True, False),        # odd geometry under stride 2
    (2, 7, 7, 2048, 512, 1, 1, True, False),         # 64 half stages
    (1, 7, 7, 512, 512, 3, 1, True, True),           # K = 4608
    (2, 14, 14, 1024, 2048, 1, 2, False, False),     # the last projection shortcut
]


def layer_figures(got, want):
    """The per-layer criterion's two figures: the worst |error| / tolerance (tolerance 2^-7 |ref| + 2e-3; <= 1 passes) and the
    share of bit-identical elements (> 0.98 passes)."""
    err = np.abs(got - want)
    tol = np.abs(want) * 2.0 ** -7 + 2e-3
    return float((err / tol).max()), float(np.mean(got == want))


def layer_ok(got, want):
    worst, same = layer_figures(got, want)
    return got.shape == want.shape and worst <= 1.0 and same > 0.98


@pytest.mark.gpu
@pytest.mark.parametrize("case", CONV_CASES)
def test_one_convolution_against_float32(ctx, case):
    n, h, w, cin, cout, k, stride, relu, with_res = case
    rng = np.random.default_rng(hash(case) % 2**32)
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    wt = (rng.standard_normal((cout, k, k, cin)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    res = rng.standard_normal((n, ho, wo, cout)).astype(np.float32) if with_res else None
    want = conv_reference(x, wt, b, stride, relu, res)
    try:
        for policy in (0, 1, 2):                     # the heuristic, the 256-pixel bodies, 128 x 128 wherever cout allows
            ctx.set_option("cnn_tiles", policy)
            got = ctx.cnn_conv(x, wt, b, stride=stride, relu=relu, residual=res)
            assert got.shape == want.shape
            err = np.abs(got - want)
            tol = np.abs(want) * 2.0 ** -7 + 2e-3
            assert np.all(err <= tol), (policy, float(err.max()), int((err > tol).sum()))
            assert np.mean(got == want) > 0.98, policy   # all but the rare rounding-boundary cases are bit-identical
    finally:
        ctx.set_option("cnn_tiles", 0)


@pytest.mark.gpu
def test_convolution_of_a_delta_is_the_flipped_kernel(ctx):
    """Known-answer: a single one at pixel (3, 4) of channel 5, 3x3 weights = small integers, no bias: the output around
    the pixel is the mirrored kernel (cross-correlation), exactly (integers are exact in bf16)."""
    x = np.zeros((1, 8, 8, 32), np.float32)
    x[0, 3, 4, 5] = 1.0
    wt = np.zeros((64, 3, 3, 32), np.float32)
    wt[:, :, :, 5] = np.arange(64 * 9).reshape(64, 3, 3) % 17 - 8
    y = ctx.cnn_conv(x, wt, np.zeros(64, np.float32), stride=1, relu=False)
    for dy in range(3):
        for dx in range(3):
            assert np.array_equal(y[0, 3 + 1 - dy, 4 + 1 - dx], wt[:, dy, dx, 5])
    assert np.count_nonzero(y) == np.count_nonzero(wt[:, :, :, 5])


@pytest.mark.gpu
def test_forward_against_float32(ctx):
    weights, biases = seeded_parameters(0)
    ctx.cnn_set_weights(weights, biases)
    frames = np.concatenate([synth.make_clip(2, 360, 640, seed=5), synth.random_frames(1, 360, 640, seed=6)])
    logits, ms = ctx.cnn_forward(frames, timing_reps=1)
    assert logits.shape == (3, 1000) and np.all(np.isfinite(logits)) and ms > 0
    want = forward_reference(frames, weights, biases)
    scale = float(np.abs(want).max())
    assert scale > 0.1                                # the seeded network does produce a signal
    # Budget: a layer's two float32 accumulation orders flip < 2 % of its bf16 roundings by one ulp (2^-8 relative, asserted
    # per layer above); 53 such layers in sequence, errors adding like a random walk and averaged over 49 pixels by the
    # pooling: sqrt(53 * 0.02) * 2^-8 ~ 0.4 % of an activation's magnitude at worst, i.e. well under 1 % of the largest logit.
    err = float(np.abs(logits - want).max()) / scale
    print(f"[cnn] end-to-end max |logit error| = {err:.5f} of the largest |logit|")
    assert err <= 0.008
    assert np.corrcoef(logits.ravel(), want.ravel())[0, 1] > 0.9999
    # negative control: a network whose LAST block forgets its residual (the smallest structural error there is) lies far
    # outside that tolerance, so this comparison would notice it
    wrong = forward_reference(frames, weights, biases, break_last_residual=True)
    assert float(np.abs(wrong - want).max()) / scale > 5 * 0.008
    # batch independence: a frame alone gives the same logits as inside the batch
    alone, _ = ctx.cnn_forward(frames[1:2])
    assert np.array_equal(alone[0], logits[1])


@pytest.mark.gpu
def test_every_tiling_gives_the_same_bits(ctx):
    """The 256 x 256 / 256 x 128 / 256 x 64 / 128 x 128 bodies accumulate an output's K terms in the same order."""
    outs = {}
    try:
        for policy in (0, 1, 2):
            ctx.set_option("cnn_tiles", policy)
            res = []
            for (n, h, w, cin, cout, k, stride) in [(2, 24, 24, 64, 256, 1, 1), (1, 40, 40, 128, 128, 3, 1), (1, 33, 31, 256, 512, 3, 2),
                                                    (1, 48, 48, 64, 64, 3, 1)]:
                r = np.random.default_rng(n * 1000 + cout + k)
                x = r.standard_normal((n, h, w, cin)).astype(np.float32)
                wt = (r.standard_normal((cout, k, k, cin)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
                b = (r.standard_normal(cout) * 0.1).astype(np.float32)
                res.append(ctx.cnn_conv(x, wt, b, stride=stride, relu=True))
            outs[policy] = res
    finally:
        ctx.set_option("cnn_tiles", 0)
    for a, b1, b2 in zip(outs[0], outs[1], outs[2]):
        assert np.array_equal(a, b1) and np.array_equal(a, b2)


@pytest.mark.gpu
def test_fused_blocks_give_the_same_bits(ctx):
    """A block's 3x3 + expanding 1x1 in one launch (k_conv3_expand, stages 1 and 2; the default) accumulates every output's K
    terms in the order of the two separate layers and rounds the mid activation to bf16 at the same place: identical logits."""
    weights, biases = seeded_parameters(0)
    ctx.cnn_set_weights(weights, biases)
    frames = synth.random_frames(5, 96, 128, seed=21)
    default = ctx.get_option("cnn_fuse")
    assert default in (1, 2)
    try:
        ctx.set_option("cnn_fuse", 0)
        plain, _ = ctx.cnn_forward(frames)
        ctx.set_option("cnn_fuse", 1)
        fused, _ = ctx.cnn_forward(frames)
        ctx.set_option("cnn_fuse", 2)                  # the 56 x 56 stage with the 3x3's input as one slab in LDS (k_slab3_expand)
        slab, _ = ctx.cnn_forward(frames)
    finally:
        ctx.set_option("cnn_fuse", default)
    assert np.isfinite(fused).all() and float(np.abs(fused).max()) > 0
    assert np.array_equal(fused, plain)
    assert np.array_equal(slab, plain)


@pytest.mark.gpu
def test_forward_in_passes_of_128_frames(ctx):
    """More frames than one pass holds: the second pass reuses every scratch buffer; frames repeat, so must the logits."""
    weights, biases = seeded_parameters(0)
    ctx.cnn_set_weights(weights, biases)
    base = synth.random_frames(3, 96, 128, seed=9)
    frames = np.concatenate([base] * 44)[:131]                       # 131 frames: 128 + 3
    logits, _ = ctx.cnn_forward(frames)
    assert logits.shape == (131, 1000)
    for i in range(131):
        assert np.array_equal(logits[i], logits[i % 3])


@pytest.mark.gpu
def test_forward_needs_weights_and_checks_counts():
    c = _lib.Context(0)
    with pytest.raises(_lib.AvdError):
        c.cnn_forward(np.zeros((1, 64, 64, 3), np.uint8))
    with pytest.raises(_lib.AvdError):
        c.cnn_set_weights(np.zeros(10, np.float32), np.zeros(10, np.float32))
    c.close()


# ---- the forward stage by stage ---------------------------------------------------------------------------------------
# Option "cnn_tap" makes a forward copy ONE intermediate aside (debug buffer "cnn_tap"); "cnn_plan" tells which kernel shape ran
# each convolution.  Every stage is checked alone and teacher-forced: its reference is computed on the CPU from the GPU's own
# taps of its producers, so the tolerance is that of one layer, never of a chain.
TAP_IMAGE, TAP_CONV0, TAP_MAXPOOL, TAP_POOLED = 1, 2, 55, 56
PLAN_FOLDED, PLAN_128X128, PLAN_256X64, PLAN_256X128, PLAN_256X256, PLAN_STEM, PLAN_CONV3_EXPAND, PLAN_SLAB3_EXPAND = range(8)


def wiring():
    """{conv i (1 ... 52): (tap of its input, tap of its residual or None, relu)} and [(conv1 index, stage, stride)] per block."""
    wires, blocks = {}, []
    li, xin = 1, TAP_MAXPOOL
    for st, depth in enumerate(DEPTH):
        for b in range(depth):
            blocks.append((li, st, 2 if (b == 0 and st > 0) else 1))
            wires[li] = (xin, None, True)
            wires[li + 1] = (TAP_CONV0 + li, None, True)
            wires[li + 2] = (TAP_CONV0 + li + 1, TAP_CONV0 + li + 3 if b == 0 else xin, True)
            if b == 0:
                wires[li + 3] = (xin, None, False)
            xin = TAP_CONV0 + li + 2
            li += 4 if b == 0 else 3
    return wires, blocks


def conv_parameters(weights, biases):
    """[(w float32 [cout][k][k][cin], bias, stride)] per convolution, then (wfc [1000][2048], bfc)."""
    out, wo, bo = [], 0, 0
    for cin, cout, k, s in topology():
        out.append((weights[wo:wo + cout * k * k * cin].reshape(cout, k, k, cin), biases[bo:bo + cout], s))
        wo += cout * k * k * cin
        bo += cout
    return out, (weights[wo:wo + 1000 * 2048].reshape(1000, 2048), biases[bo:bo + 1000])


def stage_frames():
    """Two frames: every stage ends in a partial tile (6272 rows / 256, 1568 / 128, 392, 98)."""
    return np.concatenate([synth.make_clip(1, 360, 640, seed=5), synth.random_frames(1, 360, 640, seed=6)])


def stage_reference(point, tap, convs, mutate=None):
    """Reference of tap `point` (2 ... 55) from the taps of its producers: tap(p) -> float32 NHWC (p = 1: the 224 x 224 x 3 interior).
    mutate (negative controls): applied to the float32 sums before the residual, the ReLU and the rounding."""
    if point == TAP_MAXPOOL:
        x = torch.from_numpy(tap(TAP_CONV0)).permute(0, 3, 1, 2)
        return F.max_pool2d(x, 3, 2, 1).permute(0, 2, 3, 1).contiguous().numpy()
    i = point - TAP_CONV0
    w, b, stride = convs[i]
    src, res, relu = (TAP_IMAGE, None, True) if i == 0 else wiring()[0][i]
    y = conv_preactivation(tap(src), w, b, stride)
    if mutate is not None:
        y = mutate(y)
    return conv_finish(y, relu, None if res is None else tap(res))


class Taps:
    """The GPU's taps of one forward configuration: bf16 bits as fetched; [p] widens to float32 (the image tap: its interior)."""

    def __init__(self):
        self.bits, self.logits, self.plan = {}, None, None

    def __call__(self, p):
        a = self.bits[p]
        if p == TAP_POOLED:
            return a
        return _lib.bf16_bits_to_f32(a[:, 3:227, 3:227, :3] if p == TAP_IMAGE else a)


def run_tapped(ctx, frames, point):
    """One forward with the tap at `point` -> (tap, logits, plan); the option is back at 0 afterwards."""
    ctx.set_option("cnn_tap", point)
    try:
        logits, _ = ctx.cnn_forward(frames)
        return ctx.cnn_tap(frames.shape[0]), logits, ctx.cnn_plan()
    finally:
        ctx.set_option("cnn_tap", 0)


@pytest.fixture(scope="module")
def stage_params():
    weights, biases = seeded_parameters(0)
    return weights, biases, conv_parameters(weights, biases)


@pytest.fixture(scope="module")
def gpu_taps(ctx, stage_params):
    """57 short forwards layer by layer (cnn_fuse = 0, default tiling), one per tap point."""
    weights, biases, _ = stage_params
    ctx.cnn_set_weights(weights, biases)
    frames = stage_frames()
    fuse = ctx.get_option("cnn_fuse")
    t = Taps()
    try:
        ctx.set_option("cnn_fuse", 0)
        for p in range(1, 57):
            t.bits[p], logits, plan = run_tapped(ctx, frames, p)
            if t.logits is None:
                t.logits, t.plan = logits, plan
            assert np.array_equal(logits, t.logits) and np.array_equal(plan, t.plan)   # a tap changes nothing downstream
    finally:
        ctx.set_option("cnn_fuse", fuse)
    return t


def image_is_right(img_bits, frames):
    want = input_reference(frames).transpose(0, 2, 3, 1)                             # [n,224,224,3] RGB
    assert np.array_equal(_lib.bf16_bits_to_f32(img_bits[:, 3:227, 3:227, :3]), want)
    border = img_bits.copy()
    border[:, 3:227, 3:227, :3] = 0
    assert not border.any()                                                          # every border element, the fourth channel


@pytest.mark.gpu
def test_stage_input_image(ctx, gpu_taps, stage_params):
    frames = stage_frames()
    assert gpu_taps.bits[TAP_IMAGE].shape == (2, 232, 232, 4)
    image_is_right(gpu_taps.bits[TAP_IMAGE], frames)
    # another geometry and more frames in between: no stale pixel, an untouched border
    ctx.cnn_forward(synth.random_frames(5, 96, 128, seed=21))
    again, _, _ = run_tapped(ctx, frames, TAP_IMAGE)
    image_is_right(again, frames)


def report(name, got, want):
    worst, same = layer_figures(got, want)
    print(f"[cnn-stages] {name}: worst err/tol {worst:.3f}, identical {same:.5f}")
    assert got.shape == want.shape
    assert worst <= 1.0, name
    assert same > 0.98, name


@pytest.mark.gpu
def test_stage_stem(gpu_taps, stage_params):
    assert gpu_taps.plan[0] == PLAN_STEM
    report("conv 0 (stem)", gpu_taps(TAP_CONV0), stage_reference(TAP_CONV0, gpu_taps, stage_params[2][0]))


@pytest.mark.gpu
def test_stage_max_pool(gpu_taps, stage_params):
    """A maximum of bf16 values has no rounding: equal."""
    assert np.array_equal(gpu_taps(TAP_MAXPOOL), stage_reference(TAP_MAXPOOL, gpu_taps, stage_params[2][0]))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(1, 53))
def test_stage_convolution(gpu_taps, stage_params, i):
    """Convolution i of the forward, from the GPU's taps of its input and its residual: the real geometry, the buffer rotation, its weight
    and bias offsets."""
    assert gpu_taps.plan[i] in (PLAN_128X128, PLAN_256X64, PLAN_256X128, PLAN_256X256)
    cin, cout, k, s = topology()[i]
    report(f"conv {i} ({cin} -> {cout}, {k}x{k}/{s})", gpu_taps(TAP_CONV0 + i), stage_reference(TAP_CONV0 + i, gpu_taps, stage_params[2][0]))


@pytest.mark.gpu
def test_stage_pooled_features(gpu_taps):
    """k_avgpool: a sequential float32 sum of 49 non-negative terms, then one multiply by 1.f / 49 -- 50 roundings, and the reciprocal's."""
    x = gpu_taps(TAP_CONV0 + 52).astype(np.float64)
    assert x.shape == (2, 7, 7, 2048) and x.min() >= 0
    want = x.reshape(2, 49, 2048).mean(axis=1)
    got = gpu_taps(TAP_POOLED)
    assert got.shape == want.shape and got.dtype == np.float32
    err = np.abs(got - want)
    print(f"[cnn-stages] pooled features: worst err/tol {float((err / np.maximum(64 * 2.0 ** -24 * want, 1e-300)).max()):.3f}")
    assert np.all(err <= 64 * 2.0 ** -24 * want)


@pytest.mark.gpu
def test_stage_logits(gpu_taps, stage_params):
    """k_linear: 32 FMAs per lane, six shuffle adds and the bias."""
    wfc, bfc = stage_params[2][1]
    wq = _lib.bf16_bits_to_f32(_lib.f32_to_bf16_bits(wfc)).astype(np.float64)
    pooled = gpu_taps(TAP_POOLED).astype(np.float64)
    want = pooled @ wq.T + bfc
    bound = 64 * 2.0 ** -24 * (np.abs(pooled) @ np.abs(wq).T + np.abs(bfc))
    err = np.abs(gpu_taps.logits - want)
    print(f"[cnn-stages] logits: worst err/tol {float((err / bound).max()):.3f}")
    assert gpu_taps.logits.shape == (2, 1000) and np.all(err <= bound)


# ---- negative controls (CPU only): the stage criterion must reject each restated kernel bug ------------------------------
@pytest.fixture(scope="module")
def cpu_taps(stage_params):
    """The float32 reference network on the stage frames, every tap kept (the controls need a stage's true inputs)."""
    convs = stage_params[2][0]
    taps = {TAP_IMAGE: np.ascontiguousarray(input_reference(stage_frames()).transpose(0, 2, 3, 1))}
    get = taps.__getitem__
    taps[TAP_CONV0] = stage_reference(TAP_CONV0, get, convs)
    taps[TAP_MAXPOOL] = stage_reference(TAP_MAXPOOL, get, convs)
    for li, st, s in wiring()[1]:
        first = wiring()[0][li + 2][1] == TAP_CONV0 + li + 3                        # a stage's first block: the shortcut before conv3
        for i in ([li, li + 3, li + 1, li + 2] if first else [li, li + 1, li + 2]):
            taps[TAP_CONV0 + i] = stage_reference(TAP_CONV0 + i, get, convs)
    return taps


def wrapped_right_border(x_nhwc, w):
    """Mutation of a 3x3 / 1: at the right border the dx = 2 tap reads the NEXT ROW'S FIRST pixel (the next linear pixel index) instead of the
    zero page -- what a gather that checks only the row would do."""
    x0 = bf16(torch.from_numpy(np.ascontiguousarray(x_nhwc[:, :, 0, :])))             # [n][H][c]: the first pixel of every row
    wq = bf16(torch.from_numpy(np.ascontiguousarray(w)))
    H = x_nhwc.shape[1]

    def mutate(y):
        y = y.clone()
        for dy in range(3):                                                           # tap row oy - 1 + dy inside the image, and so the row after it
            oy = [o for o in range(H) if 0 <= o - 1 + dy and o + dy < H]
            y[:, :, oy, -1] += torch.einsum("nhc,oc->noh", x0[:, [o + dy for o in oy], :], wq[:, dy, 2, :])
        return y
    return mutate


def block_conv(block, which):
    """Index of convolution `which` (0 conv1, 1 the 3x3, 2 the expanding 1x1) of block `block` (0 ... 15)."""
    return wiring()[1][block][0] + which


def test_control_stem_ignores_kernel_column_6(cpu_taps, stage_params):
    w, b, s = stage_params[2][0][0]
    wm = w.copy()
    wm[:, :, 6, :] = 0
    wrong = conv_reference(cpu_taps[TAP_IMAGE], wm, b, s, True)
    assert not layer_ok(wrong, cpu_taps[TAP_CONV0])


def test_control_stem_pads_by_replication(cpu_taps, stage_params):
    w, b, s = stage_params[2][0][0]
    x = np.pad(cpu_taps[TAP_IMAGE], ((0, 0), (3, 3), (3, 3), (0, 0)), mode="edge")
    wrong = conv_finish(conv_preactivation(x, w, b, s, padding=0), True)
    assert wrong.shape == cpu_taps[TAP_CONV0].shape and not layer_ok(wrong, cpu_taps[TAP_CONV0])


def test_control_wrapped_right_border_tap_in_block_6(cpu_taps, stage_params):
    convs = stage_params[2][0]
    i = block_conv(6, 1)
    assert topology()[i] == (128, 128, 3, 1)
    x = cpu_taps[wiring()[0][i][0]]
    wrong = stage_reference(TAP_CONV0 + i, cpu_taps.__getitem__, convs, mutate=wrapped_right_border(x, convs[i][0]))
    assert not layer_ok(wrong, cpu_taps[TAP_CONV0 + i])
    # ... and the mutation is the border's alone
    assert np.array_equal(wrong[:, :, :-1], cpu_taps[TAP_CONV0 + i][:, :, :-1])


def test_control_tail_tile_of_block_12_not_stored(cpu_taps):
    right = cpu_taps[TAP_CONV0 + block_conv(12, 2)]
    assert right.shape == (2, 14, 14, 1024)
    wrong = right.copy()
    wrong[-1].reshape(-1, 1024)[-3:] = 0                                              # the last three pixels of the last frame
    assert not layer_ok(wrong, right)


def test_control_one_bias_channel_dropped_in_conv_52(cpu_taps, stage_params):
    convs = stage_params[2][0]
    w, b, s = convs[52]
    ch = int(np.argsort(np.abs(b))[b.size // 2])                                       # a channel with the median |bias|: neither the easiest nor a bias of ~ 0

    def mutate(y):
        y = y.clone()
        y[:, ch] -= float(b[ch])
        return y
    wrong = stage_reference(TAP_CONV0 + 52, cpu_taps.__getitem__, convs, mutate=mutate)
    right = cpu_taps[TAP_CONV0 + 52]
    assert not layer_ok(wrong, right)
    others = np.arange(b.size) != ch
    assert np.array_equal(wrong[..., others], right[..., others])


def test_controls_pass_unmutated(cpu_taps, stage_params):
    """The criterion accepts the reference itself and a different float32 accumulation order of it (float64 sums): the controls above are
    rejected for their mutation, not for the way the criterion is applied."""
    convs = stage_params[2][0]
    for i in (0, block_conv(6, 1), 52):
        w, b, s = convs[i]
        src, res, relu = (TAP_IMAGE, None, True) if i == 0 else wiring()[0][i]
        x = torch.from_numpy(cpu_taps[src]).permute(0, 3, 1, 2).double()
        wq = bf16(torch.from_numpy(np.ascontiguousarray(w))).permute(0, 3, 1, 2).double()
        y = F.conv2d(x, wq, torch.from_numpy(b).double(), stride=s, padding=w.shape[1] // 2)
        if res is not None:
            y = y + torch.from_numpy(cpu_taps[res]).permute(0, 3, 1, 2).double()
        y64 = bf16((torch.relu(y) if relu else y).float()).permute(0, 2, 3, 1).contiguous().numpy()
        assert layer_ok(y64, cpu_taps[TAP_CONV0 + i]), i


# ---- fused kernels and tilings inside the forward: bit comparisons with the layer-by-layer taps ---------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fuse", [1, 2])
def test_fused_blocks_tap_by_tap(ctx, gpu_taps, fuse):
    """Every block output of the two fused stages, and the two convolutions that read the last of them from the rotated buffer, hold the bits
    of the layer-by-layer forward; cnn_plan proves which kernel ran."""
    frames = stage_frames()
    blocks = wiring()[1]
    fused = [(li, s) for li, st, s in blocks if st < 2]
    assert len(fused) == 7
    nxt = blocks[7][0]
    points = [TAP_CONV0 + li + 2 for li, s in fused] + [TAP_CONV0 + nxt, TAP_CONV0 + nxt + 3]
    default = ctx.get_option("cnn_fuse")
    try:
        ctx.set_option("cnn_fuse", fuse)
        for p in points:
            tap, logits, plan = run_tapped(ctx, frames, p)
            assert np.array_equal(tap, gpu_taps.bits[p]), p
            assert np.array_equal(logits, gpu_taps.logits)
        for li, s in fused:
            assert plan[li + 1] == (PLAN_SLAB3_EXPAND if fuse == 2 and s == 1 else PLAN_CONV3_EXPAND), li
            assert plan[li + 2] == PLAN_FOLDED, li
        unfused = [i for i in range(53) if not any(i in (li + 1, li + 2) for li, s in fused)]
        assert np.array_equal(plan[unfused], gpu_taps.plan[unfused])
        # the 3x3 of a fused block has no output of its own: an error, not the bytes of an earlier tap
        ctx.set_option("cnn_tap", TAP_CONV0 + fused[0][0] + 1)
        ctx.cnn_forward(frames)
        with pytest.raises(_lib.AvdError, match="cnn_tap"):
            ctx.cnn_tap(2)
    finally:
        ctx.set_option("cnn_tap", 0)
        ctx.set_option("cnn_fuse", default)


@pytest.mark.gpu
@pytest.mark.parametrize("policy", [1, 2])
def test_tilings_through_the_whole_forward(ctx, gpu_taps, policy):
    """All 53 real geometries under the 256-pixel bodies (policy 1) and the 128 x 128 body (policy 2): logits and three taps hold the bits of the
    default tiling, and cnn_plan proves that the bodies ran."""
    frames = stage_frames()
    convs = topology()
    fuse = ctx.get_option("cnn_fuse")
    try:
        ctx.set_option("cnn_fuse", 0)
        ctx.set_option("cnn_tiles", policy)
        for p in (54, 46, 24):
            tap, logits, plan = run_tapped(ctx, frames, p)
            assert np.array_equal(tap, gpu_taps.bits[p]), p
            assert np.array_equal(logits, gpu_taps.logits)
    finally:
        ctx.set_option("cnn_tiles", 0)
        ctx.set_option("cnn_fuse", fuse)
    assert plan[0] == PLAN_STEM
    for i in range(1, 53):
        cout = convs[i][1]
        if cout % 128:
            assert cout == 64 and plan[i] == PLAN_256X64, i
        elif policy == 1:
            assert plan[i] == (PLAN_256X256 if cout % 256 == 0 else PLAN_256X128), i
        else:
            assert plan[i] == PLAN_128X128, i
    seen = set(plan.tolist())
    assert seen == ({PLAN_STEM, PLAN_256X64, PLAN_256X128, PLAN_256X256} if policy == 1 else {PLAN_STEM, PLAN_256X64, PLAN_128X128})


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_activation_scratch_holds_the_padded_tail_tile(stage_params, n):
    """Regression: every tile stores all 256 (128) of its rows, so an activation's rows are padded to whole tiles.  The scratch buffers were
    sized by the stem's output (n x 12544 rows x 64, always whole tiles), but the 56 x 56 x 256 activations pad further unless n % 4 == 0: their
    tail tile wrote up to 96 KiB past the end of its buffer.  The forward now refuses an activation that does not fit, and a tap copies the
    padded activation whole: on a fresh context (exactly n frames of scratch) the 56 x 56 x 256 outputs are there and right."""
    weights, biases, (convs, _) = stage_params
    frames = stage_frames()[[0, 1, 0][:n]]
    with _lib.Context(0) as c:
        c.cnn_set_weights(weights, biases)
        c.set_option("cnn_fuse", 0)
        taps = Taps()
        for p in (TAP_MAXPOOL, TAP_CONV0 + 1, TAP_CONV0 + 2, TAP_CONV0 + 3, TAP_CONV0 + 4):
            taps.bits[p], _, _ = run_tapped(c, frames, p)
        for p in (TAP_CONV0 + 3, TAP_CONV0 + 4):                                       # conv3 and the shortcut of the first block
            assert taps.bits[p].shape == (n, 56, 56, 256)
            assert layer_ok(taps(p), stage_reference(p, taps, convs)), p


@pytest.mark.gpu
def test_tap_and_plan_refusals(stage_params):
    """cnn_tap / cnn_plan on a fresh context: errors before any forward; a tapped forward refuses more than one pass and timing repetitions;
    an untapped forward, a wrong size and a released workspace leave nothing to fetch."""
    weights, biases, _ = stage_params
    frames = synth.random_frames(3, 96, 128, seed=9)
    with _lib.Context(0) as c:
        c.cnn_set_weights(weights, biases)
        with pytest.raises(_lib.AvdError, match="cnn_plan"):
            c.cnn_plan()
        with pytest.raises(_lib.AvdError, match="cnn_tap"):
            c.debug_fetch("cnn_tap", (3, 2048), np.float32)
        c.set_option("cnn_tap", TAP_POOLED)
        with pytest.raises(_lib.AvdError, match="cnn_tap"):
            c.cnn_forward(frames, timing_reps=1)
        c.set_option("cnn_chunk", 2)
        with pytest.raises(_lib.AvdError, match="cnn_tap"):
            c.cnn_forward(frames)
        c.set_option("cnn_chunk", 128)
        logits, _ = c.cnn_forward(frames)
        pooled = c.cnn_tap(3)
        assert pooled.shape == (3, 2048) and np.isfinite(pooled).all() and pooled.max() > 0
        with pytest.raises(_lib.AvdError, match="cnn_tap"):
            c.debug_fetch("cnn_tap", (2, 2048), np.float32)                            # not the tap's size
        c.release_workspace()
        with pytest.raises(_lib.AvdError, match="cnn_tap"):
            c.cnn_tap(3)
        c.cnn_forward(frames)
        assert np.array_equal(c.cnn_tap(3), pooled)
        c.set_option("cnn_tap", 0)
        plain, _ = c.cnn_forward(frames)
        assert np.array_equal(plain, logits)
        with pytest.raises(_lib.AvdError, match="cnn_tap"):                            # the LAST forward was not tapped
            c.debug_fetch("cnn_tap", (3, 2048), np.float32)
        assert c.cnn_plan()[0] == PLAN_STEM
