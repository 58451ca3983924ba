"""LayerNorm / softmax (csrc/avd_norm.hip), host side: the float64 references tests/test_norm.py compares the kernels with, and a
float32 restatement of both formulas in the kernels' own order -- a lane's running sum over its pieces, then the butterfly over 64
lanes -- checked against those references on the CPU.  It shows the project's tolerances (LayerNorm 2e-6 * max(1, |want|max) absolute,
softmax rtol 2e-6 / atol 1e-9 and row sums within 1e-6 of 1) reachable by float32 arithmetic in that order before a GPU sees them;
the restatement is no bit-level model of the kernels (numpy's exp and division are not the device's)."""
import numpy as np
import pytest

f32 = np.float32


def layernorm_f64(x, g, b, eps=1e-5):
    """float64 LayerNorm of the given (float32 or bf16-rounded) values: biased variance about the mean."""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    return (x - mean) / np.sqrt(var + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def softmax_f64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def layernorm_inputs(rows, cols, seed):
    """The input family of test_layernorm_f32_against_torch: normal * 3 + a row offset * 5."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, cols)) * 3 + rng.standard_normal((rows, 1)) * 5).astype(np.float32)
    return x, rng.standard_normal(cols).astype(np.float32), rng.standard_normal(cols).astype(np.float32)


def softmax_inputs(rows, cols, seed):
    """The input family of test_softmax_against_torch (normal * 6, the 80 / -90 / 79.5 head in row 0), plus, where there are rows for
    them, a row of equal logits (row 1) and a row whose maximum sits in the last four columns (row 2)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, cols)) * 6).astype(np.float32)
    x[0, :min(3, cols)] = [80.0, -90.0, 79.5][:cols]
    if rows > 1:
        x[1] = 3.25
    if rows > 2:
        x[2, cols - 2] = 50.0
    return x


# ---- the kernels' order of operations, in float32 numpy ---------------------------------------------------------------------
def _lanes(x, cols, vec, fill):
    """[rows, cols] -> [rows, slots, 64]: the value lane l holds in slot s.  vec: slot 4 i + j is element 4 (64 i + l) + j (the
    register-resident kernels); else slot s is element 64 s + l (the general ones).  Slots past the row end hold `fill`."""
    if vec:
        p = (cols // 4 + 63) // 64
        k = (np.arange(p)[:, None, None] * 64 + np.arange(64)[None, None, :]) * 4 + np.arange(4)[None, :, None]   # [p, 4, 64]
        k = k.reshape(p * 4, 64)
    else:
        k = np.arange((cols + 63) // 64)[:, None] * 64 + np.arange(64)[None, :]
    out = np.full((x.shape[0],) + k.shape, fill, np.float32)
    ok = k < cols
    out[:, ok] = x[:, k[ok]]
    return out, ok


def _butterfly(v, op):
    """__shfl_xor over 64 lanes, offsets 32 .. 1: every lane ends with the same value."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[:, lane ^ o])
    return v[:, :1]


def _lane_sum(v, vec):
    s = np.zeros((v.shape[0], 64), np.float32)
    if vec:
        for i in range(0, v.shape[1], 4):
            s = s + ((v[:, i] + v[:, i + 1]) + (v[:, i + 2] + v[:, i + 3]))
    else:
        for i in range(v.shape[1]):
            s = s + v[:, i]
    return s


def layernorm_f32_lanes(x, g, b, eps=1e-5):
    rows, cols = x.shape
    vec = cols in (256, 512, 768, 1024, 2048)
    v, ok = _lanes(x, cols, vec, 0.0)
    total = _butterfly(_lane_sum(v, vec), np.add)
    mean = total * (f32(1) / f32(cols)) if vec else total / f32(cols)
    d = (v - mean[:, :, None]) * ok                                   # the padding slots of the general kernel add nothing
    q = np.zeros((rows, 64), np.float32)
    for i in range(v.shape[1]):
        q = q + d[:, i] * d[:, i]
    qs = _butterfly(q, np.add)
    var = qs * (f32(1) / f32(cols)) if vec else qs / f32(cols)
    rstd = f32(1) / np.sqrt(var + f32(eps))
    y = (x - mean) * rstd * g + b
    assert y.dtype == np.float32 and mean.dtype == np.float32 and rstd.dtype == np.float32
    return y


def softmax_f32_lanes(x):
    rows, cols = x.shape
    vec = cols % 4 == 0 and cols <= 4096
    v, _ = _lanes(x, cols, vec, -np.inf)
    m = _butterfly(v.max(axis=1), np.maximum)
    s = np.zeros((rows, 64), np.float32)
    for i in range(v.shape[1]):
        s = s + np.exp(v[:, i] - m)                                   # exp(-inf) = 0 for the padding
    inv = f32(1) / _butterfly(s, np.add)
    y = np.exp(x - m) * inv
    assert y.dtype == np.float32
    return y


@pytest.mark.parametrize("rows,cols", [(3, 512), (2, 2048), (2, 5000), (3, 33), (5, 256), (5, 1024), (6, 768)])
def test_float32_layernorm_in_lane_order_meets_the_tolerance(rows, cols):
    x, g, b = layernorm_inputs(rows, cols, rows + cols)
    want = layernorm_f64(x, g, b)
    got = layernorm_f32_lanes(x, g, b)
    tol = 2e-6 * max(1.0, float(np.abs(want).max()))
    worst = float(np.abs(got - want).max())
    print(f"layernorm {rows} x {cols}: float32 in lane order is {worst / tol:.3f} of the tolerance")
    assert worst <= tol
    # the restatement is a LayerNorm at all: float32 numpy in its own order agrees as well
    plain = ((x - x.mean(axis=1, keepdims=True)) / np.sqrt(x.var(axis=1, keepdims=True) + f32(1e-5)) * g + b).astype(np.float32)
    assert np.abs(plain - want).max() <= tol


@pytest.mark.parametrize("cols", [4, 1000, 1024, 1028, 1500, 2048, 2052, 4092, 4096, 4100, 33])
def test_float32_softmax_in_lane_order_meets_the_tolerance(cols):
    x = softmax_inputs(6, cols, cols)
    want = softmax_f64(x)
    got = softmax_f32_lanes(x)
    ratio = float((np.abs(got - want) / (1e-9 + 2e-6 * np.abs(want))).max())
    print(f"softmax 6 x {cols}: float32 in lane order is {ratio:.3f} of the tolerance, row sums off by {np.abs(got.sum(axis=1, dtype=np.float64) - 1).max():.2e}")
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-9)
    np.testing.assert_allclose(got.sum(axis=1), 1.0, atol=1e-6)
    np.testing.assert_allclose(got[1], 1.0 / cols, rtol=2e-6, atol=1e-9)          # equal logits
    assert got[2].argmax() == cols - 2 and want[0].argmax() == 0


def test_lane_maps_cover_every_element_once():
    for cols, vec in [(512, True), (2048, True), (1028, True), (4092, True), (33, False), (5000, False)]:
        x = np.arange(cols, dtype=np.float32)[None, :]
        v, ok = _lanes(x, cols, vec, -1.0)
        assert ok.sum() == cols and np.array_equal(np.sort(v[0][ok]), x[0]) and np.all(v[0][~ok] == -1.0)


def test_references_are_layernorm_and_softmax():
    """The float64 references against torch's float32 functions (the reference the earlier cases use): they state the same operation."""
    torch = pytest.importorskip("torch")
    x, g, b = layernorm_inputs(4, 512, 1)
    t = torch.nn.functional.layer_norm(torch.from_numpy(x), (512,), torch.from_numpy(g), torch.from_numpy(b), 1e-5).numpy()
    np.testing.assert_allclose(t, layernorm_f64(x, g, b), rtol=0, atol=2e-6 * 10)
    s = softmax_inputs(4, 1028, 2)
    np.testing.assert_allclose(torch.softmax(torch.from_numpy(s), dim=1).numpy(), softmax_f64(s), rtol=1e-5, atol=1e-9)
