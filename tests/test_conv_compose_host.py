"""Host: emph_conv_compose_pack - two Conv1d(80, 80, 3, 'same') layers with no
activation between them as one 5-tap layer, its F(4,5) pack and edge terms."""
import numpy as np

from emphases_amd import runtime

# F(4,5) on the points 0, +-1, +-2, +-1/2, inf: y = A^T [(G g) . (B^T d)]
BT = np.array([
    [1, 0, -21 / 4, 0, 21 / 4, 0, -1, 0],
    [0, 1, 1, -17 / 4, -17 / 4, 1, 1, 0],
    [0, -1, 1, 17 / 4, -17 / 4, -1, 1, 0],
    [0, 1 / 2, 1 / 4, -5 / 2, -5 / 4, 2, 1, 0],
    [0, -1 / 2, 1 / 4, 5 / 2, -5 / 4, -2, 1, 0],
    [0, 2, 4, -5 / 2, -5, 1 / 2, 1, 0],
    [0, -2, 4, 5 / 2, -5, -1 / 2, 1, 0],
    [0, -1, 0, 21 / 4, 0, -21 / 4, 0, 1]])
AT = np.array([
    [1, 1, 1, 1, 1, 1, 1, 0],
    [0, 1, -1, 2, -2, 1 / 2, -1 / 2, 0],
    [0, 1, 1, 4, 4, 1 / 4, 1 / 4, 0],
    [0, 1, -1, 8, -8, 1 / 8, -1 / 8, 1]])
PACK, BIAS, EDGE = 20 * 8 * 5 * 64, 80, 80 * 80 + 80


def unpack(pack):
    """U[j][c_out][c_in] (float64) of the k-major pack: per k-step 8 points x
    5 m-tiles x 64 lanes, lane -> (c_out = 16 m + (lane & 15), c_in = 4 step +
    (lane >> 4))."""
    blocks = pack[:PACK].astype(np.float64).reshape(20, 8, 5, 4, 16)
    return blocks.transpose(1, 2, 4, 0, 3).reshape(8, 80, 80)


def winograd(pack, x):
    """The pack applied to x float64 [80, 4 quads + 4] -> [80, 4 quads]."""
    matrices = unpack(pack)
    out = np.zeros((80, x.shape[1] - 4))
    for quad in range(out.shape[1] // 4):
        v = BT @ x[:, 4 * quad:4 * quad + 8].T              # [8, c_in]
        products = np.einsum('joc,jc->jo', matrices, v)
        out[:, 4 * quad:4 * quad + 4] = (AT @ products).T
    return out


def direct(weight, x):
    """Correlation with float64 taps [80, 80, k], no padding."""
    taps = weight.shape[2]
    return np.stack([
        np.einsum('ock,ck->o', weight, x[:, t:t + taps])
        for t in range(x.shape[1] - taps + 1)], axis=1)


def grid_weights(seed, scale):
    """Weights on a grid where the filter transform G (denominators 9, 45, 90)
    is exact in float32: multiples of 90 / 64 with small integer factors, so
    the packer's one rounding changes nothing and the comparison below is
    about its algebra and layout alone."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-8, 9, size=(80, 80, 3)) * (90. / 64.) * scale
            ).astype(np.float32)


def test_identity_second_layer_reproduces_the_first():
    """W1 = delta at the centre tap, b1 = 0: the composed layer is W0 itself
    (taps 1 .. 3 of 5).  Its F(4,5) pack, applied in float64, matches the
    direct correlation to 1e-12; the bias is b0; the edge terms vanish."""
    w0 = grid_weights(1, 1.)
    b0 = np.random.default_rng(2).integers(-8, 9, size=80).astype(np.float32)
    w1 = np.zeros((80, 80, 3), dtype=np.float32)
    w1[np.arange(80), np.arange(80), 1] = 1.
    pack = runtime.conv_compose_pack(w0, b0, w1, np.zeros(80, np.float32))
    assert pack.dtype == np.float32 and pack.size == PACK + BIAS + 2 * EDGE
    x = np.random.default_rng(3).standard_normal((80, 20))
    got = winograd(pack, x)                        # output t reads x[t .. t + 4]
    want = direct(w0.astype(np.float64), x[:, 1:-1])
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(pack[PACK:PACK + BIAS], b0)
    assert not pack[PACK + BIAS:].any()


def test_composed_taps_bias_and_edge_terms():
    """General W1: the pack is the 5-tap correlation Wc[d] = sum W1[a] W0[c]
    over a + c = d (1e-12 on the exact grid), bc = b1 + (sum_a W1[a]) b0, and
    the edge terms make the composed layer equal to conv -> conv with the
    intermediate zero-padded, at both ends and for a segment of one
    position."""
    w0, w1 = grid_weights(4, 1.), grid_weights(5, 1. / 64.)
    rng = np.random.default_rng(6)
    b0 = rng.integers(-8, 9, size=80).astype(np.float32)
    b1 = rng.integers(-8, 9, size=80).astype(np.float32)
    pack = runtime.conv_compose_pack(w0, b0, w1, b1)
    w0d, w1d = w0.astype(np.float64), w1.astype(np.float64)
    taps = np.zeros((80, 80, 5))
    for a in range(3):
        for c in range(3):
            taps[:, :, a + c] += w1d[:, :, a] @ w0d[:, :, c]
    x = rng.standard_normal((80, 16))
    got = winograd(pack, x)
    want = direct(taps, x)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    bias = pack[PACK:PACK + BIAS].astype(np.float64)
    assert np.abs(bias - (b1 + w1d.sum(2) @ b0)).max() <= 1e-6 * np.abs(bias).max()

    def same(weight, bias, value):
        padded = np.pad(value, ((0, 0), (1, 1)))
        return direct(weight, padded) + bias[:, None]

    edges = [pack[PACK + BIAS + side * EDGE:][:EDGE].astype(np.float64)
             for side in range(2)]
    for n in (1, 2, 7):
        value = rng.standard_normal((80, n))
        want = same(w1d, b1, same(w0d, b0, value))
        composed = direct(taps, np.pad(value, ((0, 0), (2, 2)))) + bias[:, None]
        for side, column in ((0, 0), (1, n - 1)):
            matrix = edges[side][:6400].reshape(80, 80)         # [c_in][c_out]
            composed[:, column] -= edges[side][6400:] + value[:, column] @ matrix
        assert np.abs(composed - want).max() <= 1e-5 * np.abs(want).max(), n
