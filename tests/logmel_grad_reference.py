"""The backward of the log-mel front-end, restated in numpy float64: the
specification `emph_logmel_backward` (csrc/frontend_grad.hip) is held to, with
every intermediate, so that a device result that misses its bound can be
traced to the stage that lost the bits.  A plain module (no fixtures, CPU
only): imported by tests/test_logmel_autograd.py, which checks it against
torch autograd of `oracle.prominence.logmel`, and by the GPU tests.

One chunk x[0..S), S > 432, F = 1 + (S - 160) // 160 frames:

    p        reflect-padded signal [S + 864]
    X_k      sum_n w_n p[160 f + n] e^{-2 pi i k n / 1024}, k = 0..512
             (re_k = sum w p cos, im_k = -sum w p sin)
    s_k      sqrt(re_k^2 + im_k^2 + 1e-6)
    m_r      sum_k B[r, k] s_k
    y_r      log(max(m_r, 1e-5))

and, for a cotangent g = dL/dy [80, F]:

    q_r      g_r / m_r where m_r >= 1e-5, else 0
    G_k      sum_r B[r, k] q_r
    dre_k    G_k re_k / s_k          dim_k = G_k im_k / s_k
    t_n      w_n sum_{k=0}^{512} (dre_k cos(2 pi k n / 1024)
                                  - dim_k sin(2 pi k n / 1024))
    P[j]     sum_f t^(f)[j - 160 f]                       (overlap-add)
    dx[n]    P[n + 432] + P[432 - n] (1 <= n <= 432)
             + P[2 (S - 1) - n + 432] (S - 433 <= n <= S - 2)

`dim_k` is the cotangent of the imaginary part as the forward defines it (with
its minus sign), so d im_k / d p_n = -w_n sin and the sine term of `t` carries
a minus: t is w times the real part of sum_k (dre_k + i dim_k) e^{+2 pi i k n /
1024}, an unnormalised inverse transform in which each of the 513 one-sided
bins counts once (no factor 2 on bins 1..511, no 1/N).
"""
import numpy as np

from oracle import prominence as oracle

FFT, HOP, PAD, BINS, MELS = 1024, 160, 432, 513, 80


def window():
    """The periodic Hann as the front-end's table holds it (float32 values)."""
    return oracle.hann_window().double().numpy()


def basis():
    return oracle.mel_basis().double().numpy()


def _trig():
    phase = (np.arange(BINS)[:, None] * np.arange(FFT)[None, :]) % FFT
    angle = 2. * np.pi * phase / FFT
    return np.cos(angle), np.sin(angle)          # [513, 1024]


def frames_of(samples):
    return 1 + (samples - HOP) // HOP


def reflect_index(samples):
    """Index into x of every padded position: int [S + 864]."""
    j = np.arange(samples + 2 * PAD) - PAD
    j = np.abs(j)
    return np.where(j >= samples, 2 * (samples - 1) - j, j)


def forward(x, mel_basis=None):
    """dict of the forward's intermediates of one chunk x float64 [S]."""
    x = np.asarray(x, dtype=np.float64)
    samples = x.shape[0]
    assert samples > PAD
    count = frames_of(samples)
    p = x[reflect_index(samples)]
    w = window()
    rows = np.stack([p[HOP * f:HOP * f + FFT] for f in range(count)]) * w
    cos, sin = _trig()
    re = rows @ cos.T                            # [F, 513]
    im = -(rows @ sin.T)
    s = np.sqrt(re * re + im * im + 1e-6)
    b = basis() if mel_basis is None else np.asarray(mel_basis, np.float64)
    m = s @ b.T                                  # [F, 80]
    y = np.log(np.maximum(m, 1e-5))
    return dict(p=p, re=re, im=im, s=s, m=m, y=y.T, basis=b, window=w)


def backward(x, g, mel_basis=None):
    """The gradient of sum(g * logmel(x)) with respect to x float64 [S], g
    [80, F]: dict with `q` [80, F], `G` [513, F], `t` [F, 1024], `P`
    [S + 864], `dx` [S] and the forward's `m` [80, F]."""
    state = forward(x, mel_basis)
    samples = len(x)
    g = np.asarray(g, dtype=np.float64)
    m = state['m'].T                             # [80, F]
    count = m.shape[1]
    assert g.shape == m.shape
    passes = m >= 1e-5
    q = np.where(passes, g / np.where(passes, m, 1.), 0.)
    big = state['basis'].T @ q                   # [513, F]
    dre = big.T * state['re'] / state['s']       # [F, 513]
    dim = big.T * state['im'] / state['s']
    cos, sin = _trig()
    t = state['window'] * (dre @ cos - dim @ sin)
    padded = np.zeros(samples + 2 * PAD)
    for f in range(count):
        padded[HOP * f:HOP * f + FFT] += t[f]
    dx = padded[PAD:PAD + samples].copy()
    n = np.arange(1, min(PAD, samples - 1) + 1)
    dx[n] += padded[PAD - n]
    n = np.arange(max(samples - PAD - 1, 0), samples - 1)
    dx[n] += padded[2 * (samples - 1) - n + PAD]
    return dict(q=q, G=big, t=t, P=padded, dx=dx, m=m, y=state['y'])
