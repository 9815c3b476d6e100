"""The f64 checker of sample-rate conversion (am_resample*, include/audiomatch.h): the filter and the output formula of
the header, in numpy, for the resampling tests."""
from math import gcd

import numpy as np

MAX_RATE, MAX_R = 768000, 8192


def ratio(src_rate: int, dst_rate: int):
    """(L, M, H): up factor, down factor, filter half length."""
    g = gcd(src_rate, dst_rate)
    L, M = dst_rate // g, src_rate // g
    return L, M, 10 * max(L, M)


def out_len(n_in: int, src_rate: int, dst_rate: int) -> int:
    L, M, _ = ratio(src_rate, dst_rate)
    return -(-n_in * L // M)


def taps(src_rate: int, dst_rate: int) -> np.ndarray:
    """h[j + H], j = -H .. H, in f64: L * w / sum(w), w = c sinc(c j) I0(5 sqrt(1 - (j/H)^2)) / I0(5), c = 1/R."""
    L, M, H = ratio(src_rate, dst_rate)
    c = 1.0 / max(L, M)
    j = np.arange(-H, H + 1, dtype=np.float64)
    w = c * np.sinc(c * j) * np.i0(5.0 * np.sqrt(1.0 - (j / H) ** 2)) / np.i0(5.0)
    return L * w / w.sum()


def resample(x, src_rate: int, dst_rate: int, k0: int = 0, k1=None, h=None, n0: int = 0, n_in=None) -> np.ndarray:
    """y[k] = sum over n in [0, n_in) with |k M - n L| <= H of x[n] h[k M - n L], for k in [k0, k1), in f64.
    Non-finite samples reach exactly the outputs whose support holds them.  x may be a window of a longer signal:
    samples n0 .. n0 + len(x) of n_in (it must hold every sample the outputs read)."""
    x = np.asarray(x, dtype=np.float64)
    L, M, H = ratio(src_rate, dst_rate)
    if n_in is None:
        n_in = n0 + x.size
    if k1 is None:
        k1 = out_len(n_in, src_rate, dst_rate)
    if h is None:
        h = taps(src_rate, dst_rate)
    k = np.arange(k0, k1, dtype=np.int64)
    a = k * M + H                       # h index of sample n: a - n L, in [0, 2H] on the support
    nh, p = a // L, a % L
    y = np.zeros(k.size, dtype=np.float64)
    if n_in == 0:
        return y
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(2 * H // L + 1):
            n = nh - t
            idx = p + t * L
            ok = (idx <= 2 * H) & (n >= 0) & (n < n_in)
            if not ok.any():
                continue
            assert (n[ok] >= n0).all() and (n[ok] < n0 + x.size).all(), "the window does not hold every sample read"
            y += np.where(ok, h[np.minimum(idx, 2 * H)] * x[np.clip(n - n0, 0, x.size - 1)], 0.0)
    return y


def downmix(interleaved) -> np.ndarray:
    """(l + r) * 0.5 * (1/65535) in f32, bit for bit as the library's down-mix."""
    a = np.asarray(interleaved, dtype=np.int16).reshape(-1, 2)
    s = a[:, 0].astype(np.float32) + a[:, 1].astype(np.float32)
    return (s * np.float32(0.5)) * np.float32(1.0 / 65535.0)
