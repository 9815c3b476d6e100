"""The f64 checker of spectral whitening (am_lag_products*, am_whiten_taps, am_fir*; include/audiomatch.h): the lag
products by math.fsum over the exact products, the Levinson-Durbin recursion as the header states it and the FIR
filter in f64, for the whitening tests."""
import math

import numpy as np

MAX_ORDER = 64
MAX_TAPS = MAX_ORDER + 1


def clean(x) -> np.ndarray:
    """x~ in f64: the samples, 0 for a non-finite one."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isfinite(x), x, 0.0)


def lag_products(x, order: int):
    """(r, mag): r[k] = sum_{i >= k} x~[i] x~[i - k] correctly rounded (a product of two f32 values is exact in f64),
    mag[k] = sum |x~[i] x~[i - k]|, k = 0 .. order."""
    x = clean(x)
    r, mag = np.zeros(order + 1), np.zeros(order + 1)
    for k in range(order + 1):
        if k < x.size:
            p = x[k:] * x[:x.size - k]
            r[k], mag[k] = math.fsum(p), math.fsum(np.abs(p))
    return r, mag


def lag_bound(n: int, mag) -> np.ndarray:
    """|sum in any order - exact| <= (n - 1) u sum|p| + O(u^2), u = 2^-53 (Higham, Accuracy and Stability, 4.2), plus
    fsum's own rounding: n u sum|p| covers every summation order of n exact products."""
    return n * 2.0 ** -53 * np.asarray(mag)


def whiten_taps(r, noise_db: float = 60.0) -> np.ndarray:
    """a[0 .. order] in f64: Levinson-Durbin on r with r[0] (1 + 10^(-noise_db / 10)); stops before step m when the
    prediction error is <= 0 and at step m when |k| >= 1, the remaining taps are 0; r[0] <= 0 gives the identity."""
    r = np.asarray(r, dtype=np.float64)
    order = r.size - 1
    a = np.zeros(order + 1)
    a[0] = 1.0
    if not r[0] > 0.0:
        return a
    err = r[0] * (1.0 + 10.0 ** (-noise_db / 10.0))
    for m in range(1, order + 1):
        if not err > 0.0:
            break
        acc = r[m]
        for i in range(1, m):
            acc += a[i] * r[m - i]
        k = -acc / err
        if not abs(k) < 1.0:
            break
        t = a.copy()
        for i in range(1, m):
            t[i] = a[i] + k * a[m - i]
        t[m] = k
        a = t
        err *= 1.0 - k * k
    return a


def fir(x, taps, lead: int = 0) -> np.ndarray:
    """y[k] = sum_j taps[j] x[lead + k - j] in f64, k < len(x) - lead, x = 0 before its first sample; a non-finite
    sample reaches exactly the len(taps) outputs whose support holds it."""
    x = np.asarray(x, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    n = x.size - lead
    y = np.zeros(max(n, 0))
    with np.errstate(invalid="ignore", over="ignore"):
        for j, t in enumerate(taps):
            lo = max(0, j - lead)              # first output that reads a sample at or behind x[0]
            if lo < n:
                y[lo:] += t * x[lead + lo - j:x.size - j]
    return y


def downmix(interleaved) -> np.ndarray:
    """(l + r) * 0.5 * (1/65535) in f32, bit for bit as the library's down-mix."""
    a = np.asarray(interleaved, dtype=np.int16).reshape(-1, 2)
    s = a[:, 0].astype(np.float32) + a[:, 1].astype(np.float32)
    return (s * np.float32(0.5)) * np.float32(1.0 / 65535.0)


def ar1(rng, n: int, rho: float) -> np.ndarray:
    """AR(1) noise x[i] = rho x[i - 1] + e[i], e standard normal, in f64 (started in the stationary distribution)."""
    e = rng.standard_normal(n)
    x = np.empty(n)
    prev = e[0] / math.sqrt(1.0 - rho * rho)
    x[0] = prev
    for i in range(1, n):
        prev = rho * prev + e[i]
        x[i] = prev
    return x


def ar2(rng, n: int, a1: float, a2: float) -> np.ndarray:
    """AR(2) noise x[i] = a1 x[i - 1] + a2 x[i - 2] + e[i] in f64, after a run-in of 2000 samples."""
    e = rng.standard_normal(n + 2000)
    x = np.zeros(n + 2000)
    for i in range(2, n + 2000):
        x[i] = a1 * x[i - 1] + a2 * x[i - 2] + e[i]
    return x[2000:]
