"""The checker of per-hit channel estimation (am_hit_channel*, include/audiomatch.h), in plain numpy f64: c, r and the
energies by np.dot, the Toeplitz matrix built explicitly and solved with np.linalg.solve, the record by the header's
formulas.  cond(T) is returned beside the result, so that a test can state what its own designs are worth."""
from dataclasses import dataclass

import numpy as np

BELOW, NONFIN, EMPTY, ILL = 2, 4, 8, 512
MAX_RADIUS = 128


def bits(q):
    return bytes(q)


def toeplitz(r, lam=0.0):
    n = len(r)
    idx = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    t = np.asarray(r, dtype=np.float64)[idx]
    t[np.arange(n), np.arange(n)] *= 1.0 + lam
    return t


def solve_ref(r, c, noise_db):
    """(h, cond(T)) of T h = c, T = toeplitz(r) with the diagonal times 1 + 10^(-noise_db / 10)."""
    t = toeplitz(r, 10.0 ** (-noise_db / 10.0))
    return np.linalg.solve(t, np.asarray(c, dtype=np.float64)), float(np.linalg.cond(t))


def sums_ref(hay, needle, t, p):
    """(c[-P .. P], r[0 .. 2P], E_w, E_x, finite) of the header, x = 0 outside the haystack."""
    x = np.asarray(hay, dtype=np.float64)
    n = np.asarray(needle, dtype=np.float64)
    s, ln = len(n), len(x)
    lo, hi = max(t - p, 0), min(t + s + p, ln)
    finite = bool(np.isfinite(n).all() and np.isfinite(x[lo:hi]).all())
    span = np.zeros(s + 2 * p)                       # span[u + p] = x[t + u]
    span[lo - (t - p):hi - (t - p)] = x[lo:hi]
    if not finite:
        return None, None, 0.0, 0.0, False
    c = np.array([np.dot(span[l + p:l + p + s], n) for l in range(-p, p + 1)])
    r = np.array([np.dot(n[k:], n[:s - k]) if k < s else 0.0 for k in range(2 * p + 1)])
    return c, r, float(np.dot(span[p:p + s], span[p:p + s])), float(np.dot(span, span)), True


@dataclass
class ChanRef:
    ncc: float
    ncc_eq: float
    gain_db: float
    residual_db: float
    main_tap: int
    main_share: float
    flags: int
    taps: np.ndarray
    cond: float


def record_ref(c, r, ew, ex, p, h, ill, floor_db=60.0, cond=float("nan")):
    """The record of the header from the sums and the (unrounded) taps h."""
    en = r[0]
    ratio = 10.0 ** (-floor_db / 10.0)
    rr = toeplitz(r)
    hc, q = float(np.dot(h, c)), float(h @ rr @ h)
    flags = ILL if ill else 0
    ncc = ncc_eq = 0.0
    if ew == 0.0 or ew < en * ratio:
        flags |= BELOW
    else:
        ncc = c[p] / np.sqrt(en * ew)
    if ex == 0.0 or not q > 0.0 or ex < en * ratio:
        flags |= BELOW
    else:
        ncc_eq = hc / np.sqrt(ex * q)
    with np.errstate(divide="ignore"):
        gain_db = 10.0 * np.log10(q / en) if q > 0.0 else -np.inf
        if ex == 0.0:
            res_db = np.nan
        else:
            num = max(ex - 2.0 * hc + q, 0.0)
            res_db = 10.0 * np.log10(num / ex) if num > 0.0 else -np.inf
    best = 0
    for k in range(1, p + 1):
        if abs(h[p - k]) > abs(h[p + best]):
            best = -k
        if abs(h[p + k]) > abs(h[p + best]):
            best = k
    hh = float(np.dot(h, h))
    share = h[p + best] ** 2 / hh if hh > 0.0 else 0.0
    return ChanRef(float(ncc), float(ncc_eq), float(gain_db), float(res_db), best, float(share), flags, np.asarray(h, dtype=np.float64), cond)


def channel_ref(hay, needle, t, p, noise_db, floor_db=60.0):
    """The ChanRef of the hit at t: the sums from the f32 inputs in f64, the explicit solve, the record."""
    c, r, ew, ex, finite = sums_ref(hay, needle, t, p)
    n = 2 * p + 1
    nan = float("nan")
    if not finite:
        return ChanRef(nan, nan, nan, nan, 0, nan, NONFIN, np.full(n, nan), nan)
    if r[0] == 0.0:
        return ChanRef(0.0, 0.0, nan, 0.0 if ex > 0.0 else nan, 0, 0.0, EMPTY, np.zeros(n), nan)
    h, cond = solve_ref(r, c, noise_db)
    return record_ref(c, r, ew, ex, p, h, False, floor_db, cond)


def close_db(a, b, tol):
    if np.isnan(b):
        return bool(np.isnan(a))
    if np.isinf(b):
        return a == b
    return abs(a - b) <= tol


def close_share(a_db, b_db):
    """residual_db: within 1e-4 dB, or -- where the filtered needle explains nearly all of the span and E_x - 2 h.c + q
    cancels -- within 1e-11 of E_x as a share: E_x, h.c and q each carry the relative error of their summation order, up
    to S 2^-53 (about 1e-12 at the sizes of these tests), and below that the difference of the three holds no digit."""
    if close_db(a_db, b_db, 1e-4):
        return True
    if np.isnan(a_db) or np.isnan(b_db):
        return False
    return abs(10.0 ** (a_db / 10.0) - 10.0 ** (b_db / 10.0)) <= 1e-11


def assert_record(got, taps, exp, who=""):
    """The tolerances of the issue: taps 1e-6 max|ref|; ncc, ncc_eq, main_share 1e-6; the dB fields 1e-4 dB (residual_db: see
    close_share); main_tap and the flags exact."""
    assert got.flags == exp.flags and got.main_tap == exp.main_tap and got.reserved == 0, (who, got, exp)
    if exp.flags & NONFIN:
        assert np.isnan(taps).all() and all(np.isnan(v) for v in (got.ncc, got.ncc_eq, got.gain_db, got.residual_db, got.main_share)), (who, got)
        return
    scale = np.abs(exp.taps).max()
    err = np.abs(taps.astype(np.float64) - exp.taps).max()
    assert err <= 1e-6 * scale, (who, err, scale, exp.cond)
    for name in ("ncc", "ncc_eq", "main_share"):
        assert abs(getattr(got, name) - getattr(exp, name)) <= 1e-6, (who, name, got, exp)
    assert close_db(got.gain_db, exp.gain_db, 1e-4), (who, "gain_db", got, exp)
    assert close_share(got.residual_db, exp.residual_db), (who, "residual_db", got, exp)


def residual_ref(hay_mono, start, needle, taps):
    """am_hit_residual restated: (model, resid) over the S + 2P elements from start - P on."""
    nd = np.asarray(needle, dtype=np.float32)
    tp = np.asarray(taps, dtype=np.float32)
    x = np.asarray(hay_mono, dtype=np.float32)
    p, s = len(tp) // 2, len(nd)
    model = np.empty(s + 2 * p, dtype=np.float32)
    resid = np.full(s + 2 * p, np.nan, dtype=np.float32)
    for u in range(s + 2 * p):
        acc = 0.0
        for l in range(-p, p + 1):
            i = u - p - l
            if 0 <= i < s:
                acc += float(tp[l + p]) * float(nd[i])
        model[u] = np.float32(acc)
        e = start - p + u
        if 0 <= e < len(x) and np.isfinite(x[e]):
            resid[u] = x[e] - model[u]
    return model, resid
