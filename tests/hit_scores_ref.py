"""The checker of per-hit scoring (am_hit_scores*): a plain numpy f64 implementation of the definition in
include/audiomatch.h -- exact NCC, least-squares gain, window level and parabolic sub-sample position of a hit, with the
flags.  A module, not a test file; the tests import it."""
import numpy as np

UNREF, BELOW, NONFIN = 1, 2, 4


def hit_ref(x, needle, t, floor_db=60):
    """(position, ncc, gain, window_db, flags) of a hit at t in f32 samples x, in f64."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    n64 = np.asarray(needle, dtype=np.float32).astype(np.float64)
    s, length = len(n64), len(x64)
    en = float(np.dot(n64, n64))
    win = x64[t:t + s]
    if not (np.all(np.isfinite(win)) and np.all(np.isfinite(n64))):
        return float(t), np.nan, np.nan, np.nan, NONFIN
    with np.errstate(invalid="ignore", over="ignore"):
        b = float(np.dot(win, n64))
        ew = float(np.dot(win, win))
        a = float(np.dot(x64[t - 1:t - 1 + s], n64)) if t > 0 else np.nan
        c = float(np.dot(x64[t + 1:t + 1 + s], n64)) if t + s < length else np.nan
    flags, pos = 0, float(t)
    den = a - 2 * b + c
    if not (np.isfinite(a) and np.isfinite(c) and den < 0):
        flags |= UNREF
    else:
        pos = t + min(max(0.5 * (a - c) / den, -0.5), 0.5)
    if ew == 0 or ew < en * 10.0 ** (-floor_db / 10.0):
        flags |= BELOW
        ncc = 0.0
    else:
        ncc = b / np.sqrt(en * ew)
    gain = b / en if en > 0 else 0.0
    wdb = -np.inf if ew == 0 else 10 * np.log10(ew / en)
    return pos, ncc, gain, wdb, flags


def assert_ref(got, exp, tol=1e-6):
    pos, ncc, gain, wdb, flags = exp
    assert got.flags == flags, (got, exp)
    if flags & NONFIN:
        assert got.position == pos and np.isnan(got.ncc) and np.isnan(got.gain)
        return
    assert abs(got.position - pos) <= tol, (got, exp)
    assert abs(got.ncc - ncc) <= tol and abs(got.gain - gain) <= tol, (got, exp)
    if np.isinf(wdb):
        assert got.window_db == wdb
    else:
        assert abs(got.window_db - wdb) <= 1e-3, (got, exp)
