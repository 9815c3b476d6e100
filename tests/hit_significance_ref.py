"""The f64 checker of per-hit significance (am_hit_significance*): given the f32 scores of a hit's zone it produces the
record of the definition in include/audiomatch.h, tie rule and flags included.  A module, not a test file; the tests
import it."""
import struct

import numpy as np

NONFIN, NO_BG, FLAT, CLIPPED = 4, 16, 32, 64
FIELDS = ("score", "bg_mean", "bg_std", "z", "side_max", "side_lag", "n_bg", "flags")


def zone(t, s, length, radius):
    """(lo, hi, clipped) of a hit at t: the zone's lags lo .. hi; the span is samples [lo, hi + s)."""
    lo, hi = max(0, t - radius), min(length - s, t + radius)
    return lo, hi, (lo > t - radius or hi < t + radius)


def significance_ref(scores, c, guard, clipped=False, nonfinite=False):
    """The record of a hit whose zone scores are `scores` (f32, r(lo) .. r(hi)) with its own score at index c."""
    r32 = np.asarray(scores, dtype=np.float32)
    r = r32.astype(np.float64)
    d = np.arange(len(r), dtype=np.int64) - int(c)
    bg = np.abs(d) > int(guard)
    n_bg = int(bg.sum())
    flags = CLIPPED if clipped else 0
    nan = float("nan")
    rec = dict(score=float(r32[c]), bg_mean=nan, bg_std=nan, z=nan, side_max=nan, side_lag=0, n_bg=n_bg, flags=flags)
    if nonfinite:
        rec.update(score=nan, flags=flags | NONFIN)
        return rec
    if n_bg < 2:
        rec["flags"] |= NO_BG
        return rec
    u = r[bg]
    mean = float(np.sum(u) / n_bg)
    std = float(np.sqrt(np.sum((u - mean) ** 2) / n_bg))
    diff = float(r[c]) - mean
    if std == 0.0:
        rec["flags"] |= FLAT
        z = float("inf") if diff > 0 else float("-inf") if diff < 0 else 0.0
    else:
        z = diff / std
    top = u.max()
    lags = d[bg][u == top]
    best = min(lags, key=lambda q: (abs(int(q)), int(q)))   # the smaller |lag|, then the negative lag
    rec.update(bg_mean=float(np.float32(mean)), bg_std=float(np.float32(std)), z=float(np.float32(z)),
               side_max=float(np.float32(top)), side_lag=int(best))
    rec["_mean64"], rec["_std64"], rec["_z64"] = mean, std, z
    return rec


def f32_bits(v):
    return struct.pack("<f", v)


def pack(q):
    """The 32 bytes of a record (a HitSignificance, or anything with its fields)."""
    return struct.pack("<fffffiII", q.score, q.bg_mean, q.bg_std, q.z, q.side_max, q.side_lag, q.n_bg, q.flags)


def assert_record(got, exp, rel=1e-6):
    """`got` (a HitSignificance) against the checker's record: score, side_max, side_lag, n_bg and flags bit for bit;
    bg_std and z within `rel` relative, bg_mean within rel * (|mean| + std) -- the f32 rounding of an f64 reduction."""
    assert got.flags == exp["flags"] and got.n_bg == exp["n_bg"] and got.side_lag == exp["side_lag"], (got, exp)
    for k in ("score", "side_max"):
        g, e = getattr(got, k), exp[k]
        assert (np.isnan(g) and np.isnan(e)) or f32_bits(g) == f32_bits(e), (k, got, exp)
    if np.isnan(exp["bg_mean"]):
        assert np.isnan(got.bg_mean) and np.isnan(got.bg_std) and np.isnan(got.z), (got, exp)
        return
    mean, std, z = exp["_mean64"], exp["_std64"], exp["_z64"]
    assert abs(got.bg_mean - mean) <= rel * (abs(mean) + std), (got, exp)
    assert abs(got.bg_std - std) <= rel * std, (got, exp)
    if np.isinf(z) or z == 0.0:
        assert got.z == z, (got, exp)
    else:
        assert abs(got.z - z) <= rel * abs(z), (got, exp)
