"""The checker of per-segment hit scoring (am_hit_segments*, am_hit_segments_summary): a plain numpy f64 implementation
of the definition in include/audiomatch.h.  A module, not a test file; the tests import it."""
import struct
from dataclasses import dataclass

import numpy as np

UNREF, BELOW, NONFIN, EMPTY = 1, 2, 4, 8


@dataclass
class SegRef:
    lag: float
    ncc: float
    gain: float
    level_db: float
    flags: int
    lstar: int       # the integer lag chosen
    margin: float    # (best - second best c_j) / |best|; inf when there is one lag, or for a flagged segment


def seg_bounds(s, m):
    """a_0 .. a_m: segment j is needle samples [a_j, a_{j+1})."""
    return [j * s // m for j in range(m + 1)]


def segments_ref(x, needle, t, m, radius, floor_db=60):
    """The m SegRef records of a hit at t in f32 samples x (x counts as 0 outside the array)."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    n64 = np.asarray(needle, dtype=np.float32).astype(np.float64)
    s, length, r = len(n64), len(x64), int(radius)
    assert 1 <= m <= s and t + s <= length
    pad = np.concatenate([np.zeros(r), x64, np.zeros(r)])     # pad[r + u] = x[u]
    a = seg_bounds(s, m)
    ratio = 10.0 ** (-floor_db / 10.0)
    out = []
    for j in range(m):
        nj = n64[a[j]:a[j + 1]]
        lo, hi = max(0, t - r + a[j]), min(length, t + r + a[j + 1])
        if not (np.all(np.isfinite(nj)) and np.all(np.isfinite(x64[lo:hi]))):
            out.append(SegRef(0.0, np.nan, np.nan, np.nan, NONFIN, 0, np.inf))
            continue
        wins = [pad[r + t + l + a[j]:r + t + l + a[j + 1]] for l in range(-r, r + 1)]
        c = [float(np.dot(w, nj)) for w in wins]            # c[r + l] = c_j(l)
        ew = [float(np.dot(w, w)) for w in wins]
        en = float(np.dot(nj, nj))
        if en == 0.0:
            out.append(SegRef(0.0, 0.0, 0.0, np.inf if ew[r] > 0 else np.nan, EMPTY, 0, np.inf))
            continue
        ls = 0                                               # ties: the smaller |l|, then the negative lag
        for k in range(1, r + 1):
            if c[r - k] > c[r + ls]:
                ls = -k
            if c[r + k] > c[r + ls]:
                ls = k
        best = c[r + ls]
        others = [v for i, v in enumerate(c) if i != r + ls]
        margin = np.inf if not others else ((best - max(others)) / abs(best) if best != 0 else 0.0)
        flags, lag = 0, float(ls)
        if r == 0 or abs(ls) == r:
            flags |= UNREF
        else:
            pa, pc = c[r + ls - 1], c[r + ls + 1]
            den = pa - 2 * best + pc
            if not den < 0:
                flags |= UNREF
            else:
                lag += min(max(0.5 * (pa - pc) / den, -0.5), 0.5)
        e = ew[r + ls]
        if e == 0 or e < en * ratio:
            flags |= BELOW
            ncc = 0.0
        else:
            ncc = best / np.sqrt(en * e)
        out.append(SegRef(lag, ncc, best / en, -np.inf if e == 0 else 10 * np.log10(e / en), flags, ls, margin))
    return out


def summary_ref(recs, s, min_ncc):
    """am_hit_segments_summary of one hit's records (anything with lag, ncc, flags), needle length s: a dict."""
    m = len(recs)
    a = seg_bounds(s, m)
    present = [j for j, q in enumerate(recs) if not q.flags & (NONFIN | BELOW | EMPTY) and q.ncc >= min_ncc]
    usable = [j for j in present if not recs[j].flags & UNREF]
    out = dict(coverage=sum(a[j + 1] - a[j] for j in present) / s, drift_ppm=np.nan, start_lag=np.nan, residual_rms=np.nan,
               first_present=present[0] if present else -1, last_present=present[-1] if present else -1,
               n_present=len(present), n_usable=len(usable))
    if len(usable) >= 2:
        xs = np.array([(a[j] + a[j + 1]) / 2 for j in usable], dtype=np.float64)
        ys = np.array([recs[j].lag for j in usable], dtype=np.float64)
        mx, my = xs.sum() / len(xs), ys.sum() / len(ys)
        slope = float(((xs - mx) * (ys - my)).sum() / ((xs - mx) ** 2).sum())
        start = float(my - slope * mx)
        out.update(drift_ppm=1e6 * slope, start_lag=start, residual_rms=float(np.sqrt(((ys - (start + slope * xs)) ** 2).sum() / len(xs))))
    return out


def f32_ulps(a, b):
    """How many f32 values lie between a and b (both taken as f32); 0 for equal infinities or two NaNs."""
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if np.isnan(a) and np.isnan(b) else 1 << 31
    if a == b:
        return 0
    if np.isinf(a) or np.isinf(b):
        return 1 << 31

    def key(v):
        i = struct.unpack("<i", struct.pack("<f", v))[0]
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))


def assert_records(got, ref, lag_tol=1e-9, margin=1e-9):
    """got: the library's records of one hit, ref: segments_ref's.  Flags equal; l* equal wherever the checker's best lag
    wins by more than `margin`; lag within lag_tol; ncc, gain, level_db within 2 f32 ulp of the checker's value."""
    assert len(got) == len(ref)
    for j, (g, e) in enumerate(zip(got, ref)):
        assert g.flags == e.flags, (j, g, e)
        if e.flags & NONFIN:
            assert g.lag == 0.0 and np.isnan(g.ncc) and np.isnan(g.gain) and np.isnan(g.level_db), (j, g)
            continue
        if e.margin > margin:
            assert abs(g.lag - e.lag) <= lag_tol and round(g.lag - (e.lag - e.lstar)) == e.lstar, (j, g, e)
        for name in ("ncc", "gain", "level_db"):
            assert f32_ulps(getattr(g, name), getattr(e, name)) <= 2, (j, name, g, e)


def bits(hit_records):
    """The records of one hit, byte for byte."""
    return [struct.pack("<dfffI", q.lag, q.ncc, q.gain, q.level_db, q.flags) for q in hit_records]
