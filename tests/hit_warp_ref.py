"""The checker of per-hit drift scoring (am_hit_warp*, am_warp_table, am_hit_window_warped): a plain numpy f64
implementation of the definition in include/audiomatch.h.  A module, not a test file; the tests import it."""
import math
import struct
from dataclasses import dataclass

import numpy as np

from hit_segments_ref import f32_ulps

UNREF, BELOW, NONFIN, EMPTY, DRIFT_UNREF = 1, 2, 4, 8, 256
PHASES, TAPS, MAX_STEPS, MAX_PPM, MAX_RADIUS = 4096, 32, 32, 50000, 16
HALF = TAPS // 2 - 1          # tap k reads sample m - HALF + k
TWO32 = 4294967296.0


def table_formula():
    """h[p][k] in f64, by the formula (row 0: the delta by definition)."""
    p = np.arange(PHASES, dtype=np.float64)[:, None]
    k = np.arange(TAPS, dtype=np.float64)[None, :]
    x = k - HALF - p / PHASES
    v = np.sinc(x) * np.i0(8.0 * np.sqrt(np.maximum(0.0, 1.0 - (x / (TAPS // 2)) ** 2))) / np.i0(8.0)
    h = v / v.sum(axis=1, keepdims=True)
    h[0] = 0.0
    h[0, HALF] = 1.0
    return h


def llround(x):
    """C's llround: half away from zero."""
    a = abs(x)
    n = int(a) if a >= 2.0 ** 52 else int(math.floor(a + 0.5))
    return -n if x < 0 else n


def inc_of(d_ppm):
    return llround(TWO32 / (1.0 + d_ppm * 1e-6))


def warp_len(s, d_ppm):
    return ((s - 1) << 32) // inc_of(d_ppm) + 1


def drifts(centre_ppm, max_ppm, steps):
    k = int(steps)
    return [float(centre_ppm)] if k == 0 else [centre_ppm + max_ppm * float(q - k) / float(k) for q in range(2 * k + 1)]


def _interp(h, x64, m, p):
    """sum_k h[p][k] x~[m - HALF + k] in f64, k ascending; x~ = 0 outside.  h: the f32 table, x64: f64 samples."""
    pad = np.concatenate([np.zeros(HALF), x64, np.zeros(TAPS)])     # pad[HALF + i] = x[i]
    h64 = h.astype(np.float64)
    acc = np.zeros(len(m))
    for k in range(TAPS):
        acc = acc + h64[p, k] * pad[m + k]
    return acc


def warp(needle, d_ppm, h):
    """The needle resampled to drift d_ppm: f32, S_d samples.  h: the table of am_warp_table (f32)."""
    n32 = np.asarray(needle, dtype=np.float32)
    s = len(n32)
    inc = inc_of(d_ppm)
    j = np.arange(warp_len(s, d_ppm), dtype=np.uint64)
    u = j * np.uint64(inc) + np.uint64(1 << 19)
    m = (u >> np.uint64(32)).astype(np.int64)
    p = ((u >> np.uint64(20)) & np.uint64(PHASES - 1)).astype(np.int64)
    assert m.max() < s
    with np.errstate(invalid="ignore", over="ignore"):
        out = _interp(h, n32.astype(np.float64), m, p).astype(np.float32)
    return np.where(p == 0, n32[m], out)


@dataclass
class WarpRef:
    drift_ppm: float
    lag: float
    ncc: float
    gain: float
    level_db: float
    ncc_centre: float
    length: int
    flags: int
    qstar: int
    lstar: int
    margin: float    # (best ncc - the best other ncc) / |best|; cells that tie with the best exactly (decided by the tie rule,
                     # e.g. every rate of a one-sample needle) do not count; inf when there is no other cell, or for a flagged hit
    cells: object = None     # ncc(q, l), shape (Q, 2 R + 1)


def cells(x, needle, t, wp, h, floor_db=60):
    """c, E_w (Q x (2R+1)), E_n (Q), ncc and the warped lengths of a hit at t; wp = (centre_ppm, max_ppm, steps, radius)."""
    centre, max_ppm, steps, r = wp
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    ds = drifts(centre, max_ppm, steps)
    ws = [warp(needle, d, h).astype(np.float64) for d in ds]
    longest = max(len(w) for w in ws)
    pad = np.concatenate([np.zeros(r), x64, np.zeros(r + longest)])   # pad[r + u] = x[u]
    ratio = 10.0 ** (-floor_db / 10.0)
    q_n, nl = len(ds), 2 * r + 1
    c, ew, en, ncc = np.zeros((q_n, nl)), np.zeros((q_n, nl)), np.zeros(q_n), np.zeros((q_n, nl))
    for q, w in enumerate(ws):
        en[q] = float(np.dot(w, w))
        for l in range(-r, r + 1):
            win = pad[r + t + l:r + t + l + len(w)]
            c[q, r + l] = float(np.dot(win, w))
            ew[q, r + l] = float(np.dot(win, win))
            if not (en[q] == 0 or ew[q, r + l] == 0 or ew[q, r + l] < en[q] * ratio):
                ncc[q, r + l] = c[q, r + l] / np.sqrt(en[q] * ew[q, r + l])
    return c, ew, en, ncc, [len(w) for w in ws], ds


def vertex(a, b, c):
    den = a - 2 * b + c
    if not den < 0:
        return None
    return min(max(0.5 * (a - c) / den, -0.5), 0.5)


def warp_ref(x, needle, t, wp, h, floor_db=60):
    """The WarpRef record of a hit at t in f32 samples x (x counts as 0 outside the array)."""
    centre, max_ppm, steps, r = wp
    kk = int(steps)
    x32 = np.asarray(x, dtype=np.float32)
    n32 = np.asarray(needle, dtype=np.float32)
    s = len(n32)
    assert t + s <= len(x32)
    longest = warp_len(s, max(drifts(centre, max_ppm, steps)))      # max_q S_q (K = 0: the one drift is centre_ppm)
    lo, hi = max(0, t - r), min(len(x32), t + r + longest)
    if not (np.all(np.isfinite(n32)) and np.all(np.isfinite(x32[lo:hi]))):
        return WarpRef(float(centre), 0.0, np.nan, np.nan, np.nan, np.nan, s, NONFIN, kk, 0, np.inf)
    c, ew, en, ncc, lens, ds = cells(x32, n32, t, wp, h, floor_db)
    qs, ls, best = kk, 0, ncc[kk, r]
    for dq in range(kk + 1):                      # candidates in the order of the tie rule; only a larger one replaces
        for q in ([kk] if dq == 0 else [kk - dq, kk + dq]):
            for dl in range(r + 1):
                for l in ([0] if dl == 0 else [-dl, dl]):
                    if ncc[q, r + l] > best:
                        qs, ls, best = q, l, ncc[q, r + l]
    others = ncc[ncc != best]
    margin = np.inf if others.size == 0 else (best - others.max()) / (abs(best) if best != 0 else 1.0)
    e_n, e_w, cc = en[qs], ew[qs, r + ls], c[qs, r + ls]
    centre_ncc = float(ncc[kk, r])
    if e_n == 0:
        return WarpRef(ds[qs], 0.0, 0.0, 0.0, np.inf if e_w > 0 else np.nan, centre_ncc, lens[qs], EMPTY, qs, ls, np.inf, ncc)
    flags, drift, lag = 0, ds[qs], float(ls)
    v = None if (kk == 0 or qs == 0 or qs == 2 * kk) else vertex(ncc[qs - 1, r + ls], best, ncc[qs + 1, r + ls])
    if v is None:
        flags |= DRIFT_UNREF
    else:
        drift += v * max_ppm / kk
    v = None if (r == 0 or abs(ls) == r) else vertex(c[qs, r + ls - 1], cc, c[qs, r + ls + 1])
    if v is None:
        flags |= UNREF
    else:
        lag += v
    if e_w == 0 or e_w < e_n * 10.0 ** (-floor_db / 10.0):
        flags |= BELOW
    return WarpRef(drift, lag, float(best), cc / e_n, -np.inf if e_w == 0 else 10 * np.log10(e_w / e_n), centre_ncc, lens[qs],
                   flags, qs, ls, margin, ncc)


def assert_records(got, ref, wp, margin=1e-9, lag_tol=1e-9):
    """got: the library's records (one per hit), ref: warp_ref's.  Flags equal; (q*, l*) equal wherever the checker's best
    cell wins by more than `margin`; lag within lag_tol; drift_ppm within 1e-6 of a grid step; ncc, gain, level_db and
    ncc_centre within 2 f32 ulp of the checker's value; length equal."""
    centre, max_ppm, steps, r = wp
    step = max_ppm / steps if steps else 0.0
    assert len(got) == len(ref)
    for i, (g, e) in enumerate(zip(got, ref)):
        assert g.flags == e.flags, (i, g, e)
        if e.flags & NONFIN:
            assert g.drift_ppm == centre and g.lag == 0.0 and g.length == e.length, (i, g, e)
            assert all(np.isnan(getattr(g, f)) for f in ("ncc", "gain", "level_db", "ncc_centre")), (i, g)
            continue
        assert f32_ulps(g.ncc, e.ncc) <= 2 and f32_ulps(g.ncc_centre, e.ncc_centre) <= 2, (i, g, e)
        if e.margin > margin:
            # the cell itself: the record's drift lies within half a step of d_q* (the vertex is clamped there) and its
            # length is S_q*; then the refined values
            d_star = drifts(centre, max_ppm, steps)[e.qstar]
            assert abs(g.drift_ppm - d_star) <= 0.5 * step * (1 + 1e-12) and g.length == e.length, (i, g, e)
            if steps:
                assert round((g.drift_ppm - (e.drift_ppm - d_star) - centre) / step) + steps == e.qstar, (i, g, e)
            assert abs(g.drift_ppm - e.drift_ppm) <= 1e-6 * step, (i, g, e)
            assert abs(g.lag - e.lag) <= lag_tol and round(g.lag - (e.lag - e.lstar)) == e.lstar, (i, g, e)
            assert g.length == e.length, (i, g, e)
            for name in ("gain", "level_db"):
                assert f32_ulps(getattr(g, name), getattr(e, name)) <= 2, (i, name, g, e)


def window_warped(x, start, scale, lag, drift_ppm, lead, length, h):
    """am_hit_window_warped of f32 samples x (NaN: absent), bit for bit."""
    x32 = np.asarray(x, dtype=np.float32)
    n = len(x32)
    inc = llround(TWO32 * (1.0 + drift_ppm * 1e-6))
    base = (int(start) << 32) + llround(lag * TWO32) + (1 << 19)
    u = np.array([base + (i - int(lead)) * inc for i in range(int(length))], dtype=object)
    m = np.array([int(v) >> 32 for v in u], dtype=np.int64)           # (floor)
    p = np.array([(int(v) >> 20) & (PHASES - 1) for v in u], dtype=np.int64)
    nz = h[p] != 0                                                     # (length, TAPS): the taps that count
    idx = m[:, None] - HALF + np.arange(TAPS)[None, :]
    inside = (idx >= 0) & (idx < n)
    xs = np.where(inside, x32[np.clip(idx, 0, max(n - 1, 0))] if n else 0.0, np.nan).astype(np.float64)
    present = np.all(~nz | (inside & np.isfinite(xs)), axis=1)
    h64 = h[p].astype(np.float64)
    acc = np.zeros(int(length))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(TAPS):
            acc = acc + np.where(nz[:, k] & present, h64[:, k] * np.where(np.isfinite(xs[:, k]), xs[:, k], 0.0), 0.0)
        v = acc.astype(np.float32)
        centre = np.where(inside[:, HALF], x32[np.clip(m, 0, max(n - 1, 0))] if n else np.float32(0), np.float32(np.nan)).astype(np.float32)
        v = np.where(p == 0, centre, v)
        out = (v * np.float32(scale)).astype(np.float32)
    return np.where(present & np.isfinite(out), out, np.float32(np.nan)).astype(np.float32)


def bits(rec):
    """One record, byte for byte."""
    return struct.pack("<ddffffII", rec.drift_ppm, rec.lag, rec.ncc, rec.gain, rec.level_db, rec.ncc_centre, rec.length, rec.flags)


def row_bits(row):
    """A row's bits with every NaN counted as the same value."""
    r = np.asarray(row, dtype=np.float32)
    return np.where(np.isnan(r), np.uint32(0x7FC00000), r.view(np.uint32))
