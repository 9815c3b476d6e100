"""Checker for needle estimation (include/audiomatch.h, "needle estimation"): the definitions in numpy, nothing else.

  hit_window(x, start, scale, lead, length)   one row: fl32(x[start - lead + n] * scale), NaN where absent
  estimate(rows, method, trim_permille)       (est f32, dev as f64 before its one rounding, count u32)
  designed_case()                             nine occurrences of a clean needle under overlays, the exactness case

Sums are f64 in the stated orders (hit order for the mean and the deviation, ascending for the trimmed mean), values are
ordered by the monotone integer key of their f32 bits, a row value is one f32 multiply."""
import numpy as np

MEAN, MEDIAN, TRIMMED = 0, 1, 2
MAX_HITS = 64
ABSENT_KEY = np.uint32(0xFFFFFFFF)


def downmix(interleaved) -> np.ndarray:
    """(l + r) * 0.5 * (1/65535) in f32, bit for bit as the library's down-mix."""
    a = np.asarray(interleaved, dtype=np.int16).reshape(-1, 2)
    s = a[:, 0].astype(np.float32) + a[:, 1].astype(np.float32)
    return s * (np.float32(0.5) * (np.float32(1.0) / np.float32(65535.0)))


def samples_f32(x) -> np.ndarray:
    a = np.asarray(x)
    return downmix(a) if a.dtype == np.int16 else a.astype(np.float32, copy=False)


def hit_window(x, start: int, scale, lead: int, length: int) -> np.ndarray:
    x = samples_f32(x)
    e = int(start) - int(lead) + np.arange(int(length), dtype=np.int64)
    inside = (e >= 0) & (e < x.size)
    row = np.full(int(length), np.nan, dtype=np.float32)
    xv = x[e[inside]]
    with np.errstate(over="ignore", invalid="ignore"):
        row[inside] = np.where(np.isfinite(xv), xv * np.float32(scale), np.float32(np.nan))
    return row


def keys(v: np.ndarray) -> np.ndarray:
    """the monotone integer key of f32 values: bits ^ 0x80000000 for a non-negative sign, ~bits otherwise"""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def unkeys(k: np.ndarray) -> np.ndarray:
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def estimate(rows, method: int, trim_permille: int = 0):
    """(est f32, dev f64 -- round it to f32 once to compare --, count u32) of rows (n x length f32)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, length = rows.shape
    present = np.isfinite(rows)
    count = present.sum(axis=0).astype(np.uint32)
    c = count.astype(np.int64)
    safe = np.maximum(c, 1)
    v64 = np.where(present, rows, np.float32(0)).astype(np.float64)
    if method == MEAN:
        s = np.zeros(length, dtype=np.float64)
        for i in range(n):                       # hit order
            s = np.where(present[i], s + v64[i], s)
        m = s / safe
    else:
        k = np.where(present, keys(rows), ABSENT_KEY)
        k.sort(axis=0)                           # absent keys last
        vs = unkeys(k).astype(np.float64)        # (absent slots decode to NaN and are never read)
        cols = np.arange(length)
        if method == MEDIAN:
            a = vs[np.maximum(c - 1, 0) // 2, cols]   # the two middle values; one and the same for an odd count
            b = vs[c // 2, cols]                      # (c // 2 <= n - 1)
            m = (a + b) / 2.0
        elif method == TRIMMED:
            d = np.minimum(c * int(trim_permille) // 1000, np.maximum(c - 1, 0) // 2)
            s = np.zeros(length, dtype=np.float64)
            for i in range(n):                   # ascending
                take = (i >= d) & (i < c - d)
                s = np.where(take, s + np.where(take, vs[i], 0.0), s)
            m = s / np.maximum(c - 2 * d, 1)
        else:
            raise ValueError("unknown method")
    m = np.where(c > 0, m, 0.0)
    acc = np.zeros(length, dtype=np.float64)
    for i in range(n):                           # hit order
        dlt = v64[i] - m
        acc = np.where(present[i], acc + dlt * dlt, acc)
    dev = np.where(c > 0, np.sqrt(acc / safe), 0.0)
    return m.astype(np.float32), dev, count


def ulps_f32(got: np.ndarray, want64: np.ndarray) -> np.ndarray:
    """|got - fl32(want64)| in units of fl32(want64)'s f32 spacing"""
    w = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - w.astype(np.float64)) / np.spacing(np.maximum(np.abs(w), np.float32(1e-45))).astype(np.float64)


GAINS = (0.25, 0.5, 1.0, 2.0, 4.0)
CLEAN_LEN = 4096
THIRD = 1366


def designed_case(seed: int = 17):
    """A clean needle c of 4096 samples; nine occurrences g_i * c, g_i a power of two (scale 1 / g_i restores c exactly),
    occurrence i under loud noise over the third [(i mod 3) * 1366, (i mod 3 + 1) * 1366) of the needle: at every sample
    at most 3 of 9 values are contaminated, at least 6 equal c[n], and the fifth smallest is c[n].
    Returns (c, occurrences [9 x 4096 f32], scales [9 f32], contaminated [9 x 4096 bool])."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.5, 0.5, CLEAN_LEN).astype(np.float32)
    occ = np.empty((9, CLEAN_LEN), dtype=np.float32)
    scales = np.empty(9, dtype=np.float32)
    dirty = np.zeros((9, CLEAN_LEN), dtype=bool)
    for i in range(9):
        g = np.float32(GAINS[i % len(GAINS)])
        occ[i] = c * g
        lo = (i % 3) * THIRD
        hi = min(lo + THIRD, CLEAN_LEN)
        occ[i, lo:hi] += rng.uniform(-1.0, 1.0, hi - lo).astype(np.float32) * g   # (louder than c, which spans +-0.5)
        dirty[i, lo:hi] = True
        scales[i] = np.float32(1.0) / g
    return c, occ, scales, dirty
