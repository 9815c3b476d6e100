"""numpy reference of the score traces (include/audiomatch.h, "score traces"): the am_trace_bin records of a score array
and the am_trace_stats summary of a list of records.  trace_loop / summary_loop are the same definitions as plain
Python loops, for checking the vectorised forms on small arrays (test_trace_host.py).

The sums here are numpy's f64 sums: the header fixes ONE order of additions for the library, and any two orders of the
same n additions of a bin differ by at most 2 n 2^-53 sum|r| (sum_bound), which is what a test may allow; on
integer-valued scores every order is exact and the sums compare bit for bit.  trace_ordered is a model of the header's
own order: on scores whose sums round, the library's records equal it bit for bit."""
import math

import numpy as np

BIN_DTYPE = np.dtype([("max", "<f4"), ("min", "<f4"), ("argmax", "<u4"), ("argmin", "<u4"), ("count", "<u4"),
                      ("reserved", "<u4"), ("sum", "<f8"), ("sumsq", "<f8")])
SUMMARY_FIELDS = ("count", "argmax", "argmin", "max", "min", "mean", "std", "median_max", "mad_max", "peak_z")


def n_bins(n, D):
    return (n + D - 1) // D


def trace(scores, D):
    """The records of scores (f32) at bin length D."""
    r = np.ascontiguousarray(scores, dtype=np.float32)
    n, nb = r.size, n_bins(r.size, D)
    out = np.zeros(nb, dtype=BIN_DTYPE)
    if nb == 0:
        return out
    pad = np.full(nb * D, np.nan, dtype=np.float32)
    pad[:n] = r
    m = pad.reshape(nb, D)
    ok = ~np.isnan(m)
    cnt = ok.sum(axis=1)
    some = cnt > 0
    hi = np.where(ok, m, -np.inf).max(axis=1)
    lo = np.where(ok, m, np.inf).min(axis=1)
    # the FIRST counted score equal (==) to the extreme: -0.0 == +0.0
    amax = np.argmax(ok & (m == hi[:, None]), axis=1)
    amin = np.argmax(ok & (m == lo[:, None]), axis=1)
    rows = np.arange(nb)
    out["max"] = np.where(some, m[rows, amax], np.float32(np.nan))
    out["min"] = np.where(some, m[rows, amin], np.float32(np.nan))
    out["argmax"] = np.where(some, amax, 0)
    out["argmin"] = np.where(some, amin, 0)
    out["count"] = cnt
    d = np.where(ok, m, np.float32(0)).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        out["sum"] = d.sum(axis=1)
        out["sumsq"] = (d * d).sum(axis=1)
    return out


def _span_sums(m):
    """The header's order for spans (rows of m, f64, a skipped score as +0.0): class j mod 256 adds in ascending j from
    +0.0, t[l] = (c[4l] + c[4l + 1]) + (c[4l + 2] + c[4l + 3]), then t[l] += t[l ^ m] for m = 32 .. 1; the sum is t[0]."""
    k, L = m.shape
    steps = (L + 255) // 256
    pad = np.zeros((k, steps * 256), dtype=np.float64)
    pad[:, :L] = m
    c = np.zeros((k, 256), dtype=np.float64)
    for s in range(steps):
        c = c + pad[:, s * 256:(s + 1) * 256]
    t = (c[:, 0::4] + c[:, 1::4]) + (c[:, 2::4] + c[:, 3::4])
    lanes = np.arange(64)
    for mask in (32, 16, 8, 4, 2, 1):
        t = t + t[:, lanes ^ mask]
    return t[:, 0]


def trace_ordered(scores, D, sliced, slice_len):
    """trace() with sum and sumsq added in the order include/audiomatch.h documents: the whole bin as one span, or
    (sliced) spans of slice_len scores from the bin's start, their sums added in ascending order from +0.0."""
    r = np.ascontiguousarray(scores, dtype=np.float32)
    out = trace(r, D)
    nb = out.size
    if nb == 0:
        return out
    pad = np.zeros(nb * D, dtype=np.float64)
    pad[:r.size] = np.where(np.isnan(r), np.float32(0), r)
    m = pad.reshape(nb, D)
    for field, v in (("sum", m), ("sumsq", m * m)):
        if not sliced:
            out[field] = _span_sums(v)
            continue
        per_bin = (D + slice_len - 1) // slice_len
        w = np.zeros((nb, per_bin * slice_len), dtype=np.float64)
        w[:, :D] = v
        parts = _span_sums(w.reshape(nb * per_bin, slice_len)).reshape(nb, per_bin)
        s = np.zeros(nb, dtype=np.float64)
        for j in range(per_bin):
            s = s + parts[:, j]
        out[field] = s
    return out


def trace_loop(scores, D):
    """trace() as a plain loop over the scores."""
    r = np.asarray(scores, dtype=np.float32)
    out = np.zeros(n_bins(r.size, D), dtype=BIN_DTYPE)
    for b in range(out.size):
        best = worst = None
        cnt, s, q = 0, 0.0, 0.0
        for j, x in enumerate(r[b * D:(b + 1) * D]):
            if x != x:
                continue
            cnt += 1
            s += float(x)
            q += float(x) * float(x)
            if best is None or x > r[b * D + best]:
                best = j
            if worst is None or x < r[b * D + worst]:
                worst = j
        nan = np.float32(np.nan)
        out[b] = (r[b * D + best] if cnt else nan, r[b * D + worst] if cnt else nan, best or 0, worst or 0, cnt, 0, s, q)
    return out


def sum_bound(scores, D):
    """Per bin (bound on |sum - ref sum|, bound on |sumsq - ref sumsq|): two orders of the same additions, each within
    (n - 1) 2^-53 sum|terms| of the exact sum to first order; 2 n 2^-53 sum|terms| covers both and the higher orders."""
    r = np.ascontiguousarray(scores, dtype=np.float32)
    nb = n_bins(r.size, D)
    pad = np.zeros(nb * D, dtype=np.float64)
    pad[:r.size] = np.where(np.isnan(r), 0, r)
    m = np.abs(pad.reshape(nb, D))
    cnt = np.minimum(D, r.size - np.arange(nb) * D)
    return 2.0 * cnt * 2.0 ** -53 * m.sum(axis=1), 2.0 * cnt * 2.0 ** -53 * (m * m).sum(axis=1)


def _median(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    m = v.size
    with np.errstate(invalid="ignore"):
        return float(v[m // 2]) if m % 2 else float(0.5 * (v[m // 2 - 1] + v[m // 2]))


def _deviations(v, med):
    """|v - med|, 0 where v equals med (an infinite maximum does not deviate from an infinite median)."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(v == med, 0.0, np.abs(v - med))


def summary(bins, D):
    """am_trace_summary as a dict of SUMMARY_FIELDS."""
    b = np.asarray(bins, dtype=BIN_DTYPE)
    b = b[b["count"] > 0] if b.size else b
    nan = float("nan")
    out = dict(count=0, argmax=0, argmin=0, max=nan, min=nan, mean=nan, std=nan, median_max=nan, mad_max=nan, peak_z=nan)
    if b.size == 0:
        return out
    idx = np.flatnonzero(np.asarray(bins, dtype=BIN_DTYPE)["count"] > 0)
    hi, lo = b["max"].astype(np.float64), b["min"].astype(np.float64)
    i, j = int(np.argmax(hi)), int(np.argmin(lo))          # the first of equals
    cnt = int(b["count"].astype(np.uint64).sum())
    s = q = 0.0
    for x in b:                                              # bins in order, as the library adds them
        s += float(x["sum"])
        q += float(x["sumsq"])
    mean = s / cnt
    var = q / cnt - mean * mean
    med = _median(hi)
    mad = float("nan") if math.isnan(med) else _median(_deviations(hi, med))
    if math.isnan(mad):
        z = float("nan")
    elif mad > 0:
        z = (float(hi[i]) - med) / (1.4826 * mad)
    else:
        z = math.inf if float(hi[i]) > med else 0.0
    out.update(count=cnt, argmax=int(idx[i]) * D + int(b["argmax"][i]), argmin=int(idx[j]) * D + int(b["argmin"][j]),
               max=float(hi[i]), min=float(lo[j]), mean=mean, std=math.sqrt(var if var > 0 else 0.0) if var == var else float("nan"),
               median_max=med, mad_max=mad,
               peak_z=z)
    return out


def summary_loop(bins, D):
    """summary() as a plain loop over the records."""
    nan = float("nan")
    out = dict(count=0, argmax=0, argmin=0, max=nan, min=nan, mean=nan, std=nan, median_max=nan, mad_max=nan, peak_z=nan)
    tops, s, q = [], 0.0, 0.0
    for k, x in enumerate(bins):
        if int(x["count"]) == 0:
            continue
        if not tops or float(x["max"]) > out["max"]:
            out["max"], out["argmax"] = float(x["max"]), k * D + int(x["argmax"])
        if not tops or float(x["min"]) < out["min"]:
            out["min"], out["argmin"] = float(x["min"]), k * D + int(x["argmin"])
        tops.append(float(x["max"]))
        out["count"] += int(x["count"])
        s += float(x["sum"])
        q += float(x["sumsq"])
    if not tops:
        return out
    mean = s / out["count"]
    var = q / out["count"] - mean * mean
    med = _median(tops)
    if math.isnan(med):                                      # (+inf and -inf as the two middle maxima)
        mad = z = nan
    else:
        mad = _median([0.0 if t == med else abs(t - med) for t in tops])
        z = (out["max"] - med) / (1.4826 * mad) if mad > 0 else (math.inf if out["max"] > med else 0.0)
    out.update(mean=mean, std=math.sqrt(max(var, 0.0)) if var == var else nan, median_max=med, mad_max=mad, peak_z=z)
    return out


def same_bits(a, b):
    """Two record arrays agree in every byte (NaN max / min included)."""
    a, b = np.ascontiguousarray(a, dtype=BIN_DTYPE), np.ascontiguousarray(b, dtype=BIN_DTYPE)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def same_fields(a, b):
    """... in every field but sum / sumsq."""
    a, b = np.asarray(a, dtype=BIN_DTYPE), np.asarray(b, dtype=BIN_DTYPE)
    if a.shape != b.shape:
        return False
    return all(a[f].tobytes() == b[f].tobytes() for f in ("max", "min", "argmax", "argmin", "count", "reserved"))
