"""numpy f64 reference of edge matching (include/audiomatch.h, "edge matching") and the case builders its tests share.

Everything follows the header's definitions literally: the correlation is a direct np.correlate in f64 over the
sanitised span, the energies are cumulative sums of squares, the candidate mask and the record rule are spelled out.
"""
import numpy as np

HEAD, TAIL = 0, 1
NO_BEST, NO_SECOND, NONFINITE, BELOW_FLOOR = 1, 2, 4, 8
FLOOR_DB = 60                                                          # default of the option score_norm_floor_db
KAPPA = np.float32(0.5) * (np.float32(1.0) / np.float32(65535.0))     # the f32 constant of the down-mix

EDGE_DTYPE = np.dtype([("start", "<i8"), ("second", "<i8"), ("overlap", "<u8"), ("ncc", "<f8"), ("ncc_second", "<f8"),
                       ("gain", "<f8"), ("share", "<f8"), ("edge", "<u4"), ("flags", "<u4")])


def downmix(pcm):
    """(l as f32 + r as f32) * 0.5 * (1 / 65535), bit for bit as the library's down-mix."""
    p = np.asarray(pcm, dtype=np.int16).reshape(-1, 2)
    return ((p[:, 0].astype(np.int32) + p[:, 1]).astype(np.float32) * KAPPA).astype(np.float32)


def geometry(length, s, edge):
    """(n_lags, first_lag) of an edge, worked out from the definitions: head u < 0 and u + S <= len with L = S + u >= 1,
    tail u >= 0 and u + S > len with L = len - u >= 1."""
    if edge == HEAD:
        lo, hi = -(s - 1), min(-1, length - s)
    else:
        lo, hi = max(0, length - s + 1), length - 1
    n = max(0, hi - lo + 1)
    return n, lo


def span_of(x, s, edge):
    """The samples an edge reads: head x[0, min(len, S - 1)), tail x[max(0, len - S + 1), len)."""
    length = x.size
    return x[:min(length, s - 1)] if edge == HEAD else x[max(0, length - s + 1):]


def sanitise(span):
    """The span with its non-finite samples zeroed (f64), and their indices."""
    bad = np.flatnonzero(~np.isfinite(span))
    clean = np.where(np.isfinite(span), span, np.float32(0)).astype(np.float64)
    return clean, bad


def edge_terms(needle, x, edge):
    """Per lag of the edge in ascending u: L, c(u), E_n(u), E_x(u) in f64 and whether the overlap is free of non-finite
    samples.  x: the f32 haystack (the down-mix of an i16 one)."""
    n = np.asarray(needle, dtype=np.float64)
    s = n.size
    w, first = geometry(x.size, s, edge)
    if w == 0:
        z = np.zeros(0)
        return dict(first=first, L=np.zeros(0, np.int64), c=z, en=z, ex=z, clean=np.zeros(0, bool), full=z)
    span, bad = sanitise(np.asarray(span_of(x, s, edge), dtype=np.float32))
    assert span.size == w
    # np.correlate(a, v, "full")[m] = sum_k a[k + m - (S - 1)] v[k]: lag u = m - (S - 1) of v against a
    full = np.correlate(span, n, "full")
    j = np.arange(w)
    n2, x2 = n * n, span * span
    if edge == HEAD:
        L = j + 1
        c = full[:w]
        en = np.cumsum(n2[::-1])[L - 1]            # suffix sums of the needle
        ex = np.cumsum(x2)                         # prefix sums of the span
        clean = np.ones(w, bool) if bad.size == 0 else L <= bad.min()
    else:
        L = w - j
        c = full[s - 1:s - 1 + w]
        en = np.cumsum(n2)[L - 1]                  # prefix sums of the needle
        ex = np.cumsum(x2[::-1])[::-1]             # suffix sums of the span
        clean = np.ones(w, bool) if bad.size == 0 else j > bad.max()
    return dict(first=first, L=L.astype(np.int64), c=c, en=en, ex=ex, clean=clean, full=full)


def floor_ratio(floor_db=FLOOR_DB):
    return 10.0 ** (-float(floor_db) / 10.0)


def scores_of(t, floor_db=FLOOR_DB):
    """ncc(u) in f64 for the terms of edge_terms, and where the floor rule made it 0."""
    below = (t["ex"] == 0.0) | (t["ex"] < t["en"] * floor_ratio(floor_db))
    den = np.sqrt(t["en"] * t["ex"])
    live = ~below & (t["en"] > 0.0)
    ncc = np.zeros(t["c"].size)
    ncc[live] = t["c"][live] / den[live]
    return ncc, below


def candidates(t, needle, min_overlap, min_share):
    e_n = float(np.sum(np.asarray(needle, dtype=np.float64) ** 2))
    return (t["L"] >= int(min_overlap)) & (t["en"] >= float(np.float32(min_share)) * e_n) & t["clean"]


def coarse(needle, x, edge, min_overlap, min_share, floor_db=FLOOR_DB):
    """The f64 scores of every lag of the edge, NaN where the lag is no candidate; also the terms and the mask."""
    t = edge_terms(needle, x, edge)
    ncc, _ = scores_of(t, floor_db)
    mask = candidates(t, needle, min_overlap, min_share)
    out = np.where(mask, ncc, np.nan)
    return out, t, mask


def pick(scores, separation):
    """The record rule of am_probe_scores on an array with NaN for non-candidates: (best, second), None where none."""
    cand = np.flatnonzero(~np.isnan(scores))
    if cand.size == 0:
        return None, None
    best = int(cand[np.argmax(scores[cand])])             # (argmax: the first of equals)
    far = cand[np.abs(cand - best) >= int(separation)]
    second = int(far[np.argmax(scores[far])]) if far.size else None
    return best, second


def record(needle, x, edge, min_overlap, separation, min_share, floor_db=FLOOR_DB, on=None):
    """The edge's record in f64 (EDGE_DTYPE).  on: the array the two lags are chosen on (default: the reference's own
    scores); the exact values always come from the f64 terms."""
    needle = np.asarray(needle, dtype=np.float32)
    r = np.zeros((), dtype=EDGE_DTYPE)
    r["edge"] = edge
    r["ncc"] = r["ncc_second"] = r["gain"] = r["share"] = np.nan
    if not np.all(np.isfinite(needle)):
        r["flags"] = NONFINITE
        return r
    sc, t, _ = coarse(needle, x, edge, min_overlap, min_share, floor_db)
    best, second = pick(sc if on is None else np.asarray(on), separation if separation else min_overlap)
    if best is None:
        r["flags"] = NO_BEST | NO_SECOND
        return r
    ncc, below = scores_of(t, floor_db)
    e_n = float(np.sum(needle.astype(np.float64) ** 2))
    r["start"] = t["first"] + best
    r["overlap"] = t["L"][best]
    r["ncc"] = ncc[best]
    r["gain"] = t["c"][best] / t["en"][best] if t["en"][best] > 0 else 0.0
    r["share"] = t["en"][best] / e_n
    flags = BELOW_FLOOR if below[best] else 0
    if second is None:
        flags |= NO_SECOND
    else:
        r["second"] = t["first"] + second
        r["ncc_second"] = ncc[second]
    r["flags"] = flags
    return r


def naive_terms(needle, x, edge):
    """The definitions as plain loops over u (small sizes only): [(u, L, c, E_n, E_x)]."""
    n = np.asarray(needle, dtype=np.float64)
    xs = np.asarray(x, dtype=np.float64)
    s, length = n.size, xs.size
    out = []
    for u in range(-(s - 1), length):
        if edge == HEAD and u < 0 and u + s <= length:
            k, L = -u, s + u
            out.append((u, L, sum(xs[i] * n[k + i] for i in range(L)), sum(n[i] ** 2 for i in range(k, s)), sum(xs[i] ** 2 for i in range(L))))
        if edge == TAIL and u >= 0 and u + s > length:
            L = length - u
            out.append((u, L, sum(xs[u + i] * n[i] for i in range(L)), sum(n[i] ** 2 for i in range(L)), sum(xs[i] ** 2 for i in range(u, length))))
    return out


# ---- case builders ---------------------------------------------------------------------------------------------------
def white(n, seed, amp=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * amp).astype(np.float32)


PLANT = dict(S=6000, length=20000, noise=0.5, gain=0.8, head_missing=2500, tail_kept=2000, min_overlap=512, min_share=0.05)
PLANT_SEEDS = (1, 2, 3, 4, 5)


def planted(seed, p=PLANT):
    """(needle, haystack, head lag, tail lag): a white needle planted at gain p.gain with its first head_missing samples
    before the recording's start and only its first tail_kept samples before its end, in noise."""
    s, length = p["S"], p["length"]
    needle = white(s, 1000 + seed)
    x = white(length, 2000 + seed, p["noise"])
    k = p["head_missing"]
    x[:s - k] += np.float32(p["gain"]) * needle[k:]
    x[length - p["tail_kept"]:] += np.float32(p["gain"]) * needle[:p["tail_kept"]]
    return needle, x, -k, length - p["tail_kept"]


def clip_inside(seed, p=PLANT, clip=2000, at=1500):
    """(needle, haystack, head lag): the haystack is a clip of `clip` samples from inside the needle's span whose end is
    the needle's end -- the recording holds the needle's last `clip` samples and nothing else, so len < S and the head
    lag u = clip - S is in scope (cut at the head only)."""
    s = p["S"]
    needle = white(s, 3000 + seed)
    x = (np.float32(p["gain"]) * needle[s - clip:] + white(clip, 4000 + seed, 0.2)).astype(np.float32)
    return needle, x, clip - s


def noise_only(seed, p=PLANT):
    return white(p["S"], 5000 + seed), white(p["length"], 6000 + seed, p["noise"])


def silent_tenths(s, seed):
    """A white needle whose first and last tenth are digital silence."""
    n = white(s, seed)
    n[:s // 10] = 0
    n[s - s // 10:] = 0
    return n


def to_pcm(x, scale=9000.0):
    """An i16 stereo signal (frames, 2) whose two channels differ, from a float signal."""
    a = np.asarray(x, dtype=np.float64)
    l = np.clip(np.round(a * scale), -32768, 32767).astype(np.int16)
    r = np.clip(np.round(a * scale * 0.5 + 3), -32768, 32767).astype(np.int16)
    return np.stack([l, r], axis=1)


def case_signals(s, length, seed):
    """(needle f32, pcm haystack (frames, 2)): the f32 haystack of a case is downmix(pcm), so one reference serves both
    sample formats.  The needle lies at both edges, cut about in half where it fits, over noise."""
    rng = np.random.default_rng(seed)
    needle = rng.standard_normal(s).astype(np.float32)
    x = rng.standard_normal(length) * 0.5
    kh = min(length, (s + 1) // 2)          # the needle's last kh samples at the start
    x[:kh] += 0.8 * needle[s - kh:]
    kt = min(length, s // 2)                # its first kt samples at the end
    if kt:
        x[length - kt:] += 0.8 * needle[:kt]
    return needle, to_pcm(x)


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))
