"""The checker of envelope matching (am_envelope*, am_envelope_scores*, am_envelope_pick, am_match_envelope*): numpy,
Python integers or int64, and the formulas of include/audiomatch.h ("envelope matching") literally.  Also the seeded
signals the tests share.  A module, not a test file; the tests import it."""
import math

import numpy as np

STEPS_PER_DB, MAX_LEVEL, ABSENT, NO_Q = 8, 1023, 0xFFFF, 0xFFFFFFFF
MAX_PPM, MAX_FRAMES, MAX_NEEDLES, MAX_STEPS = 250000, 16384, 257, 128
KAPPA = np.float32(0.5) * (np.float32(1.0) / np.float32(65535.0))     # the f32 constant of the down-mix
PICK_DTYPE = np.dtype([("frame", "<u8"), ("pos", "<f8"), ("score", "<f4"), ("q", "<u4")])
HIT_DTYPE = np.dtype([("start", "<u8"), ("length", "<u8"), ("drift_ppm", "<f8"), ("score", "<f4"), ("q", "<u4")])


def llround(x):
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def inc_of(d_ppm):
    return llround(4294967296.0 / (1.0 + d_ppm * 1e-6))


def frame_starts(length, frame_log2, d_ppm=0.0):
    """a_j for every j with a_j + F <= length (Python integers)."""
    f = 1 << frame_log2
    h, inc, out, j = f // 2, inc_of(d_ppm), [], 0
    while True:
        a = (j * h * inc + (1 << 31)) >> 32
        if a + f > length:
            return out
        out.append(a)
        j += 1


def mono(x):
    """The samples as f32: an f32 array as it is, an i16 (frames, 2) array through the bit-exact down-mix."""
    a = np.asarray(x)
    if a.dtype == np.int16:
        a = a.reshape(-1, 2)
        return (a[:, 0].astype(np.int32) + a[:, 1].astype(np.int32)).astype(np.float32) * KAPPA
    return a.astype(np.float32)


def window(f):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(f, dtype=np.float64) / f)


def levels(x, frame_log2, edges, floor_db=80.0, d_ppm=0.0):
    """(u, eight_v): the (B, J) uint16 levels of a signal and the f64 values 8 v they were rounded from (NaN in absent
    frames)."""
    s = mono(x).astype(np.float64)
    f, nb = 1 << frame_log2, len(edges) - 1
    starts = frame_starts(len(s), frame_log2, d_ppm)
    u = np.zeros((nb, len(starts)), dtype=np.uint16)
    ev = np.full((nb, len(starts)), np.nan)
    w = window(f)
    p0 = (f / 4.0) ** 2 * 10.0 ** (-floor_db / 10.0)
    for j, a in enumerate(starts):
        fr = s[a:a + f]
        if not np.all(np.isfinite(fr)):
            u[:, j] = ABSENT
            continue
        spec = np.fft.rfft(w * fr)
        pw = spec.real ** 2 + spec.imag ** 2
        for b in range(nb):
            v = 10.0 * math.log10((float(pw[edges[b]:edges[b + 1]].sum()) + p0) / p0)
            ev[b, j] = STEPS_PER_DB * v
            u[b, j] = min(llround(STEPS_PER_DB * v), MAX_LEVEL)
    return u, ev


def near_half(eight_v, eps=1e-6):
    """The cells whose 8 v lies within eps of a half-integer: where an implementation may differ by 1."""
    fr = eight_v - np.floor(eight_v)
    return np.abs(fr - 0.5) <= eps


def edges_log(sr, frame_log2, lo_hz, hi_hz, n_bands):
    f = 1 << frame_log2
    edges, prev = [], -1
    for b in range(n_bands + 1):
        e = max(int(math.floor(lo_hz * (hi_hz / lo_hz) ** (b / n_bands) * f / sr + 0.5)), prev + 1)
        edges.append(e)
        prev = e
    return edges


def xcorr_int(e, n):
    """sum_j n[j] e[t + j] for every t, exact int64: np.correlate where it is quick, else through an f64 FFT whose
    distance from an integer is asserted."""
    e64, n64 = np.asarray(e, dtype=np.int64), np.asarray(n, dtype=np.int64)
    t = e64.size - n64.size + 1
    if t * n64.size <= 40_000_000:
        return np.correlate(e64, n64, "valid")
    m = 1 << int(e64.size + n64.size).bit_length()
    r = np.fft.irfft(np.fft.rfft(e64.astype(np.float64), m) * np.conj(np.fft.rfft(n64.astype(np.float64), m)), m)[:t]
    k = np.rint(r)
    assert np.max(np.abs(r - k)) < 0.05
    return k.astype(np.int64)


def scores_one(n, e):
    """score_q[0 .. T_q) of one (B, J) needle matrix against the (B, Jh) haystack matrix, as f32."""
    n, e = np.asarray(n, dtype=np.uint16), np.asarray(e, dtype=np.uint16)
    nb, j = n.shape
    jh = e.shape[1]
    tq = max(jh - j + 1, 0)
    if tq == 0:
        return np.zeros(0, dtype=np.float32)
    assert n[n != ABSENT].max(initial=0) <= MAX_LEVEL and e[e != ABSENT].max(initial=0) <= MAX_LEVEL
    n_absent = bool(np.any(n == ABSENT))
    e_abs = np.any(e == ABSENT, axis=0).astype(np.int64)
    nn = np.where(n == ABSENT, 0, n).astype(np.int64)
    ee = np.where(e == ABSENT, 0, e).astype(np.int64)
    num = np.zeros(tq, dtype=np.int64)
    dd = np.zeros(tq, dtype=np.int64)
    big_e = 0
    for b in range(nb):
        xc = xcorr_int(ee[b], nn[b])
        c1 = np.concatenate([[0], np.cumsum(ee[b])])
        c2 = np.concatenate([[0], np.cumsum(ee[b] * ee[b])])
        s1, s2 = c1[j:j + tq] - c1[:tq], c2[j:j + tq] - c2[:tq]
        n1, n2 = int(nn[b].sum()), int((nn[b] * nn[b]).sum())
        num += j * xc - n1 * s1
        dd += j * s2 - s1 * s1
        big_e += j * n2 - n1 * n1
    assert big_e < 2 ** 53 and int(dd.max(initial=0)) < 2 ** 53 and int(np.abs(num).max(initial=0)) < 2 ** 53
    ca = np.concatenate([[0], np.cumsum(e_abs)])
    absent = (ca[j:j + tq] - ca[:tq]) > 0
    out = np.zeros(tq, dtype=np.float32)
    ok = (dd != 0) & (big_e != 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.sqrt(np.float64(big_e) * dd.astype(np.float64))
        out[ok] = (num.astype(np.float64)[ok] / den[ok]).astype(np.float32)
    out[absent] = np.nan
    if n_absent:
        out[:] = np.nan
    return out


def scores(needles, e):
    """(z, qi) of a list of needle matrices against e."""
    jh = np.asarray(e).shape[1]
    n_out = max([jh - np.asarray(n).shape[1] + 1 for n in needles if jh >= np.asarray(n).shape[1]], default=0)
    z = np.full(n_out, np.nan, dtype=np.float32)
    qi = np.full(n_out, NO_Q, dtype=np.uint32)
    for q, n in enumerate(needles):
        s = scores_one(n, e)
        for t in range(s.size):
            if s[t] == s[t] and (qi[t] == NO_Q or s[t] > z[t]):
                z[t], qi[t] = s[t], q
    return z, qi


def pick(z, qi, min_score, separation):
    """am_envelope_pick: an array of PICK_DTYPE."""
    z = np.asarray(z, dtype=np.float32)
    n, out = z.size, []
    for t in range(n):
        v = z[t]
        if v != v or not v >= np.float32(min_score):
            continue
        lo, hi = max(0, t - separation), min(n - 1, t + separation)
        if any((z[u] > v) or (z[u] == v and u < t) for u in range(lo, hi + 1) if u != t):
            continue
        e = 0.0
        if 0 < t < n - 1 and z[t - 1] == z[t - 1] and z[t + 1] == z[t + 1]:
            a, b, c = float(z[t - 1]), float(v), float(z[t + 1])
            den = a - 2.0 * b + c
            if den < 0.0:
                e = min(0.5, max(-0.5, (a - c) / (2.0 * den)))
        out.append((t, t + e, v, qi[t]))
    return np.array(out, dtype=PICK_DTYPE)


def grid_drifts(centre_ppm, max_ppm, steps):
    if steps == 0:
        return [float(centre_ppm)]
    return [centre_ppm + max_ppm * float(q - steps) / float(steps) for q in range(2 * steps + 1)]


def hits_from(needle_levels, hay_levels, drifts, needle_len, hay_len, frame_log2, min_score):
    """The composition behind the levels: scores, the pick with separation J_K, the records (HIT_DTYPE)."""
    z, qi = scores(needle_levels, hay_levels)
    k = (len(drifts) - 1) // 2
    picks = pick(z, qi, min_score, needle_levels[k].shape[1])
    h = (1 << frame_log2) // 2
    out = np.zeros(picks.size, dtype=HIT_DTYPE)
    for i, p in enumerate(picks):
        d = drifts[int(p["q"])]
        out[i] = (min(max(llround(float(p["pos"]) * h), 0), hay_len - 1), llround(needle_len * (1.0 + d * 1e-6)), d, p["score"], p["q"])
    return out, z, qi


def match(needle, hay, frame_log2, edges, floor_db, centre_ppm, max_ppm, steps, min_score):
    """am_match_envelope from the samples: (hits, needle level matrices, haystack level matrix)."""
    drifts = grid_drifts(centre_ppm, max_ppm, steps)
    nl = [levels(needle, frame_log2, edges, floor_db, d)[0] for d in drifts]
    hl = levels(hay, frame_log2, edges, floor_db, 0.0)[0]
    hits, _, _ = hits_from(nl, hl, drifts, len(mono(needle)), len(mono(hay)), frame_log2, min_score)
    return hits, nl, hl


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ---- seeded signals ----------------------------------------------------------------------------------------------------
def burst_tones(rng, n, sr, amp=0.25):
    """Tone bursts of 60 - 250 ms at random pitches between 200 and 5000 Hz with gaps of 20 - 200 ms, raised-cosine edges."""
    x = np.zeros(n)
    at = 0
    while at < n:
        ln = int(rng.uniform(0.06, 0.25) * sr)
        f = 200.0 * (5000.0 / 200.0) ** rng.uniform()
        t = np.arange(ln) / sr
        env = np.minimum(1.0, np.minimum(np.arange(ln), np.arange(ln)[::-1]) / (0.005 * sr))
        seg = amp * np.sin(2.0 * np.pi * f * t + rng.uniform(0, 2 * np.pi)) * (0.5 - 0.5 * np.cos(np.pi * env))
        m = min(ln, n - at)
        x[at:at + m] += seg[:m]
        at += ln + int(rng.uniform(0.02, 0.2) * sr)
    return x


def stretch(x, d_ppm):
    """The signal as it sounds when played (1 + d 1e-6) times as long: y[i] = x(i / (1 + d 1e-6)), linear interpolation."""
    r = 1.0 + d_ppm * 1e-6
    m = int(math.floor((len(x) - 1) * r)) + 1
    return np.interp(np.arange(m) / r, np.arange(len(x)), x)


def random_allpass(rng, x, sections=6):
    """A cascade of second-order all-pass sections with random poles (radius 0.5 - 0.9): every phase moves, no level does."""
    from scipy.signal import lfilter
    y = np.asarray(x, dtype=np.float64)
    for _ in range(sections):
        r, th = rng.uniform(0.5, 0.9), rng.uniform(0.1, 3.0)
        a = np.array([1.0, -2.0 * r * math.cos(th), r * r])
        y = lfilter(a[::-1], a, y)
    return y


def detection_design(sr=44100, needle_s=10.0, hay_s=60.0, seed=2025):
    """The design of the issue's prototype: a burst-tone needle, a haystack of other bursts at equal level plus noise, the
    needle planted at +30 000 ppm and -20 000 ppm through a random all-pass and at 0 ppm as it is.
    (needle, hay, plants): plants = [(start sample, drift ppm)]."""
    rng = np.random.default_rng(seed)
    needle = burst_tones(rng, int(needle_s * sr), sr)
    hay = burst_tones(rng, int(hay_s * sr), sr) + 0.01 * rng.standard_normal(int(hay_s * sr))
    plants = []
    for at_s, d, ap in ((6.0, 30000.0, True), (24.0, -20000.0, True), (43.0, 0.0, False)):
        y = stretch(needle, d)
        if ap:
            y = random_allpass(rng, y)
        at = int(at_s * sr)
        hay[at:at + len(y)] += y
        plants.append((at, d))
    return needle.astype(np.float32), hay.astype(np.float32), plants


def composition_design(sr=16000, seed=77):
    """A 3 s burst-tone needle planted at +3 % (linear interpolation) at 11 s of 30 s of noise plus bursts."""
    rng = np.random.default_rng(seed)
    needle = burst_tones(rng, 3 * sr, sr)
    hay = 0.5 * burst_tones(rng, 30 * sr, sr) + 0.01 * rng.standard_normal(30 * sr)
    y = stretch(needle, 30000.0)
    at = 11 * sr
    hay[at:at + len(y)] += y
    return needle.astype(np.float32), hay.astype(np.float32), at


def to_s16_stereo(x):
    """An i16 (frames, 2) signal whose down-mix is near x: both channels round(x 32767)."""
    v = np.clip(np.rint(np.asarray(x, dtype=np.float64) * 32767.0), -32768, 32767).astype(np.int16)
    return np.ascontiguousarray(np.stack([v, v], axis=1))
