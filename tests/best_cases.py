"""Designed score arrays for the k-best selection (am_best.hip) and a numpy model of its threshold ladder.

`ladder` is the single place in the tests that mirrors the head comment of am_best.hip and the host logic of
`best_select` / `pick`: the order-preserving height key, the plateau rule for maxima, M = max(8k, 4096), the one
refinement of a crowded bin, the eightfold descent and the fallback past 2^20 candidates.  A change of those rules in the
library is a change here.  tests/test_best_cases_host.py holds every family below to the branch it is designed to reach
(model and checker only); tests/test_gpu_best_ladder.py compares the library with the checker on them, bit for bit.

A family is a function returning (name, y, [(k, min_prominence, min_distance), ...]); CASES maps a name to its builder.
Pure numpy: no GPU, no library."""
import functools
from collections import namedtuple

import numpy as np

BINS = 4096                 # kBestBins: 12 key bits per histogram level
CAP = 1 << 20               # kBestCap: candidates before the finite fallback
TRANS_CAP = 4096            # kBestTransCap: transitions the scan lists itself
F32 = np.float32


# ---------------------------------------------------------------------------
# the model
def height_keys(h):
    """height_key of am_best.hip: h + 0.0f (so -0.0 and +0.0 are one key), then the sign fold."""
    u = (np.asarray(h, dtype=F32) + F32(0.0)).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def maxima(y):
    """(start, end, height) of every local maximum by max_at's rule: a run of equal scores (== : -0.0 equals +0.0)
    strictly above its finite left and right neighbours, itself finite; the height is the run's first score."""
    y = np.asarray(y, dtype=F32)
    n = y.size
    if n < 3:
        z = np.zeros(0, dtype=np.int64)
        return z, z, np.zeros(0, dtype=F32)
    change = np.ones(n, dtype=bool)
    change[1:] = ~(y[1:] == y[:-1])
    starts = np.flatnonzero(change)
    ends = np.append(starts[1:], n)
    v = y[starts]
    fin = np.isfinite(v)
    r = np.arange(1, starts.size - 1)
    ok = fin[r - 1] & fin[r] & fin[r + 1] & (v[r - 1] < v[r]) & (v[r + 1] < v[r])
    r = r[ok]
    return starts[r].astype(np.int64), ends[r].astype(np.int64), v[r]


def transitions(y):
    """The i in [0, n] with finite(y[i]) != finite(y[i - 1]), y[-1] and y[n] counting as finite (BestScan)."""
    f = np.concatenate([[True], np.isfinite(np.asarray(y, dtype=F32)), [True]])
    return np.flatnonzero(f[1:] != f[:-1])


Ladder = namedtuple("Ladder", "rounds refined fallback total ntrans keys")
# rounds: [(tau, count, fresh)] per listing round; refined: [(bin, occupied second-level bins)] per best_refine launch;
# fallback: the finite whole-array pick is taken (no round is listed for it); keys: the keys of all maxima


def ladder(y, k):
    """The listing rounds best_select runs when no round yields k survivors (rounds_needed says where it stops)."""
    _, _, h = maxima(y)
    keys = height_keys(h)
    total = int(keys.size)
    ntrans = int(transitions(y).size)
    finite = ntrans == 0
    hist = np.bincount(keys >> 20, minlength=BINS).astype(np.int64)
    state = {"bin": -1, "hist2": None}
    refined = []

    def pick(M):
        cum = 0
        for b in range(BINS - 1, -1, -1):
            hb = int(hist[b])
            if cum + hb < M:
                cum += hb
                continue
            if cum + hb > 8 * M and hb > 1 and state["bin"] != b:
                inside = keys[(keys >> 20) == b]
                state["hist2"] = np.bincount((inside >> 8) & 0xFFF, minlength=BINS).astype(np.int64)
                state["bin"] = b
                refined.append((b, int(np.count_nonzero(state["hist2"]))))
            if state["bin"] == b:
                for q in range(BINS - 1, -1, -1):
                    cum += int(state["hist2"][q])
                    if cum >= M or q == 0:
                        return (b << 20) | (q << 8), cum
            return b << 20, cum + hb
        return 0, cum

    rounds, fallback = [], False
    M, listed = max(8 * int(k), 4096), 0
    while total:
        tau, count = pick(M)
        if count > CAP and finite:
            fallback = True
            break
        rounds.append((tau, count, count - listed))
        listed = count
        if listed >= total or tau == 0:
            break
        M = max(8 * M, listed + 1)
    return Ladder(rounds, refined, fallback, total, ntrans, keys)


def rounds_needed(taus, full, k):
    """The listing rounds best_select runs for k (counted from 1): the first round r at which at least k peaks of the
    checker's full list `full` ((start, end, height, prominence) tuples) have key >= taus[r - 1], else the last round.
    (The survivors among the candidates of height >= tau are exactly the full list's peaks of height >= tau.)"""
    keys = height_keys(np.array([p[2] for p in full], dtype=F32)) if len(full) else np.zeros(0, dtype=np.uint32)
    for r, tau in enumerate(taus):
        if int(np.count_nonzero(keys >= np.uint32(tau))) >= k:
            return r + 1
    return len(taus)


# ---------------------------------------------------------------------------
# the families
N18 = 1 << 18


def _crowded_scores(n, seed):
    return (1.0 + 0.01 * np.random.default_rng(seed).standard_normal(n)).astype(F32)


def crowded():
    """1 + 0.01 N(0, 1): about 87 000 maxima, about 76 000 of them in key bin 3064 ([1.0, 1.125)): refine on the first pick."""
    return "crowded", _crowded_scores(N18, 21), [(10, 0.0, 0), (40, 0.052, 0), (200, 0.0, 700), (25, 0.03, 3000)]


def crowded_negated():
    """The negation of crowded: every key from the ~u half, the crowd in bin 1032."""
    return "crowded_negated", -_crowded_scores(N18, 21), [(10, 0.0, 0), (40, 0.052, 0), (200, 0.0, 700)]


def crowded_minus_two():
    """crowded - 2: negative heights around -1."""
    return "crowded_minus_two", (_crowded_scores(N18, 21) - F32(2.0)).astype(F32), [(10, 0.0, 0), (40, 0.052, 0), (200, 0.0, 700)]


RAMP_HITS = 12


def _ramp(first, last, dip, seed=31, n=N18):
    """1 + 0.1 t/n + 0.002 sin(0.9 t) + 2e-4 N with twelve clean hits (-dip over +-30 scores, +0.03 at the hit) between
    the fractions first and last of the ramp: the ripple crests above a hit are taller than it and not prominent."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = 1.0 + 0.1 * t / n + 0.002 * np.sin(0.9 * t) + 2e-4 * rng.standard_normal(n)
    for p in np.linspace(first * n, last * n, RAMP_HITS).astype(np.int64) + 17:
        x[p - 30:p + 31] -= dip
        x[p] += 0.03
    return x.astype(F32)


def ramp():
    """Hits of height ramp + 0.02 at 0.20 .. 0.50 of the ramp: with min_prominence 0.02 the first round (the about 4100
    tallest crests) yields none of them, the second all twelve."""
    return "ramp", _ramp(0.20, 0.50, 0.01), [(RAMP_HITS, 0.02, 0), (RAMP_HITS, 0.02, 50), (5, 0.0, 4000)]


def ramp_low():
    """Hits level with the ramp (-0.03, +0.03) in its lowest twentieth: more than 32 768 crests are taller than the lowest
    hit, so k = 12 needs the third round, whose tau is 0."""
    return "ramp_low", _ramp(0.005, 0.05, 0.03), [(RAMP_HITS, 0.02, 0), (RAMP_HITS, 0.02, 50), (3, 0.02, 0)]


def _one_key_scores(n, seed):
    """Troughs 0.5 + j 2^-20 at even, maxima 1 + j 2^-23 (j < 256) at odd indices: every maximum shares key bits
    8..31.  j = 8 * (trailing zeros of the maximum's number) + (3 random bits), so a maximum of level z has a taller one
    within 2^(z + 2) maxima: many ties, and the checker's prominence walks stay short at any n."""
    rng = np.random.default_rng(seed)
    m = n // 2
    i = np.arange(1, m + 1, dtype=np.int64)
    tz = np.zeros(m, dtype=np.int64)
    for b in range(1, 24):
        tz += (i % (1 << b)) == 0
    j = 8 * tz + rng.integers(0, 8, m)
    assert int(j.max()) < 256
    y = np.empty(n, dtype=np.float64)
    y[0::2] = 0.5 + rng.integers(0, 256, (n + 1) // 2) * 2.0 ** -20
    y[1::2] = 1.0 + j[:n // 2] * 2.0 ** -23
    return y.astype(F32)


def one_key():
    """65 535 maxima in ONE second-level bin: refine cannot split it, the first round lists all of them."""
    n = 1 << 17
    return "one_key", _one_key_scores(n, 41), [(10, 0.0, 0), (300, 0.0, 0), (20, 0.0, 5000), (50, 0.4999, 0)]


def around_zero():
    """j * 2^-149, j in -40..40: denormals of both signs, +0.0 and -0.0 (as maxima and inside plateaus), 81 heights
    shared by about 19 000 maxima."""
    n = 1 << 16
    rng = np.random.default_rng(51)
    j = rng.integers(-40, 41, n)
    y = (j * 2.0 ** -149).astype(F32)
    neg = (j == 0) & (rng.integers(0, 2, n) == 1)
    y[neg] = F32(-0.0)
    return "around_zero", y, [(10, 0.0, 0), (500, 0.0, 0), (100, 30 * 2.0 ** -149, 0), (50, 0.0, 300)]


EDGE_VALUES = [F32(4.0), np.nextafter(F32(4.0), F32(0)), F32(2.0 * (1 + 2.0 ** -12)), np.nextafter(F32(2.0 * (1 + 2.0 ** -12)), F32(0)),
               F32(2.0), np.nextafter(F32(2.0), F32(0))]


def _edges(n, counts, seed):
    """Maxima at odd indices drawn from EDGE_VALUES (counts[i] of value i, the rest spread over values 2..5 by
    `counts[-1]` weights) over troughs near 1."""
    rng = np.random.default_rng(seed)
    m = n // 2 - (1 if n % 2 == 0 else 0)              # maxima: the odd indices below n - 1
    fixed, weights = counts
    pick = np.concatenate([np.full(c, i) for i, c in enumerate(fixed)])
    rest = rng.choice(np.arange(len(fixed), 6), size=m - pick.size, p=weights)
    idx = rng.permutation(np.concatenate([pick, rest]))
    y = (1.0 + 0.01 * rng.random(n)).astype(F32)
    y[1:2 * m:2] = np.array(EDGE_VALUES, dtype=F32)[idx]
    return y


def bin_edges():
    """600 maxima each at 4.0 and below it, 1500 each at 2 (1 + 2^-12) and below it, the rest at 2.0 and below it: bin
    0xC00 is refined, the first tau falls between the second-level bins 8 and 7, the second on 2.0 itself."""
    return "bin_edges", _edges(N18, ((600, 600, 1500, 1500), (0.5, 0.5)), 61), [(10, 0.0, 0), (500, 0.0, 0), (3000, 0.0, 0), (100, 0.0, 40)]


def bin_edges_4096():
    """Exactly 4096 = M maxima in the top bin: `cum + hist[b] < M` fails at equality, tau is the top bin's edge."""
    return "bin_edges_4096", _edges(1 << 15, ((4096,), (0.2,) * 5), 62), [(10, 0.0, 0), (512, 0.0, 0), (512, 0.0, 5)]


def bin_edges_4095():
    """4095 maxima in the top bin: one short of M, the first round takes the next bin too."""
    return "bin_edges_4095", _edges(1 << 15, ((4095,), (0.2,) * 5), 63), [(10, 0.0, 0), (512, 0.0, 0), (512, 0.0, 5)]


NONFINITE = [F32(np.nan), F32(np.inf), F32(-np.inf)]


def _gaps(y, runs, seed, first=False, last=False):
    rng = np.random.default_rng(seed)
    n = y.size
    for p in rng.choice(np.arange(8, n - 8, 8), size=runs, replace=False) + rng.integers(0, 4, runs):
        y[p:p + rng.integers(1, 4)] = NONFINITE[rng.integers(0, 3)]
    if first:
        y[0] = NONFINITE[seed % 3]
    if last:
        y[n - 1] = NONFINITE[(seed + 1) % 3]
    return y


def many_gaps(n, crowd, first, last, seed):
    """2500 runs of NaN, +inf and -inf, 1 to 3 long: about 5000 transitions, past the 4096 the scan lists itself."""
    y = _crowded_scores(n, seed) if crowd else np.random.default_rng(seed).standard_normal(n).astype(F32)
    name = "many_gaps_%d_%s%s%s" % (n, "crowded" if crowd else "white", "_first" if first else "", "_last" if last else "")
    return name, _gaps(y, 2500, seed + 1, first, last), [(10, 0.0, 0), (400, 0.02 if crowd else 2.0, 0)]


ENDS_N = (3, 1024, 1025, 2048)
ENDS_WHERE = ("first", "last", "both", "nowhere")


def ends(n, where):
    """A non-finite score at index 0, at n - 1, at both or nowhere, n around and on multiples of the 1024-score tile."""
    y = np.random.default_rng(70 + n).standard_normal(n).astype(F32)
    if where in ("first", "both"):
        y[0] = NONFINITE[n % 3]
    if where in ("last", "both"):
        y[n - 1] = NONFINITE[(n + 1) % 3]
    return "ends_%d_%s" % (n, where), y, [(5, 0.0, 0), (3, 0.5, 0)]


PAST_CAP_N = (1 << 21) + (1 << 13)


def past_cap(with_nan):
    """The one-key design with just over 2^20 maxima.  All finite: the fallback to the whole-array pick.  With one NaN:
    the descent that lists every candidate.  (min_distance = n: every two positions are closer than that, so only the
    first peak of the order survives.)"""
    n = PAST_CAP_N
    y = _one_key_scores(n, 81)
    if with_nan:
        y[n // 2] = np.nan
    return "past_cap_nan" if with_nan else "past_cap_finite", y, [(10, 0.0, 0), (3, 0.0, n)]


SMALL = [crowded, crowded_negated, crowded_minus_two, ramp, ramp_low, one_key, around_zero, bin_edges, bin_edges_4096, bin_edges_4095]
MANY_GAPS = [(128 * 1024 - 1, False, True, False, 91), (128 * 1024, False, False, True, 92), (128 * 1024 + 1, True, False, False, 93),
             (128 * 1024, True, True, False, 94), (128 * 1024 - 1, True, False, True, 95)]

CASES = {f.__name__: f for f in SMALL}
for _a in MANY_GAPS:
    CASES["many_gaps_%d_%s%s%s" % (_a[0], "crowded" if _a[1] else "white", "_first" if _a[2] else "", "_last" if _a[3] else "")] = \
        functools.partial(many_gaps, *_a)
for _n in ENDS_N:
    for _w in ENDS_WHERE:
        CASES["ends_%d_%s" % (_n, _w)] = functools.partial(ends, _n, _w)
BIG = {"past_cap_finite": functools.partial(past_cap, False), "past_cap_nan": functools.partial(past_cap, True)}

FAMILY_OF = {name: ("many_gaps" if name.startswith("many_gaps") else "ends" if name.startswith("ends") else name) for name in CASES}


@functools.lru_cache(maxsize=None)
def case(name):
    """(name, y, triples) of a case at or below 2^18 scores, built once (y is read-only)."""
    nm, y, triples = CASES[name]()
    assert nm == name and y.dtype == F32 and y.size <= N18
    y.setflags(write=False)
    return nm, y, triples


# crowded and ramp under every (peak_filter_order, distance_rule) of policy_cases.PEAK_POLICIES, with a prominence bound
# and a min_distance that both remove peaks.  The first round of ramp holds the about 4100 tallest crests, 300 apart at
# most 100 of them survive: k = 200 needs the second round under either order, and under order 1 the crests that fail
# the bound still suppress their neighbours (the two orders keep different lists).
POLICY_TRIPLES = {"crowded": [(30, 0.03, 1500)], "ramp": [(200, 0.004, 300)]}
