"""Designed score arrays for the score traces (include/audiomatch.h, "score traces"), each with the claim it makes.

A case is a rule that, for a bin length D and a score count n, builds the array and says per bin what the record must
hold.  Every value is an integer-valued f32 with |v| <= 2^12 (or a NaN, a zero of either sign, +-inf) and n <= 2^22, so
every f64 sum is exact in whatever order it is added: the sums compare bit for bit with trace_ref's.  The background is
integers of [-100, 100]; the deciding scores are +-TOP.  Where a bin has room, a case that decides the maximum at offset
p decides the minimum at the mirrored offset L - 1 - p with the negated values, so both halves of the record are under
test in one array.

CASES[name] = (rule, claim text); build(name, D, n, slice_len) -> (scores, claims), claims[b] = dict of the record
fields the case pins for bin b (argmax, argmin, count, max_bits, min_bits); a key that starts with '_' says where the case
put its deciding scores (test_trace_host.py checks that the designs reach what they are for)."""
import numpy as np

TOP = 4096.0
NAN = np.float32(np.nan)


def bits(v):
    return int(np.float32(v).view(np.uint32))


def _background(D, n, salt):
    rng = np.random.default_rng(1000003 * salt + 31 * D + n)
    return rng.integers(-100, 101, size=n).astype(np.float32)


def _mirror(x, lo, L, p, claim, vmax=TOP):
    """+vmax at offset p of the bin [lo, lo + L) and -vmax at the mirrored offset (when that is another one)."""
    x[lo + p] = vmax
    claim.update(argmax=p, max_bits=bits(vmax))
    pm = L - 1 - p
    if pm != p:
        x[lo + pm] = -vmax
        claim.update(argmin=pm, min_bits=bits(-vmax))


def _slices(L, SL):
    return (L + SL - 1) // SL


# ---- the rules: fill bin b = x[lo, lo + L) and its claim ----------------------------------------------------------
def first_offset(x, b, lo, L, D, SL, claim):
    _mirror(x, lo, L, 0, claim)                       # ... and the minimum at the last offset


def last_offset(x, b, lo, L, D, SL, claim):
    _mirror(x, lo, L, L - 1, claim)                   # the ragged last bin: its own last offset


def _slice_first(k):
    def rule(x, b, lo, L, D, SL, claim):
        s = (b + k) % _slices(L, SL)                  # k = 0 .. 5 and bins 0 .. 2: every slice of a six-slice bin decides once
        claim["_slice"] = s
        _mirror(x, lo, L, s * SL, claim)
    return rule


def _slice_last(k):
    def rule(x, b, lo, L, D, SL, claim):
        s = (b + k) % _slices(L, SL)
        claim["_slice"] = s
        _mirror(x, lo, L, min(L, (s + 1) * SL) - 1, claim)   # (the ragged last slice: its own last offset)
    return rule


def _group_edge(g):
    def rule(x, b, lo, L, D, SL, claim):
        k = 1 + b                                    # the last offset of group k - 1 (even bins) / the first of group k (odd)
        p = min(L - 1, k * g - 1 + (b & 1))
        _mirror(x, lo, L, p, claim)
    return rule


TWICE = ("1", "3", "64", "256", "slice", "slice+1")   # the distances between the two equal extremes


def _twice(which, sign):
    """The same maximum (sign +1) or minimum (sign -1) twice, `which` scores apart: the earlier one wins.  1 and 3 put the
    two in two lanes, 64 and 256 in two steps of a wave (256: the same lane and place), slice and slice + 1 in two
    slices.  In a bin longer than a slice the pair always straddles a slice boundary (the boundary moves with the bin),
    so the two meet only when the partials are folded.  A bin too short for the distance takes the largest that fits."""
    def rule(x, b, lo, L, D, SL, claim):
        want = {"slice": SL, "slice+1": SL + 1}.get(which) or int(which)
        fits = [d for d in (1, 3, 64, 256, SL, SL + 1) if d <= want and d + 1 <= L]
        if not fits:
            return
        d = max(fits)
        if L > SL:
            B = SL * (1 + b % (_slices(L, SL) - 1))   # p < B <= p + d
            p = min(B - 1 - (d - 1) // 2, L - 1 - d)
        else:
            p = (L - 1 - d) // 2
        x[lo + p] = x[lo + p + d] = sign * TOP
        claim["_pair"] = (p, p + d)
        if sign > 0:
            claim.update(argmax=p, max_bits=bits(TOP))
        else:
            claim.update(argmin=p, min_bits=bits(-TOP))
    return rule


def nan_at_winner(x, b, lo, L, D, SL, claim):
    """A NaN exactly where the winner would be: the runner-up wins, the NaN is not counted."""
    if L < 5:
        x[lo] = NAN
        claim.update(count=L - 1)
        return
    p = (L - 4) // 3                                   # p + 1 < pm - 1
    x[lo + p] = NAN
    x[lo + p + 1] = TOP - 1
    pm = L - 1 - p
    x[lo + pm] = NAN
    x[lo + pm - 1] = -(TOP - 1)
    claim.update(argmax=p + 1, argmin=pm - 1, count=L - 2, max_bits=bits(TOP - 1), min_bits=bits(-(TOP - 1)))


def all_nan_bin(x, b, lo, L, D, SL, claim):
    """Odd bins (and a lone bin) are all NaN: count 0, NaN extremes, offsets 0, sums +0.0."""
    if b & 1 or (lo == 0 and L == x.size):
        x[lo:lo + L] = NAN
        claim.update(count=0, argmax=0, argmin=0, max_bits=bits(NAN), min_bits=bits(NAN), sum_bits=0, sumsq_bits=0)
    else:
        _mirror(x, lo, L, L // 2, claim)


def _zeros(first, second):
    def rule(x, b, lo, L, D, SL, claim):
        """The bin's maximum is zero, held twice with different signs: the first one's bits come back (== ties them)."""
        x[lo:lo + L] = -np.abs(x[lo:lo + L]) - 1
        if L < 2:
            return
        p = (L - 2) // 2 if b & 1 else max(0, min(L - 2, 63 + b))
        x[lo + p], x[lo + p + 1] = first, second
        claim.update(argmax=p, max_bits=bits(first))
    return rule


def _zeros_min(first, second):
    def rule(x, b, lo, L, D, SL, claim):
        x[lo:lo + L] = np.abs(x[lo:lo + L]) + 1
        if L < 2:
            return
        p = L - 2 if b & 1 else min(L - 2, 255)
        x[lo + p], x[lo + p + 1] = first, second
        claim.update(argmin=p, min_bits=bits(first))
    return rule


def plus_inf(x, b, lo, L, D, SL, claim):
    """+inf is a score like any other: it wins, and sum and sumsq are +inf."""
    p = (2 * L) // 3
    x[lo + p] = np.inf
    claim.update(argmax=p, max_bits=bits(np.inf), count=L)


def minus_inf(x, b, lo, L, D, SL, claim):
    p = L // 5
    x[lo + p] = -np.inf
    claim.update(argmin=p, min_bits=bits(-np.inf), count=L)


CASES = {
    "first_offset": (first_offset, "max at the first offset of each bin, min at the last"),
    "last_offset": (last_offset, "max at the last offset of each bin (the ragged last bin's own), min at the first"),
    "group64_edge": (_group_edge(64), "max at the last / first offset of a 64-score group"),
    "group256_edge": (_group_edge(256), "max at the last / first offset of a 256-score group"),
    "nan_at_winner": (nan_at_winner, "a NaN where the winner would be: skipped, not counted"),
    "all_nan_bin": (all_nan_bin, "an all-NaN bin: count 0, NaN extremes, offsets 0, +0.0 sums"),
    "pos_zero_first": (_zeros(np.float32(0.0), np.float32(-0.0)), "+0.0 before -0.0 as the max: +0.0's bits"),
    "neg_zero_first": (_zeros(np.float32(-0.0), np.float32(0.0)), "-0.0 before +0.0 as the max: -0.0's bits"),
    "pos_zero_first_min": (_zeros_min(np.float32(0.0), np.float32(-0.0)), "+0.0 before -0.0 as the min: +0.0's bits"),
    "neg_zero_first_min": (_zeros_min(np.float32(-0.0), np.float32(0.0)), "-0.0 before +0.0 as the min: -0.0's bits"),
    "plus_inf": (plus_inf, "+inf wins the max; the sums are +inf"),
    "minus_inf": (minus_inf, "-inf wins the min; sum -inf, sumsq +inf"),
}


for _k in range(6):
    CASES["slice_first_%d" % _k] = (_slice_first(_k), "max at the first offset of slice (bin + %d) mod slices, min mirrored" % _k)
    CASES["slice_last_%d" % _k] = (_slice_last(_k), "max at the last offset of slice (bin + %d) mod slices, min mirrored" % _k)
for _w in TWICE:
    CASES["twice_max_" + _w] = (_twice(_w, 1), "the same max twice, %s scores apart: the earlier wins" % _w)
    CASES["twice_min_" + _w] = (_twice(_w, -1), "the same min twice, %s scores apart: the earlier wins" % _w)


def build(name, D, n, slice_len):
    rule = CASES[name][0]
    x = _background(D, n, sorted(CASES).index(name))
    claims = []
    for b in range((n + D - 1) // D):
        lo = b * D
        L = min(D, n - lo)
        claim = {}
        rule(x, b, lo, L, D, slice_len, claim)
        claims.append(claim)
    return x, claims


def bin_lengths(wave_bin_max, slice_len):
    W, SL = wave_bin_max, slice_len
    return sorted({1, 2, 3, 63, 64, 65, 255, 256, 257, W - 1, W, W + 1, SL - 1, SL, SL + 1, 2 * SL + 1, 5 * SL + 7})


def score_counts(D):
    return sorted({n for n in (1, D - 1, D, D + 1, 3 * D + 1) if n > 0})


def check_claims(rec, claims):
    """The failures of the records `rec` against the claims (an empty list: the claims hold)."""
    bad = []
    for b, claim in enumerate(claims):
        r = rec[b]
        got = dict(argmax=int(r["argmax"]), argmin=int(r["argmin"]), count=int(r["count"]), max_bits=bits(r["max"]),
                   min_bits=bits(r["min"]), sum_bits=int(np.float64(r["sum"]).view(np.uint64)),
                   sumsq_bits=int(np.float64(r["sumsq"]).view(np.uint64)))
        for k, v in claim.items():
            if not k.startswith("_") and got[k] != v:       # (a key with '_' in front describes the array, not the record)
                bad.append((b, k, v, got[k]))
    return bad
