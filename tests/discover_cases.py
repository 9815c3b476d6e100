"""Designed score arrays for the record rule of needle discovery (am_probe_scores*): integer scores of magnitude at most
2^12 whose deciding scores sit where the kernels can go wrong -- the first and last offset, either side of the excluded
range, at distance separation - 1 and separation from the best, either side of every slice and load-step boundary --
with equal maxima in two lanes, two steps and two slices, no runner-up, nothing left, n = 1, 2, 3, +-inf and +-0.0.

A case is (name, x, ex_lo, ex_hi, separation, claim); the claim names `best`, `second` (None: no runner-up) or
`none` (no candidate), and the reference must agree with it (tests/test_discover_host.py)."""
import numpy as np

TOP, NEXT, TRAP = 4096.0, 3000.0, 4000.0   # the best, the runner-up, and what must not be picked
STEP, UNROLL = 256, 1024                   # scores a wave loads per step; steps it keeps in flight together


def background(n, seed):
    return np.random.default_rng(seed).integers(-50, 51, size=n).astype(np.float32)


def plant(n, best, second=None, traps=(), ex=(0, 0), sep=1, nan=(), seed=1, name=""):
    """Background noise below every planted score; TOP at best, NEXT at second, TRAP at the trap offsets (each excluded,
    or inside the zone of the best), NaN at `nan`."""
    x = background(n, seed + n)
    for t in traps:
        assert (ex[0] <= t < ex[1]) or abs(t - best) < sep or t in nan, (name, t)
        x[t] = TRAP
    for t in nan:
        x[t] = np.nan
    x[best] = TOP
    if second is not None:
        assert abs(second - best) >= sep and not ex[0] <= second < ex[1]
        x[second] = NEXT
    return (name, x, ex[0], ex[1], sep, {"best": best, "second": second})


def boundaries(n, SL):
    """Offsets q in (0, n) at which a slice or one of its steps begins, for every alignment of the array (the wave's
    steps start at the 16-byte boundary at or below a slice's start: up to three scores earlier).  Every step of every
    slice: among them the steps at which a group of four begins and the one at which the guarded tail takes over."""
    qs = set()
    for s0 in range(0, n, SL):
        for k in range(SL // STEP + 1):
            for a in range(4):
                q = s0 + k * STEP - a
                if 0 < q < n:
                    qs.add(q)
    return sorted(qs)


def sizes(SL):
    return [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 259, 1023, 1024, 1025, 1279, 1280, 1283, SL - 1, SL, SL + 1, 2 * SL + 5,
            64 * SL - 1, 64 * SL, 65 * SL + 3]


def cases(SL, big=1 << 22):
    out = []
    # the ends, and every array length around the kernel's sizes
    for n in sizes(SL) + [big]:
        if n >= 2:
            out.append(plant(n, 0, n - 1, name="ends_%d" % n))
            out.append(plant(n, n - 1, 0, name="ends_rev_%d" % n))
        if n >= 3:
            out.append(plant(n, n // 2, None, sep=n, traps=(0, n - 1), name="no_second_%d" % n))
    out.append(("n1", np.float32([7]), 0, 0, 1, {"best": 0, "second": None}))
    out.append(("n1_nan", np.float32([np.nan]), 0, 0, 1, {"none": True}))
    out.append(("n1_excluded", np.float32([7]), 0, 1, 1, {"none": True}))
    out.append(("n2_tie", np.float32([5, 5]), 0, 0, 1, {"best": 0, "second": 1}))
    out.append(("n2_sep2", np.float32([5, 9]), 0, 0, 2, {"best": 1, "second": None}))
    out.append(("n3", np.float32([1, 9, 5]), 0, 0, 1, {"best": 1, "second": 2}))
    out.append(("n3_sep2", np.float32([1, 5, 9]), 0, 0, 2, {"best": 2, "second": 0}))
    out.append(("n3_mid_excluded", np.float32([1, 9, 1]), 1, 2, 1, {"best": 0, "second": 2}))
    # either side of the excluded range
    for n, lo, hi in ((100, 10, 20), (3 * SL, SL - 2, SL + 3), (3 * SL, SL, 2 * SL), (3 * SL, 255, 2 * SL + 257), (2 * SL + 9, 0, 2 * SL + 8),
                      (2 * SL + 9, 1, 2 * SL + 9), (big, big // 2 - 1, big // 2 + SL + 1)):
        inside = tuple(sorted({lo, hi - 1, (lo + hi) // 2}))
        if lo > 0 and hi < n:
            out.append(plant(n, lo - 1, hi, traps=inside, ex=(lo, hi), name="ex_below_%d_%d_%d" % (n, lo, hi)))
            out.append(plant(n, hi, lo - 1, traps=inside, ex=(lo, hi), name="ex_above_%d_%d_%d" % (n, lo, hi)))
        elif lo > 0:
            out.append(plant(n, lo - 1, None, traps=inside, ex=(lo, hi), sep=n, name="ex_tail_%d_%d" % (n, lo)))
        else:
            out.append(plant(n, hi, None, traps=inside, ex=(lo, hi), sep=n, name="ex_head_%d_%d" % (n, hi)))
    # at distance separation - 1 and separation from the best, on both sides; the zone inside one slice, across a slice
    # boundary, over a whole slice and more, and clipped by the array's ends
    for n, b, sep in ((1000, 500, 7), (3 * SL, SL + 100, 50), (3 * SL, SL - 3, 10), (3 * SL, SL + 2, 10), (4 * SL + 1, 2 * SL + 17, SL + 300),
                      (4 * SL + 1, 2 * SL, SL), (4 * SL + 1, 2 * SL - 1, 2 * SL - 1), (3 * SL, 5, 9), (3 * SL, 3 * SL - 4, 9), (big, big - SL - 7, 2 * SL),
                      (66 * SL, 33 * SL + 9, 20 * SL + 5)):
        zone = [t for t in (b - sep + 1, b + sep - 1, b - 1, b + 1) if 0 <= t < n and t != b]
        for side in (-1, 1):
            s, o = b + side * sep, b - side * sep
            if not 0 <= s < n:
                continue
            out.append(plant(n, b, s, traps=zone, sep=sep, name="sep_%d_%d_%d_%+d" % (n, b, sep, side)))
            if 0 <= o < n:   # the same score at both ends of the zone: the lower offset
                name, x, lo, hi, sp, claim = plant(n, b, min(s, o), traps=zone, sep=sep, name="sep_both_%d_%d_%d_%+d" % (n, b, sep, side))
                x[max(s, o)] = NEXT
                out.append((name, x, lo, hi, sp, claim))
        # nothing outside the zone but NaN and excluded scores: no runner-up
        if b - sep >= 0 and b + sep < n and n <= 4 * SL + 1:
            x = np.full(n, np.nan, np.float32)
            x[b - sep + 1:b + sep] = background(2 * sep - 1, 3)
            x[b] = TOP
            x[0] = TRAP
            out.append(("zone_only_%d_%d_%d" % (n, b, sep), x, 0, 1, sep, {"best": b, "second": None}))
    # either side of every slice and load-step boundary: best just below, runner-up just above, and the reverse
    for n in (SL - 1, SL + 1, 2 * SL + 5):
        for q in boundaries(n, SL):
            out.append(plant(n, q - 1, q, name="edge_%d_%d" % (n, q)))
            out.append(plant(n, q, q - 1, name="edge_rev_%d_%d" % (n, q)))
    # equal maxima in two lanes, two steps, two groups of steps and two slices; equal runners-up likewise
    n = 3 * SL + 11
    for p in (0, 3, 700, SL - 1, SL, 2 * SL + 1):
        for dist in (1, 4, 8, STEP, UNROLL, SL, SL + 1, 2 * SL):
            if p + dist >= n:
                continue
            name, x, lo, hi, sp, claim = plant(n, p, p + dist, name="tie_best_%d_%d" % (p, dist))
            x[p + dist] = TOP
            out.append((name, x, lo, hi, sp, claim))
            far = n - 1 if p + dist < n - 1 else None
            if far:   # ... with a zone that holds the second maximum: the runner-up lies elsewhere
                name, x, lo, hi, sp, claim = plant(n, p, far, sep=dist + 1, name="tie_zone_%d_%d" % (p, dist))
                x[p + dist] = TOP
                out.append((name, x, lo, hi, sp, claim))
            if p >= 2:
                name, x, lo, hi, sp, claim = plant(n, 1, p, name="tie_second_%d_%d" % (p, dist))
                x[p + dist] = NEXT
                out.append((name, x, lo, hi, sp, claim))
    # nothing left
    out.append(("all_nan", np.full(SL + 5, np.nan, np.float32), 0, 0, 1, {"none": True}))
    out.append(("all_excluded", background(SL + 5, 2), 0, SL + 5, 1, {"none": True}))
    x = background(2 * SL, 4)
    x[SL:] = np.nan
    out.append(("nan_or_excluded", x, 0, SL, 1, {"none": True}))
    # +-inf are scores like any other; -0.0 and +0.0 tie, and the first one's bits come back
    x = background(SL + 9, 5)
    x[17], x[SL + 2], x[300] = np.inf, np.inf, -np.inf
    out.append(("inf", x, 0, 0, 1, {"best": 17, "second": SL + 2}))
    x = np.full(600, -np.inf, np.float32)
    x[::2] = np.nan
    out.append(("only_minus_inf", x, 0, 0, 4, {"best": 1, "second": 5}))
    x = np.full(SL + 3, -7, np.float32)
    x[5], x[300], x[SL + 1] = -0.0, 0.0, -0.0
    out.append(("zeros", x, 0, 0, 1, {"best": 5, "second": 300}))
    x = np.full(SL + 3, -7, np.float32)
    x[5], x[300] = 0.0, -0.0
    out.append(("zeros_rev", x.copy(), 0, 0, 296, {"best": 5, "second": 301}))   # (300 lies in the zone: the first -7 behind it)
    x[SL + 2] = -0.0
    out.append(("zeros_rev_far", x.copy(), 0, 0, 296, {"best": 5, "second": SL + 2}))
    return out


def check_claim(rec, x, claim):
    """What of the claim the record (discover_ref.PROBE_DTYPE) misses: a list of strings."""
    bad = []
    if claim.get("none"):
        if int(rec["flags"]) != 3 or int(rec["best"]) or int(rec["second"]) or not (np.isnan(rec["ncc"]) and np.isnan(rec["ncc_second"])):
            bad.append("a record without candidates expected")
        return bad
    if int(rec["flags"]) & 1 or int(rec["best"]) != claim["best"] or np.float32(rec["ncc"]).tobytes() != x[claim["best"]].tobytes():
        bad.append("best %d expected, got %d" % (claim["best"], int(rec["best"])))
    if claim["second"] is None:
        if int(rec["flags"]) != 2 or int(rec["second"]) or not np.isnan(rec["ncc_second"]):
            bad.append("no runner-up expected")
    elif int(rec["flags"]) or int(rec["second"]) != claim["second"] or np.float32(rec["ncc_second"]).tobytes() != x[claim["second"]].tobytes():
        bad.append("second %d expected, got %d" % (claim["second"], int(rec["second"])))
    return bad
