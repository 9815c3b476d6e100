"""Designed score arrays for the peak pick (csrc/am_peaks.hip, am_walk.h, am_best.hip): every case puts the sample that
decides a keep / reject at one of the pick's boundary constants (the 8-wide fetch, kNear = 32, the 64-wide wave step,
the 256-score halo, the 32-score run summaries and their 8-run reach, the 1024-score tile, the 32-tile bound, the 8-tile
group and 64-lane ballots of the walk, 4 inline peaks, 1024 peaks and 1024 candidate tiles per chunk).

A case is a tuple (name, scores_f32, min_prom, min_dist) with an attribute `meta` (a dict: family, side, d, pm, dip,
equal, the candidate's start `cand`, the name of its `pair` / `twin`, ...).  Every value is a multiple of 1/64 of
magnitude below 8, so every difference is exact in f32.  Families are generators (FAMILIES): thousands of 8-tile arrays
are never alive at once.  Used by tests/test_peak_cases_host.py (CPU: a second reference, and the design properties of
every case) and tests/test_gpu_peak_cases.py (library == checker bit for bit).

The probe: a candidate maximum of height H on a flat floor; on the probed side a stopper at distance d (strictly higher,
or in the `equal` variant exactly H) and a dip to Q at distance d - 1 ("in": the walk passes it) or d + 1 ("out": it
must not count).  The other side is settled at once: a stopper at distance 3 behind a two-score trench (TRENCH < Q --
prominence is height - max(left min, right min), so the probed side only decides when the other side is lower).
min_prom = 1.5 lies between the two outcomes H - Q = 2 (kept) and H - floor = 1 (rejected).  An `equal` probe has a
further dip Q2 < Q at d + 2: the walk must pass the equal stopper and find it (prominence H - Q2 = 2.5).
d = 1 has no "in" placement (the dip would be the candidate), and with a higher stopper next to it the candidate is no
maximum at all."""
import numpy as np

T = 1024
G = np.float32(1.0 / 64)
H, FLOOR, STOP, Q, Q2, TRENCH = (np.float32(v) for v in (1.0, 0.0, 2.0, -1.0, -1.5, -2.0))
PROBE_PROM = np.float32(1.5)
BIG_TILES = 1100


class Case(tuple):
    def __new__(cls, name, y, prom, dist, **meta):
        y = np.ascontiguousarray(y, dtype=np.float32)
        self = super().__new__(cls, (name, y, np.float32(prom), int(dist)))
        self.meta = meta
        return self


def on_grid(y):
    return bool(np.all(y * 64 == np.round(y * 64)) and np.all(np.abs(y) < 8))


def probe(n, p, plen, side, d, dip, equal, floor=FLOOR):
    """The probe described in the module header, candidate plateau [p, p + plen)."""
    y = np.full(n, floor, dtype=np.float32)
    y[p:p + plen] = H
    sgn = 1 if side == "R" else -1
    edge, other = (p + plen - 1, p) if side == "R" else (p, p + plen - 1)
    s = edge + sgn * d
    assert 0 <= s + 2 * sgn < n and 0 <= other - 3 * sgn < n and (dip != "in" or d >= 2)
    y[s] = H if equal else STOP
    if dip == "in":
        y[s - sgn] = Q
    elif dip == "out":
        y[s + sgn] = Q
    if equal:
        y[s + 2 * sgn] = Q2
    y[other - sgn] = y[other - 2 * sgn] = TRENCH
    y[other - 3 * sgn] = STOP
    return y


def place(n, pm, plen, side, d):
    """The candidate start congruent pm mod T that is closest to the chunk edge on the probed side."""
    if side == "L":
        p = pm
        while p - d - 2 < 0 or p < 1:
            p += T
    else:
        p = (n // T) * T + pm
        while p + plen - 1 + d + 2 > n - 1:
            p -= T
    return p


# ---------------------------------------------------------------------------
F1_D = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 34, 63, 64, 65, 255, 256, 257, 258, 1023, 1024, 1025, 1279, 1280, 1281)
F1_PM = (1, 31, 32, 255, 256, 512, 767, 768, 1022, 1023, 0)
F1_N = {"L": (8 * T,), "R": (8 * T, 6 * T + 37)}   # (the array's end only matters to the right-hand walk)


def probe_cases(fam, n, pm, plen, side, d, p=None):
    p = place(n, pm, plen, side, d) if p is None else p
    base = dict(family=fam, side=side, d=d, pm=pm, n=n, plen=plen)
    for equal in (False, True):
        base["cand"] = p - 1 if equal and d == 1 and side == "L" else p   # (an equal neighbour extends the plateau)
        for dip in ("in", "out"):
            if dip == "in" and d < 2:
                continue
            name = f"{fam}-{side}-d{d}-pm{pm}-n{n}-len{plen}-{dip}-{'equal' if equal else 'higher'}"
            other = name.replace("-in-", "-out-") if dip == "in" else name.replace("-out-", "-in-")
            yield Case(name, probe(n, p, plen, side, d, dip, equal), PROBE_PROM, 0, dip=dip, equal=equal,
                       pair=other if d >= 2 else None, twin=name.replace("-equal", "-higher") if equal else None, **base)


def f1(side):
    for n in F1_N[side]:
        for d in F1_D:
            for pm in F1_PM:
                yield from probe_cases("F1", n, pm, 1, side, d)


# ---------------------------------------------------------------------------
# F2: run summaries (stage 0).  min_prom 1, candidate H = 1 on a floor of 1/64: one grid step short of min_prom below
# it.  The stopper sits in run j (0 = the candidate's own) on the probed side; `k` names the run on the way (k <= j)
# that holds one score of 0 -- the drop reaches min_prom exactly there -- or is None: the drop stays short and the
# stopper rejects.  The candidate is the first (R) / last (L) score of its run, so the other side's trench lies in the
# neighbouring run and leaves the own run's summary alone.  `equal`: the stopper has height H; two runs beyond it the
# floor drops to -1, and the array's edge ends the walk: kept, whatever k.
F2_J = tuple(range(0, 10))
F2_K = (0, 1, 7, 8, 9)


def f2(side):
    n = 4 * T
    sgn = 1 if side == "R" else -1
    for pm in (512, 0 if side == "R" else T - 1):     # mid-tile; at a tile edge (the window's run 8 / run 0)
        p = ((T + pm) // 32) * 32 + (0 if side == "R" else 31)
        for j in F2_J:
            for k in (None,) + tuple(kk for kk in F2_K if kk <= j):
                for equal in (False, True):
                    y = np.full(n, G, dtype=np.float32)
                    y[p] = H
                    run0 = (p // 32) * 32                       # first score of the candidate's run
                    rj = run0 + sgn * 32 * j
                    s = rj + 20 if j else p + sgn * 9           # the stopper, inside run j, beyond the candidate
                    y[s] = H if equal else STOP
                    if k is not None:
                        rk = run0 + sgn * 32 * k
                        dpos = rk + 10 if k else p + sgn * 4
                        if k == j and j:                        # in the stopper's run: on the candidate's side of it
                            dpos = s - sgn * 3
                        y[dpos] = 0.0
                    if equal:
                        y[rj + sgn * 64 + 5] = -1.0
                    y[p - sgn] = y[p - 2 * sgn] = TRENCH
                    y[p - 3 * sgn] = STOP
                    name = f"F2-{side}-pm{pm}-j{j}-k{k}-{'equal' if equal else 'higher'}"
                    yield Case(name, y, 1.0, 0, family="F2", side=side, pm=pm, j=j, k=k, equal=equal, cand=p,
                               keep=bool(equal or k is not None), twin=name.replace("-equal", "-higher") if equal else None)


# ---------------------------------------------------------------------------
# F3: the tile bound.  min_prom 1; the candidate (H = 1) stands on a floor of 1/4 in a tile whose own range (3/4) cannot
# qualify; the tiles towards the first taller tile, D tiles away, keep the floor.  "reject": the taller tile's stopper is
# the first score the walk meets there (drop 3/4: no peak, and the summaries alone say so).  "keep": a score of 0 comes
# just before the stopper (the drop reaches min_prom inside that tile).  "equal": the tile D away only reaches H; the drop
# to 0 and the real stopper come one tile later: kept.  The other side drops to -1 in the neighbouring tile and ends at
# the array's edge.  `tail` scores of floor are appended (n mod 1024 in {0, 1, 37, 1023}); a tail of 37 or 1023 holds a
# maximum of its own, which the tail piece's own range already rejects.
F3_D = (1, 2, 31, 32, 33, 34)


def f3(side):
    fl = np.float32(0.25)
    for D in F3_D:
        for ti, tail in enumerate((0, 1, 37, 1023)):
            for kind in ("reject", "keep", "equal"):
                nt = D + 4
                n = nt * T + tail
                y = np.full(n, fl, dtype=np.float32)
                ct = 1 if side == "R" else nt - 2                 # candidate tile; the other side's tile is 0 / nt - 1
                sgn = 1 if side == "R" else -1
                pm = (512, 0, T - 1, 700)[(ti + F3_D.index(D)) % 4]
                p = ct * T + pm
                y[p] = H
                near = (ct + sgn * D) * T + (0 if side == "R" else T - 1)   # first score the walk meets in the tile D away
                if kind == "reject":
                    y[near] = STOP
                elif kind == "keep":
                    y[near] = 0.0
                    y[near + sgn] = STOP
                else:
                    y[near + sgn * 5] = H
                    y[near + sgn * T] = 0.0
                    y[near + sgn * (T + 1)] = STOP
                ot = (ct - sgn) * T + (T - 1 if side == "R" else 0)
                y[ot] = -1.0
                if tail >= 37:
                    y[nt * T + 20] = H
                name = f"F3-{side}-D{D}-tail{tail}-pm{pm}-{kind}"
                yield Case(name, y, 1.0, 0, family="F3", side=side, D=D, tail=tail, pm=pm, kind=kind, cand=p,
                           pair=name.replace("-reject", "-keep") if kind == "reject" else
                           name.replace("-keep", "-reject") if kind == "keep" else None)


# ---------------------------------------------------------------------------
# F4: long walks, 1100 tiles.  The candidate stands in tile 1050 (walk left) or 40 (walk right), the stopper D tiles
# away at in-tile offset `off`.  where = "tile": the dip lies in the tile before / beyond the stopper's tile;
# "near": next to the stopper, on either side of it.  For each D one side gets the in / out pair; the other side gets
# one array with both dips (Q before, Q2 beyond the stopper) and min_prom = H - Q exactly: the peak is kept at the bound,
# a walk that misses the first dip drops it, one that takes the second reports another prominence.
F4_D = (7, 8, 9, 63, 64, 65, 72, 511, 512, 513, 520, 1000)
F4_OFF = (0, 1, T - 1)


def long_probe(side, D, off, where, dips, equal, stopper=True):
    n = BIG_TILES * T
    y = np.full(n, FLOOR, dtype=np.float32)
    sgn = 1 if side == "R" else -1
    p = (40 if side == "R" else 1050) * T + 512
    y[p] = H
    st = (p // T + sgn * D) * T
    s = st + off
    if stopper:
        y[s] = H if equal else STOP
        for dip, v in dips:
            if where == "near":
                y[s - sgn if dip == "in" else s + sgn] = v
            else:
                y[st - sgn * T + 300 if dip == "in" else st + sgn * T + 300] = v
        if equal:
            y[st + sgn * 2 * T + 7] = Q2
    else:
        y[(5 if side == "R" else BIG_TILES - 5) * T + 3] = Q     # behind the candidate: the other side
        y[p + sgn * 600 * T + 11] = Q
    y[p - sgn] = y[p - 2 * sgn] = TRENCH
    y[p - 3 * sgn] = STOP
    return y, p


def f4(side):
    for i, D in enumerate(F4_D):
        off = F4_OFF[i % 3]
        where = ("tile", "near")[(i // 3 + (side == "R")) % 2]
        base = dict(family="F4", side=side, D=D, off=off, where=where)
        stem = f"F4-{side}-D{D}-off{off}-{where}"
        if (i % 2 == 0) == (side == "L"):
            for dip in ("in", "out"):
                y, p = long_probe(side, D, off, where, [(dip, Q)], False)
                yield Case(f"{stem}-{dip}-higher", y, PROBE_PROM, 0, dip=dip, equal=False, cand=p,
                           pair=f"{stem}-{'out' if dip == 'in' else 'in'}-higher", **base)
        else:
            y, p = long_probe(side, D, off, where, [("in", Q), ("out", Q2)], False)
            yield Case(f"{stem}-both-higher", y, H - Q, 0, dip="both", equal=False, cand=p, **base)
        if D in (8, 64, 512):
            y, p = long_probe(side, D, off, where, [("out", Q)], True)
            yield Case(f"{stem}-out-equal", y, PROBE_PROM, 0, dip="out", equal=True, cand=p, **base)
    # the two full-ballot distances at the remaining in-tile offsets (what the 60-array budget leaves room for)
    for D, sd in ((64, "L"), (512, "R")):
        for off in F4_OFF:
            if side == sd and off != F4_OFF[F4_D.index(D) % 3]:
                y, p = long_probe(side, D, off, "near", [("in", Q), ("out", Q2)], False)
                yield Case(f"F4-{side}-D{D}-off{off}-near-both-higher", y, H - Q, 0, family="F4", side=side, D=D, off=off,
                           where="near", dip="both", equal=False, cand=p)
    y, p = long_probe(side, 0, 0, "tile", [], False, stopper=False)
    yield Case(f"F4-{side}-no-stopper", y, PROBE_PROM, 0, family="F4", side=side, D=None, dip="edge", equal=False, cand=p)


# ---------------------------------------------------------------------------
# F5: plateaus as the candidate of a probe measured from the plateau's end (R) or start (L); `behind` = what lies on the
# other side: "lower" (the probe's trench: a maximum), "higher" (no maximum), "edge" (the plateau reaches the array's end
# or starts at 0: no maximum; a plain probe elsewhere keeps the answer non-empty).
F5_LEN = (2, 31, 32, 33, 257, 1024, 1281, 2200)
F5_PM = (1, 700, 1000, 1023)
F5_D = (2, 33, 257)


def f5(side):
    n = 8 * T
    sgn = 1 if side == "R" else -1
    for plen in F5_LEN:
        for pm in F5_PM:
            for d in F5_D:
                p = pm + T                        # one placement for all lengths: the start's offset is what is swept
                for c in probe_cases("F5", n, pm, plen, side, d, p):
                    c.meta["behind"] = "lower"
                    yield c
            y = probe(n, p, plen, side, 33, "in", False)
            other = p if side == "R" else p + plen - 1
            y[other - sgn] = STOP
            yield Case(f"F5-{side}-len{plen}-pm{pm}-behind-higher", y, PROBE_PROM, 0, family="F5", side=side, plen=plen, pm=pm,
                       behind="higher", cand=p)
        y = np.full(n, FLOOR, dtype=np.float32)
        if side == "R":
            y[n - plen:] = H
        else:
            y[:plen] = H
        q = 4 * T + 100 if side == "R" else 6 * T + 100
        y[q], y[q - 1], y[q + 1] = H, Q, Q
        yield Case(f"F5-{side}-len{plen}-edge", y, PROBE_PROM, 0, family="F5", side=side, plen=plen, behind="edge",
                   cand=0 if side == "L" else n - plen)
    if side == "R":
        yield from zero_cases()


def zero_cases():
    """+0.0 and -0.0 are one height: mixed inside one plateau, and as two separate peaks of equal height (earlier start
    first; the height keeps the sign bit of the plateau's first score)."""
    for dist in (0, 10 ** 9):
        y = np.full(3 * T, -0.5, dtype=np.float32)
        y[1000:1040] = np.where(np.arange(40) % 3 == 0, np.float32(-0.0), np.float32(0.0))
        yield Case(f"F5-zeros-one-plateau-dist{dist}", y, 0.25, dist, family="F5", side="R", behind="zeros", cand=1000)
        y = np.full(3 * T, -0.5, dtype=np.float32)
        y[700], y[2100] = 0.0, -0.0
        yield Case(f"F5-zeros-plus-then-minus-dist{dist}", y, 0.25, dist, family="F5", side="R", behind="zeros", cand=700)
        y = np.full(3 * T, -0.5, dtype=np.float32)
        y[700], y[2100] = -0.0, 0.0
        yield Case(f"F5-zeros-minus-then-plus-dist{dist}", y, 0.25, dist, family="F5", side="R", behind="zeros", cand=700)


# ---------------------------------------------------------------------------
# F6: min_dist >= n (the reference's default).  label: "fast" (the chunk maximum is a prominent peak: it is the whole
# answer), "fall" (the maximum is no peak -- at an edge, or on a plateau that reaches one: the best prominent peak below
# it is the answer), "notprom" (the maximum is a peak but not prominent: the best prominent peak below it under
# prominence -> distance, nothing under distance -> prominence).  `expect` = the start of the answer under order 0.
F6_N = (3, T + T // 2, 8 * T, BIG_TILES * T)


def f6(side=None):
    for n in F6_N:
        def base():
            y = np.full(n, FLOOR, dtype=np.float32)
            if n > 100:
                for q, h in ((n // 3, 1.0), (n // 3 + 50, 1.25), (2 * n // 3 + 1, 1.25)):   # lower peaks, the best one tied
                    y[q] = h
            return y
        low = n // 3 + 50 if n > 100 else None
        out = []
        y = base(); y[n // 2] = 3.0
        out.append(("fast-interior", y, "fast", n // 2))
        y = base(); y[0] = 3.0
        out.append(("max-at-0", y, "fall", low))
        y = base(); y[n - 1] = 3.0
        out.append(("max-at-end", y, "fall", low))
        if n > 100:
            y = base(); y[n - 40:] = 3.0
            out.append(("plateau-to-end", y, "fall", low))
            y = base(); y[:40] = 3.0
            out.append(("plateau-from-0", y, "fall", low))
            y = base(); y[:n // 8] = 2.75; y[n // 8] = 3.0
            out.append(("max-not-prominent", y, "notprom", low))
            # the maximum value in three tiles; the first occurrence is a plateau across a tile edge
            y = base()
            t0 = T - 2 if n > 2 * T else 200
            y[t0:t0 + 5] = 3.0
            y[n // 2 + 3] = 3.0
            y[n - 30] = 3.0
            y[t0 - 7] = Q                      # the winner's prominence is not the array's range
            y[t0 + 9] = -0.5
            out.append(("max-in-three-tiles", y, "fast", t0))
        for name, y, label, expect in out:
            yield Case(f"F6-n{n}-{name}", y, 0.5, 10 ** 9 if n % 2 else n, family="F6", n=n, label=label, expect=expect)


# ---------------------------------------------------------------------------
# F7: list sizes and ties.
F7_COUNTS = (3, 4, 5, 1023, 1024, 1025, 5000)
F7_DIST = (0, 1, 2, 7, 8, 9)


def f7(side=None):
    for cnt in F7_COUNTS:                              # spikes every 4 scores, heights 1, 1, 1.5, 1, 1, 1.5, ...
        y = np.full(4 * cnt + 3, FLOOR, dtype=np.float32)
        y[2:2 + 4 * cnt:4] = np.where(np.arange(cnt) % 3 == 2, np.float32(1.5), np.float32(1.0))
        yield Case(f"F7-count{cnt}", y, 0.5, 0, family="F7", kind="count", count=cnt)
    for md in F7_DIST:                                 # tied plateaus of length 1, 2, 3 at gaps md - 1, md, md + 1
        for by in ("start", "centre"):
            y = np.full(2 * T, FLOOR, dtype=np.float32)
            pos, starts = 5, []
            for i in range(45):
                plen = (1, 2, 3)[(i // 3) % 3]
                y[pos:pos + plen] = H if i % 5 else np.float32(1.25)
                starts.append(pos)
                gap = (md - 1, md, md + 1)[i % 3]
                if by == "start":
                    nxt = pos + gap
                else:                                   # centre of the next plateau `gap` from this centre
                    nlen = (1, 2, 3)[((i + 1) // 3) % 3]
                    nxt = pos + (plen - 1) // 2 + gap - (nlen - 1) // 2
                pos = max(nxt, pos + plen + 1)
            yield Case(f"F7-ties-md{md}-by-{by}", y, 0.5, md, family="F7", kind="ties", md=md, by=by)
    for lead in (62, 63):                               # the chain A > B > C: A removes B, which frees C
        md = 8
        y = np.full(24 * T, FLOOR, dtype=np.float32)
        y[16:16 + 16 * 1100:16] = H                     # 1100 tied peaks, far enough apart
        base = 18 * T
        for i in range(lead):
            y[base + 32 * i] = np.float32(3.0) + np.float32(i) * G
        a = 22 * T + 100 - 100 % md + md - 4            # A, B, C in three neighbouring buckets
        y[a], y[a + md - 1], y[a + 2 * (md - 1)] = 2.5, 2.25, 2.0
        yield Case(f"F7-chain-lead{lead}", y, 0.5, md, family="F7", kind="chain", chain=(a, a + md - 1, a + 2 * (md - 1)),
                   count=1100 + lead + 2)


# ---------------------------------------------------------------------------
# F8: every tile holds exactly one qualifying peak: more candidate tiles than the hand-over list holds (1024).
def f8(side=None):
    for nt, order in ((BIG_TILES, "ascend"), (BIG_TILES, "descend"), (BIG_TILES, "tie"), (1024, "descend"), (1025, "ascend")):
        y = np.full(nt * T, FLOOR, dtype=np.float32)
        t = np.arange(nt)
        hs = {"ascend": 1 + (t // 4) / 64.0, "descend": 1 + ((nt - 1 - t) // 4) / 64.0, "tie": np.ones(nt)}[order]
        y[t * T + (t * 37) % T] = hs.astype(np.float32)
        y[0] = FLOOR                                    # (tile 0's peak would sit at index 0)
        y[5] = hs[0]
        yield Case(f"F8-{nt}tiles-{order}", y, 0.5, 0, family="F8", tiles=nt, order=order, count=nt)


FAMILIES = {"F1": f1, "F2": f2, "F3": f3, "F4": f4, "F5": f5, "F6": f6, "F7": f7, "F8": f8}
SIDED = ("F1", "F2", "F3", "F4", "F5")
PARAMS = [(f, s) for f in FAMILIES for s in (("L", "R") if f in SIDED else (None,))]


def cases(family, side=None):
    return FAMILIES[family](side)


def is_big(c):
    return c[1].size >= 1000 * T


# ---------------------------------------------------------------------------
# Haystacks for am_match (sparse scores, the run-level skip of the walk, chunks that start off a tile boundary): 8 kHz, a
# 1 s white needle with a DC component, twin plants of gain 1.0 and 0.5 at the distances of MATCH_D in both orders.  A DC
# stretch in the haystack lifts the score floor on one side of every pair (after the pair, or well before it, in turn).
# chunk = 80001 samples (odd chunk starts at 80001, 240003, ...), overlap = 2 s: a window holds chunk + 8001 scores.
# One pair straddles the end of window 0 (score 88002), one the chunk start 240003.
MATCH_SR = 8000
MATCH_D = (31, 32, 33, 255, 256, 257, 1023, 1024, 1025)
MATCH_CHUNK, MATCH_OVERLAP, MATCH_PROM = 80001, 16000, 0.13


def match_haystack(synth_uniform, seed=51):
    """(needle, haystack, [(start of the first twin, start of the second, gain of the first, gain of the second)])."""
    s = MATCH_SR
    needle = synth_uniform(seed, 0, 0, s) + np.float32(0.05)
    hay = synth_uniform(seed, 1, 0, 60 * s)
    plants = []
    for i, (d, order) in enumerate((d, o) for d in MATCH_D for o in (0, 1)):
        ta = 16000 + 24000 * i
        if i == 3:
            ta = MATCH_CHUNK + MATCH_OVERLAP - s + 1 - d // 2      # straddles the end of window 0
        if i == 9:
            ta = 3 * MATCH_CHUNK - d // 2                          # straddles a chunk start
        ga, gb = (1.0, 0.5) if order == 0 else (0.5, 1.0)
        hay[ta:ta + s] += np.float32(ga) * needle
        hay[ta + d:ta + d + s] += np.float32(gb) * needle
        lo = ta + d + 2000 if i % 2 == 0 else ta - 10000
        hay[lo:lo + 8000] += np.float32(0.05)
        plants.append((ta, ta + d, ga, gb))
    return needle, hay, plants
