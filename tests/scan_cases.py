"""Designed score arrays for K3's fused scan and the sparse-score certificate (csrc/am_fft.hip k3_finish, csrc/am_peaks.hip
peaks_kernel): every case puts the score that decides a write, a certificate or a keep / reject one grid step from the
boundary, at a chosen (block, row, column tile, lane) of the plan's layout.

How a design reaches K3: a needle of S samples that is 1.0 at index 0 and 0 elsewhere has sum(needle^2) = 1 and the Valid
correlation G[j] = hay[j]; the haystack `design ++ zeros(S - 1)` therefore has the score array `design` (to the
transforms' rounding) under AM_SCALE_NONE and AM_SCALE_LIB alike.  With S > 64 the needle takes K1 / K2 / K3.

Layout (used ONLY to place values and to word failures, as plan_geometry_ref's is): block b starts at score b * hop;
inside a block, score r * 8192 + 32 c + i is row r, column tile c (0 .. 255), lane i; a run is (block, r, c); a run whose
first score lies at or beyond min(hop, count - b * hop) is invalid; blocks 2g and 2g + 1 share one write threshold per
tile: theta = min(minimum of the tile's valid scores in both blocks, the needle's hist_min) + min_prominence / 2.  A run
is written when its maximum reaches theta or when it holds a chunk edge (score i * chunk, or i * chunk + d with d the
index of a full window's last score).  Chunk [a, b) passes its certificate when max theta over the blocks a / hop ..
(b - 1) / hop, minus the chunk's minimum, is < min_prominence.

Every value is a multiple of 1/64 of magnitude <= 4; every comparison a case decides lies at least 1/64 from equality
(test_scan_cases_host.py holds every case to that under model()).  min_prominence is 1 throughout: theta = tile minimum
+ 1/2.

A note on what can be designed.  A peak that qualifies in a chunk has height >= chunk minimum + min_prominence, and a
chunk that passes has every theta < chunk minimum + min_prominence: a qualifying peak BELOW its tile's theta and a passing
certificate exclude each other.  So the twin of an "unwritten, certificate fails" case is not the same peak one step
above theta (its certificate would sit at exact equality) but the same array with the tile's comb three steps lower:
run maximum = theta + 2/64, certificate passes by 1/64.  For the same reason the chunk-edge family (S5) does not hide a
qualifying peak below theta in an edge run; it makes the edge run's raw scores decide a prominence instead (a low score
one place inside / outside the chunk), with every certificate passing: a run the edge rule missed would be read as its
summary and give the wrong answer on one side of the twin.

expected() is the reference of every GPU assertion; model() only places values and words failures."""
import collections

import numpy as np

import plan_geometry_ref as R

ROW, RUN, TILES = 8192, 32, 256
G = np.float32(1.0 / 64)
PROM = np.float32(1.0)
SR = 8000
HOP = 65536                     # forced plans: S = N - 65535, 8 valid rows
RAGGED_HOP, RAGGED_RAW = 8192 * 7 + 4096, 8192 * 7 + 4096 + 500    # S = N - 61939: 7.5 rows, a block computes 500 scores beyond its hop
NATURAL_S = 20000               # the 2^21 plan by the library's own choice: hop 2 076 672 = 253.5 rows
FORCED = (21, 22, 23)

Params = collections.namedtuple("Params", "sr S chunk overlap prom dist overshadow_s")


class Layout:
    """hop / count / chunking of a case.  raw_hop = N - S + 1 (forced plans: the same design serves every N), or a fixed
    needle length `s_fixed` on the plan the library picks itself."""
    def __init__(self, hop, count, chunk, ov, raw_hop=None, s_fixed=None):
        self.hop, self.count, self.chunk, self.ov = int(hop), int(count), int(chunk), int(ov)
        self.raw_hop, self.s_fixed = raw_hop if raw_hop is not None else hop, s_fixed
        self.d = self.chunk + self.ov - 1                  # index of a full window's last score
        self.nblocks = -(-self.count // self.hop)

    def needle_len(self, log_n):
        s = self.s_fixed if self.s_fixed is not None else (1 << log_n) - self.raw_hop + 1
        assert R.hop_of(log_n, s) == self.hop, (log_n, s, self.hop)
        return s

    def params(self, log_n, prom=PROM, dist=0):
        s = self.needle_len(log_n)
        return Params(SR, s, self.chunk, s - 1 + self.ov, float(prom), int(dist), 0.0)

    def chunks(self):
        out, a = [], 0
        while a < self.count:
            out.append((a, min(a + self.chunk + self.ov, self.count)))
            a += self.chunk
        return out

    def lim(self, b):
        return min(self.hop, self.count - b * self.hop)

    def run_of(self, pos):
        b = pos // self.hop
        off = pos - b * self.hop
        return b, off // ROW, (off % ROW) // RUN, off % RUN

    def run_lo(self, b, r, c):
        return b * self.hop + r * ROW + RUN * c

    def place(self, pos):
        return "score %d = block %d (pair %d) row %d tile %d lane %d" % ((pos,) + (pos // self.hop, pos // self.hop // 2) + self.run_of(pos)[1:])


class Case:
    def __init__(self, name, y, layout, prom=PROM, dist=0, natural=False, **meta):
        self.name, self.layout, self.prom, self.dist, self.natural = name, layout, np.float32(prom), int(dist), natural
        self.y = np.ascontiguousarray(y, dtype=np.float32)
        assert self.y.size == layout.count
        self.meta = meta

    def log_ns(self):
        """The plans the case runs on: the three forced ones, or (natural = 21 / 22) the one the library picks itself."""
        return (int(self.natural),) if self.natural else FORCED

    def params(self, log_n):
        return self.layout.params(log_n, self.prom, self.dist)

    def haystack(self, log_n, out=None):
        n = self.y.size + self.layout.needle_len(log_n) - 1
        hay = np.zeros(n, dtype=np.float32) if out is None else out
        hay[:self.y.size] = self.y
        return hay


def on_grid(y):
    return bool(np.all(y * 64 == np.round(y * 64)) and np.all(np.abs(y) <= 4))


# ---------------------------------------------------------------------------
def expected(design, params, pol=None):
    """calc_chunks (oracle.c) computed from a score array: window i starts at i * chunk, holds w = min(chunk + overlap,
    H - i * chunk) samples (H = scores + S - 1), is skipped when w < S (or, policy tail_window = 1, when it is short) and has
    the scores design[i * chunk : i * chunk + w - S + 1]; per window oracle.find_peaks, the offset added; stable sort by
    start; is_overshadowed against the neighbours of the sorted unfiltered list (policy surrounding_from = 1: the last
    element kept)."""
    import pyoracle as oracle
    design = np.ascontiguousarray(design, dtype=np.float32)
    h = design.size + params.S - 1
    window = params.chunk + params.overlap
    all_ = []
    for i in range(-(-h // params.chunk)):
        off = i * params.chunk
        w = min(window, h - off)
        if w < params.S or (pol is not None and pol.tail_window and w < window):
            continue
        sc = design[off:off + w - params.S + 1]
        found = oracle.find_peaks(sc, params.prom, params.dist, cap=4096, pol=pol)
        if len(found) == 4096:                          # (the list may have been cut: once more with room for every maximum)
            found = oracle.find_peaks(sc, params.prom, params.dist, cap=sc.size // 2 + 1, pol=pol)
        all_ += [(s + off, e + off, ht, pr) for s, e, ht, pr in found]
    all_.sort(key=lambda q: q[0])                       # (stable)
    out, last = [], None
    from_kept = pol is not None and pol.surrounding_from
    for i, q in enumerate(all_):
        before = last if from_kept else (all_[i - 1] if i else None)
        after = all_[i + 1] if i + 1 < len(all_) else None
        if oracle.is_overshadowed(q, before, params.sr, params.overshadow_s) or oracle.is_overshadowed(q, after, params.sr, params.overshadow_s):
            continue
        last = q
        out.append(q)
    return out


# ---------------------------------------------------------------------------
Model = collections.namedtuple("Model", "tile_min theta rmin rmax valid written chunks")
INF = np.float32(np.inf)


def model(design, layout, min_prom=PROM, hist_min=INF):
    """A CPU model of K3's decisions: tile_min / theta [pair][tile]; per block rmin / rmax / valid / written [row][tile]
    (written includes the chunk-edge runs); per chunk a dict a, b, b0, b1, theta_max, cmin, passes."""
    y = np.ascontiguousarray(design, dtype=np.float32)
    lay = layout
    nb = lay.nblocks
    npairs = (nb + 1) // 2
    rmin, rmax, valid = [], [], []
    for b in range(nb):
        lim = lay.lim(b)
        rows = -(-lim // ROW)
        pad = np.full(rows * ROW, np.nan, dtype=np.float32)
        pad[:lim] = y[b * lay.hop:b * lay.hop + lim]
        v = pad.reshape(rows, TILES, RUN)
        ok = ~np.isnan(v)
        rmin.append(np.where(ok, v, INF).min(axis=2))
        rmax.append(np.where(ok, v, -INF).max(axis=2))
        valid.append(ok[:, :, 0])
    tile_min = np.full((npairs, TILES), INF, dtype=np.float32)
    for b in range(nb):
        tile_min[b // 2] = np.minimum(tile_min[b // 2], rmin[b].min(axis=0))
    theta = (np.minimum(tile_min, np.float32(hist_min)) + np.float32(0.5) * np.float32(min_prom)).astype(np.float32)
    written = []
    for b in range(nb):
        rows = rmin[b].shape[0]
        lo = b * lay.hop + np.arange(rows)[:, None] * ROW + np.arange(TILES)[None, :] * RUN
        edge = ((lo + 31) % lay.chunk) <= 31
        hi2 = lo + 31 - lay.d
        edge |= (hi2 >= 0) & ((hi2 % lay.chunk) <= 31)
        written.append(valid[b] & ((rmax[b] >= theta[b // 2][None, :]) | edge))
    chunks = []
    for a, e in lay.chunks():
        b0, b1 = a // lay.hop, (e - 1) // lay.hop
        # (K3 stores theta per block; both blocks of a pair hold the pair's value, so the block range is a pair range)
        tmax = np.float32(theta[b0 // 2:b1 // 2 + 1].max())
        cmin = np.float32(y[a:e].min())
        chunks.append(dict(a=a, b=e, b0=b0, b1=b1, theta_max=tmax, cmin=cmin,
                           passes=bool(e - a < 3 or (tmax - cmin) < np.float32(min_prom))))
    return Model(tile_min, theta, rmin, rmax, valid, written, chunks)


def failing(m):
    return {i for i, c in enumerate(m.chunks) if not c["passes"]}


# ---------------------------------------------------------------------------
# building blocks
def comb(y, lay, pair, tile, level):
    """Every valid score of column tile `tile` in both blocks of `pair` set to `level`: the tile's minimum."""
    for b in (2 * pair, 2 * pair + 1):
        if b >= lay.nblocks:
            continue
        lim = lay.lim(b)
        for r in range(-(-lim // ROW)):
            off = r * ROW + RUN * tile
            if off < lim:
                y[b * lay.hop + off:b * lay.hop + min(off + RUN, lim)] = level


CMIN = np.float32(-0.25)
H1 = np.float32(0.75) + G                    # qualifies by one step over the dips at CMIN
L_UNWRITTEN = np.float32(0.25) + 2 * G       # theta = H1 + 1/64: run unwritten, theta - CMIN = 1 + 2/64: certificate fails
L_WRITTEN = np.float32(0.25) - G             # theta = H1 - 2/64: run written,   theta - CMIN = 1 - 1/64: certificate passes


def hidden_peak_pair(fam, stem, lay, pos, dl=ROW - 3200, dr=ROW - 3200, natural=False, chunk=0):
    """The S1 twins: a peak of height H1 at `pos` between two dips at CMIN (the chunk minimum, in other tiles), its tile
    combed to L_UNWRITTEN / L_WRITTEN in both blocks of its pair.  Everywhere else theta = 1/2, 3/4 above the minimum."""
    b, r, c, lane = lay.run_of(pos)
    for side, level in (("unwritten", L_UNWRITTEN), ("written", L_WRITTEN)):
        y = np.zeros(lay.count, dtype=np.float32)
        comb(y, lay, b // 2, c, level)
        y[pos] = H1
        y[pos - dl] = y[pos + dr] = CMIN
        yield Case(f"{stem}-{side}", y, lay, natural=natural, family=fam, side=side, pos=pos, run=(b, r, c), run_written=side == "written",
                   fails={chunk} if side == "unwritten" else set(), dips=(pos - dl, pos + dr), comb=(b // 2, c),
                   twin=f"{stem}-{'written' if side == 'unwritten' else 'unwritten'}", differ="comb")


# ---------------------------------------------------------------------------
# S1: the write decision.  7 blocks (the last pair has an empty second block), chunks of 3 hops - 1000 with 5000 scores of
# overlap: chunk 0 = [0, 200 608) over blocks 0 .. 3, chunk 1 over blocks 2 .. 6 (minimum 0 there: it passes).
LAY7 = Layout(HOP, 7 * HOP, 3 * HOP - 1000, 5000)
S1_AT = ((0, 3, 0, 5), (0, 7, 255, 31), (1, 0, 0, 0), (1, 4, 127, 17), (1, 7, 128, 1), (2, 1, 1, 30), (2, 5, 200, 12))


def s1():
    for b, r, c, lane in S1_AT:
        yield from hidden_peak_pair("S1", f"S1-b{b}-r{r}-t{c}-l{lane}", LAY7, LAY7.run_lo(b, r, c) + lane)


# ---------------------------------------------------------------------------
# S2: the certificate boundary.  An anchor peak of height 5/2 (written under any theta) and one dip at CMIN inside the probed
# chunk only; one tile of one pair combed so that theta - CMIN = 1 -/+ 1/64.  Every other chunk has minimum 0 and passes.
ANCHOR = np.float32(2.5)      # (half of it still clears min_prominence by 1/4: the multi-needle test halves the scores)
L_CERT = {"pass": np.float32(0.25) - G, "fail": np.float32(0.25) + G}
TILE_CYCLE = (0, 1, 127, 128, 255)


def cert_cases(fam, stem, lay, probed, dip, anchor, combos, natural=False):
    for pair, tile, overlaps, where in combos:
        for side in ("pass", "fail"):
            y = np.zeros(lay.count, dtype=np.float32)
            comb(y, lay, pair, tile, L_CERT[side])
            y[dip], y[anchor] = CMIN, ANCHOR
            name = f"{stem}-{where}-p{pair}-t{tile}-{side}"
            yield Case(name, y, lay, natural=natural, family=fam, side=side, comb=(pair, tile), probed=probed, where=where,
                       fails={probed} if side == "fail" and overlaps else set(), dip=dip, anchor=anchor,
                       twin=name[:-4] + ("fail" if side == "pass" else "pass"), differ="comb")


# 8 hops + 8192 + 40 scores (block 8 = the first block of pair 4, whose second block is empty: one full row and 40 scores
# of a second, the last run with 8 scores), chunk = 3 hops.  A: overlap 2 hops + 40: chunk 1 = [3 hop, 8 hop + 40) = the
# second block of pair 1 .. 40 scores into block 8.  B: overlap 2 hops: chunk 1 ends with the last score of block 7.  The
# dip and the anchor lie in [5 hop + 40, 6 hop): in chunk 1 alone.
# (A last block WITHOUT a partner that holds fewer than 8192 scores has column tiles with no valid score at all; K3 gives
# such a tile theta = min(FLT_MAX, hist_min) + margin, which on a handle without history fails every chunk that reaches
# into the block -- one more launch, the same hits.  model() says the same; the layouts here keep a full row there.)
LAY9A = Layout(HOP, 8 * HOP + ROW + 40, 3 * HOP, 2 * HOP + 40)
LAY9B = Layout(HOP, 8 * HOP + ROW + 40, 3 * HOP, 2 * HOP)
S2_DIP, S2_ANCHOR = 5 * HOP + 3 * ROW + RUN * 77 + 9, 5 * HOP + 5 * ROW + RUN * 33 + 3
# natural 2^21 plan: three blocks (the third holds 8192 + 40 scores), chunk = hop, overlap 40
NAT_HOP = R.hop_of(21, NATURAL_S)
LAYN = Layout(NAT_HOP, 2 * NAT_HOP + ROW + 40, NAT_HOP, 40, s_fixed=NATURAL_S)


def s2():
    a = [(0, 255, False, "not-overlapped"), (1, 127, True, "b0-second-of-pair")]
    a += [(2, t, True, "middle") for t in TILE_CYCLE]
    a += [(3, 128, True, "inner"), (4, 0, True, "b1-40-scores-first-of-pair"), (4, 1, True, "b1-40-scores-partial-run-in-tile")]
    yield from cert_cases("S2", "S2-A", LAY9A, 1, S2_DIP, S2_ANCHOR, a)
    b = [(3, 1, True, "b1-last-score"), (4, 0, False, "not-overlapped")]
    yield from cert_cases("S2", "S2-B", LAY9B, 1, S2_DIP, S2_ANCHOR, b)


def s2_natural():
    dip, anchor = NAT_HOP + 100 * ROW + RUN * 77 + 9, NAT_HOP + 150 * ROW + RUN * 33 + 3
    combos = [(0, 128, True, "b0-second-of-pair"), (1, 0, True, "b1-40-scores"), (1, 1, True, "b1-40-scores-partial-run")]
    yield from cert_cases("S2", "S2-N", LAYN, 1, dip, anchor, combos, natural=21)


# ---------------------------------------------------------------------------
# S3: walks over unwritten runs.  A written peak (3/4) whose other side is settled at once (a trench T3 and a stopper, as in
# peak_cases.probe); on the probed side a stopper (3/2, the only score >= theta of its run) k runs away and one low score
# Q3 > T3 in an unwritten run: "in" = the last score before the stopper (prominence 3/4 - Q3 = 1 + 1/64: kept), "out" = the
# first score beyond it (must not count: prominence 3/4: rejected).  Every certificate passes.
H3, STOP3, Q3, T3 = np.float32(0.75), np.float32(1.5), CMIN - G, CMIN - 2 * G
S3_K = (1, 7, 8, 9, 31, 32, 33)


def walk_case(stem, lay, pos, side, k, dip):
    sgn = 1 if side == "R" else -1
    y = np.zeros(lay.count, dtype=np.float32)
    y[pos] = H3
    y[pos - sgn] = y[pos - 2 * sgn] = T3
    y[pos - 3 * sgn] = STOP3
    run = (pos // RUN + sgn * k) * RUN                 # first score of the dip's run
    near, far = (run, run + RUN - 1) if side == "R" else (run + RUN - 1, run)   # its first / last score as the walk meets them
    if dip == "in":
        q, s = far, far + sgn                          # stopper: the first score of the run beyond
    else:
        q, s = near, near - sgn                        # stopper: the last score of the run before
    y[q], y[s] = Q3, STOP3
    name = f"{stem}-{side}-k{k}-{dip}"
    return Case(name, y, lay, family="S3", side=side, k=k, dip=dip, pos=pos, q=q, stopper=s, keep=dip == "in", fails=set(),
                q_run_written=False, twin=name.replace("-in", "-out") if dip == "in" else name.replace("-out", "-in"), differ="probe")


def s3():
    mid = LAY7.run_lo(1, 3, 100) + 10
    for k in S3_K:
        for dip in ("in", "out"):
            yield walk_case("S3-mid", LAY7, mid, "R", k, dip)
    for k in (2, 8, 32):
        for dip in ("in", "out"):
            yield walk_case("S3-mid", LAY7, mid, "L", k, dip)
    seam = LAY7.run_lo(0, 7, 250) + 10                 # six runs before block 1: the dip's run lies across the seam
    for k in (3, 6, 9):
        for dip in ("in", "out"):
            yield walk_case("S3-seam", LAY7, seam, "R", k, dip)
    seam = LAY7.run_lo(2, 0, 3) + 10                   # three runs into block 2 (the first block of pair 1), walking left
    for k in (2, 4):
        for dip in ("in", "out"):
            yield walk_case("S3-seam", LAY7, seam, "L", k, dip)


# ---------------------------------------------------------------------------
# S4: ragged and invalid runs.  hop 61 440 = 7.5 rows (row 7 holds tiles 0 .. 127 only) and a block computes 500 scores
# beyond its hop: block b's invalid runs (7, 128 ..) hold the first scores of block b + 1.  Six blocks, the last with
# 177 scores (its last run holds 17); chunks of 2 hops + 777 with 3000 scores of overlap.
LAYR = Layout(RAGGED_HOP, 5 * RAGGED_HOP + RUN * 5 + 17, 2 * RAGGED_HOP + 777, 3000, raw_hop=RAGGED_RAW)
LAYNR = Layout(NAT_HOP, 2 * NAT_HOP + ROW + 40, NAT_HOP + 5000, 40, s_fixed=NATURAL_S)


def end_of_array_pair(fam, stem, lay, natural=False):
    """The peak at the last-but-one score, the chunk minimum at the very last; kept / rejected by one step."""
    last_chunk = len(lay.chunks()) - 1
    for side, h in (("keep", np.float32(0.75) + G), ("reject", np.float32(0.75) - G)):
        y = np.zeros(lay.count, dtype=np.float32)
        p = lay.count - 2
        y[p], y[p + 1], y[p - (ROW - 3200)] = h, CMIN, CMIN
        yield Case(f"{stem}-{side}", y, lay, natural=natural, family=fam, side=side, pos=p, keep=side == "keep", fails=set(), chunk=last_chunk,
                   twin=f"{stem}-{'reject' if side == 'keep' else 'keep'}", differ="peak")


def s4():
    h = RAGGED_HOP
    yield from hidden_peak_pair("S4", "S4-last-valid-run", LAYR, 2 * h - 1, dr=500)           # (block 1, row 7, tile 127, lane 31)
    yield from hidden_peak_pair("S4", "S4-first-score-of-block", LAYR, 2 * h, dr=500)        # (block 2, row 0, tile 0, lane 0)
    # the right-hand dip is block 2's score 100 = block 1's invalid run (7, 131): it must not lower pair 0's tile 131
    yield from hidden_peak_pair("S4", "S4-invalid-run-holds-dip", LAYR, LAYR.run_lo(1, 6, 131) + 9, dr=2 * h + 100 - (LAYR.run_lo(1, 6, 131) + 9))
    yield from end_of_array_pair("S4", "S4-end-of-array", LAYR)


def s4_natural():
    yield from hidden_peak_pair("S4", "S4-N-last-valid-run", LAYNR, NAT_HOP - 1, dr=1000, natural=21)
    yield from end_of_array_pair("S4", "S4-N-end-of-array", LAYNR, natural=21)


# ---------------------------------------------------------------------------
# S5: chunk edges.  The run that holds a chunk's first or last score has maximum 0 < theta: only the edge rule writes it.
# A peak (1 - 1/64) 40 scores inside the chunk, its other side settled by a trench; towards the edge the floor is 0 and one
# low score Q5 sits ON the edge score ("in": prominence 5/4 - 1/64, kept) or one place beyond it ("out": prominence
# 1 - 1/64, rejected in this chunk).  Every certificate passes.
H5, Q5, T5 = np.float32(1.0) - G, CMIN, CMIN - G


def edge_case(stem, lay, edge, kind, dip, natural=False):
    """kind "end": `edge` is chunk i's last score, the walk goes right; "start": its first score, the walk goes left."""
    sgn = 1 if kind == "end" else -1
    y = np.zeros(lay.count, dtype=np.float32)
    p = edge - sgn * 40
    y[p] = H5
    y[p - sgn] = y[p - 2 * sgn] = T5
    y[p - 3 * sgn] = STOP3
    q = edge if dip == "in" else edge + sgn
    y[q] = Q5
    name = f"{stem}-{kind}-lane{edge % RUN}-{dip}"
    return Case(name, y, lay, natural=natural, family="S5", kind=kind, dip=dip, edge=edge, lane=edge % RUN, pos=p, q=q, fails=set(),
                edge_run=lay.run_of(edge)[:3], twin=name[:-len(dip)] + ("out" if dip == "in" else "in"), differ="probe")


def s5_layouts():
    """(layout, kind, edge): start edges with no overlap (the peak lies in one chunk; the previous chunk's last score is
    the start edge's neighbour), at a block seam and one score either side of it; end edges on the last and the first score of a block and mid-block; short chunks (chunk < hop + 32:
    K3 finds the edges per run, not per block)."""
    n = 7 * HOP
    for chunk in (3 * HOP, 3 * HOP + 1, 3 * HOP - 1, 3 * HOP - 1000 + 6):          # lanes 0 (on the seam), 1, 31, 30
        yield Layout(HOP, n, chunk, 0), "start", chunk
    # ... and with 5000 scores of overlap: the previous chunk's end edge lies elsewhere, so the start-edge run is written for
    # the start edge alone (lanes 31, 1, 30; chunk 0 holds the peak too and keeps it either way: "in" adds chunk 1's copy)
    for chunk in (3 * HOP - 1, 3 * HOP + 1, 3 * HOP - 1000 + 6):
        yield Layout(HOP, n, chunk, 5000), "start", chunk
    c = 3 * HOP - 1000
    for e in (4 * HOP, 4 * HOP - 1, 3 * HOP + 5 * ROW + RUN * 9 + 1, 3 * HOP + 2 * ROW + RUN * 200 + 30):   # lanes 0, 31, 1, 30
        yield Layout(HOP, n, c, e + 1 - c), "end", e
    for lane in (1, 30):
        chunk = next(ch for ch in range(30001, 30200) if (5 * ch) % RUN == lane)
        yield Layout(HOP, n, chunk, 0), "start", 5 * chunk
    for lane, ov in ((0, 701), (31, 700)):
        chunk = next(ch for ch in range(30001, 30200) if (6 * ch + ov - 1) % RUN == lane)
        yield Layout(HOP, n, chunk, ov), "end", 6 * chunk + ov - 1


def s5():
    for i, (lay, kind, edge) in enumerate(s5_layouts()):
        for dip in ("in", "out"):
            yield edge_case(f"S5-{i}-c{lay.chunk}-o{lay.ov}", lay, edge, kind, dip)


def s5_natural():
    h = NAT_HOP
    for i, (lay, kind, edge) in enumerate(((Layout(h, 2 * h + ROW + 40, h + 1, 0, s_fixed=NATURAL_S), "start", h + 1),
                                           (Layout(h, 2 * h + ROW + 40, h - 3000, 3000, s_fixed=NATURAL_S), "end", h - 1))):
        for dip in ("in", "out"):
            yield edge_case(f"S5-N-{i}", lay, edge, kind, dip, natural=21)


# ---------------------------------------------------------------------------
# S6: the ring of a handle's recent chunk minima (8 entries per scale).  U: an S1 "unwritten" case (fails on a fresh
# handle; its tile's comb lies at L_UNWRITTEN).  D: a chunk minimum of -2 -- once in the ring, theta = -3/2 everywhere and U
# passes.  Q: a floor of 1/2 > L_UNWRITTEN with one peak: passes, and its minimum in the ring lowers no theta of U.
def s6_designs():
    u = next(c for c in s1() if c.name == "S1-b1-r4-t127-l17-unwritten")
    d = np.zeros(LAY7.count, dtype=np.float32)
    d[LAY7.run_lo(1, 2, 40) + 3], d[LAY7.run_lo(4, 2, 40) + 3] = -2.0, 2.0
    q = np.full(LAY7.count, 0.5, dtype=np.float32)
    q[LAY7.run_lo(3, 3, 30) + 7] = 2.5
    return u, Case("S6-D", d, LAY7, family="S6", fails={0}), Case("S6-Q", q, LAY7, family="S6", fails=set())


def s6():
    yield from s6_designs()


# ---------------------------------------------------------------------------
# T: the 2^22 plan by the library's own choice (a needle of 441 000 samples) with an odd block count of 3: with the option
# tail_block = 1 the last block runs on the 2^21 plan with every run written, with 0 as the first half of a pair of its own.
# The hidden peak of S1 in block nblocks - 2 and in the tail block.  (meta describes tail_block = 0.)
TAIL_S = 441000
T_HOP = R.hop_of(22, TAIL_S)
LAYT = Layout(T_HOP, 2 * T_HOP + ROW + 40, 2 * T_HOP - 5000, 3000, s_fixed=TAIL_S)


def tail_cases():
    yield from hidden_peak_pair("T", "T-block1", LAYT, LAYT.run_lo(1, 200, 77) + 5, natural=22, chunk=0)
    yield from hidden_peak_pair("T", "T-tail-block", LAYT, LAYT.run_lo(2, 0, 77) + 5, natural=22, chunk=1)


FAMILIES = {"S1": s1, "S2": s2, "S3": s3, "S4": s4, "S5": s5}
NATURAL = {"S2": s2_natural, "S4": s4_natural, "S5": s5_natural, "T": tail_cases}


def cases(family, natural=False):
    return (NATURAL if natural else FAMILIES)[family]()


def all_cases():
    for f in FAMILIES:
        yield from FAMILIES[f]()
    for f in NATURAL:
        yield from NATURAL[f]()
    yield from s6()


# ---------------------------------------------------------------------------
# The several-needle engine: three impulse needles of one length give three score arrays of one haystack.
MULTI_Q = 37


def multi_cases():
    by = {c.name: c for c in list(s1()) + list(s2()) if c.name in MULTI_NAMES}
    return [by[n] for n in MULTI_NAMES] + [c for c in s5() if c.name.startswith(("S5-4-", "S5-7-"))]


MULTI_NAMES = ("S1-b1-r4-t127-l17-unwritten", "S1-b1-r4-t127-l17-written", "S1-b1-r0-t0-l0-unwritten", "S2-A-middle-p2-t127-fail",
               "S2-A-middle-p2-t127-pass", "S2-A-b1-40-scores-partial-run-in-tile-p4-t1-fail")


def multi_scores(y):
    """Needle (index 0, gain 1): the design; (index 0, gain 2): design / 2 under AM_SCALE_LIB -- no S1 peak reaches
    min_prominence and the certificate that fails for the first needle passes; (index MULTI_Q, gain 1): the design
    shifted by MULTI_Q -- every run, tile and chunk edge holds other scores."""
    return [y, y * np.float32(0.5), np.concatenate([y[MULTI_Q:], np.zeros(MULTI_Q, dtype=np.float32)])]


def shrink(case, k=16):
    """The case at 1/k of its size, for a run through the checker's own correlation: of every k scores the one of largest
    magnitude (combs, peaks, dips, trenches and stoppers survive in order), chunk and overlap divided by k."""
    y = case.y[:case.y.size // k * k].reshape(-1, k)
    z = y[np.arange(y.shape[0]), np.abs(y).argmax(axis=1)]
    lay = case.layout
    return z, max(lay.chunk // k, 1), lay.ov // k
