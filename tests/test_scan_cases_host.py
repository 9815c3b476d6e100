"""CPU: the designed score arrays of tests/scan_cases.py are what they claim to be.  expected() is held to
oracle.calc_chunks on an impulse needle; every case is on the grid, keeps its margins under model(), has the meta its
generator states (which run is written, which chunks fail, where the chunk minimum lies), differs from its twin only in
the intended scores, and gives the same hits when every score moves by up to TOL (rounding must not decide a case).
(tests/test_gpu_scan_cases.py runs them through am_match*.)"""
import numpy as np
import pytest

import plan_geometry_ref as R
import scan_cases as sc
from policy_cases import PEAK_POLICIES

GROUPS = [(f, False) for f in sc.FAMILIES] + [(f, True) for f in sc.NATURAL] + [("S6", False)]
STEP = float(sc.G)


def family_cases(family, natural):
    return sc.s6() if family == "S6" else sc.cases(family, natural)


def small_params(s, chunk, ov, prom=1.0, dist=0, overshadow=0.0):
    return sc.Params(sc.SR, s, chunk, s - 1 + ov, prom, dist, overshadow)


def check_against_oracle(oracle, z, p, pol, what):
    needle = np.zeros(p.S, dtype=np.float32)
    needle[0] = 1.0
    hay = np.concatenate([z, np.zeros(p.S - 1, dtype=np.float32)])
    want = oracle.calc_chunks(p.sr, hay, needle, p.chunk, p.overlap, p.prom, p.dist, p.overshadow_s, pol=pol)
    got = sc.expected(z, p, pol)
    assert [(g[0], g[1]) for g in got] == [(w[0], w[1]) for w in want], what
    for g, w in zip(got, want):
        assert abs(g[2] - w[2]) <= 1e-6 and abs(g[3] - w[3]) <= 1e-6, (what, g, w)
    return len(want)


def test_expected_equals_calc_chunks_on_an_impulse_needle(oracle):
    """S = 100, a few 10^4 scores: a designed-style array (grid values, peaks, trenches, twins at distances around a
    min_distance of 40, neighbours within the overshadow distance) under several chunk / overlap choices -- one with a
    short last window, one whose last window is shorter than the needle -- and every policy."""
    rng = np.random.default_rng(11)
    z = (np.round(rng.standard_normal(30011) * 8) / 64).astype(np.float32)
    for i, q in enumerate(range(500, 30000, 700)):
        z[q] = 1.5 + (i % 7) / 64.0
        z[q + (25, 39, 40, 41, 90)[i % 5]] = 1.25 + (i % 5) / 64.0
    n = 0
    for chunk, ov in ((30011, 0), (8000, 0), (8000, 500), (7001, 2999), (2999, 41), (29950, 0), (30011 + 50, 0)):
        for order, rule in PEAK_POLICIES:
            for tail, surr in ((0, 0), (1, 0), (0, 1), (1, 1)):
                pol = oracle.policy(order, rule, tail, surr)
                for dist, shadow in ((0, 0.0), (40, 0.0), (40, 0.02), (10 ** 9, 1.0)):
                    n += check_against_oracle(oracle, z, small_params(100, chunk, ov, 1.0, dist, shadow), pol, (chunk, ov, order, rule, tail, surr, dist, shadow))
    assert n > 1000


@pytest.mark.parametrize("family,natural", GROUPS)
def test_expected_equals_calc_chunks_on_shrunk_cases(oracle, family, natural):
    """A sample of every family at 1/16 (1/128 for the natural plan's layouts) of its size, through the checker's own
    correlation, with and without policies."""
    k = 128 if natural else 16
    pols = [None, oracle.policy(1, 3, 1, 1)]
    for i, c in enumerate(family_cases(family, natural)):
        if i % 3 and family != "S6":
            continue
        z, chunk, ov = sc.shrink(c, k)
        for pol in pols:
            check_against_oracle(oracle, z, small_params(100, chunk, ov, float(c.prom), c.dist), pol, (c.name, pol is not None))


def margins(c, m, oracle):
    """Every comparison K3, the certificate and the pick make on this design lies at least one grid step from equality."""
    for b in range(c.layout.nblocks):
        gap = np.abs(m.rmax[b] - m.theta[b // 2][None, :])[m.valid[b]]
        assert gap.min() >= STEP, (c.name, "run maximum against theta", b)
    for i, ch in enumerate(m.chunks):
        if ch["b"] - ch["a"] < 3:
            continue
        assert abs(float(ch["theta_max"] - ch["cmin"]) - float(c.prom)) >= STEP, (c.name, "certificate", i, ch)
        for s, e, h, pr in oracle.find_peaks(c.y[ch["a"]:ch["b"]], 0.0, 0, cap=1 << 16):
            assert abs(h - float(ch["cmin"]) - float(c.prom)) >= STEP and abs(pr - float(c.prom)) >= STEP, (c.name, "peak", i, s, h, pr)
            assert e - s == 1 or pr < float(c.prom), (c.name, "a designed peak is a plateau", i, s, e)


def meta_agrees(c, m):
    lay, meta = c.layout, c.meta
    assert sc.failing(m) == meta["fails"], (c.name, sc.failing(m), meta["fails"], m.chunks)
    if "run_written" in meta:                        # S1 / S4: the hidden peak
        b, r, t = meta["run"]
        assert lay.run_of(meta["pos"])[:3] == (b, r, t) and bool(m.written[b][r, t]) == meta["run_written"], (c.name, lay.place(meta["pos"]))
        assert m.tile_min[b // 2, t] == c.y[lay.run_lo(b, r, t)] or meta["pos"] == lay.run_lo(b, r, t), c.name   # the comb is the tile's minimum
        for d in meta["dips"]:                       # the chunk minimum lies in other tiles, inside the failing chunk
            assert lay.run_of(d)[2] != t or lay.run_of(d)[0] // 2 != b // 2, (c.name, lay.place(d))
            assert c.y[d] == min(ch["cmin"] for ch in m.chunks), c.name
        others = np.delete(m.theta[b // 2], t)
        assert others.max() < m.theta[b // 2, t], (c.name, "only the peak's tile has the deciding theta")
    if c.meta["family"] == "S2":
        p, t = meta["comb"]
        assert m.theta[p, t] == m.theta.max() and (m.theta == m.theta.max()).sum() == 1, c.name
        ch = m.chunks[meta["probed"]]
        assert ch["a"] <= meta["dip"] < ch["b"] and sum(q["a"] <= meta["dip"] < q["b"] for q in m.chunks) == 1, c.name
        assert (ch["b0"] // 2 <= p <= ch["b1"] // 2) == (meta["where"] != "not-overlapped"), (c.name, ch)
    if c.meta["family"] == "S3":
        b, r, t, _ = lay.run_of(meta["q"])
        assert not m.written[b][r, t] and m.valid[b][r, t], (c.name, lay.place(meta["q"]))
        b, r, t, _ = lay.run_of(meta["stopper"])
        v = c.y[lay.run_lo(b, r, t):lay.run_lo(b, r, t) + sc.RUN]
        assert m.written[b][r, t]
        if (b, r, t) != lay.run_of(meta["pos"])[:3]:
            assert (v >= m.theta[b // 2, t]).sum() == 1, (c.name, "the stopper is the only score >= theta of its run")
        b, r, t, _ = lay.run_of(meta["pos"])
        assert m.written[b][r, t]
    if c.meta["family"] == "S5":
        b, r, t = meta["edge_run"]
        assert m.written[b][r, t] and m.rmax[b][r, t] < m.theta[b // 2, t], (c.name, "only the edge rule writes the edge run")
        assert meta["edge"] in [ch["a"] for ch in m.chunks] + [ch["b"] - 1 for ch in m.chunks], c.name
        qb, qr, qt, _ = lay.run_of(meta["q"])
        assert m.rmax[qb][qr, qt] < m.theta[qb // 2, qt], c.name            # (Q5's run too: written, if at all, by the edge rule)


def twin_differs_as_intended(c, other):
    lay = c.layout
    assert other.layout.__dict__ == lay.__dict__ and other.prom == c.prom and other.dist == c.dist
    at = np.flatnonzero(c.y != other.y)
    assert at.size > 0
    how = c.meta["differ"]
    if how == "comb":
        p, t = c.meta["comb"]
        for q in at:
            b, r, tt, _ = lay.run_of(int(q))
            assert b // 2 == p and tt == t, (c.name, lay.place(int(q)))
    elif how == "peak":
        assert at.tolist() == [c.meta["pos"]]
    else:
        allowed = {m[k] for m in (c.meta, other.meta) for k in ("q", "stopper") if k in m}
        assert {c.meta["q"], other.meta["q"]} <= set(at.tolist()) <= allowed, (c.name, at)


@pytest.mark.parametrize("family,natural", GROUPS)
def test_design_properties(oracle, family, natural):
    waiting = {}
    n = 0
    for c in family_cases(family, natural):
        n += 1
        assert sc.on_grid(c.y), c.name
        for log_n in c.log_ns():
            assert R.hop_of(log_n, c.layout.needle_len(log_n)) == c.layout.hop
        m = sc.model(c.y, c.layout, c.prom)
        margins(c, m, oracle)
        meta_agrees(c, m)
        twin = c.meta.get("twin")
        if twin is None or family == "S6":
            continue
        if twin in waiting:
            twin_differs_as_intended(c, waiting.pop(twin))
        else:
            waiting[c.name] = c
    assert n > 0 and not waiting, list(waiting)


@pytest.mark.parametrize("family,natural", GROUPS)
def test_both_sides_of_every_boundary_are_present(family, natural):
    """Twins come in pairs with opposite outcomes: one fails a certificate and the other passes (S1, S2, S4's hidden peaks),
    or one keeps the probed peak and the other rejects it (S3, S4's end of the array, S5)."""
    by = {c.name: c.meta for c in family_cases(family, natural)}
    for name, meta in by.items():
        if meta.get("twin") not in by:
            continue
        o = by[meta["twin"]]
        if meta["differ"] == "comb":
            if meta.get("where") == "not-overlapped":
                assert not meta["fails"] and not o["fails"]
            else:
                assert bool(meta["fails"]) != bool(o["fails"]), name
        else:
            assert meta.get("keep", meta.get("dip") == "in") != o.get("keep", o.get("dip") == "in"), name


@pytest.mark.parametrize("family,natural", GROUPS)
def test_rounding_does_not_decide(oracle, family, natural):
    """expected(design + e), e uniform in +-TOL, three seeds: the same (start, end) list; heights within TOL and
    prominences within 2 TOL of the unperturbed ones.  A condition on the designs -- no case is left out."""
    for c in family_cases(family, natural):
        same_hits_under_rounding(c.name, c.y, c.params(c.log_ns()[0]))


def same_hits_under_rounding(name, y, p):
    base = sc.expected(y, p)
    for seed in (1, 2, 3):
        e = (np.random.default_rng([seed, y.size]).random(y.size, dtype=np.float32) * 2 - 1) * np.float32(R.TOL)
        got = sc.expected(y + e, p)
        assert [(g[0], g[1]) for g in got] == [(b[0], b[1]) for b in base], (name, seed)
        for g, b in zip(got, base):
            assert abs(g[2] - b[2]) <= R.TOL * 1.001 and abs(g[3] - b[3]) <= 2 * R.TOL * 1.001, (name, seed, g, b)
    return base


def test_multi_needle_scores_are_robust_too():
    """The three score arrays the several-needle test derives from a case (the design, half of it, shifted by 37): rounding
    decides none of them; half an S1 design holds no hit, half an S2 design keeps its anchor, and the certificate that
    fails for the design passes for its half."""
    for c in sc.multi_cases():
        p = c.params(c.log_ns()[0])
        own = sc.multi_scores(c.y)
        hits = [same_hits_under_rounding((c.name, j), y, p) for j, y in enumerate(own)]
        assert sc.on_grid(own[1] * 2) and own[2][:-sc.MULTI_Q].tolist() == c.y[sc.MULTI_Q:].tolist()
        if c.meta["family"] == "S1":
            assert hits[1] == [] and len(hits[0]) >= 1
        if c.meta["family"] == "S2":
            assert [h[0] for h in hits[1]] == [c.meta["anchor"]] == [h[0] + sc.MULTI_Q for h in hits[2]]
        assert sc.failing(sc.model(own[1], c.layout, c.prom)) == set()


def test_the_ring_sequence_is_what_the_model_says():
    """S6 under model(): U fails on a fresh handle (hist_min = none) and with Q's minimum in the ring; it passes with D's
    or its own minimum there.  D fails, Q passes -- whatever the ring holds for Q."""
    u, d, q = sc.s6_designs()
    lay = u.layout
    u_min, d_min, q_min = (float(c.y.min()) for c in (u, d, q))
    assert sc.failing(sc.model(u.y, lay)) == {0}
    assert sc.failing(sc.model(u.y, lay, hist_min=q_min)) == {0}
    assert sc.failing(sc.model(u.y, lay, hist_min=d_min)) == set()
    assert sc.failing(sc.model(u.y, lay, hist_min=u_min)) == set()
    assert sc.failing(sc.model(d.y, lay)) == {0} and sc.failing(sc.model(q.y, lay)) == set()
    assert sc.failing(sc.model(q.y, lay, hist_min=d_min)) == set()
    for hist in (u_min, d_min, q_min):        # ... and none of these sits within a grid step of a boundary
        m = sc.model(u.y, lay, hist_min=hist)
        for ch in m.chunks:
            assert abs(float(ch["theta_max"] - ch["cmin"]) - 1.0) >= STEP
