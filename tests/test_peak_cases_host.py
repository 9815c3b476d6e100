"""CPU: the designed arrays of tests/peak_cases.py decide what they were designed to decide, and the checker
(oracle.find_peaks) equals a second, independent reference on them -- the definition in the header of am_peaks.hip as
the obvious loop in f32, both filter orders and the four distance rules.  A generator that fails here is a bug of the
test, found before any GPU time is spent."""
import numpy as np
import pytest

import peak_cases as pk
from policy_cases import PEAK_POLICIES


def ref_find_peaks(y, min_prom, min_dist, order=0, rule=0):
    y = np.asarray(y, dtype=np.float32)
    n = y.size
    if n < 3:
        return []
    chg = np.flatnonzero(y[1:] != y[:-1]) + 1                  # y[k] != y[k - 1]
    found = []
    for i in np.flatnonzero(y[1:n - 1] > y[:n - 2]) + 1:       # left edges: y[i - 1] < y[i], 1 <= i < n - 1
        j = np.searchsorted(chg, i, side="right")
        end = min(int(chg[j]) if j < chg.size else n, n - 1)   # the flat top never takes the last score in
        if not y[end] < y[i]:
            continue
        h = y[i]
        hi = np.flatnonzero(y[:i] > h)
        left = y[hi[-1] + 1:i] if hi.size else y[:i]
        hi = np.flatnonzero(y[end:] > h)
        right = y[end:end + hi[0]] if hi.size else y[end:]
        lmin = min(h, left.min()) if left.size else h
        rmin = min(h, right.min()) if right.size else h
        found.append((int(i), end, float(h), float(np.float32(h) - np.float32(max(lmin, rmin)))))
    passes = lambda p: np.float32(p[3]) >= np.float32(min_prom)
    if order == 0:
        found = [p for p in found if passes(p)]
    found.sort(key=lambda p: (-p[2], p[0]))
    if min_dist > 0:
        inclusive, from_start = rule & 1, (rule >> 1) & 1
        kept, pos = [], np.empty(len(found), dtype=np.int64)
        for p in found:
            m = p[0] if from_start else (p[0] + p[1]) // 2
            d = np.abs(pos[:len(kept)] - m)
            if np.any(d <= min_dist if inclusive else d < min_dist):
                continue
            pos[len(kept)] = m
            kept.append(p)
        found = kept
    return found if order == 0 else [p for p in found if passes(p)]


def bits(peaks):
    return [(int(s), int(e), np.float32(h).tobytes(), np.float32(p).tobytes()) for s, e, h, p in peaks]


def cand_of(c, peaks):
    hit = [p for p in peaks if p[0] == c.meta["cand"]]
    return hit[0] if hit else None


BIG_SAMPLE = 8


def big_sample():
    names = sorted(c[0] for f, s in pk.PARAMS for c in pk.cases(f, s) if pk.is_big(c))
    assert len(names) <= 60                      # each is a 4.5 MB host copy per call on the GPU side
    rng = np.random.default_rng(2024)
    return set(rng.choice(names, size=BIG_SAMPLE, replace=False))


@pytest.fixture(scope="module")
def sampled():
    return big_sample()


@pytest.mark.parametrize("family,side", pk.PARAMS)
def test_cases_hold_their_design(oracle, sampled, family, side):
    seen, problems, names = {}, [], set()
    for c in pk.cases(family, side):
        name, y, prom, dist = c
        m = c.meta
        assert name not in names, name
        names.add(name)
        assert y.dtype == np.float32 and pk.on_grid(y), name
        exp = oracle.find_peaks(y, prom, dist, cap=y.size)
        if not pk.is_big(c) or name in sampled:
            pols = PEAK_POLICIES if family in ("F6", "F7") and y.size <= 8 * pk.T + 1023 else [(0, 0)]
            for order, rule in pols:
                e = exp if (order, rule) == (0, 0) else oracle.find_peaks(y, prom, dist, cap=y.size, pol=oracle.policy(order, rule))
                if bits(ref_find_peaks(y, prom, dist, order, rule)) != bits(e):
                    problems.append((name, "second reference differs", order, rule))
        cd = cand_of(c, exp) if "cand" in m else None
        seen[name] = cd
        if family in ("F1", "F4", "F5") and "dip" in m:
            if m["equal"]:
                ok = cd is not None and cd[3] == 2.5            # the walk passed the equal stopper and found Q2
            elif m["dip"] in ("in", "both", "edge"):
                ok = cd is not None and cd[3] == 2.0
            else:
                ok = cd is None                                  # "out": beyond the stopper, must not count
            if m.get("d") == 1 and not m["equal"]:
                ok = cd is None                                  # a higher neighbour: no maximum at all
            if not ok:
                problems.append((name, "candidate", cd))
        if family == "F5" and m.get("behind") in ("higher", "edge") and cd is not None:
            problems.append((name, "no maximum expected", cd))
        if family == "F2" and (cd is not None) != m["keep"]:
            problems.append((name, "keep", cd))
        if family == "F3" and (cd is not None) != (m["kind"] != "reject"):
            problems.append((name, "keep", cd))
        if family == "F6":
            e1 = oracle.find_peaks(y, prom, dist, cap=y.size, pol=oracle.policy(1, 0))
            top = int(np.argmax(y))                               # first position of the chunk maximum
            want0 = [] if m["expect"] is None else [m["expect"]]
            is_peak = any(p[0] == top for p in oracle.find_peaks(y, 0.0, 0, cap=y.size))
            if m["label"] == "fast":
                ok = is_peak and [p[0] for p in exp] == [top] == want0 and [p[0] for p in e1] == [top]
            elif m["label"] == "fall":
                ok = not is_peak and [p[0] for p in exp] == want0 == [p[0] for p in e1]
            else:
                ok = is_peak and [p[0] for p in exp] == want0 and want0 != [top] and e1 == []
            if not ok:
                problems.append((name, m["label"], exp[:3], e1[:3]))
        if family in ("F7", "F8") and "count" in m:
            if len(exp) != m["count"] or exp != sorted(exp, key=lambda p: (-p[2], p[0])):
                problems.append((name, "count / order", len(exp)))
        if m.get("kind") == "chain":
            a, b, cc = m["chain"]
            starts = {p[0] for p in exp}
            if not (a in starts and b not in starts and cc in starts):
                problems.append((name, "chain"))
        if m.get("kind") == "ties" and m["md"] >= 2:
            # a gap of exactly min_dist, measured the way the array was laid out: the inclusive rule must change the answer
            r0 = 2 if m["by"] == "start" else 0
            keeps = [[p[0] for p in oracle.find_peaks(y, prom, dist, pol=oracle.policy(0, r))] for r in (r0, r0 + 1)]
            if keeps[0] == keeps[1]:
                problems.append((name, "d < min_dist and d <= min_dist agree"))
    # pairs and twins (all inside one family and side)
    for c in pk.cases(family, side) if family in ("F1", "F2", "F3", "F4", "F5") else ():
        m = c.meta
        if m.get("pair") and not m.get("equal"):
            if m["pair"] not in seen:
                problems.append((c[0], "pair missing"))
            elif (seen[c[0]] is None) == (seen[m["pair"]] is None):
                problems.append((c[0], "pair does not flip"))
        if m.get("twin"):
            if m["twin"] not in seen:
                problems.append((c[0], "twin missing"))
            elif seen[c[0]] == seen[m["twin"]]:
                problems.append((c[0], "equal variant answers as its higher twin"))
    assert not problems, problems[:20]


def test_second_reference_on_plain_inputs(oracle):
    """The second reference is not tuned to the designed arrays: noise on a coarse grid, every policy."""
    rng = np.random.default_rng(5)
    for n in (3, 4, 50, 3000):
        y = (np.round(rng.standard_normal(n) * 4) / 4).astype(np.float32)
        for order, rule in PEAK_POLICIES:
            for prom, dist in ((0.0, 0), (0.5, 0), (0.5, 3), (1.0, 40)):
                assert bits(ref_find_peaks(y, prom, dist, order, rule)) == \
                    bits(oracle.find_peaks(y, prom, dist, cap=n, pol=oracle.policy(order, rule))), (n, order, rule, prom, dist)


def test_match_haystack_decisions_have_a_margin(oracle):
    """The am_match haystacks of peak_cases.match_haystack: in every window every local maximum of the checker's scores
    lies at least 1e-3 from the prominence bound, so a score error of 1e-4 (the tolerance of the GPU comparison) cannot
    flip a keep / reject; both twins of every pair are reported, and two pairs straddle a window end / an odd chunk start."""
    needle, hay, plants = pk.match_haystack(oracle.synth_uniform)
    s, chunk, window = needle.size, pk.MATCH_CHUNK, pk.MATCH_CHUNK + pk.MATCH_OVERLAP
    margins, starts = [], set()
    for w0 in range(0, hay.size, chunk):
        w = hay[w0:w0 + window]
        if w.size < s:
            continue
        scores = oracle.correlate(w, needle, oracle.MODE_VALID, oracle.SCALE_LIB)
        for p in oracle.find_peaks(scores, 0.0, 0, cap=scores.size):
            margins.append(abs(p[3] - pk.MATCH_PROM))
            if p[3] >= pk.MATCH_PROM:
                starts.add(p[0] + w0)
    assert min(margins) >= 1e-3, min(margins)
    exp = oracle.calc_chunks(pk.MATCH_SR, hay, needle, chunk, pk.MATCH_OVERLAP, pk.MATCH_PROM, 0, 0.0)
    want = {t for pl in plants for t in pl[:2]}
    assert {e[0] for e in exp} == want == starts
    ends = {k * chunk + window - s + 1 for k in range(4)}
    assert any(a < e <= b for a, b, _, _ in plants for e in ends)
    assert any(a < k * chunk <= b and (k * chunk) % 2 for a, b, _, _ in plants for k in range(1, 6))
