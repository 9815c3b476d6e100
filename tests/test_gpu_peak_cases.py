"""GPU: the peak pick on the designed arrays of tests/peak_cases.py.  am_find_peaks must equal the checker bit for bit
(start, end, height bits, prominence bits, order) on every case -- under every peak policy for F1, F5, F6 and F7 -- and
am_find_peaks_top must return the head of that list, also with the array placed behind a non-finite separator (the only
public route on which the walk of am_walk.h runs between chunk edges that are no multiples of 32 or 1024).
(tests/test_peak_cases_host.py holds the cases and the checker to their design, without a GPU.)"""
import numpy as np
import pytest

import peak_cases as pk
from policy_cases import PEAK_POLICIES
from test_gpu_best import union_top
from test_gpu_policy import policy_set

pytestmark = pytest.mark.gpu

SEP_OFFSETS = (1, 31, 33, 1023, 1025)
NOISE_LEN = 1500          # the stretch in front of the separator: the embedded stretch starts at an odd index


def bits(peaks):
    out = []
    for q in peaks:
        s, e, h, p = q if isinstance(q, tuple) else (q.start, q.end, q.height, q.prominence)
        out.append((int(s), int(e), np.float32(h).tobytes(), np.float32(p).tobytes()))
    return out


def describe(c):
    m = c.meta
    return {k: m[k] for k in ("family", "side", "d", "D", "pm", "dip", "equal", "j", "k", "kind", "label", "behind") if k in m} | {"name": c[0]}


def report(bad):
    assert not bad, f"{len(bad)} mismatches, first: {bad[:5]}"


@pytest.mark.parametrize("family,side", pk.PARAMS)
def test_find_peaks_equals_checker(gpu, oracle, family, side):
    bad = []
    for c in pk.cases(family, side):
        name, y, prom, dist = c
        exp = oracle.find_peaks(y, prom, dist, cap=y.size)
        got = gpu.find_peaks(y, prom, dist, cap=y.size)
        if bits(got) != bits(exp):
            bad.append((describe(c), [g for g, e in zip(bits(got), bits(exp)) if g != e][:1], len(got), len(exp)))
    report(bad)


@pytest.mark.parametrize("family,side", [p for p in pk.PARAMS if p[0] in ("F1", "F5", "F6", "F7")])
def test_find_peaks_equals_checker_under_every_policy(gpu, oracle, family, side):
    """F6 (min_dist >= n) under both filter orders; F1, F5 and F7 under both orders x the four distance rules."""
    bad = []
    pols = [p for p in PEAK_POLICIES if p != (0, 0) and (family != "F6" or p[1] == 0)]
    for c in pk.cases(family, side):
        name, y, prom, dist = c
        for order, rule in pols:
            exp = oracle.find_peaks(y, prom, dist, cap=y.size, pol=oracle.policy(order, rule))
            with policy_set(gpu, peak_filter_order=order, distance_rule=rule):
                got = gpu.find_peaks(y, prom, dist, cap=y.size)
            if bits(got) != bits(exp):
                bad.append((describe(c), order, rule, len(got), len(exp)))
    report(bad)


class checker_as_gpu:
    """What union_top needs of `gpu`, served by the checker: per-stretch expectations cost no GPU call."""
    def __init__(self, gpu, oracle):
        self.Peak, self.oracle = gpu.Peak, oracle

    def find_peaks(self, y, prom, dist, cap=None):
        return [self.Peak(*e) for e in self.oracle.find_peaks(y, prom, dist, cap=cap)]


CRITICAL_D = (32, 33, 256, 257, 1024, 1025)   # every separator offset for these (at three in-tile offsets), one for the rest
# the families of 1100-tile arrays go in four parts: a part stays within a few seconds
TOP_PARAMS = [(f, s, part, 4 if f in ("F4", "F8") else 1) for f, s in pk.PARAMS for part in range(4 if f in ("F4", "F8") else 1)]


@pytest.mark.parametrize("family,side,part,nparts", TOP_PARAMS)
def test_top_equals_head_of_find_peaks(gpu, oracle, family, side, part, nparts):
    """k in {1, 2, all}; for cases without a distance rule also behind a NaN placed o scores before the array's start, a
    noise stretch in front: every o of SEP_OFFSETS for the probes at CRITICAL_D, else one o, cycling from case to case.
    (A 1100-tile array: k in {1, all}, embedded with k = all.)"""
    rng = np.random.default_rng(77)
    noise = (np.round(rng.standard_normal(NOISE_LEN) * 16) / 64).astype(np.float32)
    ref = checker_as_gpu(gpu, oracle)
    bad = []
    for i, c in enumerate(pk.cases(family, side)):
        if i % nparts != part:
            continue
        name, y, prom, dist = c
        big = pk.is_big(c)
        full = oracle.find_peaks(y, prom, dist, cap=y.size)
        for k in sorted({1, max(1, len(full))} | (set() if big else {2})):
            got = gpu.find_peaks_top(y, k, prom, dist)
            if bits(got) != bits(full[:k]):
                bad.append((describe(c), "k", k, len(got)))
        if dist != 0:
            continue       # (the distance rule applies to the union of the stretches: not the per-stretch answer)
        m = c.meta
        every = family == "F1" and m["d"] in CRITICAL_D and m["pm"] in (0, 512, 1023)
        for o in SEP_OFFSETS if every else (SEP_OFFSETS[i % len(SEP_OFFSETS)],):
            emb = np.concatenate([noise, [np.float32(np.nan)], np.full(o - 1, y[0], dtype=np.float32), y])
            stretches = [(0, NOISE_LEN), (NOISE_LEN + 1, emb.size)]
            whole = union_top(ref, emb, prom, 0, emb.size, stretches)
            for k in sorted({max(1, len(whole))} | (set() if big else {1, 2})):
                got = gpu.find_peaks_top(emb, k, prom, 0)
                if bits(got) != bits(whole[:k]):
                    bad.append((describe(c), "embedded", o, k, len(got)))
    report(bad)


def test_match_twin_plants_sparse_and_dense(gpu, oracle):
    """am_match on the haystack of peak_cases.match_haystack (twin plants 31 .. 1025 scores apart, odd chunk starts,
    a pair across a window end and one across a chunk start) == oracle.calc_chunks: positions exact, height and
    prominence within 1e-4.  Three calls on one handle (the first writes every score, the later ones only the runs
    that can matter) and one with dense_scores = 1 give identical tuples."""
    needle, hay, plants = pk.match_haystack(oracle.synth_uniform)
    sr = pk.MATCH_SR
    p = gpu.Config(chunk_size_s=10.0, overlap_length_s=2.0, distance_s=0.0, prominence=pk.MATCH_PROM).params(sr, gpu.Scale.LIB)
    p.chunk, p.overlap, p.min_distance, p.overshadow_distance_s = pk.MATCH_CHUNK, pk.MATCH_OVERLAP, 0, 0.0
    exp = oracle.calc_chunks(sr, hay, needle, p.chunk, p.overlap, pk.MATCH_PROM, 0, 0.0)
    algo = gpu.HipConvolve(needle)
    runs = [algo.match(hay, p) for _ in range(3)]
    gpu.set_option("dense_scores", 1)
    try:
        runs.append(algo.match(hay, p))
    finally:
        gpu.set_option("dense_scores", 0)
    algo.close()
    got = runs[0]
    assert [g.start for g in got] == [e[0] for e in exp]
    print("match twin plants:", len(got), "hits; max |height error|", max(abs(g.height - e[2]) for g, e in zip(got, exp)),
          "max |prominence error|", max(abs(g.prominence - e[3]) for g, e in zip(got, exp)))
    for g, e in zip(got, exp):
        assert abs(g.height - e[2]) < 1e-4 and abs(g.prominence - e[3]) < 1e-4, (g, e)
    for r in runs[1:]:
        assert bits(r) == bits(got)
