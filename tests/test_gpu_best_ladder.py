"""GPU: the k-best selection (am_best.hip) on the designed arrays of tests/best_cases.py, which reach every rung of its
ladder: the refinement of a crowded bin, both descent depths, the second listing pass of the transitions, the finite
fallback past 2^20 candidates and the descent that lists them all.  am_find_peaks_top must equal the head of the
checker's list bit for bit (start, end, height bits, prominence bits, order); with non-finite scores the expectation is
union_top over the finite stretches, served by the checker.  am_match_best is held to the same on a haystack whose
samples hold thousands of non-finite runs.
(tests/test_best_cases_host.py holds the designs and the model to their claims, without a GPU.)

The round count: profile name "peaks" brackets best_compact + best_prom, once per listing round of best_select and
nothing else on the routes that do not fall back (ProfScope counts every launch of a class under the default options
profile_mask = -1, profile_every = 1), so gpu.Profile's count for "peaks" must equal best_cases.rounds_needed."""
import numpy as np
import pytest

import best_cases as bc
from policy_cases import PEAK_POLICIES
from test_gpu_best import SR, planted, policy_set, stretches_of, union_top
from test_gpu_peak_cases import bits, checker_as_gpu

pytestmark = pytest.mark.gpu

_FULL = {}       # (case, prom, dist, order, rule) -> the checker's whole list, computed once and never changed
_LADDER = {}     # (case, M) -> the model's rounds


def full_list(gpu, oracle, name, y, prom, dist, pol=(0, 0)):
    key = (name, prom, dist) + tuple(pol)
    if key not in _FULL:
        if bc.transitions(y).size == 0:
            _FULL[key] = oracle.find_peaks(y, prom, dist, cap=y.size, pol=oracle.policy(*pol) if pol != (0, 0) else None)
        else:
            assert dist == 0 and pol == (0, 0)      # (the distance rule between stretches is not the per-stretch answer)
            _FULL[key] = [(q.start, q.end, q.height, q.prominence) for q in union_top(checker_as_gpu(gpu, oracle), y, prom, 0, y.size)]
    return _FULL[key]


def taus(name, y, k):
    key = (name, max(8 * k, 4096))
    if key not in _LADDER:
        L = bc.ladder(y, k)
        assert not L.fallback
        _LADDER[key] = [r[0] for r in L.rounds]
    return _LADDER[key]


def ks_of(k, full):
    return sorted({1, k, max(1, len(full))})


def run_triple(gpu, name, y, full, triple, bad, label=()):
    """k in {1, k, all}: the library's list against the head of `full`, its listing rounds against the model's."""
    k0, prom, dist = triple
    for k in ks_of(k0, full):
        with gpu.Profile(0) as prof:
            got = gpu.find_peaks_top(y, k, prom, dist)
            rounds = prof.query("peaks")[1]
        exp_rounds = bc.rounds_needed(taus(name, y, k), full, k)
        print("%s %s k=%d: %d peaks, %d listing rounds (model %d)" % (name, label + (k0, prom, dist), k, len(got), rounds, exp_rounds))
        if bits(got) != bits(full[:k]):
            first = next((i for i, (g, e) in enumerate(zip(bits(got), bits(full[:k]))) if g != e), min(len(got), len(full[:k])))
            bad.append((name, label, triple, k, "peaks", len(got), len(full[:k]), "first difference at", first))
        if rounds != exp_rounds:
            bad.append((name, label, triple, k, "rounds", rounds, exp_rounds))


def report(bad):
    assert not bad, f"{len(bad)} mismatches, first: {bad[:5]}"


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_top_equals_checker_and_runs_the_models_rounds(gpu, oracle, name):
    """Every triple of the case, k in {1, k, all}: the checker's head, and as many listing rounds as the model says."""
    _, y, triples = bc.case(name)
    bad = []
    for triple in triples:
        run_triple(gpu, name, y, full_list(gpu, oracle, name, y, triple[1], triple[2]), triple, bad)
    report(bad)


FAMILY_FIRST = sorted({fam: name for name, fam in sorted(bc.FAMILY_OF.items(), reverse=True)}.values())


@pytest.mark.parametrize("name", FAMILY_FIRST)
def test_device_form_equals_host_form(gpu, oracle, name):
    _, y, triples = bc.case(name)
    buf = gpu.DeviceBuffer.from_numpy(0, np.ascontiguousarray(y))
    k, prom, dist = triples[-1]
    full = full_list(gpu, oracle, name, y, prom, dist)
    for kk in ks_of(k, full):
        dev = gpu.find_peaks_top_device(0, buf.ptr, y.size, kk, prom, dist)
        assert bits(dev) == bits(gpu.find_peaks_top(y, kk, prom, dist)) == bits(full[:kk]), (name, kk)


POLICY_PARAMS = [(name, order) for name in sorted(bc.POLICY_TRIPLES) for order in (0, 1)]


@pytest.mark.parametrize("name,order", POLICY_PARAMS)
def test_policies(gpu, oracle, name, order):
    """crowded and ramp under every (peak_filter_order, distance_rule), a prominence bound and a min_distance both
    active; under order 1 a candidate that fails the bound still suppresses its neighbours."""
    _, y, _ = bc.case(name)
    bad = []
    for o, rule in PEAK_POLICIES:
        if o != order:
            continue
        for triple in bc.POLICY_TRIPLES[name]:
            full = full_list(gpu, oracle, name, y, triple[1], triple[2], (o, rule))
            with policy_set(gpu, peak_filter_order=o, distance_rule=rule):
                run_triple(gpu, name, y, full, triple, bad, (o, rule))
    report(bad)


# ---------------------------------------------------------------------------
# past the cap: the only arrays above 2^18
class head_checker(checker_as_gpu):
    """The checker's first 64 peaks of a stretch: enough for a k of 10, without a million tuples."""
    def find_peaks(self, y, prom, dist, cap=None):
        return checker_as_gpu.find_peaks(self, y, prom, dist, cap=64)


def test_past_the_cap_finite_falls_back_to_the_whole_array_pick(gpu, oracle):
    """More than 2^20 candidates in one key, all finite: find_peaks_host_array, truncated == the checker's head."""
    name, y, triples = bc.BIG["past_cap_finite"]()
    for k0, prom, dist in triples:
        head = oracle.find_peaks(y, prom, dist, cap=64)
        for k in sorted({1, k0}):
            assert bits(gpu.find_peaks_top(y, k, prom, dist)) == bits(head[:k]), (name, k, dist)
    assert len(oracle.find_peaks(y, 0.0, y.size, cap=64)) == 1


def test_past_the_cap_with_a_nan_lists_every_candidate(gpu, oracle):
    """The same array with one NaN keeps descending: one listing round of more than 2^20 candidates.  min_distance = n:
    any two positions are closer than n, so the first peak of the order suppresses every other one, also across the
    NaN -- the expectation is the head of the min_distance = 0 list."""
    name, y, triples = bc.BIG["past_cap_nan"]()
    n = y.size
    assert triples == [(10, 0.0, 0), (3, 0.0, n)]
    whole = union_top(head_checker(gpu, oracle), y, 0.0, 0, 10, [(0, n // 2), (n // 2 + 1, n)])
    assert len(whole) == 10
    for k, dist, exp in ((1, 0, whole[:1]), (10, 0, whole), (3, n, whole[:1])):
        with gpu.Profile(0) as prof:
            got = gpu.find_peaks_top(y, k, 0.0, dist)
            rounds = prof.query("peaks")[1]
        assert bits(got) == bits(exp), (name, k, dist)
        assert rounds == 1, (name, k, dist, rounds)


# ---------------------------------------------------------------------------
def gapped_haystack():
    """60 s at 8 kHz with five plants; every fifth sample of a 12 000-sample zone non-finite (2400 runs, 4800
    transitions), a single NaN and a single +inf elsewhere, the last sample -inf."""
    S = SR // 2
    needle, hay, offs = planted(14, 60, S, [0.9, 0.6, 1.2, 0.8, 1.0])
    zone = np.arange(200001, 212001, 5)
    hay[zone] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[np.arange(zone.size) % 3]
    hay[100000] = np.nan
    hay[300000] = np.inf
    hay[-1] = -np.inf
    return S, needle, hay


@pytest.mark.parametrize("norm", [False, True])
def test_match_best_with_thousands_of_nonfinite_runs_in_the_samples(gpu, oracle, norm):
    """f32 samples: the transitions of the samples overflow the scan's own list (the second listing pass, mode 1 twice).
    Expected as in test_nonfinite_samples_cost_their_windows: per finite stretch of at least S samples the library's own
    scores, then the checker's per-stretch peaks, ordered and truncated."""
    S, needle, hay = gapped_haystack()
    assert bc.transitions(hay).size > bc.TRANS_CAP and (~np.isfinite(hay)).sum() > 2100
    algo = gpu.HipConvolve(needle, score_norm=norm)
    sample_stretches = stretches_of(hay)
    score_stretches = [(a, b - S + 1) for a, b in sample_stretches if b - a >= S]
    assert len(score_stretches) == 4 and len(sample_stretches) > 2100
    scores = np.full(hay.size - S + 1, np.nan, dtype=np.float32)
    for a, b in sample_stretches:
        if b - a >= S:
            scores[a:b - S + 1] = algo.correlate_with_sample(hay[a:b], gpu.Mode.Valid, scale=True)
    ref = checker_as_gpu(gpu, oracle)
    # (k = 1000 is more than min_distance = S leaves: every survivor of every stretch is compared)
    for k, dist, prom in ((20, S // 2, 0.0), (5, 0, 0.0), (1000, S, 0.0)):
        got = algo.match_best(hay, k, min_distance=dist, min_prominence=prom)
        assert bits(got) == bits(union_top(ref, scores, prom, dist, k, score_stretches)), (k, dist, prom)
        assert len(got) == k or k == 1000
        if k == 1000:   # every score stretch contributes
            assert {i for q in got for i, (a, b) in enumerate(score_stretches) if a <= q.start < b} == {0, 1, 2, 3}
        for q in got:
            assert np.all(np.isfinite(hay[q.start:q.start + S]))
    algo.close()


@pytest.mark.parametrize("norm", [False, True])
def test_match_best_i16_stereo_form_of_the_gapped_signal(gpu, oracle, norm):
    """The i16 stereo form of the same signal (i16 holds no non-finite sample: they become 0): am_match_best on the frames
    equals the checker's head over the library's scores of the bit-exact down-mix."""
    S, needle, hay = gapped_haystack()
    fin = np.where(np.isfinite(hay), hay, np.float32(0))
    rng = np.random.default_rng(15)
    st = np.stack([fin * 20000, fin * 20000 + rng.normal(0, 300, fin.size)], axis=1).clip(-32768, 32767).astype(np.int16)
    mono = gpu.pcm_s16_stereo_to_mono(st)
    algo = gpu.HipConvolve(needle, score_norm=norm)
    scores = algo.correlate_with_sample(mono, gpu.Mode.Valid, scale=True)
    exp = oracle.find_peaks(scores, 0.0, S // 2, cap=scores.size)[:20]
    assert bits(algo.match_best(st, 20, min_distance=S // 2)) == bits(exp)
    algo.close()
