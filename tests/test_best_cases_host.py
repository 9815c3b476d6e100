"""CPU: the designed arrays of tests/best_cases.py reach the branches of am_best.hip they are designed for, by the model
of the ladder (best_cases.ladder) and the checker alone, and the model's maxima are the checker's.  No device is needed.
(tests/test_gpu_best_ladder.py runs the library on the same arrays.)"""
from collections import namedtuple

import numpy as np
import pytest

import best_cases as bc
from policy_cases import PEAK_POLICIES
from test_gpu_best import union_top

Peak = namedtuple("Peak", "start end height prominence")


class checker_only:
    """What union_top needs of `gpu`, served by the checker."""
    def __init__(self, oracle):
        self.Peak, self.oracle = Peak, oracle

    def find_peaks(self, y, prom, dist, cap=None):
        return [Peak(*e) for e in self.oracle.find_peaks(y, prom, dist, cap=cap)]


def full_list(oracle, y, prom, dist, pol=None):
    """The checker's whole list; over the finite stretches where y has non-finite scores (min_distance 0 only)."""
    if bc.transitions(y).size == 0:
        return oracle.find_peaks(y, prom, dist, cap=y.size, pol=pol)
    assert dist == 0 and pol is None
    return [tuple(q) for q in union_top(checker_only(oracle), y, prom, 0, y.size)]


def taus_of(L):
    return [r[0] for r in L.rounds]


@pytest.mark.parametrize("name,bin_", [("crowded", 3064), ("crowded_negated", 1032), ("crowded_minus_two", 1032), ("ramp", 3064),
                                       ("ramp_low", 3064)])
def test_crowded_and_ramp_refine_a_bin_on_the_first_pick(name, bin_):
    _, y, triples = bc.case(name)
    for k, _, _ in triples:
        L = bc.ladder(y, k)
        assert L.refined and L.refined[0][0] == bin_, "best_refine does not run"
        assert L.refined[0][1] > 1000, "the refined bin is not split"
        tau = L.rounds[0][0]
        assert tau >> 20 == bin_ and tau & 0xFFF00, "the first tau is not inside the refined bin"
        assert L.rounds[0][1] < 2 * max(8 * k, 4096), "the refinement does not thin the first round"
        assert L.rounds[-1][0] == 0 and len(L.rounds) == 3 and not L.fallback
    if "crowded" in name:
        assert np.count_nonzero(L.keys >> 20 == bin_) > 70000


def test_negative_families_use_the_inverted_half_of_the_key():
    for name in ("crowded_negated", "crowded_minus_two"):
        _, y, _ = bc.case(name)
        L = bc.ladder(y, 10)
        assert L.total > 80000 and int(L.keys.max()) < 0x80000000, "a height is not negative"
        h = bc.maxima(y)[2]
        assert np.all(np.diff(L.keys[np.argsort(h, kind="stable")].astype(np.int64)) >= 0), "the key does not preserve the order"


def test_one_key_cannot_be_split():
    _, y, triples = bc.case("one_key")
    for k, _, _ in triples:
        L = bc.ladder(y, k)
        assert L.total == 65535 and np.unique(L.keys >> 8).size == 1
        assert L.refined == [(3064, 1)], "not a single second-level bin"
        assert L.rounds == [(L.rounds[0][0], 65535, 65535)], "the first round does not list every maximum"
    assert np.unique(L.keys).size > 100     # (many heights inside the one 24-bit key)


def test_around_zero_has_keys_on_both_sides_and_both_zeros():
    _, y, _ = bc.case("around_zero")
    s, e, h = bc.maxima(y)
    keys = bc.height_keys(h)
    assert np.count_nonzero(keys < 0x80000000) > 1000 and np.count_nonzero(keys > 0x80000000) > 1000
    zero = h == 0
    assert np.count_nonzero(zero & np.signbit(h)) > 10 and np.count_nonzero(zero & ~np.signbit(h)) > 10
    assert np.unique(keys[zero]).tolist() == [0x80000000], "-0.0 and +0.0 are not one key"
    assert np.all(np.abs(h[~zero]) < np.finfo(np.float32).tiny), "a height is not denormal"
    assert np.count_nonzero(e - s > 1) > 100, "no plateaus"
    L = bc.ladder(y, 10)
    assert [r[0] for r in L.rounds] == [0x80000000, 0], "the first tau is not the key of zero"


def test_bin_edges_sit_on_both_levels_and_on_the_comparison_at_equality():
    _, y, _ = bc.case("bin_edges")
    keys = bc.ladder(y, 10).keys
    first = sorted(set((keys >> 20).tolist()))
    assert first == [0xBFF, 0xC00, 0xC07, 0xC08], "not both sides of two first-level edges"
    inside = sorted(set(((keys[keys >> 20 == 0xC00] >> 8) & 0xFFF).tolist()))
    assert inside == [0, 7, 8], "not both sides of a second-level edge"
    L = bc.ladder(y, 10)
    assert L.refined == [(0xC00, 3)]
    assert taus_of(L) == [0xC0000700, 0xC0000000, 0], "tau does not fall between the second-level bins, then on 2.0"
    assert bc.ladder(y, 3000).refined == []
    # exactly M maxima in the top bin: taken alone; M - 1: the next bin too
    _, y, _ = bc.case("bin_edges_4096")
    L = bc.ladder(y, 10)
    assert L.rounds[0] == (0xC08 << 20, 4096, 4096)
    _, y, _ = bc.case("bin_edges_4095")
    L = bc.ladder(y, 10)
    assert L.rounds[0][0] == 0xC07 << 20 and L.rounds[0][1] > 4096
    assert np.count_nonzero(L.keys >> 20 == 0xC08) == 4095


def test_many_gaps_overflow_the_transition_list():
    names = [n for n in bc.CASES if bc.FAMILY_OF[n] == "many_gaps"]
    assert {int(n.split("_")[2]) for n in names} == {128 * 1024 - 1, 128 * 1024, 128 * 1024 + 1}
    first = last = crowd_refined = 0
    for name in names:
        _, y, _ = bc.case(name)
        L = bc.ladder(y, 10)
        assert L.ntrans > bc.TRANS_CAP, "no second listing pass"
        assert not L.fallback and len(L.rounds) == 3
        for v in (np.nan, np.inf, -np.inf):
            assert np.count_nonzero(y == v if v == v else np.isnan(y)) > 500
        first += not np.isfinite(y[0])
        last += not np.isfinite(y[-1])
        crowd_refined += bool(L.refined)
        if y.size % 1024 == 0 and not np.isfinite(y[-1]):
            assert bc.transitions(y)[-1] == y.size      # the transition that lies in no tile
    assert first >= 2 and last >= 2 and crowd_refined == 3
    assert any(not np.isfinite(bc.case(n)[1][-1]) and bc.case(n)[1].size % 1024 == 0 for n in names)


def test_ends_cover_the_tile_multiples():
    for n in bc.ENDS_N:
        for where in bc.ENDS_WHERE:
            _, y, _ = bc.case("ends_%d_%s" % (n, where))
            t = bc.transitions(y).tolist()
            exp = ([0, 1] if where in ("first", "both") else []) + ([n - 1, n] if where in ("last", "both") else [])
            assert y.size == n and t == exp


def test_past_the_cap_falls_back_only_when_finite():
    _, y, triples = bc.BIG["past_cap_finite"]()
    assert y.size == bc.PAST_CAP_N and triples == [(10, 0.0, 0), (3, 0.0, y.size)]
    L = bc.ladder(y, 10)
    assert L.total > bc.CAP and L.fallback and L.rounds == [], "the finite array does not fall back"
    assert L.refined == [(3064, 1)]
    _, y, _ = bc.BIG["past_cap_nan"]()
    L = bc.ladder(y, 10)
    assert L.ntrans == 2 and not L.fallback
    assert len(L.rounds) == 1 and L.rounds[0][1] == L.total > bc.CAP, "the descent does not list more than 2^20 candidates"


def test_both_descent_depths_are_present(oracle):
    """ramp (12, 0.02, 0) stops in the second of three rounds, ramp_low (12, 0.02, 0) in the third, whose tau is 0; the
    crowded arrays reach both with k = all."""
    depth = {}
    for name in ("ramp", "ramp_low", "crowded"):
        _, y, triples = bc.case(name)
        for k, prom, dist in triples:
            L = bc.ladder(y, k)
            full = full_list(oracle, y, prom, dist)
            depth[(name, k, prom, dist)] = (bc.rounds_needed(taus_of(L), full, k), len(L.rounds), L.rounds[-1][0])
    assert depth[("ramp", 12, 0.02, 0)] == (2, 3, 0)
    assert depth[("ramp_low", 12, 0.02, 0)] == (3, 3, 0)
    assert {d[0] for d in depth.values()} == {1, 2, 3}
    _, y, _ = bc.case("ramp")
    assert [r[1] for r in bc.ladder(y, 12).rounds] == [4104, 32771, 37566]


def test_rounds_needed_on_a_hand_made_list():
    full = [(5, 6, 3.0, 1.0), (9, 10, 2.0, 1.0), (1, 2, -1.0, 1.0)]
    k3, k2, km = (int(bc.height_keys(np.float32(v))) for v in (3.0, 2.0, -1.0))
    assert k3 > k2 > 0x80000000 > km
    taus = [k3, k2, 0]
    assert [bc.rounds_needed(taus, full, k) for k in (1, 2, 3, 4)] == [1, 2, 3, 3]
    assert bc.rounds_needed(taus, [], 1) == 3 and bc.rounds_needed([], [], 1) == 0


def test_policy_list_has_both_bounds_active_and_a_second_round_under_order_1(oracle):
    second_under_order_1 = False
    for name, triples in bc.POLICY_TRIPLES.items():
        _, y, _ = bc.case(name)
        for k, prom, dist in triples:
            taus = taus_of(bc.ladder(y, k))
            lists = {}
            for order in (0, 1):
                pol = oracle.policy(order, 0)
                full = oracle.find_peaks(y, prom, dist, cap=y.size, pol=pol)
                assert len(full) < len(oracle.find_peaks(y, 0.0, dist, cap=y.size, pol=pol)), "the prominence bound is idle"
                assert len(full) < len(oracle.find_peaks(y, prom, 0, cap=y.size, pol=pol)), "min_distance is idle"
                lists[order] = full
                if order == 1 and bc.rounds_needed(taus, full, k) >= 2:
                    second_under_order_1 = True
                    # ... and a maximum that fails the bound suppresses a neighbour: the two orders differ
                    assert lists[0] != lists[1]
    assert second_under_order_1
    assert len(PEAK_POLICIES) == 8


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_model_maxima_are_the_checkers_peaks(oracle, name):
    """start, end and count at prominence 0 and distance 0: pins the plateau rule and the +-0.0 rule of the model."""
    _, y, _ = bc.case(name)
    s, e, h = bc.maxima(y)
    full = full_list(oracle, y, 0.0, 0)
    assert len(full) == s.size
    got = sorted(zip(s.tolist(), e.tolist(), np.asarray(h).view(np.uint32).tolist()))
    exp = sorted((p[0], p[1], int(np.float32(p[2]).view(np.uint32))) for p in full)
    assert got == exp
    # the checker's order is the key's order (height descending, start ascending)
    keys = bc.height_keys(np.array([p[2] for p in full], dtype=np.float32)).astype(np.int64)
    assert np.all(np.diff(keys) <= 0)
