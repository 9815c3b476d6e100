"""CPU check of the checker itself at the shapes of test_gpu_plan_geometry.py and test_gpu_generic_plans.py.  There the oracle is one f64
transform of 2^23 points and more that nothing else looks at; here about 200 of its scores per shape -- every seam of
the block layout plus and minus 1, the first and last three scores of each mode, the rest pseudo-random -- are
recomputed as plain f64 dot products in numpy.  The oracle's output is f32 and the scores are at most about 1, so the
bound of 1e-6 is several f32 ulps above what correct f64 arithmetic gives and a hundredth of the 1e-4 the library is
held to: that margin is what makes the 1e-4 mean something."""
import numpy as np
import pytest

import plan_geometry_ref as R

ORACLE_TOL = 1e-6


def test_crops_of_the_full_output_are_the_other_modes(oracle):
    """all_modes() takes Same and Valid from the oracle's Full output: the same bits as asking for them."""
    needle, within = R.signals(oracle, 12, 3001, 9000, 500)
    exp = R.all_modes(oracle, within, needle)
    for mode in R.MODES:
        assert np.array_equal(exp[mode], oracle.correlate(within, needle, mode, oracle.SCALE_LIB)), R.MODE_NAMES[mode]
    # and the prefix property the Valid cases of one needle share a reference by
    short = oracle.correlate(within[:7000], needle, oracle.MODE_VALID, oracle.SCALE_LIB)
    assert np.abs(short - exp[2][:short.size]).max() < 1e-9


def against_dot_products(oracle, needle, within, hop, what):
    """The oracle's scores of every mode at the seam_indices() against dot_scores(), within ORACLE_TOL."""
    exp = R.all_modes(oracle, within, needle)
    rng = np.random.default_rng(needle.size)
    worst = {}
    for mode in R.MODES:
        idx = R.seam_indices(exp[mode].size, hop, rng, 70, max_seams=None if mode == 2 else 4)
        ref = R.dot_scores(oracle, within, needle, mode, idx)
        err = np.abs(ref.astype(np.float64) - exp[mode][idx].astype(np.float64))
        k = int(np.argmax(err))
        worst[R.MODE_NAMES[mode]] = (len(idx), float(err[k]))
        assert err[k] < ORACLE_TOL, (what, R.MODE_NAMES[mode], R.place(idx[k], hop), float(ref[k]), float(exp[mode][idx[k]]))
    print("%s, hop %d: (indices, max error) %r" % (what, hop, worst))
    return exp


@pytest.mark.parametrize("s,blocks,extra", [((1 << 21) - 5000, 5, 2), (R.LARGE_HOP_S, 5, 7)], ids=["raw-odd-hop", "large-hop"])
def test_oracle_against_dot_products(oracle, s, blocks, extra):
    log_n = 21
    hop = R.hop_of(log_n, s)
    count = blocks * hop + extra
    needle, within = R.signals(oracle, log_n, s, count + s - 1, hop)
    exp = against_dot_products(oracle, needle, within, hop, "2^%d" % log_n)
    assert exp[2].size == count and float(exp[2].max()) > 0.9       # the plants: scores of order 1 on the seams


GENERIC_SHAPES = [(12, (1 << 12) - 1), (19, (1 << 19) - 2), (20, (1 << 20) - 8191), (14, (1 << 14) // 4 + 1)]


@pytest.mark.parametrize("log_n,s", GENERIC_SHAPES, ids=["2^12-hop2", "2^19-hop3", "2^20-hop8192", "2^14-large-hop"])
def test_oracle_against_dot_products_generic(oracle, log_n, s):
    """The shapes of test_gpu_generic_plans.py: the smallest hops, the first floored one, a large floored one."""
    assert s in R.generic_needle_lengths(log_n)
    hop = R.hop_of(log_n, s)
    count = 5 * hop + 2
    needle, within = R.signals(oracle, log_n, s, count + s - 1, hop)
    exp = against_dot_products(oracle, needle, within, hop, "2^%d" % log_n)
    assert exp[2].size == count and float(exp[2].max()) > 0.9


@pytest.mark.parametrize("log_n", [12, 20])
def test_oracle_against_dot_products_comb(oracle, log_n):
    """A comb is the input for which a transform-based reference could itself be off: all of the energy sits in 32
    bins.  The last comb of the plan, with the needle and the five blocks test_gpu_generic_plans.py uses."""
    s = R.comb_needle_length(log_n)
    hop = R.hop_of(log_n, s)
    which = R.comb_count(log_n) - 1
    needle, within = R.comb_signals(log_n, s, 5 * hop + s - 1, which)
    assert needle.size == s and np.array_equal(needle, within[:s]) and 0.2 < float(np.abs(within).max()) <= 1.0
    bins, _ = R.comb_bins(log_n, which)
    n1 = R.n1_of(log_n)
    assert sorted(int(k) % n1 for k in bins) == list(range(n1 - 16, n1)) and int(bins.max()) < (1 << log_n)
    exp = against_dot_products(oracle, needle, within, hop, "2^%d comb %d" % (log_n, which))
    assert float(np.abs(exp[2]).max()) > 0.5        # score 0 is the needle on itself


@pytest.mark.parametrize("log_n", range(10, 21))
def test_combs_cover_every_row(log_n):
    """Over the combs of a plan every row k1 of the work matrix carries a tone, on a bin of the N-point transform."""
    n1 = R.n1_of(log_n)
    assert n1 == {19: 64, 20: 128}.get(log_n, 32) and R.comb_count(log_n) == n1 // 16
    rows = []
    for which in range(R.comb_count(log_n)):
        bins, phases = R.comb_bins(log_n, which)
        assert bins.size == phases.size == 16 and 0 <= int(bins.min()) and int(bins.max()) < (1 << log_n)
        rows += [int(k) % n1 for k in bins]
    assert sorted(rows) == list(range(n1))
