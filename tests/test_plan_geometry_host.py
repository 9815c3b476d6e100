"""CPU check of the checker itself at the shapes of test_gpu_plan_geometry.py.  There the oracle is one f64
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


@pytest.mark.parametrize("s,blocks,extra", [((1 << 21) - 5000, 5, 2), (R.LARGE_HOP_S, 5, 7)], ids=["raw-odd-hop", "large-hop"])
def test_oracle_against_dot_products(oracle, s, blocks, extra):
    log_n = 21
    hop = R.hop_of(log_n, s)
    count = blocks * hop + extra
    needle, within = R.signals(oracle, log_n, s, count + s - 1, hop)
    exp = R.all_modes(oracle, within, needle)
    assert exp[2].size == count and float(exp[2].max()) > 0.9       # the plants: scores of order 1 on the seams
    rng = np.random.default_rng(s)
    worst = {}
    for mode in R.MODES:
        idx = R.seam_indices(exp[mode].size, hop, rng, 70, max_seams=None if mode == 2 else 4)
        ref = R.dot_scores(oracle, within, needle, mode, idx)
        err = np.abs(ref.astype(np.float64) - exp[mode][idx].astype(np.float64))
        k = int(np.argmax(err))
        worst[R.MODE_NAMES[mode]] = (len(idx), float(err[k]))
        assert err[k] < ORACLE_TOL, (R.MODE_NAMES[mode], R.place(idx[k], hop), float(ref[k]), float(exp[mode][idx[k]]))
    print("hop %d: (indices, max error) %r" % (hop, worst))
