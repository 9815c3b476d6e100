"""What test_gpu_plan_geometry.py, test_gpu_generic_plans.py and test_plan_geometry_host.py share: the block layout of
a plan -- the register-kernel ones (N = 2^21, 2^22, 2^23) and the generic ones (N = 2^10 .. 2^20) alike -- as
am_correlate.hip's plan_geometry computes it, the signals of a case, the checker's scores of all three modes from one
transform, a plain f64 dot-product reference of single scores, and a comparison whose failure names the place (block,
offset in the block, half of the pair).

The layout is used ONLY to choose lengths and to word failures: every expectation is the checker's.  Should the
library's layout change, the cases land elsewhere and stay correct."""
import numpy as np

TOL = 1e-4          # north_star: correlation scores within 1e-4 (f32), as in test_gpu_correlate.py
K_TILE = 1024       # am_kernels.h kTile

MODES = (0, 1, 2)   # Full, Same, Valid (the values of gpu.Mode and oracle.MODE_*)
MODE_NAMES = {0: "Full", 1: "Same", 2: "Valid"}

LARGE_HOP_S = 1_572_864      # on 2^21: hop 524 289, floored to 523 264 -- the rounded regime with real pair packing


def hop_of(log_n, s):
    """plan_geometry: hop = N - s + 1, floored to a multiple of the score tile when it is at least 8 tiles (any plan:
    a hop of 8192 and more exists from N = 2^13 up, and below N = 2^14 only for a needle of one sample)."""
    hop = (1 << log_n) - s + 1
    if hop >= 8 * K_TILE:
        hop = hop // K_TILE * K_TILE
    return hop


def needle_lengths(log_n):
    """The four small-hop needles of a register plan: raw odd hop 5001, raw even hop 5000, the smallest rounded hop 8192,
    and a raw hop of 9001 that is floored to 8192 (the block reads more input than it emits)."""
    n = 1 << log_n
    return [n - 5000, n - 4999, n - 8191, n - 9000]


def generic_needle_lengths(log_n):
    """The needles of a generic plan (N = 2^10 .. 2^20): hop 2, hop 3 (odd) and, where N > 5000, the raw even hop 5000;
    from 2^14 up also hop 8191 (the last raw hop), hop 8192 (the first floored one) and a raw hop of 9001 floored to
    8192 (the block reads more input than it emits); on 2^14 and 2^20 a large floored hop with real pair packing, the
    analogue of LARGE_HOP_S."""
    n = 1 << log_n
    out = [n - 1, n - 2]
    if n > 5000:
        out.append(n - 4999)
    if log_n >= 14:
        out += [n - 8190, n - 8191, n - 9000]
    if log_n in (14, 20):
        out.append(n // 4 + 1)
    return out


def n1_of(log_n):
    """Rows of the work matrix (the column transform's length) as am_context.hip's get_plan computes it:
    max(5, log_n - 13) bits, capped at 10."""
    return 1 << min(max(5, log_n - 13), 10)


def score_counts(hop):
    """Odd and even block counts, a last block of 1 or 2 scores, one short of full, an exact fit."""
    return [3 * hop, 3 * hop + 1, 4 * hop - 1, 4 * hop, 4 * hop + 1, 5 * hop + 2]


def plants(hop, n_blocks=6, stride=1):
    """(offset, gain) of needle copies added to `within`: a Valid score of about `gain` on alternating sides of each
    seam (last score of a block, first score of the next, second score, ...).  White noise alone scores about
    1 / sqrt(s), a few TOL; these make a score that lands one place off, or in the other half of its pair, miss by
    about 1.  The gains differ, so two plants that swapped places would show as well.  `stride` plants on every
    stride-th seam only: with a hop of 2 or 3 and many blocks the plants, each nearly as long as `within`, would
    otherwise pile up (and their gains run out)."""
    return [(b * hop + (-1, 0, 1)[i % 3], 1.0 - 0.07 * i) for i, b in enumerate(range(stride, n_blocks, stride), 1)]


def signals(oracle, log_n, s, w, hop=None, n_blocks=6, stride=1):
    """Needle and `within` of a case, seeded from (log_n, s): uniform noise of amplitude 0.25 with the
    plants(hop, n_blocks, stride) added (a plant the window cuts off is added as far as it fits).  A shorter `within`
    of the same (log_n, s, hop, n_blocks, stride) is a prefix of a longer one, which is what lets the cases of one
    needle share one reference."""
    seed = ((log_n << 24) ^ s) & 0x7FFFFFFF
    needle = oracle.synth_uniform(seed, 0, 0, s)
    within = oracle.synth_uniform(seed, 1, 0, w)
    if hop is not None:
        for p, gain in plants(hop, n_blocks, stride):
            k = min(s, w - p)
            if k > 0:
                within[p:p + k] += np.float32(gain) * needle[:k]
    return needle, within


COMB_TONES = 16


def comb_count(log_n):
    """How many combs cover every row of the plan's work matrix: N1 / 16."""
    return n1_of(log_n) // COMB_TONES


def comb_needle_length(log_n):
    """The needle of the comb cases: hop 8192, the first floored hop, from 2^14 up; the raw hop 5000 on 2^13; below
    that (N < 5000) a raw hop of N / 8."""
    n = 1 << log_n
    return n - 8191 if log_n >= 14 else n - 4999 if n > 5000 else n - n // 8 + 1


def comb_bins(log_n, which):
    """(bins, phases) of comb `which`: bin k1 + N1 * k2 for the 16 rows k1 = 16 * which .. 16 * which + 15 of the work
    matrix (row k1 holds the bins that are k1 modulo N1), k2 seeded random in [0, N2), so over comb_count(log_n)
    combs every k1 in [0, N1) occurs; phases seeded random in [0, 2 pi)."""
    n1 = n1_of(log_n)
    n2 = (1 << log_n) // n1
    assert 0 <= which < comb_count(log_n)
    rng = np.random.default_rng([log_n, which])
    k1 = np.arange(COMB_TONES * which, COMB_TONES * (which + 1), dtype=np.int64)
    k2 = rng.integers(0, n2, COMB_TONES).astype(np.int64)
    return k1 + n1 * k2, rng.uniform(0.0, 2.0 * np.pi, COMB_TONES)


def comb_signals(log_n, s, w, which):
    """Needle and `within` of a comb case: `within` is the sum of 16 cosines of amplitude 1/16 exactly on bins of the
    N-point transform, cos(2 pi k_m n / N + phi_m) with the comb_bins(); the needle is its first s samples.  Every
    tone carries about 1/16 of a score, so a wrong twiddle on its row of the work matrix moves the scores by far more
    than TOL whatever N is -- white noise spreads over all N bins, and one wrong bin moves a score by about
    1 / sqrt(s * N) only.  The phase k_m * n modulo N is reduced in integers, so the f64 argument is exact to an ulp."""
    n = 1 << log_n
    bins, phases = comb_bins(log_n, which)
    idx = np.arange(w, dtype=np.int64)
    acc = np.zeros(w, dtype=np.float64)
    for k, phi in zip(bins, phases):
        acc += np.cos((2.0 * np.pi / n) * ((int(k) * idx) & (n - 1)) + phi)
    within = (acc / COMB_TONES).astype(np.float32)
    assert float(np.abs(within).max()) <= 1.0
    return within[:s].copy(), within


def mode_start(w, s, mode):
    """centered(): first index of the mode's crop in the full correlation (audio_matcher.rs:460-464)."""
    full = w + s - 1
    ln = {0: full, 1: w, 2: max(w - s, 0) + 1}[mode]
    return (full - ln) // 2, ln


def all_modes(oracle, within, needle):
    """oracle.correlate(within, needle, mode, SCALE_LIB) of every mode from ONE transform: the checker computes the
    full correlation and crops it (oracle.c correlate_impl), so the crops of its Full output are its Same and Valid
    outputs bit for bit (test_plan_geometry_host.py holds it to that)."""
    full = oracle.correlate(within, needle, oracle.MODE_FULL, oracle.SCALE_LIB)
    out = {}
    for mode in MODES:
        a, ln = mode_start(within.size, needle.size, mode)
        out[mode] = full[a:a + ln]
    return out


def place(i, hop):
    """Where score i of an output array sits: block b yields scores [b * hop, (b + 1) * hop) of it in every mode."""
    b = i // hop
    return "score %d = block %d (pair %d, %s half) + %d of hop %d" % (i, b, b // 2, "im" if b & 1 else "re", i - b * hop, hop)


def check_scores(got, exp, hop, what):
    """Shapes equal, every score within TOL; the failure names the worst score's place."""
    assert got.dtype == np.float32 and got.shape == exp.shape, (what, got.shape, exp.shape)
    err = np.abs(got.astype(np.float64) - exp.astype(np.float64))
    err[~np.isfinite(err)] = np.inf
    i = int(np.argmax(err))
    n_bad = int(np.count_nonzero(err >= TOL))
    assert err[i] < TOL, "%s: max error %.3g at %s (got %r, expected %r); %d of %d scores off, the first at %s" % (
        what, err[i], place(i, hop), float(got[i]), float(exp[i]), n_bad, err.size, place(int(np.argmax(err >= TOL)), hop))
    return float(err[i])


def seam_indices(n_scores, hop, rng, total, max_seams=None):
    """About `total` score indices: every seam (or the first and last max_seams of them) plus and minus 1, the first
    and last three scores, the rest pseudo-random."""
    seams = list(range(hop, n_scores, hop))
    if max_seams is not None and len(seams) > 2 * max_seams:
        seams = seams[:max_seams] + seams[-max_seams:]
    idx = {i for k in seams for i in (k - 1, k, k + 1)} | {0, 1, 2, n_scores - 3, n_scores - 2, n_scores - 1}
    idx = {i for i in idx if 0 <= i < n_scores}
    if len(idx) < total:
        idx |= {int(i) for i in rng.integers(0, n_scores, total - len(idx))}
    return sorted(idx)


def dot_scores(oracle, within, needle, mode, idx):
    """The mode's scores at `idx` as plain f64 dot products, score[j] = sum_n X[j + n - lead] * needle[n] with X = 0
    outside `within`, scaled as SCALE_LIB does: the f32 of the sum times the f32 factor, an f32 product."""
    w, s = within.size, needle.size
    a, _ = mode_start(w, s, mode)
    lead = (s - 1) - a
    x, h = within.astype(np.float64), needle.astype(np.float64)
    factor = np.float32(oracle.inv_autocorr(needle))
    out = np.empty(len(idx), dtype=np.float32)
    for k, j in enumerate(idx):
        lo = j - lead
        a0, b0 = max(lo, 0), min(lo + s, w)
        acc = float(np.dot(x[a0:b0], h[a0 - lo:b0 - lo])) if b0 > a0 else 0.0
        out[k] = np.float32(acc) * factor
    return out
