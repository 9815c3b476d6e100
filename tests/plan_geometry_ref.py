"""What test_gpu_plan_geometry.py and test_plan_geometry_host.py share: the block layout of the register-kernel plans
(N = 2^21, 2^22, 2^23) as am_correlate.hip's plan_geometry computes it, the signals of a case, the checker's scores of
all three modes from one transform, a plain f64 dot-product reference of single scores, and a comparison whose failure
names the place (block, offset in the block, half of the pair).

The layout is used ONLY to choose lengths and to word failures: every expectation is the checker's.  Should the
library's layout change, the cases land elsewhere and stay correct."""
import numpy as np

TOL = 1e-4          # north_star: correlation scores within 1e-4 (f32), as in test_gpu_correlate.py
K_TILE = 1024       # am_kernels.h kTile

MODES = (0, 1, 2)   # Full, Same, Valid (the values of gpu.Mode and oracle.MODE_*)
MODE_NAMES = {0: "Full", 1: "Same", 2: "Valid"}

LARGE_HOP_S = 1_572_864      # on 2^21: hop 524 289, floored to 523 264 -- the rounded regime with real pair packing


def hop_of(log_n, s):
    """plan_geometry: hop = N - s + 1, floored to a multiple of the score tile when it is at least 8 tiles."""
    hop = (1 << log_n) - s + 1
    if hop >= 8 * K_TILE:
        hop = hop // K_TILE * K_TILE
    return hop


def needle_lengths(log_n):
    """The four small-hop needles of a plan: raw odd hop 5001, raw even hop 5000, the smallest rounded hop 8192,
    and a raw hop of 9001 that is floored to 8192 (the block reads more input than it emits)."""
    n = 1 << log_n
    return [n - 5000, n - 4999, n - 8191, n - 9000]


def score_counts(hop):
    """Odd and even block counts, a last block of 1 or 2 scores, one short of full, an exact fit."""
    return [3 * hop, 3 * hop + 1, 4 * hop - 1, 4 * hop, 4 * hop + 1, 5 * hop + 2]


def plants(hop, n_blocks=6):
    """(offset, gain) of needle copies added to `within`: a Valid score of about `gain` on alternating sides of each
    seam (last score of a block, first score of the next, second score, ...).  White noise alone scores about
    1 / sqrt(s), a few TOL; these make a score that lands one place off, or in the other half of its pair, miss by
    about 1.  The gains differ, so two plants that swapped places would show as well."""
    return [(b * hop + (-1, 0, 1)[b % 3], 1.0 - 0.07 * b) for b in range(1, n_blocks)]


def signals(oracle, log_n, s, w, hop=None):
    """Needle and `within` of a case, seeded from (log_n, s): uniform noise of amplitude 0.25 with the plants() of
    `hop` added (a plant the window cuts off is added as far as it fits).  A shorter `within` of the same (log_n, s,
    hop) is a prefix of a longer one, which is what lets the cases of one needle share one reference."""
    seed = ((log_n << 24) ^ s) & 0x7FFFFFFF
    needle = oracle.synth_uniform(seed, 0, 0, s)
    within = oracle.synth_uniform(seed, 1, 0, w)
    if hop is not None:
        for p, gain in plants(hop):
            k = min(s, w - p)
            if k > 0:
                within[p:p + k] += np.float32(gain) * needle[:k]
    return needle, within


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
