"""Masked window energies (masked_norm_scores_kernel, csrc/am_norm.hip), exact at every span, tile, block and path edge.

The masked energy of EVERY score is recovered from two score arrays of one correlation, as test_gpu_score_norm_edges.py
recovers window energies (see the docstring of its test_window_energy_from_two_arrays for the identity and the count of
roundings behind score_norm_ref.ENERGY_BOUND): two handles over one masked needle, one plain with AM_SCALE_LIB and one
with score_norm, on the integer spike signals of mask_ref.mask_signal.  test_mask_host.py holds the designs to their
claims: integer energies below 2^8, and every span edge moved by one sample changes some energy by 1000 bounds or more.
Every problem is below 2^19 samples, where the identity holds (the factor enters as one f32 multiply)."""
import numpy as np
import pytest

import mask_ref as mr
import score_norm_ref as ref

pytestmark = pytest.mark.gpu


def test_mask_roundtrip_and_ordinary_handles(gpu):
    """am_needle_mask gives the gaps back; an ordinary handle and one made with n_gaps = 0 have none; the handle's
    1 / energy is that of the kept samples; the _device form agrees."""
    s, kept, gaps = mr.DESIGNS["sixteen"]
    needle = mr.mask_needle(s)
    masked = gpu.HipConvolve(needle, gaps=gaps)
    assert masked.mask() == gaps and len(gaps) == 15
    assert gpu.HipConvolve(needle).mask() == [] and gpu.HipConvolve(needle, gaps=[]).mask() == []
    en = float(np.sum(mr.zero_filled(needle, gaps).astype(np.float64) ** 2))
    assert abs(masked.inverse_sample_auto_correlation() * en - 1.0) <= 4 * ref.U
    buf = gpu.DeviceBuffer.from_numpy(0, needle)
    try:
        dev = gpu.HipConvolve.from_device(0, buf.ptr, s, gaps=gaps)
    finally:
        buf.free()
    assert dev.mask() == gaps
    assert np.float32(dev.inverse_sample_auto_correlation()).tobytes() == np.float32(masked.inverse_sample_auto_correlation()).tobytes()
    # too few slots: AM_ERR_CAPACITY, the count still reported
    import ctypes as C
    arr, n = (gpu.AmSpan * 2)(), C.c_size_t(0)
    assert gpu.lib().am_needle_mask(masked._h, arr, 2, C.byref(n)) == gpu.AM_ERR_CAPACITY and n.value == 15
    assert (arr[1].begin, arr[1].end) == gaps[1]
    # NaN under a gap of the needle never reaches the handle
    poisoned = needle.copy()
    poisoned[gaps[3][0]] = np.nan
    assert np.float32(gpu.HipConvolve(poisoned, gaps=gaps).inverse_sample_auto_correlation()).tobytes() == \
        np.float32(masked.inverse_sample_auto_correlation()).tobytes()


@pytest.mark.parametrize("name", sorted(mr.DESIGNS))
def test_masked_energy_from_two_arrays(gpu, name):
    """E_x^M(t) = (lib / mncc)^2 (b / a)^2 for every score of all three modes, against the exact f64 sum, within
    ENERGY_BOUND = 16 u; where the masked energy is 0 the score is exactly 0.  With score_norm = 0 the masked handle is
    the zero-filled needle's: the plain handle's bits are those of an ordinary handle over the zero-filled needle."""
    s, kept, gaps = mr.DESIGNS[name]
    needle = mr.mask_needle(s)
    plain, normed = gpu.HipConvolve(needle, gaps=gaps), gpu.HipConvolve(needle, gaps=gaps, score_norm=True)
    zeroed = gpu.HipConvolve(mr.zero_filled(needle, gaps))
    a = np.float32(plain.inverse_sample_auto_correlation())
    a_host, b = ref.scale_pair(float(np.sum(mr.zero_filled(needle, gaps).astype(np.float64) ** 2)))
    assert abs(float(a) / float(a_host) - 1.0) <= 2 * ref.U
    w = mr.design_width(s)
    worst = 0.0
    for mode in ref.SPIKE_MODES:
        within = mr.mask_signal(s, kept, w, mode)
        lead, n = ref.lead_of(w, s, mode), ref.mode_len(w, s, mode)
        assert n > ref.NORM_TILE and n % ref.NORM_TILE != 0   # more than one tile, a ragged last one
        E = mr.masked_energy(within, kept, lead, n)
        lib = plain.correlate_with_sample(within, gpu.Mode(mode), True)
        ncc = normed.correlate_with_sample(within, gpu.Mode(mode), True)
        assert lib.tobytes() == zeroed.correlate_with_sample(within, gpu.Mode(mode), True).tobytes()
        assert lib.shape == ncc.shape == E.shape
        assert np.all(np.isfinite(lib)) and np.all(np.isfinite(ncc))
        pos = E > 0
        assert pos.any() and np.all(lib[pos] != 0) and np.all(ncc[pos] != 0), (name, mode)
        assert np.all(ncc[~pos] == 0.0), (name, mode, np.flatnonzero(ncc[~pos] != 0)[:8])
        err = np.abs(ref.recovered_energy(lib[pos], ncc[pos], a, b) / E[pos] - 1.0)
        k = int(np.argmax(err))
        print("%s, mode %d: %d scores, %d of energy 0, worst energy error %.3g = %.2f bounds (score %d)"
              % (name, mode, n, np.count_nonzero(~pos), err[k], err[k] / ref.ENERGY_BOUND, np.flatnonzero(pos)[k]))
        assert err[k] <= ref.ENERGY_BOUND, (name, mode, int(np.flatnonzero(pos)[k]), float(E[pos][k]), float(err[k]))
        worst = max(worst, float(err[k]))
    print("%s: worst energy error %.3g = %.2f of the bound" % (name, worst, worst / ref.ENERGY_BOUND))


@pytest.mark.parametrize("mode", ref.SPIKE_MODES)
def test_loud_gaps_over_silent_kept_spans_score_zero(gpu, mode):
    """Loud spikes under the gap only, digital silence under both kept spans: every such score is exactly 0 (no "whole
    window minus gaps": 10^6 - 10^6 would have to cancel).  The same needle without its mask scores non-zero there."""
    needle, gaps, within, lo, hi = mr.silent_case(mode)
    masked = gpu.HipConvolve(needle, gaps=gaps, score_norm=True).correlate_with_sample(within, gpu.Mode(mode), True)
    whole = gpu.HipConvolve(needle, score_norm=True).correlate_with_sample(within, gpu.Mode(mode), True)
    assert hi - lo > 800
    assert np.all(masked[lo:hi] == 0.0), np.flatnonzero(masked[lo:hi] != 0)[:8]
    assert np.all(np.signbit(masked[lo:hi]) == 0)
    assert np.all(whole[lo:hi] > 0.0)
    assert masked[lo - 1] > 0.0 and masked[hi] > 0.0   # one spike under a kept span's first or last sample
