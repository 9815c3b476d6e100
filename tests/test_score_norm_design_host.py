"""The designs of test_gpu_score_norm_edges.py, checked without a device: that every window energy of the spike cases is
exact and positive where it must be, that a window one sample too short or too long shows far above the device test's
bound, and that the two-array identity recovers the energy within that bound under the library's f32 roundings."""
import numpy as np
import pytest

import score_norm_ref as ref

CASES = ref.spike_cases()


def case_energy(s, w, mode):
    needle, within = ref.spike_case(s, w, mode)
    lead, n = ref.lead_of(w, s, mode), ref.mode_len(w, s, mode)
    return needle, within, lead, n, ref.window_energy(within, s, lead, n)


def test_lead_and_length():
    # Full: the window of score 0 ends on sample 0; Valid: it starts there; Same: centred, the odd sample in front
    assert [ref.lead_of(100, 7, m) for m in ref.SPIKE_MODES] == [6, 3, 0]
    assert [ref.lead_of(100, 8, m) for m in ref.SPIKE_MODES] == [7, 4, 0]
    assert [ref.mode_len(100, 8, m) for m in ref.SPIKE_MODES] == [107, 100, 93]


@pytest.mark.parametrize("mode", ref.SPIKE_MODES)
def test_window_energy_brute_force(mode):
    s, w = 5, 23
    x = np.random.default_rng(mode).integers(-3, 4, size=w).astype(np.float32)
    lead, n = ref.lead_of(w, s, mode), ref.mode_len(w, s, mode)
    exp = np.zeros(n)
    for t in range(n):
        for i in range(t - lead, t - lead + s):
            if 0 <= i < w:
                exp[t] += float(x[i]) ** 2
    assert np.array_equal(ref.window_energy(x, s, lead, n), exp)
    for k, (ds, dl) in enumerate(((-1, -1), (-1, 0), (1, 1), (1, 0))):   # the variants are windows too
        assert np.array_equal(ref.energy_variants(x, s, lead, n)[k], ref.window_energy(x, s + ds, lead + dl, n))


def test_shapes_cover_the_edges():
    assert {4095, 4096, 4097} <= set(ref.SPIKE_S) and ref.NORM_TILE + 2 * ref.NORM_BLOCK == 4096
    assert {1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 5121, 8193} <= set(ref.SPIKE_S)
    for s in ref.SPIKE_S:
        ws = ref.spike_widths(s)
        assert {ref.mode_len(w, s, ref.MODE_VALID) for w in ws} >= {1, 2047, 2048, 2049, 3 * 2048, 3 * 2048 + 1}
        assert {w % 1024 for w in ws} >= {1, 1023}
        assert max(ws) + s < 1 << 19   # (the generic transform plans, whose K3 applies the factor as one multiply)
    for s, w, mode in CASES:
        lead = ref.lead_of(w, s, mode)
        assert (lead != 0) == (mode != ref.MODE_VALID and s > 1)


@pytest.mark.parametrize("s", ref.SPIKE_S)
def test_spike_design(s):
    worst_defect, worst_e, worst_id = np.inf, 0.0, 0.0
    for w in ref.spike_widths(s):
        for mode in ref.SPIKE_MODES:
            needle, within, lead, n, E = case_energy(s, w, mode)
            assert needle.dtype == within.dtype == np.float32 and needle.min() >= 0.25 and needle.max() <= 1.0
            assert set(np.unique(within)) <= {0.0, 1.0, 2.0, 3.0} and within[0] > 0 and within[-1] > 0
            assert np.array_equal(E, np.round(E)) and E.max() < 2 ** 20          # integers: exact
            pos = E > 0
            corr = ref.sparse_corr(needle, within, lead, n)
            assert pos.any() and corr[pos].min() >= 0.25 and np.all(corr[~pos] == 0.0)
            # windows of exact zeros directly beside windows that hold a spike
            beside = (~pos[1:] & pos[:-1]).any() or (pos[1:] & ~pos[:-1]).any()
            assert bool(beside) == bool((~pos).any())
            if ref.zero_windows_expected(s, n):
                assert beside, (s, w, mode)
            if s > ref.MAX_ZERO_RUN:
                assert pos.all(), (s, w, mode)
            # one sample too few or too many, at either end
            for k, Ev in enumerate(ref.energy_variants(within, s, lead, n)):
                d = np.abs(Ev - E)
                # (the sample in front of every window, or behind every window, may lie outside the signal)
                inside = {2: n >= lead + 2, 3: w + lead - s >= 1}.get(k, True)
                assert (d > 0).any() == inside, (s, w, mode, k)
                rel = d[d > 0] / np.maximum(Ev, E)[d > 0]
                worst_defect = min(worst_defect, rel.min(initial=np.inf))
            worst_e = max(worst_e, E.max())
            # the identity under the library's roundings
            en = float(np.sum(needle.astype(np.float64) ** 2))
            lib, ncc, a, b = ref.simulate_pair(corr[pos], E[pos], en)
            assert np.all(lib != 0) and np.all(ncc != 0)
            worst_id = max(worst_id, np.max(np.abs(ref.recovered_energy(lib, ncc, a, b) / E[pos] - 1.0)))
    print("s = %d: smallest one-sample defect %.3g, largest energy %g, identity error %.3g (%.2f u)"
          % (s, worst_defect, worst_e, worst_id, worst_id / ref.U))
    assert worst_defect >= ref.MIN_DEFECT
    assert ref.MIN_DEFECT >= 100 * ref.ENERGY_BOUND      # the device test's bound: at least 100 times below a defect
    assert worst_id <= ref.ENERGY_BOUND


@pytest.mark.parametrize("s", ref.SPIKE_S)
def test_gap_design(s):
    """Windows of exact zeros for every needle length: GAP_EXTRA + 1 in a row, over a tile edge, a spike on the last
    sample of the window in front and on the first sample of the window behind."""
    for mode in ref.SPIKE_MODES:
        needle, within = ref.gap_case(s, mode)
        w = len(within)
        lead, n = ref.lead_of(w, s, mode), ref.mode_len(w, s, mode)
        E = ref.window_energy(within, s, lead, n)
        assert np.array_equal(E, np.round(E))
        first = ref.GAP_LO + lead                                  # the score whose window starts on the gap's first sample
        run = np.arange(first, first + ref.GAP_EXTRA + 1)
        assert 0 < first and run[-1] + 1 < n
        assert np.all(E[run] == 0) and E[first - 1] == 4 and E[run[-1] + 1] == 4
        assert len({t // ref.NORM_TILE for t in run}) >= 2
        pos = E > 0
        corr = ref.sparse_corr(needle, within, lead, n)
        assert corr[pos].min() >= 0.25 and np.all(corr[~pos] == 0.0)
        en = float(np.sum(needle.astype(np.float64) ** 2))
        lib, ncc, a, b = ref.simulate_pair(corr[pos], E[pos], en)
        assert np.max(np.abs(ref.recovered_energy(lib, ncc, a, b) / E[pos] - 1.0)) <= ref.ENERGY_BOUND
        assert w + s < 1 << 19


def test_spike_positions():
    """The spikes the kernel's edges ask for are there, case by case."""
    for s, w, mode in CASES:
        _, within = ref.spike_case(s, w, mode)
        lead, n = ref.lead_of(w, s, mode), ref.mode_len(w, s, mode)
        want = [0, w - 1]
        want += [m + d for m in range(0, w + 1024, 1024) for d in (-1, 0, 1)]
        for t0 in range(0, n, 2048):
            for first in (t0 - lead, t0 + 2047 - lead):
                want += [e + d for e in (first, first + s - 1) for d in (-1, 0, 1)]
        want = [q for q in want if 0 <= q < w]
        assert np.all(within[want] > 0), (s, w, mode)
        extra = np.count_nonzero(within) - len(set(want))
        assert 0 <= extra <= max(1, round(w / 700))


def test_plant_offsets():
    chunk = 20 * ref.SR
    for S in ref.PLANT_S:
        plants = ref.plant_offsets(S)
        ts = [t for t, _ in plants]
        assert min(np.diff(ts)) > 5 * ref.SR and ts == sorted(ts)
        assert ts[0] == 0 and ts[-1] == ref.PLANT_LEN - S
        # the residues the kernel's edges ask for, among the plants that can be hits
        inner = ref.inner_plants(S)
        ti = [t for t, _ in inner]
        assert ti == ts[1:-1] and len(ti) >= 6
        assert {t % 2048 for t in ti} >= {0, 1, 2047}
        assert {(t + S) % 1024 for t in ti} >= {0, 1, 1023}
        assert any(0 < (-t) % chunk <= 8 and t + S <= (t // chunk + 1) * chunk + S for t in ti)   # just below a chunk start
        assert {k for _, k in inner} == {"in", "out"}
        assert ref.PLANT_LEN <= 1 << 20
    assert ref.PLANT_S[0] < ref.NORM_TILE + 2 * ref.NORM_BLOCK <= ref.PLANT_S[1]


@pytest.mark.parametrize("S", ref.PLANT_S)
def test_plants_checker_sees_the_guards(oracle, S):
    """The expectation itself: every plant is a hit, at about 1 with the guards outside the window and about 0.58 with
    them inside; a window one sample off would give about 0.71 either way."""
    import audiomatch_amd as am
    needle, hays, exps, plants, p = ref.plant_setup(am, oracle, S)
    exp = exps[0]
    assert len(plants) >= 6
    assert [e[0] for e in exp] == [t for t, _ in plants] and all(e[1] == e[0] + 1 for e in exp)
    for e, (t, kind) in zip(exp, plants):
        assert abs(e[2] - (1.0 if kind == "out" else 3 ** -0.5)) < 0.02, (e, kind)
    cut = 2 * p.chunk - 3
    assert exps[1][-1][0] == cut == len(hays[1]) - S - 1 and exps[2][0][0] == 1
    assert [e[0] for e in exps[1]] == [t for t, _ in plants if t <= cut]
    assert [e[0] + cut - 1 for e in exps[2]] == [t for t, _ in plants if t >= cut]


def test_stereo_frames():
    x = np.array([0.5, -13.0, 1e-3, 0.0], dtype=np.float32)
    f = ref.stereo(x)
    assert f.dtype == np.int16 and f.shape == (4, 2) and f[1, 0] == -32000 and f[1, 1] == -24000 and f[3].tolist() == [0, 0]
