"""Host-side checks (no device) of what test_gpu_resample_edges.py is built on: the geometry mirror of resample_ref.py
against the constants in the sources, that the pair list reaches every kernel form and geometry regime, that the
designed inputs are what they claim to be under the f64 checker, and that a plain sequential f32 sum misses the
header's 1e-5 on the long-filter inputs (so the long-filter test cannot pass by accident)."""
import os
import re

import numpy as np
import pytest

import resample_ref as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "audio-matcher_amd", "csrc")


def _const(text, name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert m, name
    return int(m.group(1))


def _sources():
    return open(os.path.join(CSRC, "am_kernels.h")).read(), open(os.path.join(CSRC, "am_resample.hip")).read()


def test_mirror_constants_match_the_sources():
    kh, rs = _sources()
    assert (_const(kh, "kRsThreads"), _const(kh, "kRsJ"), _const(kh, "kRsTc")) == (ref.K_RS_THREADS, ref.K_RS_J, ref.K_RS_TC)
    assert (_const(rs, "kRsXsMax"), _const(rs, "kRsTabMax"), _const(rs, "kRsWMax")) == \
        (ref.K_RS_XS_MAX, ref.K_RS_TAB_MAX, ref.K_RS_W_MAX)
    assert re.search(r"constexpr\s+long long\s+kResampleMaxR\s*=\s*%d\s*;" % ref.MAX_R, rs)
    assert re.search(r"constexpr\s+uint32_t\s+kResampleMaxRate\s*=\s*%d\s*;" % ref.MAX_RATE, rs)


def test_geometry_of_known_pairs():
    """The figures the kernel's own comments and profiles state, and the ones this suite's design relies on."""
    g = ref.geometry(384000, 8000)
    assert (g["L"], g["M"], g["T"], g["form"]) == (1, 48, 961, "table")          # "384 -> 8 kHz fits 18 work items"
    assert ref.geometry(11025, 384000)["W"] == 5120
    g = ref.geometry(409, 8192)
    assert (g["W"], g["xs_cap"]) == (8192, 3304)
    assert ref.geometry(1, 8192)["xs_cap"] == 40
    assert ref.geometry(499, 500)["xs_cap"] == 8016
    g = ref.geometry(48000, 8000)
    assert (g["W"], g["xs_cap"]) == (167, 8148)
    assert (ref.geometry(44100, 16000)["T"], ref.geometry(192000, 44100)["T"]) == (56, 88)


def test_pair_list_covers_every_form_and_regime():
    gs = [ref.geometry(s, d) for s, d in ref.EDGE_PAIRS]
    for g in gs:
        assert max(g["L"], g["M"]) <= ref.MAX_R and g["W"] % g["L"] == 0
        assert g["xs_cap"] <= ref.K_RS_XS_MAX and g["xs_cap"] % 4 == 0
    assert {g["form"] for g in gs} == set(ref.FORMS)
    for form in ref.FORMS:
        assert sum(g["form"] == form for g in gs) >= 2, form
    assert any(g["L"] > ref.K_RS_W_MAX and g["xs_cap"] for g in gs)              # many passes of the w loop, staged
    assert any(g["L"] > ref.K_RS_W_MAX and not g["xs_cap"] for g in gs)          # ... and not staged
    assert any(g["W"] == 8192 for g in gs)
    assert any(g["T"] == g["ts"] for g in gs)                                    # a table row without padding
    assert any(g["T"] == g["ts"] and g["tab_lds"] for g in gs)                     # ... in a staged table
    assert any(0 < ref.K_RS_XS_MAX - g["xs_cap"] <= 64 for g in gs)
    assert any(g["W"] % 2 == 1 for g in gs)
    assert any(g["xs_cap"] and g["xs_cap"] <= 64 for g in gs)                    # a tiny staged span
    assert any(min(g["L"], g["M"]) >= 8191 for g in gs)                          # v = r0 + w M at its largest
    assert max(ref.geometry(s, d)["T"] for s, d in ref.LONG_PAIRS) > 150000
    # a last staged quad with one live sample, put there by the start phase's carry: under both staged forms
    assert {g["form"] for g in gs if ref.last_quad_carry(g)} == {"both", "input"}


@pytest.mark.parametrize("src,dst", ref.EDGE_PAIRS)
def test_designs_have_three_blocks_and_edges_inside(src, dst):
    g = ref.geometry(src, dst)
    for extra in range(4):
        n_in = ref.design_len(g, extra)
        n_out = ref.out_len(n_in, src, dst)
        assert 2 * g["bo"] < n_out < 3 * g["bo"] and n_out % g["bo"], (n_in, n_out, g["bo"])   # a partial last block
        pos = ref.edge_samples(g, n_in)
        assert pos.size and pos.min() >= 0 and pos.max() < n_in
        assert {0, n_in - 1} <= set(pos.tolist())
    assert {ref.design_len(g, e) % 4 for e in range(4)} == {0, 1, 2, 3}
    n_in = ref.design_len(g)
    sep = 2 * g["H"] // g["L"] + 2
    groups = ref.far_apart(g, ref.edge_samples(g, n_in))
    assert sorted(n for grp in groups for n in grp) == ref.edge_samples(g, n_in).tolist()
    for grp in groups:
        assert (np.diff(grp) >= sep).all()
    # the block edges' own reads are among the positions: the last output of block 0 and the first of block 1
    for k in (g["bo"] - 1, g["bo"]):
        lo, hi = ref.support(g, k)
        assert {max(lo, 0), min(hi, n_in - 1)} <= set(ref.edge_samples(g, n_in).tolist())


@pytest.mark.parametrize("src,dst", ref.EDGE_PAIRS)
def test_checker_leaves_the_expected_support_and_nothing_else(src, dst):
    """On every impulse input the looped checker gives a h[idx] on the supports (one tap per output: no two supports
    overlap) and 0.0 everywhere else."""
    g = ref.geometry(src, dst)
    h = ref.taps(src, dst)
    n_in = ref.design_len(g)
    n_out = ref.out_len(n_in, src, dst)
    designs = ref.impulse_designs(g, n_in)
    assert sum(d[0].size for d in designs) >= ref.edge_samples(g, n_in).size
    if g["T"] <= 128:                               # (the i16 designs share everything but the amplitudes)
        designs += [d[:3] for d in ref.impulse_designs(g, n_in, i16=True)]
    for pos, amp, x in designs:
        assert np.count_nonzero(x) == pos.size and np.array_equal(x[pos], amp)
        k, idx, a, want = ref.impulse_expectation(g, n_out, pos, amp, h)
        assert k.size and np.unique(k).size == k.size                       # no output holds two impulses
        assert idx.min() >= 0 and idx.max() <= 2 * g["H"]
        dense = np.zeros(n_out)
        dense[k] = want
        if g["T"] <= 128 or pos is designs[0][0]:
            assert np.array_equal(ref.resample(x, src, dst, h=h), dense)
        else:                                       # (a long filter: each support and the outputs around it)
            edges = np.flatnonzero(np.diff(k) != 1)
            for a0, a1 in zip(np.r_[k[0], k[edges + 1]], np.r_[k[edges], k[-1]]):
                k0, k1 = max(0, int(a0) - 4), min(n_out, int(a1) + 5)
                assert np.array_equal(ref.resample(x, src, dst, k0, k1, h=h), dense[k0:k1])
    # some tap meets the same amplitude at two places, so the bit-identity check of the GPU test compares something
    ex = [ref.impulse_expectation(g, n_out, d[0], d[1], h) for d in ref.impulse_designs(g, n_in)]
    pairs = np.stack([np.concatenate([e[1] for e in ex]), np.concatenate([e[2] for e in ex])], axis=1)
    assert np.unique(pairs, axis=0).shape[0] < pairs.shape[0]
    amps = np.concatenate([d[1] for d in designs])
    assert (amps > 0).any() and (amps < 0).any() and np.unique(np.abs(amps)).size >= 2


def test_dot_checker_equals_the_looped_one():
    rng = np.random.default_rng(11)
    for src, dst in ((48000, 44100), (44100, 48000), (300, 7), (3, 2)):
        L, M, H = ref.ratio(src, dst)
        n = 3 * (2 * H // L + 1) + 17
        x = rng.standard_normal(n)
        a, b = ref.resample(x, src, dst), ref.resample_dot(x, src, dst)
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-13 * np.abs(x).max()
        k0, k1 = a.size // 3, a.size // 3 + 5
        assert np.array_equal(ref.resample_dot(x, src, dst, k0, k1), b[k0:k1])
        x[n // 2], x[0] = np.nan, np.inf
        a, b = ref.resample(x, src, dst), ref.resample_dot(x, src, dst)
        assert np.array_equal(np.isfinite(a), np.isfinite(b)) and not np.isfinite(a).all()
        ok = np.isfinite(a)
        assert np.abs(a[ok] - b[ok]).max() <= 1e-13 * np.abs(x[np.isfinite(x)]).max()


@pytest.mark.parametrize("src,dst,name", [(8192, 1, "ones"), (8191, 2, "ones"), (768000, 100, "ones"), (3000, 1, "sign")])
def test_a_sequential_f32_sum_misses_the_bound_on_long_filters(src, dst, name):
    """Discrimination: one f32 fma chain over t = 0, 1, ... (exact products, so np.add.accumulate reproduces it) is
    off by more than the header's 1e-5 max |x| on the long-filter inputs; the control pair is far inside."""
    g = ref.geometry(src, dst)
    h = ref.taps(src, dst)
    n_in, xs = ref.long_inputs(g)
    x = xs[name]
    n_out = ref.out_len(n_in, src, dst)
    full = [k for k in range(n_out) if k * g["M"] - g["H"] >= 0 and k * g["M"] + g["H"] <= (n_in - 1) * g["L"]]
    assert 8 <= len(full) <= 20 and full[0] > 0 and full[-1] < n_out - 1      # both ends present as well
    want = ref.resample_dot(x, src, dst, h=h)
    worst = max(abs(float(ref.sequential_f32(x, g, k, h)) - want[k]) for k in full)
    assert worst > 1e-5, worst
    gc = ref.geometry(384000, 8000)
    n_c, xc = ref.long_inputs(gc)
    wc = ref.resample_dot(xc[name], 384000, 8000)
    assert max(abs(float(ref.sequential_f32(xc[name], gc, k)) - wc[k]) for k in range(wc.size)) < 2e-6


def test_sum_form_threshold_holds_the_bound_a_priori():
    """am_resample.hip sums rows of up to kRsSeqTaps taps as one f32 chain and longer ones chunk-wise into f64.  With
    u = 2^-24 a chain of n fmas is off by at most n u sum |h x|, the chunked form by (kRsTc + 1) u sum |h x| (chunk
    chain, final rounding), and the f32 table by u sum |h x|: both stay below 1e-5 max |x| given the largest
    sum |h| of a phase, which is below 3 (about 2.25 at the half-sample phases)."""
    _, rs = _sources()
    seq = _const(rs, "kRsSeqTaps")
    worst = 0.0
    for src, dst in ref.EDGE_PAIRS + ref.LONG_PAIRS + [(48000, 44100), (96000, 44100), (22050, 44100)]:
        L = ref.ratio(src, dst)[0]
        a = np.abs(ref.taps(src, dst))
        worst = max(worst, max(a[p::L].sum() for p in range(0, L, max(1, L // 64))))
    assert 2.0 < worst < 3.0, worst
    u = 2.0 ** -24
    assert (seq + 1) * u * 3.0 <= 1e-5 and (ref.K_RS_TC + 2) * u * 3.0 <= 2e-6
    assert ref.geometry(48000, 44100)["ts"] <= seq and ref.geometry(44100, 48000)["ts"] <= seq   # the common pairs: one chain
    assert all(ref.geometry(s, d)["ts"] > seq for s, d in ref.LONG_PAIRS)
