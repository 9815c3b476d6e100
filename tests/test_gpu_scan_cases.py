"""GPU: the designed score arrays of tests/scan_cases.py through K3's fused scan, the sparse-score certificate and both
redo paths.  An impulse needle (1.0 at index 0) of S > 64 samples makes the score array of `design ++ zeros(S - 1)` equal
to the design, on the real K1 / K2 / K3 path: forced onto 2^21, 2^22 and 2^23 with S = N - hop + 1, and on the plans the
library picks itself.  Every expectation is scan_cases.expected() of the design (positions exact, height and prominence
within TOL); every result also equals the same call with dense_scores = 1 bit for bit; and the K3 launch counts of the
two calls show that a design built to fail a certificate really took a redo, and one built to pass took none.
(tests/test_scan_cases_host.py holds the designs and expected() to their claims, without a GPU.)"""
import numpy as np
import pytest

import scan_cases as sc
from plan_geometry_ref import TOL
from test_gpu_plan_geometry import peak_key

pytestmark = pytest.mark.gpu


def gpu_params(gpu, p, scale=None):
    q = gpu.Config(chunk_size_s=1.0, overlap_length_s=0.0, distance_s=0.0, prominence=p.prom).params(p.sr, gpu.Scale.LIB if scale is None else scale)
    q.chunk, q.overlap, q.min_distance, q.overshadow_distance_s = p.chunk, p.overlap, p.dist, p.overshadow_s
    return q


def impulse(s, index=0, gain=1.0):
    needle = np.zeros(s, dtype=np.float32)
    needle[index] = gain
    return needle


def handle(gpu, c, log_n, index=0, gain=1.0):
    algo = gpu.HipConvolve(impulse(c.layout.needle_len(log_n), index, gain))
    if not c.natural:
        algo.set_option("log_n", log_n)
    return algo


class Haystacks:
    """One zeroed buffer per length: a case writes its design into the front and clears it again."""
    def __init__(self):
        self.bufs = {}

    def __call__(self, c, log_n):
        n = c.y.size + c.layout.needle_len(log_n) - 1
        if n not in self.bufs:
            self.bufs = {n: np.zeros(n, dtype=np.float32)}          # (one at a time: the 2^23 ones hold 36 MB)
        return c.haystack(log_n, out=self.bufs[n])

    def clear(self, c):
        for b in self.bufs.values():
            b[:c.y.size] = 0


class counting:
    """K3 launches ("k3_cols_inv") and launches of the class "other" inside the block; every option restored."""
    def __init__(self, gpu, **opts):
        self.gpu, self.opts = gpu, dict(profile_mask=-1, profile_every=1, **opts)

    def __enter__(self):
        self.keep = {k: self.gpu.get_option(k) for k in self.opts}
        try:
            for k, v in self.opts.items():
                self.gpu.set_option(k, v)
            self.prof = self.gpu.Profile(0)
            self.prof.__enter__()
        except Exception:
            self.restore()
            raise
        return self

    def restore(self):
        for k, v in self.keep.items():
            self.gpu.set_option(k, v)

    def __exit__(self, *exc):
        try:
            self.k3, self.other = self.prof.query("k3_cols_inv")[1], self.prof.query("other")[1]
            self.prof.__exit__(*exc)
        finally:
            self.restore()


def compare(got, exp, what, bad):
    """Positions exact, height and prominence within TOL; returns the worst height error."""
    if [(g.start, g.end) for g in got] != [(e[0], e[1]) for e in exp]:
        bad.append((what, "positions", [(g.start, g.end) for g in got][:6], [(e[0], e[1]) for e in exp][:6]))
        return 0.0
    worst = 0.0
    for g, e in zip(got, exp):
        worst = max(worst, abs(g.height - e[2]))
        if not (abs(g.height - e[2]) < TOL and abs(g.prominence - e[3]) < TOL):
            bad.append((what, "values", (g.start, g.height, g.prominence), e))
    return worst


def sparse_and_dense(gpu, algo, hay, p):
    """(hits, K3 launches) of a sparse call and of the same call with dense_scores = 1."""
    with counting(gpu) as sparse:
        got = algo.match(hay, p)
    with counting(gpu, dense_scores=1) as dense:
        full = algo.match(hay, p)
    return got, sparse.k3, full, dense.k3


def run_family(gpu, cases, log_n, where=""):
    bad, worst, n = [], 0.0, 0
    hays = Haystacks()
    for c in cases:
        n += 1
        what = (c.name, log_n, where)
        p = c.params(log_n)
        exp = sc.expected(c.y, p)
        hay = hays(c, log_n)
        algo = handle(gpu, c, log_n)                                # a fresh handle: no history of minima
        try:
            got, k3, full, k3_dense = sparse_and_dense(gpu, algo, hay, gpu_params(gpu, p))
        finally:
            algo.close()
            hays.clear(c)
        worst = max(worst, compare(got, exp, what, bad))
        if peak_key(got) != peak_key(full):
            bad.append((what, "sparse != dense", peak_key(got)[:4], peak_key(full)[:4]))
        if c.meta["fails"] and not k3 > k3_dense:
            bad.append((what, "built to fail a certificate, but no K3 launch beyond the dense call's", k3, k3_dense, sorted(c.meta["fails"])))
        if not c.meta["fails"] and k3 != k3_dense:
            bad.append((what, "built to pass every certificate, but K3 launches differ from the dense call's", k3, k3_dense))
    print("scan cases %s on 2^%d%s: %d cases, worst |height error| %.3g" % (cases_name(cases), log_n, where, n, worst))
    assert n > 0
    assert not bad, "%d mismatches, first: %s" % (len(bad), bad[:4])


def cases_name(cases):
    return getattr(cases, "__name__", "")


@pytest.mark.parametrize("log_n", sc.FORCED)
@pytest.mark.parametrize("family", sorted(sc.FAMILIES))
def test_forced_plans(gpu, oracle, family, log_n):
    """Every case of the family on the plan forced with the per-handle option log_n: hop 65 536 (8 valid rows), S4 hop
    61 440 (7.5 rows, 500 scores computed beyond the hop)."""
    run_family(gpu, sc.cases(family), log_n, " " + family)


@pytest.mark.parametrize("family", sorted(f for f in sc.NATURAL if f != "T"))
def test_natural_2_21_plan(gpu, oracle, family):
    """S2, S4 and S5 at the geometry the library picks for a needle of 20 000 samples: hop 2 076 672 = 253.5 rows, three
    blocks, the last one alone in its pair."""
    run_family(gpu, sc.cases(family, natural=True), 21, " natural " + family)


# ---------------------------------------------------------------------------
# the ring of recent chunk minima
def ring_sequences(u, d, q):
    """(name, [(design, scale name, fails: True / False / None = not asserted)])."""
    return [("D-then-7-quiet", [(u, "LIB", True), (d, "LIB", None)] + [(q, "LIB", False)] * 7 + [(u, "LIB", False)]),
            ("D-then-8-quiet", [(u, "LIB", True), (d, "LIB", None)] + [(q, "LIB", False)] * 8 + [(u, "LIB", True)]),
            ("own-minimum", [(u, "LIB", True), (u, "LIB", False)] + [(q, "LIB", False)] * 7 + [(u, "LIB", False)] + [(q, "LIB", False)] * 8 + [(u, "LIB", True)]),
            # a call with Scale.NONE feeds ring 0 only, one with Scale.LIB ring 1 only
            ("none-feeds-ring-0", [(d, "NONE", None), (u, "LIB", True), (u, "NONE", False)]),
            ("lib-feeds-ring-1", [(d, "LIB", None), (u, "NONE", True), (u, "LIB", False)])]


@pytest.mark.parametrize("log_n", sc.FORCED)
def test_ring_of_recent_minima(gpu, oracle, log_n):
    """S6: sequences of haystacks on ONE handle through am_match.  A haystack's lowest chunk minimum stays in the ring for
    the next 8 haystacks of the same scale index (AM_SCALE_LIB has its own) and lowers every theta: U fails on a fresh handle,
    passes while D's (or its own) minimum is remembered, and fails again once 8 quiet haystacks have pushed it out.  Pass
    or fail is read from the K3 launch counts against the dense call's; every result equals expected()."""
    u, d, q = sc.s6_designs()
    p = u.params(log_n)
    exp = {c.name: sc.expected(c.y, p) for c in (u, d, q)}
    hays = {c.name: c.haystack(log_n) for c in (u, d, q)}
    other = handle(gpu, u, log_n)
    try:
        with counting(gpu, dense_scores=1) as dense:
            other.match(hays[u.name], gpu_params(gpu, p))
    finally:
        other.close()
    bad = []
    for name, steps in ring_sequences(u, d, q):
        algo = handle(gpu, u, log_n)
        try:
            for i, (c, scale, fails) in enumerate(steps):
                with counting(gpu) as cnt:
                    got = algo.match(hays[c.name], gpu_params(gpu, p, getattr(gpu.Scale, scale)))
                compare(got, exp[c.name], (name, i, c.name, scale), bad)
                if fails is not None and (cnt.k3 > dense.k3) != fails:
                    bad.append((name, "step", i, c.name, scale, "expected to fail" if fails else "expected to pass", cnt.k3, dense.k3))
        finally:
            algo.close()
    assert not bad, "%d mismatches, first: %s" % (len(bad), bad[:4])


# ---------------------------------------------------------------------------
# the other engines, on twins of S1, S2 and S5
def pick(gen, *names):
    by = {c.name: c for c in gen if c.name in names}
    return [by[n] for n in names]


def batches():
    """Failing and passing designs of one layout in the order F, P, F, F, P (both score-side sets see a redo)."""
    s1 = pick(sc.s1(), "S1-b1-r4-t127-l17-unwritten", "S1-b1-r4-t127-l17-written", "S1-b0-r7-t255-l31-unwritten",
              "S1-b2-r1-t1-l30-unwritten", "S1-b2-r1-t1-l30-written")
    s2 = pick(sc.s2(), "S2-A-middle-p2-t127-fail", "S2-A-middle-p2-t127-pass", "S2-A-b0-second-of-pair-p1-t127-fail",
              "S2-A-b1-40-scores-first-of-pair-p4-t0-fail", "S2-A-b1-40-scores-first-of-pair-p4-t0-pass")
    s5 = [c for c in sc.s5() if c.name.startswith("S5-1-")] + [c for c in sc.s5() if c.name.startswith("S5-1-")][:1]
    return [("S1", s1), ("S2", s2), ("S5", s5)]


@pytest.mark.parametrize("log_n", sc.FORCED)
def test_batch_engine_and_both_redo_paths(gpu, oracle, log_n):
    """match_batch_device with debug_redo_arm_at = -1 (failed chunks redone from the host: more K3 launches) and 0 (on the
    device: one launch of the class "other" per haystack): each haystack equals expected() and its single call bit for bit."""
    bad = []
    for fam, cs in batches():
        p = cs[0].params(log_n)
        gp = gpu_params(gpu, p)
        hays = [c.haystack(log_n) for c in cs]
        bufs = [gpu.DeviceBuffer.from_numpy(0, h) for h in hays]
        single = []
        for c, b, h in zip(cs, bufs, hays):
            algo = handle(gpu, c, log_n)
            single.append(peak_key(algo.match_device(b.ptr, h.size, gp)))
            algo.close()
        counts = {}
        for arm in (-1, 0):
            algo = handle(gpu, cs[0], log_n)
            try:
                with counting(gpu, debug_redo_arm_at=arm) as cnt:
                    res = algo.match_batch_device([b.ptr for b in bufs], [h.size for h in hays], gp)
            finally:
                algo.close()
            counts[arm] = (cnt.k3, cnt.other)
            for c, r, s in zip(cs, res, single):
                compare(r, sc.expected(c.y, p), (fam, c.name, log_n, "arm", arm), bad)
                if peak_key(r) != s:
                    bad.append((fam, c.name, log_n, "arm", arm, "batch != single call"))
        any_fail = any(c.meta["fails"] for c in cs)
        if counts[0][1] - counts[-1][1] != len(cs):
            bad.append((fam, log_n, "device redo launches", counts))
        if any_fail and not counts[-1][0] > counts[0][0]:
            bad.append((fam, log_n, "the host path launched no K3 beyond the device path's", counts))
        if not any_fail and counts[-1][0] != counts[0][0]:
            bad.append((fam, log_n, "no design fails, yet the K3 launches differ", counts))
        for b in bufs:
            b.free()
    assert gpu.get_option("debug_redo_arm_at") == -2
    assert not bad, "%d mismatches, first: %s" % (len(bad), bad[:4])


@pytest.mark.parametrize("k3_group", (1, 0))
@pytest.mark.parametrize("log_n", sc.FORCED)
def test_multi_needle_engine(gpu, oracle, log_n, k3_group):
    """match_multi_device with three impulse needles of one length: index 0 gain 1 (scores = design), index 0 gain 2 (the
    LIB scale makes the scores design / 2: nothing reaches min_prominence and the certificate that fails for needle 0
    passes), index 37 gain 1 (scores = design shifted by 37: every run, tile and chunk edge holds other scores).  K3 of
    the group as one launch (k3_group = 1) and one launch per needle; each needle against expected() of its own scores."""
    cs = sc.multi_cases()
    bad = []
    hays = Haystacks()
    keep = gpu.get_option("k3_group")
    gpu.set_option("k3_group", k3_group)
    try:
        for c in cs:
            p = c.params(log_n)
            own = sc.multi_scores(c.y)
            algos = [handle(gpu, c, log_n), handle(gpu, c, log_n, 0, 2.0), handle(gpu, c, log_n, sc.MULTI_Q)]
            buf = gpu.DeviceBuffer.from_numpy(0, hays(c, log_n))
            try:
                res = gpu.match_multi_device(algos, buf.ptr, c.y.size + p.S - 1, gpu_params(gpu, p))
            finally:
                for a in algos:
                    a.close()
                buf.free()
                hays.clear(c)
            for j, (r, y) in enumerate(zip(res, own)):
                compare(r, sc.expected(y, p), (c.name, log_n, "needle", j), bad)
    finally:
        gpu.set_option("k3_group", keep)
    assert not bad, "%d mismatches, first: %s" % (len(bad), bad[:4])


@pytest.mark.parametrize("log_n", sc.FORCED)
def test_streaming_ingest(gpu, oracle, log_n):
    """MatchStream with pushes of 150 001 samples and an announced length 2.5 hops beyond the real one (the side buffer is
    laid out for more blocks than the haystack has): equals expected(), and am_match on a fresh handle bit for bit."""
    cs = pick(sc.s1(), "S1-b1-r4-t127-l17-unwritten", "S1-b1-r4-t127-l17-written", "S1-b0-r7-t255-l31-unwritten")
    cs += pick(sc.s2(), "S2-A-b0-second-of-pair-p1-t127-fail", "S2-A-b0-second-of-pair-p1-t127-pass", "S2-A-b1-40-scores-first-of-pair-p4-t0-fail",
               "S2-A-b1-40-scores-partial-run-in-tile-p4-t1-fail", "S2-A-b1-40-scores-partial-run-in-tile-p4-t1-pass")
    cs += [c for c in sc.s5() if c.name.startswith(("S5-2-", "S5-4-", "S5-7-"))]
    bad = []
    hays = Haystacks()
    for c in cs:
        p = c.params(log_n)
        gp = gpu_params(gpu, p)
        hay = hays(c, log_n)
        ref = handle(gpu, c, log_n)
        algo = handle(gpu, c, log_n)
        st = None
        try:
            want = peak_key(ref.match(hay, gp))
            st = gpu.MatchStream(algo, gp, hay.size + 2 * c.layout.hop + c.layout.hop // 2)
            for off in range(0, hay.size, 150001):
                st.push(hay[off:off + 150001])
            got = st.finish()
        finally:
            if st is not None:
                st.close()
            algo.close()
            ref.close()
            hays.clear(c)
        compare(got, sc.expected(c.y, p), (c.name, log_n, "stream"), bad)
        if peak_key(got) != want:
            bad.append((c.name, log_n, "stream != am_match"))
    assert not bad, "%d mismatches, first: %s" % (len(bad), bad[:4])


def test_tail_block_on_the_natural_2_22_plan(gpu, oracle):
    """A needle of 441 000 samples, three blocks of the 2^22 plan: with tail_block = 1 the last block runs on the 2^21 plan
    (every run written), with 0 as the first half of a pair of its own.  The hidden peak of S1 in block nblocks - 2 and in
    the tail block: expected() under both settings (the two plans' scores agree to rounding only); a hit in front of the
    tail block is the same bit for bit."""
    bad = []
    hays = Haystacks()
    keep = gpu.get_option("tail_block")
    assert keep == 1
    try:
        for c in sc.tail_cases():
            p = c.params(22)
            exp = sc.expected(c.y, p)
            hay = hays(c, 22)
            runs = {}
            for setting in (1, 0):
                gpu.set_option("tail_block", setting)
                algo = handle(gpu, c, 22)
                try:
                    got, k3, full, k3_dense = sparse_and_dense(gpu, algo, hay, gpu_params(gpu, p))
                finally:
                    algo.close()
                compare(got, exp, (c.name, "tail_block", setting), bad)
                if peak_key(got) != peak_key(full):
                    bad.append((c.name, "tail_block", setting, "sparse != dense"))
                in_tail = c.meta["run"][0] == c.layout.nblocks - 1
                fails = bool(c.meta["fails"]) and not (setting == 1 and in_tail)     # (the tail block's runs are all written)
                if fails != (k3 > k3_dense):
                    bad.append((c.name, "tail_block", setting, "certificate", "fails" if fails else "passes", k3, k3_dense))
                runs[setting] = got
            hays.clear(c)
            front = [peak_key([g for g in runs[s] if g.start < (c.layout.nblocks - 1) * c.layout.hop]) for s in (1, 0)]
            if front[0] != front[1] or [g.start for g in runs[1]] != [g.start for g in runs[0]]:
                bad.append((c.name, "tail_block 1 != 0", front))
    finally:
        gpu.set_option("tail_block", keep)
    assert not bad, "%d mismatches, first: %s" % (len(bad), bad[:4])
