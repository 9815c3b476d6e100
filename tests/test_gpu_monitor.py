"""Live monitoring (am_monitor_*): what poll and end return for a needle, concatenated, equals am_match_part_device
over the fixed window groups merged by am_merge_peaks, bit for bit and for every push pattern; offsets equal am_match on
the whole recording; hits come back as soon as am_merge_ready declares them final; the sample buffer never grows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 8000
S = 1000                       # needle length (samples)
L = 60 * SR + 777              # recording length
HITS = [3.3, 9.7, 15.95, 20.0, 21.5, 31.99, 47.2, 58.6]   # 15.95: across a window boundary; 21.5 shadows 20.0 or v.v.
PUSHES = ["1152", "1s", "random", "all"]


def make_params(am, overlap=S, distance=3.0, prom=0.3):
    p = am.Config(chunk_size_s=2.0, overlap_length_s=0.0, distance_s=distance, prominence=prom).params(SR, am.Scale.LIB)
    p.overlap = int(overlap)
    return p


def signal(oracle, kind, needle, seed=7):
    if kind == "white":
        x = oracle.synth_uniform(seed, 1, 0, L).astype(np.float64)
    else:   # AR(1)
        e = np.random.default_rng(seed).standard_normal(L) * 0.05
        x = np.empty(L)
        acc = 0.0
        a = 0.9
        for i in range(L):     # (scipy may be missing: a plain loop, 0.5 s)
            acc = a * acc + e[i]
            x[i] = acc
    for t in HITS:
        o = int(t * SR)
        x[o:o + len(needle)] += needle * (1.5 if t == 21.5 else 1.0)
    return x.astype(np.float32)


def to_pcm16(x):
    m = np.clip(np.round(x * 16384.0), -32768, 32767).astype(np.int16)
    return np.repeat(m, 2)     # l == r: the down-mix gives the same mono signal


def groups(length, chunk, overlap, G):
    g, out = 0, []
    span = (G - 1) * chunk + chunk + overlap
    while g * G * chunk < length:
        first = g * G * chunk
        out.append((first, min(length, first + span) - first))
        g += 1
    return out


def reference(am, algo, buf, length, p, G, fmt):
    """am_match_part_device over the fixed groups, then am_merge_peaks (and the raw union, per group)"""
    raw, per_group = [], []
    for first, n in groups(length, p.chunk, p.overlap, G):
        part = am.match_part_device(algo, buf.ptr + 4 * first, n, p, G, first, fmt)
        per_group.append(part)
        raw += part
    return am.merge_peaks(p, raw), per_group


def bits(peaks):
    return [(q.start, q.end, np.float32(q.height).tobytes(), np.float32(q.prominence).tobytes()) for q in peaks]


def pieces(n_frames, how, seed=3):
    if how == "all":
        return [(0, n_frames)]
    if how == "1152":
        step = [1152]
    elif how == "1s":
        step = [SR]
    else:
        step = list(np.random.default_rng(seed).integers(1, 3 * SR, size=400))
    out, a, i = [], 0, 0
    while a < n_frames:
        b = min(n_frames, a + int(step[i % len(step)]))
        out.append((a, b))
        a, i = b, i + 1
    return out


def run_monitor(am, algos, params, data, fmt, G, how, frame=1):
    """every (needle, peak) in the order poll / end return them, and the index of the push after which each came"""
    m = am.HipMonitor(algos, params, fmt, group_windows=G)
    got, when = [], []
    for k, (a, b) in enumerate(pieces(len(data) // frame, how)):
        new = m.push(data[a * frame:b * frame])
        got += new
        when += [k] * len(new)
    new = m.end()
    got += new
    when += [None] * len(new)
    m.close()
    return got, when


def per_needle(got, j):
    return [q for (i, q) in got if i == j]


@pytest.mark.parametrize("fmt_kind", [("f32", "white"), ("s16", "ar1")])
@pytest.mark.parametrize("G", [1, 3])
def test_monitor_equals_parts_for_every_push_pattern(gpu, oracle, fmt_kind, G):
    am = gpu
    fmtname, kind = fmt_kind
    needle = oracle.synth_uniform(11, 2, 0, S)
    x = signal(oracle, kind, needle)
    p = make_params(am)
    algo = am.HipConvolve(needle)
    if fmtname == "f32":
        fmt, data, frame = am.Fmt.F32_MONO, x, 1
        whole = algo.match(x, p)
    else:   # i16 at half scale: a needle of half the amplitude keeps the LIB scores of planted hits at 1
        algo = am.HipConvolve(needle * np.float32(0.5))
        fmt, data, frame = am.Fmt.S16_STEREO, to_pcm16(x), 2
        whole = algo.match_pcm16(data, p)
    buf = am.DeviceBuffer.from_numpy(0, data)
    X, _ = reference(am, algo, buf, L, p, G, fmt)
    assert len(X) >= 6, X
    first = None
    for how in PUSHES:
        got, _ = run_monitor(am, [algo], p, data, fmt, G, how, frame)
        assert all(i == 0 for i, _ in got)
        mine = bits(per_needle(got, 0))
        assert mine == bits(X), (how, G)
        if first is None:
            first = mine
        assert mine == first, how
    # against am_match on the whole recording: offsets exact, values to f32 rounding
    assert [(q.start, q.end) for q in X] == [(q.start, q.end) for q in whole]
    for a, b in zip(X, whole):
        assert abs(a.height - b.height) <= 1e-5 * max(1.0, abs(b.height))
        assert abs(a.prominence - b.prominence) <= 1e-5 * max(1.0, abs(b.prominence))
    buf.free()


def test_two_needles_of_different_lengths(gpu, oracle):
    am = gpu
    n1 = oracle.synth_uniform(11, 2, 0, S)
    n2 = oracle.synth_uniform(12, 3, 0, 1600)
    x = signal(oracle, "white", n1)
    for t in (7.1, 26.3, 44.4):
        o = int(t * SR)
        x[o:o + 1600] += n2
    a1, a2 = am.HipConvolve(n1), am.HipConvolve(n2)
    p1, p2 = make_params(am, S), make_params(am, 1600)
    for G in (1, 3):
        got, _ = run_monitor(am, [a1, a2], [p1, p2], x, am.Fmt.F32_MONO, G, "random")
        keys = [(q.start, i) for i, q in got]
        assert keys == sorted(keys)
        alone1, _ = run_monitor(am, [a1], p1, x, am.Fmt.F32_MONO, G, "1s")
        alone2, _ = run_monitor(am, [a2], p2, x, am.Fmt.F32_MONO, G, "1s")
        assert bits(per_needle(got, 0)) == bits(per_needle(alone1, 0))
        assert bits(per_needle(got, 1)) == bits(per_needle(alone2, 0))
        assert [q.start for q in per_needle(got, 1)] == [int(t * SR) for t in (7.1, 26.3, 44.4)]


def nanos(start):
    return start * (10 ** 9 // SR)      # exact at 8 kHz (start_nanos of the library)


def test_latency_follows_the_finality_rule(gpu, oracle):
    am = gpu
    needle = oracle.synth_uniform(11, 2, 0, S)
    x = signal(oracle, "white", needle)
    p = make_params(am)
    algo = am.HipConvolve(needle)
    G = 1
    buf = am.DeviceBuffer.from_numpy(0, x)
    X, per_group = reference(am, algo, buf, L, p, G, am.Fmt.F32_MONO)
    raw = sorted([q for part in per_group for q in part], key=lambda q: q.start)
    got, when = run_monitor(am, [algo], p, x, am.Fmt.F32_MONO, G, "1s")
    assert bits([q for _, q in got]) == bits(X)
    step, span = G * p.chunk, (G - 1) * p.chunk + p.chunk + p.overlap
    maxd = int(round(p.overshadow_distance_s * 1e9))
    n_groups = len(groups(L, p.chunk, p.overlap, G))
    for (_, q), k in zip(got, when):
        i = next(i for i, r in enumerate(raw) if (r.start, r.end, r.height) == (q.start, q.end, q.height))
        succ = raw[i + 1].start if i + 1 < len(raw) else None
        g = 1
        while g <= n_groups:
            H = g * step
            if H > q.start and ((succ is not None and succ < H) or nanos(H) - nanos(q.start) >= maxd):
                break
            g += 1
        done_at = (g - 1) * step + span          # samples that complete group g - 1, the g-th matched
        if g > n_groups or done_at > L:
            assert k is None, (q, k)
        else:
            assert k == (done_at + SR - 1) // SR - 1, (q, k, done_at)
            assert (k + 1) * SR >= q.start + S    # never before its own window has arrived
    buf.free()


def test_memory_is_bounded_and_horizon_advances(gpu, oracle):
    am = gpu
    needle = oracle.synth_uniform(11, 2, 0, S)
    x = signal(oracle, "white", needle)
    p = make_params(am)
    algo = am.HipConvolve(needle)
    G = 3
    span = (G - 1) * p.chunk + p.chunk + p.overlap
    bound = 4 * (2 * span + 65536)
    m = am.HipMonitor([algo], p, am.Fmt.F32_MONO, group_windows=G)
    r0 = m.info().resident_bytes
    assert 0 < r0 <= bound
    pushed, last_h = 0, 0
    rng = np.random.default_rng(1)
    while pushed < 10 * 2 * span:
        n = int(rng.integers(1, 20000))
        a = pushed % (L - n)
        m.push(x[a:a + n])
        pushed += n
        inf = m.info()
        assert inf.received == pushed
        assert inf.resident_bytes == r0
        assert inf.horizon >= last_h and pushed - inf.horizon < span
        last_h = inf.horizon
    assert last_h > 8 * span
    m.end()
    assert m.info().resident_bytes == r0 and m.info().pending == 0
    m.close()


def test_nan_run_costs_only_its_windows(gpu, oracle):
    am = gpu
    needle = oracle.synth_uniform(11, 2, 0, S)
    x = signal(oracle, "white", needle)
    x[int(33.5 * SR):int(33.5 * SR) + 50] = np.nan
    p = make_params(am)
    algo = am.HipConvolve(needle)
    buf = am.DeviceBuffer.from_numpy(0, x)
    for G in (1, 3):
        X, _ = reference(am, algo, buf, L, p, G, am.Fmt.F32_MONO)
        got, _ = run_monitor(am, [algo], p, x, am.Fmt.F32_MONO, G, "random")
        assert bits([q for _, q in got]) == bits(X)
        whole = algo.match(x, p)
        assert [(q.start, q.end) for q in X] == [(q.start, q.end) for q in whole]
    buf.free()


def test_half_pipeline_keeps_exact_offsets_and_options_are_read_at_begin(gpu, oracle):
    am = gpu
    needle = oracle.synth_uniform(11, 2, 0, S)
    x = signal(oracle, "white", needle)
    p = make_params(am)
    algo = am.HipConvolve(needle)
    exact = [q.start for q in algo.match(x, p)]
    old = am.get_option("half_pipeline")
    try:
        am.set_option("half_pipeline", 1)
        m = am.HipMonitor([algo], p, am.Fmt.F32_MONO, group_windows=2)
    finally:
        am.set_option("half_pipeline", old)
    got = m.push(x) + m.end()
    m.close()
    assert [q.start for _, q in got] == exact


def test_refusals(gpu, oracle):
    am = gpu
    needle = oracle.synth_uniform(11, 2, 0, S)
    p = make_params(am)
    nc = am.HipConvolve(needle, score_norm=True)
    with pytest.raises(am.AudioMatchError, match="score_norm: not supported by this entry point"):
        am.HipMonitor([nc], p)
    algo = am.HipConvolve(needle)
    with pytest.raises(am.AudioMatchError, match="sample_format"):
        am.HipMonitor([algo], p, fmt=7)
    bad = make_params(am)
    bad.chunk = 0
    with pytest.raises(am.AudioMatchError, match=r"params\[0\]: chunk"):
        am.HipMonitor([algo], bad)
    other = make_params(am)
    other.sr = SR * 2
    with pytest.raises(am.AudioMatchError, match=r"params\[1\]: sr"):
        am.HipMonitor([algo, algo], [p, other])
    import ctypes as C
    out = C.c_void_p()
    assert am.lib().am_monitor_begin(None, 0, C.byref(p), 0, 1, C.byref(out)) == am.AM_ERR_INVALID_ARG
    assert "needles" in am.lib().am_last_error_string().decode()
    m = am.HipMonitor([algo], p)
    m.end()
    with pytest.raises(am.AudioMatchError, match="ended"):
        m.push(np.zeros(10, np.float32))
    m.close()
