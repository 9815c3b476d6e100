"""GPU tests of needle discovery (include/audiomatch.h, "needle discovery").

Array forms: am_probe_scores / am_probe_scores_device against discover_ref on every designed array of
discover_cases.py, bit for bit, at all four 4-byte alignments of the device array (the kernels have one form: slices and
a finish, at every length).

Discovery: every non-skipped probe's record equals am_probe_scores_device over the scores am_correlate_device writes for
that probe's own needle, bit for bit, and -- with no exclusion -- the argmax and max of am_match_trace_device with one
bin; against the f64 reference the places are equal and the scores lie within NCC_BOUND.

NCC_BOUND = 2e-5 is the bound tests/test_gpu_score_norm.py (test_level1_against_checker) holds am_correlate's NCC scores to
for needles of 3 to 40000 samples in haystacks of this size; L = 2048 lies inside that range."""
import ctypes as C

import numpy as np
import pytest

import discover_cases as dc
import discover_ref as dr

pytestmark = pytest.mark.gpu

NCC_BOUND = 2e-5
LP, HP = dr.PAIR["L"], dr.PAIR["H"]


def as_ref(rec):
    return np.asarray(rec, dtype=dr.PROBE_DTYPE)


def upload_at_every_alignment(gpu, buf, x):
    """x four times in buf, copy k starting k floats behind a 16-byte boundary; the device address of each copy."""
    n = x.size
    stride = (n + 3 + 3) // 4 * 4
    packed = np.zeros(4 * stride, dtype=np.float32)
    for k in range(4):
        packed[k * stride + k:k * stride + k + n] = x
    assert packed.nbytes <= buf.nbytes
    assert gpu.lib().am_memcpy_h2d(0, buf.ptr, packed.ctypes.data, packed.nbytes) == 0
    return [buf.ptr + 4 * (k * stride + k) for k in range(4)]


# ---- array forms -----------------------------------------------------------------------------------------------------
def test_designed_arrays_at_every_alignment(gpu):
    cases = dc.cases(gpu.AM_DISCOVER_SLICE)
    buf = gpu.DeviceBuffer(0, 4 * 4 * ((1 << 22) + 8))
    for name, x, lo, hi, sep, claim in cases:
        ref = dr.record(x, lo, hi, sep)
        host = as_ref(gpu.probe_scores(x, lo, hi, sep))
        assert dc.check_claim(host, x, claim) == [], name
        assert dr.same_bits(host, ref), (name, host, ref)
        ptrs = upload_at_every_alignment(gpu, buf, x)
        assert ptrs[0] % 16 == 0
        for k, p in enumerate(ptrs):
            got = as_ref(gpu.probe_scores_device(0, p, x.size, lo, hi, sep))
            assert dr.same_bits(got, ref), (name, "device, base + %d floats" % k, got, ref)
    buf.free()


def test_probe_scores_ranges_and_errors(gpu):
    lib = gpu.lib()
    x = dc.background(1000, 9)
    x[400], x[700] = dc.TOP, dc.NEXT
    # ranges beyond the array and beyond 2^63 are clamped; an empty range excludes nothing
    for lo, hi, sep in ((5, 5, 1), (9, 3, 1), (2000, 1 << 63, 1), (1 << 63, (1 << 64) - 1, 1), (0, 0, (1 << 64) - 1), (0, 0, 1 << 40),
                        (300, (1 << 64) - 1, 1), (401, (1 << 64) - 1, 300)):
        assert dr.same_bits(as_ref(gpu.probe_scores(x, lo, hi, sep)), dr.record(x, lo, hi, sep)), (lo, hi, sep)
    out = np.zeros(1, gpu.PROBE_HIT_DTYPE)
    assert lib.am_probe_scores(0, None, 0, 0, 0, 1, out.ctypes.data) == 0 and int(out[0]["flags"]) == 3 and np.isnan(out[0]["ncc"])
    assert lib.am_probe_scores(0, x.ctypes.data, x.size, 0, 0, 0, out.ctypes.data) == gpu.AM_ERR_INVALID_ARG
    assert b"separation" in lib.am_last_error_string()
    assert lib.am_probe_scores(0, None, 5, 0, 0, 1, out.ctypes.data) == gpu.AM_ERR_INVALID_ARG
    assert lib.am_probe_scores(0, x.ctypes.data, x.size, 0, 0, 1, None) == gpu.AM_ERR_INVALID_ARG
    assert lib.am_probe_scores_device(0, x.ctypes.data, x.size, 0, 0, 1, out.ctypes.data) == gpu.AM_ERR_INVALID_ARG   # host memory
    assert b"d_scores" in lib.am_last_error_string()
    buf = gpu.DeviceBuffer.from_numpy(0, x)
    assert lib.am_probe_scores_device(0, buf.ptr + 2, 10, 0, 0, 1, out.ctypes.data) == gpu.AM_ERR_INVALID_ARG
    assert b"aligned" in lib.am_last_error_string()
    buf.free()


# ---- discovery -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(gpu):
    a, b, recs, arrays = dr.pair_reference()
    da, db = gpu.DeviceBuffer.from_numpy(0, a), gpu.DeviceBuffer.from_numpy(0, b)
    dp = gpu.discover_params(LP, HP)
    got = gpu.discover_device(0, da.ptr, a.size, db.ptr, b.size, dp)
    yield dict(a=a, b=b, ref=recs, arrays=arrays, da=da, db=db, dp=dp, got=got)
    da.free()
    db.free()


def scores_of_own_needle(gpu, d_probe, d_b, len_b, out_buf):
    """The scores am_correlate_device writes for a needle made from the probe (score_norm 1, Valid, LIB), in out_buf."""
    algo = gpu.HipConvolve.from_device(0, d_probe, LP)
    algo.set_option("score_norm", 1)
    n = C.c_size_t(0)
    assert gpu.lib().am_correlate_device(algo._h, d_b, len_b, int(gpu.Mode.Valid), int(gpu.Scale.LIB), out_buf.ptr, len_b - LP + 1, C.byref(n)) == 0
    assert n.value == len_b - LP + 1
    return algo, n.value


def check_against_f64(got, ref, arrays, ex_of, what):
    """Places equal, scores within NCC_BOUND; runner-up places where the reference's second and third differ enough."""
    assert got.size == ref.size
    worst, compared = 0.0, 0
    for i in range(ref.size):
        g, r = got[i], ref[i]
        assert int(g["probe"]) == int(r["probe"]) and int(g["flags"]) == int(r["flags"]) and int(g["reserved"]) == 0, (what, i, g, r)
        if int(r["flags"]) & ~dr.NO_SECOND:
            assert int(g["best"]) == 0 and int(g["second"]) == 0 and np.isnan(g["ncc"]) and np.isnan(g["ncc_second"]), (what, i, g)
            continue
        assert int(g["best"]) == int(r["best"]), (what, i, g, r)
        lo, hi = ex_of(i)
        f = arrays[i]
        e1, e2 = abs(float(g["ncc"]) - f[int(r["best"])]), abs(float(g["ncc_second"]) - f[int(g["second"])])
        worst = max(worst, e1, e2)
        assert e1 <= NCC_BOUND and e2 <= NCC_BOUND, (what, i, e1, e2)
        # the device's runner-up is a legitimate one: far enough from the best, not excluded, as large as the reference's
        assert abs(int(g["second"]) - int(g["best"])) >= LP and not lo <= int(g["second"]) < hi
        assert abs(float(g["ncc_second"]) - float(r["ncc_second"])) <= NCC_BOUND, (what, i)
        if float(r["ncc_second"]) - dr.third_candidate(f, r, lo, hi, LP) > 4 * NCC_BOUND:
            assert int(g["second"]) == int(r["second"]), (what, i, g, r)
            compared += 1
    print("%s: largest |score - f64| %.3g (bound %.3g), runner-up places compared in %d of %d probes" % (what, worst, NCC_BOUND, compared, ref.size))
    assert 2 * compared >= ref.size


def test_pair_equals_todays_api_bit_for_bit(gpu, pair):
    a, b, got = pair["a"], pair["b"], pair["got"]
    n = b.size - LP + 1
    out = gpu.DeviceBuffer(0, 4 * n)
    skipped = 0
    for i in range(got.size):
        p = i * HP
        assert int(got[i]["probe"]) == p
        if int(got[i]["flags"]) & (gpu.AM_PROBE_NONFINITE | gpu.AM_PROBE_QUIET):
            skipped += 1
            continue
        algo, cnt = scores_of_own_needle(gpu, pair["da"].ptr + 4 * p, pair["db"].ptr, b.size, out)
        want = as_ref(gpu.probe_scores_device(0, out.ptr, cnt, 0, 0, LP))
        want["probe"] = p
        assert dr.same_bits(as_ref(got[i]), want), (i, got[i], want)
        one = algo.match_trace_device(pair["db"].ptr, b.size, gpu.trace_params(n))
        assert one.size == 1 and int(one[0]["argmax"]) == int(got[i]["best"])
        assert np.float32(one[0]["max"]).tobytes() == np.float32(got[i]["ncc"]).tobytes()
        algo.close()
    out.free()
    assert skipped == 1 and int(got[20]["flags"]) == gpu.AM_PROBE_QUIET


def test_pair_against_f64_and_its_region(gpu, pair):
    got = pair["got"]
    check_against_f64(got, pair["ref"], pair["arrays"], lambda i: (0, 0), "pair design")
    d = got["best"].astype(np.int64) - got["probe"].astype(np.int64)
    assert all(d[i] == 31000 and got[i]["ncc"] >= 0.918 - NCC_BOUND for i in range(9, 15))
    assert int(got[20]["flags"]) == gpu.AM_PROBE_QUIET
    reg = gpu.discover_regions(got, pair["dp"], gpu.region_params(0.6, 128, 2, 1))
    assert reg.size == 1
    assert (int(reg[0]["a_start"]), int(reg[0]["length"]), int(reg[0]["displacement"]), int(reg[0]["good"]), int(reg[0]["count"])) == (9216, 8192, 31000, 7, 7)
    want = dr.regions(got, LP, 0.6, 128, 2, 1)
    assert dr.same_regions(np.asarray(reg, dtype=dr.REGION_DTYPE), want)


@pytest.mark.parametrize("fresh", [False, True])
def test_self_design(gpu, fresh):
    x, ref, arrays = dr.self_reference(fresh)
    dx = gpu.DeviceBuffer.from_numpy(0, x)
    dp = gpu.discover_params(LP, HP, exclude=LP, flags=gpu.AM_DISCOVER_SELF)
    got = gpu.discover_device(0, dx.ptr, x.size, dx.ptr, x.size, dp)
    ex_of = lambda i: (max(0, i * HP - LP + 1), i * HP + LP)
    check_against_f64(got, ref, arrays, ex_of, "self design (fresh generator)" if fresh else "self design")
    for i in range(got.size):                                 # no record has its best inside its excluded zone
        assert abs(int(got[i]["best"]) - i * HP) >= LP
    fold = gpu.discover_regions(got, dp, gpu.region_params(0.6, 128, 2, 1, flags=gpu.AM_REGION_FOLD))
    both = gpu.discover_regions(got, dp, gpu.region_params(0.6, 128, 2, 1))
    assert fold.size == 1 and (int(fold[0]["a_start"]), int(fold[0]["length"]), int(fold[0]["displacement"])) == (5120, 6144, 45000)
    assert both.size == 2 and (int(both[1]["a_start"]), int(both[1]["length"]), int(both[1]["displacement"])) == (50176, 6144, -45000)
    # equality with today's API where a zone is excluded: two probes, one of each occurrence
    out = gpu.DeviceBuffer(0, 4 * (x.size - LP + 1))
    for i in (6, 50):
        algo, cnt = scores_of_own_needle(gpu, dx.ptr + 4 * i * HP, dx.ptr, x.size, out)
        lo, hi = ex_of(i)
        want = as_ref(gpu.probe_scores_device(0, out.ptr, cnt, lo, hi, LP))
        want["probe"] = i * HP
        assert dr.same_bits(as_ref(got[i]), want), (i, got[i], want)
        algo.close()
    out.free()
    dx.free()


def test_host_form_equals_device_form_and_capacity(gpu, pair):
    a, b, dp = pair["a"], pair["b"], pair["dp"]
    host = gpu.discover(a, b, dp)
    assert dr.same_bits(as_ref(host), as_ref(pair["got"]))
    # cap < P: what fits is filled, P is reported
    out = np.zeros(5, gpu.PROBE_HIT_DTYPE)
    n = C.c_size_t(0)
    rc = gpu.lib().am_discover_device(0, pair["da"].ptr, a.size, pair["db"].ptr, b.size, int(gpu.Fmt.F32_MONO), C.byref(dp), out.ctypes.data, 5, C.byref(n))
    assert rc == gpu.AM_ERR_CAPACITY and n.value == 31 == gpu.discover_len(a.size, dp)
    assert dr.same_bits(as_ref(out), as_ref(pair["got"][:5]))
    rc = gpu.lib().am_discover_device(0, pair["da"].ptr, a.size, pair["db"].ptr, b.size, int(gpu.Fmt.F32_MONO), C.byref(dp), None, 0, C.byref(n))
    assert rc == gpu.AM_ERR_CAPACITY and n.value == 31
    # len_a < L: no records; len_b < L: no probe has a candidate
    assert gpu.discover(a[:LP - 1], b, dp).size == 0
    none = gpu.discover(a[:3 * LP], b[:LP - 1], dp)
    assert none.size == 5 and all(int(f) == 3 for f in none["flags"]) and np.all(np.isnan(none["ncc"]))
    # a separation of its own; L = len_b: one score
    far = gpu.discover(a[:LP], b, gpu.discover_params(LP, HP, separation=30000))
    want = dr.record(pair["arrays"][0], 0, 0, 30000)
    assert far.size == 1 and int(far[0]["flags"]) == 0 and (int(far[0]["best"]), int(far[0]["second"])) == (int(want["best"]), int(want["second"]))
    assert abs(int(far[0]["second"]) - int(far[0]["best"])) >= 30000
    one = gpu.discover(a[:LP], b[:LP], dp)
    assert one.size == 1 and int(one[0]["flags"]) == gpu.AM_PROBE_NO_SECOND and int(one[0]["best"]) == 0


def test_nonfinite_samples(gpu, pair):
    """A NaN in one probe: that probe (and the neighbour that overlaps it there) is AM_PROBE_NONFINITE, every other record keeps its
    bits.  A NaN in B far from the copy costs exactly the windows that hold it."""
    a, b, dp = pair["a"].copy(), pair["b"].copy(), pair["dp"]
    a[5 * HP + 1500] = np.nan                              # inside probe 5 and the first half of probe 6
    got = gpu.discover(a, b, dp)
    for i in range(got.size):
        if i in (5, 6):
            assert int(got[i]["flags"]) == gpu.AM_PROBE_NONFINITE and int(got[i]["best"]) == 0 and np.isnan(got[i]["ncc"])
        else:
            assert dr.same_bits(as_ref(got[i]), as_ref(pair["got"][i])), i
    a = pair["a"]
    b[10000], b[10001], b[60000] = np.nan, np.inf, -np.inf
    got = gpu.discover(a, b, dp)
    ref, arrays = dr.discover(a, b, LP, HP)
    dead = np.zeros(b.size - LP + 1, bool)
    for t in (10000, 10001, 60000):
        dead[max(0, t - LP + 1):t + 1] = True
    assert np.array_equal(np.isnan(arrays[0]), dead)
    for i in range(got.size):
        if int(ref[i]["flags"]):
            assert int(got[i]["flags"]) == int(ref[i]["flags"])
            continue
        assert int(got[i]["best"]) == int(ref[i]["best"]) and not dead[int(got[i]["best"])] and not dead[int(got[i]["second"])], i
        assert abs(float(got[i]["ncc"]) - arrays[i][int(ref[i]["best"])]) <= NCC_BOUND
    # the copy's probes are untouched: their windows lie far from the dead ones
    for i in range(9, 15):
        assert int(got[i]["best"]) == int(pair["got"][i]["best"])
    # a score array whose first and last windows are dead, read through the array form: exactly those are skipped
    algo = gpu.HipConvolve(a[:LP], score_norm=True)
    trace = algo.match_trace(b, b.size - LP + 1)
    assert int(trace[0]["count"]) == int((~dead).sum())
    algo.close()


def test_s16_stereo_gives_the_same_places(gpu, pair):
    """The same signals as i16 stereo frames (both channels the signal, scaled to +-4 sigma = full scale)."""
    def frames(x):
        q = np.clip(np.rint(x.astype(np.float64) * 8000.0), -32768, 32767).astype(np.int16)
        return np.stack([q, q], axis=1)
    a16, b16 = frames(pair["a"]), frames(pair["b"])
    dp = pair["dp"]
    got = gpu.discover(a16, b16, dp)
    want = pair["got"]
    assert got.size == want.size
    ma, mb = gpu.pcm_s16_stereo_to_mono(a16), gpu.pcm_s16_stereo_to_mono(b16)
    mono = gpu.discover(ma, mb, dp)
    assert dr.same_bits(as_ref(got), as_ref(mono))           # the bit-exact down-mix, done inside
    for i in range(8, 16):                                 # the copy's probes: the places of the f32 signals
        assert int(got[i]["best"]) == int(want[i]["best"]) and abs(float(got[i]["ncc"]) - float(want[i]["ncc"])) < 1e-3
    assert np.array_equal(got["flags"], want["flags"])
    da, db = gpu.DeviceBuffer.from_numpy(0, a16), gpu.DeviceBuffer.from_numpy(0, b16)
    dev = gpu.discover_device(0, da.ptr, a16.shape[0], db.ptr, b16.shape[0], dp, fmt=gpu.Fmt.S16_STEREO)
    assert dr.same_bits(as_ref(dev), as_ref(got))
    da.free()
    db.free()


def test_discovery_is_ncc_whatever_the_default_and_is_profiled(gpu, pair):
    a, b, dp = pair["a"], pair["b"], pair["dp"]
    keep = gpu.get_option("score_norm")
    try:
        for v in (0, 1):
            gpu.set_option("score_norm", v)
            got = gpu.discover_device(0, pair["da"].ptr, 4 * LP, pair["db"].ptr, b.size, dp)
            assert dr.same_bits(as_ref(got), as_ref(pair["got"][:got.size])), v
    finally:
        gpu.set_option("score_norm", keep)
    lib = gpu.lib()
    ms, launches = C.c_double(0), C.c_uint64(0)
    assert lib.am_profile_reset(0) == 0 and lib.am_profile_enable(0, 1) == 0
    try:
        gpu.discover_device(0, pair["da"].ptr, 4 * LP, pair["db"].ptr, b.size, dp)
    finally:
        assert lib.am_profile_enable(0, 0) == 0
    assert lib.am_profile_query(0, b"discover", C.byref(ms), C.byref(launches)) == 0
    assert launches.value == 1 + 7 and ms.value > 0          # the energy launch and one reduction per probe


def test_invalid_arguments(gpu, pair):
    lib = gpu.lib()
    a, b = pair["a"], pair["b"]
    out = np.zeros(40, gpu.PROBE_HIT_DTYPE)
    n = C.c_size_t(0)
    F32 = int(gpu.Fmt.F32_MONO)

    def dev(dp, pa=pair["da"].ptr, pb=pair["db"].ptr, fmt=F32, o=out.ctypes.data, cap=40, cnt=C.byref(n)):
        return lib.am_discover_device(0, pa, a.size, pb, b.size, fmt, dp, o, cap, cnt)

    def host(dp, pa=a.ctypes.data, pb=b.ctypes.data, fmt=F32, o=out.ctypes.data, cap=40, cnt=C.byref(n)):
        return lib.am_discover(0, pa, a.size, pb, b.size, fmt, dp, o, cap, cnt)

    good = gpu.discover_params(LP, HP)
    for call in (dev, host):
        assert call(None) == gpu.AM_ERR_INVALID_ARG
        assert call(C.byref(good), pa=None) == gpu.AM_ERR_INVALID_ARG
        assert call(C.byref(good), pb=None) == gpu.AM_ERR_INVALID_ARG
        assert call(C.byref(good), o=None) == gpu.AM_ERR_INVALID_ARG
        assert call(C.byref(good), cnt=None) == gpu.AM_ERR_INVALID_ARG
        assert call(C.byref(good), fmt=7) == gpu.AM_ERR_INVALID_ARG and b"format" in lib.am_last_error_string()
        for kw, word in ((dict(probe_len=0, hop=HP), b"probe_len"), (dict(probe_len=LP, hop=0), b"hop"),
                         (dict(probe_len=LP, hop=HP, exclude=LP), b"exclude"), (dict(probe_len=LP, hop=HP, flags=4), b"flags")):
            assert call(C.byref(gpu.discover_params(**kw))) == gpu.AM_ERR_INVALID_ARG
            assert word in lib.am_last_error_string(), kw
        bad = gpu.discover_params(LP, HP)
        bad.reserved = 9
        assert call(C.byref(bad)) == gpu.AM_ERR_INVALID_ARG and b"reserved" in lib.am_last_error_string()
    # more probe parts than one energy launch has workgroups for: refused by name, nothing launched
    long_probe = gpu.discover_params(1 << 16, 1)           # 256 parts per probe, 74465 probes: more than 2^24 workgroups
    big = np.zeros(74465, gpu.PROBE_HIT_DTYPE)
    wide = np.ones((1 << 16) + 74464, np.float32)
    rc = lib.am_discover(0, wide.ctypes.data, wide.size, b.ctypes.data, b.size, F32, C.byref(long_probe), big.ctypes.data, big.size, C.byref(n))
    assert rc == gpu.AM_ERR_INVALID_ARG and b"too many probes" in lib.am_last_error_string()
    # host memory where device memory is expected
    assert dev(C.byref(good), pa=a.ctypes.data) == gpu.AM_ERR_INVALID_ARG and b"d_a" in lib.am_last_error_string()
    assert dev(C.byref(good), pb=b.ctypes.data) == gpu.AM_ERR_INVALID_ARG and b"d_b" in lib.am_last_error_string()
    if gpu.device_count() > 1:
        other = gpu.DeviceBuffer.from_numpy(1, b)
        assert dev(C.byref(good), pb=other.ptr) == gpu.AM_ERR_INVALID_ARG
        other.free()
