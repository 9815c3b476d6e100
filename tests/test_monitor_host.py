"""am_merge_ready (the finality rule of live monitoring) is host code: for every horizon the prefix it declares ready
keeps its kept / overshadowed pattern under am_merge_peaks whatever peaks at or after the horizon follow, and it is the
longest such prefix.  The header declares the monitor, the binding and the library export it, the CLI offers --live."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MONITOR = ["am_merge_ready", "am_monitor_begin", "am_monitor_push", "am_monitor_poll", "am_monitor_end",
           "am_monitor_info_get", "am_monitor_destroy"]


@pytest.fixture(params=[0, 1], ids=["surrounding_unfiltered", "surrounding_kept"])
def surrounding(request, amlib):
    old = amlib.get_option("surrounding_from")
    amlib.set_option("surrounding_from", request.param)
    yield request.param
    amlib.set_option("surrounding_from", old)


def params(amlib, sr, dist):
    return amlib.AmMatchParams(sr=sr, chunk=sr, overlap=0, min_prominence=0.1, min_distance=0, overshadow_distance_s=dist,
                               scale=1)


def peak(amlib, start, prom, ident):
    return amlib.Peak(int(start), int(ident), 1.0, float(prom))    # `end` carries an identity through the merge


def pattern(amlib, p, peaks, k):
    kept = {q.end for q in amlib.merge_peaks(p, peaks, cap=len(peaks) + 1)}
    return [q.end in kept for q in peaks[:k]]


def random_list(amlib, rng, n, span, ident0=0):
    if n == 0:
        return []
    starts = np.sort(rng.integers(0, span, size=n))
    starts[rng.random(n) < 0.2] = starts[0]          # ties in start
    starts = np.sort(starts)
    proms = rng.choice([0.2, 0.5, 0.5, 0.9, 1.3, 2.0], size=n)
    return [peak(amlib, s, pr, ident0 + i) for i, (s, pr) in enumerate(zip(starts, proms))]


@pytest.mark.parametrize("sr,dist", [(8000, 3.0), (44100, 2.5), (48000, 0.7), (22050, 10.0)])
def test_ready_prefix_is_final_and_longest(amlib, surrounding, sr, dist):
    rng = np.random.default_rng(sr + int(dist * 10) + surrounding)
    p = params(amlib, sr, dist)
    span = int(12 * dist * sr)
    for trial in range(25):
        full = random_list(amlib, rng, int(rng.integers(1, 18)), span)
        assert amlib.merge_ready(p, full, span, ended=True) == len(full)
        for horizon in sorted(set([0, span] + [int(x) for x in rng.integers(0, span, size=6)] + [q.start + 1 for q in full])):
            prefix = [q for q in full if q.start < horizon]
            k = amlib.merge_ready(p, prefix, horizon)
            assert k in (len(prefix), len(prefix) - 1) or (not prefix and k == 0)
            ref = pattern(amlib, p, prefix, k)
            for c in range(6):
                cont = random_list(amlib, rng, int(rng.integers(0, 6)), int(3 * dist * sr), ident0=1000)
                cont = [peak(amlib, horizon + q.start * (c % 3) // 2, q.prominence, q.end) for q in cont]
                cont.sort(key=lambda q: q.start)
                assert pattern(amlib, p, prefix + cont, k) == ref, (trial, horizon, c)
            if prefix and k < len(prefix):
                # not ready: a strong peak at the horizon decides against what happens without it
                strong = peak(amlib, horizon, 1e30, 2000)
                assert pattern(amlib, p, prefix, len(prefix))[-1] != pattern(amlib, p, prefix + [strong], len(prefix))[-1]


def test_lone_peak_at_the_overshadow_distance(amlib, surrounding):
    sr, dist = 8000, 3.0
    p = params(amlib, sr, dist)
    d = int(dist * sr)
    one = [peak(amlib, 1000, 0.5, 0)]
    assert amlib.merge_ready(p, one, 1000 + d) == 1        # distance == max: not overshadowed (strict <)
    assert amlib.merge_ready(p, one, 1000 + d - 1) == 0    # one sample closer: a stronger peak there would win
    assert amlib.merge_ready(p, one, 1001) == 0
    assert amlib.merge_ready(p, one, 1001, ended=True) == 1
    assert amlib.merge_ready(p, [], 5) == 0
    # the last peak under its stronger predecessor is settled (overshadowed whatever comes)
    two = [peak(amlib, 1000, 2.0, 0), peak(amlib, 2000, 0.5, 1)]
    assert amlib.merge_ready(p, two, 2001) == 2
    # a successor present settles its predecessor; the last, stronger, waits
    two = [peak(amlib, 1000, 0.5, 0), peak(amlib, 1500, 0.9, 1)]
    assert amlib.merge_ready(p, two, 1501) == 1


def test_merge_ready_refuses_bad_lists(amlib):
    p = params(amlib, 8000, 3.0)
    with pytest.raises(amlib.AudioMatchError, match="not sorted"):
        amlib.merge_ready(p, [peak(amlib, 10, 1, 0), peak(amlib, 5, 1, 1)], 100)
    with pytest.raises(amlib.AudioMatchError, match="horizon"):
        amlib.merge_ready(p, [peak(amlib, 10, 1, 0)], 10)
    p.sr = 0
    with pytest.raises(amlib.AudioMatchError, match="sr"):
        amlib.merge_ready(p, [peak(amlib, 10, 1, 0)], 100)


def test_header_binding_and_library_carry_the_monitor(amlib):
    txt = open(os.path.join(ROOT, "include", "audiomatch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", amlib.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (am_[a-z0-9_]+)\b", out))
    for name in MONITOR:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in amlib.declared_symbols() and name in exported, name
    assert "typedef struct am_monitor_info" in code
    assert callable(amlib.HipMonitor) and callable(amlib.merge_ready)
    hpp = open(os.path.join(ROOT, "include", "audiomatch.hpp")).read()
    assert "am_monitor_begin(" in hpp and "am_merge_ready(" in hpp


def test_cli_help_shows_live():
    import build as am_build
    cli = am_build.build_cli()
    out = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--live" in out.stdout and "--rate R" in out.stdout
    r = subprocess.run([cli, "--live", "--snippet", "a.wav"], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert r.returncode == 2 and "--rate" in r.stderr
