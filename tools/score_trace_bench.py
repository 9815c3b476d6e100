#!/usr/bin/env python3
"""Score traces (am_match_trace_device) on the headline shape: 1 h at 44.1 kHz, a 10 s needle, 8 plants, raw (LIB) and
NCC scores, bins of D in {4410, 44100, 2646000} scores (0.1 s, 1 s, 1 min).

Per row: the call's time (host clock around the C entry point, which ends in a device synchronise; median, min and max
of --reps), and from profiled calls (am_profile_*, device events per kernel class) the trace kernels alone (class
"trace": median, min and max of --reps profiled calls) and that time as bytes per second over the 4 n bytes of scores
they read.  In the same run, per score kind: am_match_best_device with k = 1 and min_distance = S -- its call time and
its scan over the same array (class "tile_stats": median, min and max), the yardstick for one read of the scores --
and the composition a user had before: am_correlate_device, the scores copied to the host, numpy's max / min / sums
per bin of 44100.  The trace's global maximum is checked against am_match_best's hit.  Prints one JSON line.

  python tools/score_trace_bench.py [--reps R] [--warmup W] [--out FILE] [--no-composition]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd"))
import audiomatch_amd as am  # noqa: E402

SR = 44100
S = 10 * SR
H = 3600 * SR
BINS = (4410, 44100, 2646000)


def clock(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def profiled(fn, kernel, reps):
    ts = []
    for _ in range(reps):
        with am.Profile(0) as p:
            fn()
            ts.append(p.query(kernel)[0])
    return ts


def spread(ts, name):
    return {name + "_ms": round(float(np.median(ts)), 4), name + "_min_ms": round(float(np.min(ts)), 4),
            name + "_max_ms": round(float(np.max(ts)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-composition", action="store_true", help="skip the composition (seconds per row)")
    a = ap.parse_args()
    L = am.lib()
    needle = am.synth_uniform_device(0, S, seed=7, stream=0)
    hay = am.synth_uniform_device(0, H, seed=7, stream=1)
    plants = [int(t) for t in np.linspace(3 * S, H - 3 * S, 8).astype(np.int64) + np.arange(8) * 977]
    for t in plants:
        am.axpy_device(0, hay, t, needle.ptr, S, 1.0)
    n_scores = H - S + 1
    scores = am.DeviceBuffer(0, 4 * n_scores)
    host_scores = np.empty(n_scores, dtype=np.float32)
    rows, bests = [], []
    for norm in (False, True):
        algo = am.HipConvolve.from_device(0, needle.ptr, S)
        algo.set_option(am.OPT_SCORE_NORM, int(norm))
        # the yardstick: am_match_best with k = 1, and its scan of the same score array
        bp = am.best_params(1, S)
        hit = (am.AmPeak * 1)()
        got = C.c_size_t(0)

        def best():
            rc = L.am_match_best_device(algo._h, hay.ptr, H, 0, C.byref(bp), hit, C.byref(got))
            assert rc == 0, L.am_last_error_string()
        best_row = dict(score_norm=int(norm), **spread(clock(best, a.reps, a.warmup), "best_call"),
                        **spread(profiled(best, "tile_stats", a.reps), "best_scan"))

        def compose():
            m = C.c_size_t(0)
            rc = L.am_correlate_device(algo._h, hay.ptr, H, int(am.Mode.Valid), int(am.Scale.LIB), scores.ptr, n_scores, C.byref(m))
            assert rc == 0
            assert L.am_memcpy_d2h(0, host_scores.ctypes.data, scores.ptr, 4 * n_scores) == 0
            nb = n_scores // 44100
            v = host_scores[:nb * 44100].reshape(nb, 44100)
            d = v.astype(np.float64)
            return v.max(axis=1), v.min(axis=1), d.sum(axis=1), (d * d).sum(axis=1)
        if not a.no_composition:
            best_row.update(spread(clock(compose, max(1, a.reps // 3), 1), "composition"))
        bests.append(best_row)
        print(json.dumps(best_row), file=sys.stderr)
        for D in BINS:
            tp = am.trace_params(D)
            nb = am.trace_len(n_scores, D)
            out = np.zeros(nb, dtype=am.TRACE_BIN_DTYPE)

            def trace():
                rc = L.am_match_trace_device(algo._h, hay.ptr, H, 0, C.byref(tp), out.ctypes.data, nb, C.byref(got))
                assert rc == 0, L.am_last_error_string()
            call = clock(trace, a.reps, a.warmup)
            kern = profiled(trace, "trace", a.reps)
            st = am.trace_summary(out, D)
            row = dict(score_norm=int(norm), bin=D, n_bins=nb, **spread(call, "trace_call"), **spread(kern, "trace_kernels"),
                       trace_kernels_gb_per_s=round(4 * n_scores / (float(np.median(kern)) * 1e-3) / 1e9, 1),
                       argmax_is_best_hit=bool(st.argmax == int(hit[0].start)), peak_z=round(st.peak_z, 2))
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
        algo.close()
    res = dict(shape=dict(sr=SR, needle_s=10, haystack_s=3600), rows=rows, match_best=bests, score_bytes_gb=round(4 * n_scores / 1e9, 3))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
