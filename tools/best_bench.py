#!/usr/bin/env python3
"""The k best matches (am_match_best_device) on the headline shape: 1 h at 44.1 kHz, a 10 s needle, 8 plants,
min_distance = S, k in {1, 10, 100}, raw (LIB) and NCC scores.

Per row: the call's time (host clock around the C entry point, which ends in a device synchronise; median and min of
--reps), and from a profiled call (am_profile_*, device events per kernel class) the correlation kernels (K1 / K2 / K3
and, under NCC, the normalisation: "other") against the selection kernels (the scan: class "tile_stats"; compaction
and prominence walks: class "peaks").  For comparison, the same question answered by composition --
am_correlate_device, the scores copied to the host, whole-array am_find_peaks with min_prominence 0 (one chunk, every
local maximum), the first k kept -- and am_match_device at the CLI's default parameters (60 s chunks, prominence 0.13,
min_distance 8 min), for scale.  The plants are checked (k >= 8: all eight found).  Prints one JSON line.

  python tools/best_bench.py [--reps R] [--warmup W] [--out FILE] [--no-composition]"""
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
CLASSES = ("k1_cols_fwd", "k2_rows", "k3_cols_inv", "tile_stats", "peaks", "other")


def clock(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def profiled(fn):
    with am.Profile(0) as p:
        fn()
        return {k: p.query(k)[0] for k in CLASSES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-composition", action="store_true", help="skip the composition (seconds per row): profiler runs")
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
    rows = []
    for norm in (False, True):
        algo = am.HipConvolve.from_device(0, needle.ptr, S)
        algo.set_option(am.OPT_SCORE_NORM, int(norm))
        for k in (1, 10, 100):
            bp = am.best_params(k, S)
            out = (am.AmPeak * k)()
            n = C.c_size_t(0)

            def best():
                rc = L.am_match_best_device(algo._h, hay.ptr, H, 0, C.byref(bp), out, C.byref(n))
                assert rc == 0, am.lib().am_last_error_string()
            med, mn = clock(best, a.reps, a.warmup)
            got = sorted(int(q.start) for q in out[:n.value])
            ok = set(plants) <= set(got) if k >= 8 else set(got) <= set(plants)
            prof = profiled(best)
            corr = sum(prof[c] for c in ("k1_cols_fwd", "k2_rows", "k3_cols_inv", "other"))
            sel = prof["tile_stats"] + prof["peaks"]

            # the composition: all scores, then the whole-array pick
            cap = 1 << 22
            buf = (am.AmPeak * cap)()

            def compose():
                got_n = C.c_size_t(0)
                rc = L.am_correlate_device(algo._h, hay.ptr, H, int(am.Mode.Valid), int(am.Scale.LIB), scores.ptr, n_scores, C.byref(got_n))
                assert rc == 0
                assert L.am_memcpy_d2h(0, host_scores.ctypes.data, scores.ptr, 4 * n_scores) == 0
                rc = L.am_find_peaks(0, host_scores.ctypes.data, n_scores, 0.0, S, buf, cap, C.byref(got_n))
                assert rc in (0, 2)
            cmed = float("nan") if a.no_composition else clock(compose, max(1, a.reps // 2), 1)[0]
            rows.append(dict(score_norm=int(norm), k=k, best_ms=round(med, 3), best_min_ms=round(mn, 3),
                             correlation_kernels_ms=round(corr, 3), selection_kernels_ms=round(sel, 3),
                             scan_ms=round(prof["tile_stats"], 3), compact_and_walks_ms=round(prof["peaks"], 3),
                             composition_ms=round(cmed, 3), plants_ok=bool(ok)))
            print(json.dumps(rows[-1]), file=sys.stderr)
        algo.close()
    # am_match_device at the CLI's defaults, for scale
    algo = am.HipConvolve.from_device(0, needle.ptr, S)
    p = am.Config(overlap_length_s=10.0).params(SR, am.Scale.LIB)
    med, mn = clock(lambda: algo.match_device(hay.ptr, H, p), a.reps, a.warmup)
    algo.close()
    res = dict(shape=dict(sr=SR, needle_s=10, haystack_s=3600, min_distance=S), rows=rows,
               match_device_default_ms=round(med, 3), match_device_default_min_ms=round(mn, 3),
               score_bytes_gb=round(4 * n_scores / 1e9, 3))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
