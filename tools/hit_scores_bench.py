#!/usr/bin/env python3
"""Per-hit scoring (am_hit_scores*) on the headline needle: a 10 s needle at 44.1 kHz.

  batch    am_hit_scores_batch_device on 1, 64, 1000 and 10000 hits spread at random over NH resident 1 h f32
           haystacks (one needle, the layout of am_match_batch_device's result)
  host     am_hit_scores on 8 hits in a 1 h and in an 8 h host buffer (only the hits' spans travel)

Per row: the call's time (host clock around the C entry point, whose work ends in a device synchronise; its ctypes
arguments are built before the clock starts; median and min of --reps), the same through the Python binding
(py_call_ms: adds building the AmPeak array and reading the results into HitScore records), the kernels' time (device events around the launch sequence, option "profile_mask" untouched: am_profile_*, the
"other" class), the design bytes 4 (S + 2) per hit and those bytes over the kernel time against 8 TB/s.  Every timed
call's planted hits are checked (ncc > 0.5).  Prints one JSON line.

  python tools/hit_scores_bench.py [--reps R] [--warmup W] [--only batch|host]"""
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
NH = 2
PEAK_BW = 8.0e12


def timed(fn, reps, warmup, dev):
    for _ in range(warmup):
        fn()
    ts, ks = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        ts.append(time.perf_counter() - t0)
    for _ in range(reps):   # (kernel times in calls of their own: the events are not in the calls timed above)
        with am.Profile(dev) as prof:
            fn()
        ks.append(prof.query("other")[0])
    ts.sort()
    ks.sort()
    return res, ts[len(ts) // 2] * 1e3, ts[0] * 1e3, ks[len(ks) // 2]


def py_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e3


def c_args(peaks):
    k = len(peaks)
    arr = (am.AmPeak * max(1, k))(*[am.AmPeak(q.start, q.end, q.height, q.prominence) for q in peaks])
    return arr, (am.AmHitScore * max(1, k))()


def row(nhits, call_med, call_min, kernel_ms, py_med):
    design = 4.0 * (S + 2) * nhits
    return {"hits": nhits, "call_ms_median": call_med, "call_ms_min": call_min, "py_call_ms_median": py_med,
            "kernel_ms_median": kernel_ms,
            "design_bytes": design, "bytes_per_s_kernel": design / (kernel_ms * 1e-3) if kernel_ms > 0 else None,
            "fraction_of_8TBps_kernel": design / (kernel_ms * 1e-3) / PEAK_BW if kernel_ms > 0 else None,
            "fraction_of_8TBps_call": design / (call_med * 1e-3) / PEAK_BW}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("batch", "host"), default=None)
    a = ap.parse_args()
    dev = 0
    rng = np.random.default_rng(1)
    needle = am.synth_uniform_device(dev, S, 7, 0, amp=0.5)
    algo = am.HipConvolve.from_device(dev, needle.ptr, S)
    out = {"shape": f"needle {S} samples (10 s at 44.1 kHz)", "reps": a.reps}

    if a.only in (None, "batch"):
        hays = [am.synth_uniform_device(dev, H, 7, k + 1, amp=0.1) for k in range(NH)]
        planted = [[600 * SR * m + 30 * SR + 17 * k for m in range(6)] for k in range(NH)]
        for k, b in enumerate(hays):
            for t in planted[k]:
                am.axpy_device(dev, b, t, needle.ptr, S, 1.0)
        rows = []
        for nhits in (1, 64, 1000, 10000):
            per = [[] for _ in range(NH)]
            for i in range(nhits):   # the planted hits first, then random offsets
                k = i % NH
                j = i // NH
                t = planted[k][j] if j < len(planted[k]) else int(rng.integers(0, H - S))
                per[k].append(am.Peak(t, t + 1, 0.0, 0.0))
            pp = [[p] for p in per]
            # the C entry point on prebuilt arguments: haystack k's hits in slots [k cap, k cap + len(per[k]))
            cap = max(len(x) for x in per)
            L = am.lib()
            handles = (C.c_void_p * 1)(algo._h)
            ptrs = (C.c_void_p * NH)(*[b.ptr for b in hays])
            lens = (C.c_size_t * NH)(*([H] * NH))
            counts = (C.c_size_t * NH)(*[len(x) for x in per])
            pk, outs = c_args([q for x in per for q in x + [am.Peak(0, 0, 0.0, 0.0)] * (cap - len(x))])
            _, med, mn, kms = timed(lambda: am._check(L.am_hit_scores_batch_device(handles, 1, ptrs, lens, NH, 0, pk, cap, counts, outs)),
                                    a.reps, a.warmup, dev)
            for k in range(NH):
                for i, q in enumerate(per[k]):
                    if q.start in planted[k]:
                        assert outs[k * cap + i].ncc > 0.5, (q, outs[k * cap + i].ncc)
            pym = py_ms(lambda: am.hit_scores_batch_device([algo], [b.ptr for b in hays], [H] * NH, pp), a.reps)
            rows.append(row(nhits, med, mn, kms, pym))
        out["batch"] = rows
        for b in hays:
            b.free()

    if a.only in (None, "host"):
        d = np.empty(S, dtype=np.float32)
        am._check(am.lib().am_memcpy_d2h(dev, d.ctypes.data, needle.ptr, 4 * S))
        rows = []
        for hours in (1, 8):
            n = hours * H
            hay = np.zeros(n, dtype=np.float32)   # (pages nobody touches are never materialised)
            starts = [int((i + 0.25) * n / 8) + int(rng.integers(0, SR)) for i in range(8)]   # (spans never overlap)
            for t in starts:
                hay[t - 1:t + S + 1] = rng.uniform(-0.1, 0.1, S + 2).astype(np.float32)
                hay[t:t + S] += d
            peaks = [am.Peak(t, t + 1, 0.0, 0.0) for t in starts]
            pk, outs = c_args(peaks)
            L = am.lib()
            _, med, mn, kms = timed(lambda: am._check(L.am_hit_scores(algo._h, hay.ctypes.data, n, 0, pk, len(peaks), outs)),
                                    a.reps, a.warmup, dev)
            assert all(outs[i].ncc > 0.5 for i in range(len(peaks)))
            r = row(len(peaks), med, mn, kms, py_ms(lambda: algo.hit_scores(hay, peaks), a.reps))
            r["hours"] = hours
            rows.append(r)
            del hay
        out["host"] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
