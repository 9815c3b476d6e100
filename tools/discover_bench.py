#!/usr/bin/env python3
"""Needle discovery (am_discover_device) in milliseconds per probe per hour of B: B is 1 h at 44.1 kHz, A is --a-seconds
of audio whose middle third is planted in B, probes of --probe-seconds every half probe.

On the same build and inputs, the composition a caller had before -- per probe am_needle_create_device,
am_needle_set_option("score_norm", 1), am_match_trace_device with one bin, am_needle_destroy -- which is the baseline:
it down-mixes nothing here (f32 input) but scans B for non-finite samples, copies the probe, sums its energy and
synchronises once per probe.  Both are timed by the host clock around calls that end in a device synchronise (median,
min and max of --reps); a profiled call gives the discovery kernels alone (class "discover": the energy launch and the
two reduction launches per probe).  The best places of both are compared.  Prints one JSON line.

  python tools/discover_bench.py [--reps R] [--warmup W] [--probe-seconds S] [--a-seconds T] [--out FILE]"""
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
LEN_B = 3600 * SR


def clock(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def spread(ts, name, per):
    return {name + "_ms": round(float(np.median(ts)) / per, 4), name + "_min_ms": round(float(np.min(ts)) / per, 4),
            name + "_max_ms": round(float(np.max(ts)) / per, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--probe-seconds", type=float, default=10.0)
    ap.add_argument("--a-seconds", type=float, default=120.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = am.lib()
    probe_len, len_a = int(a.probe_seconds * SR), int(a.a_seconds * SR)
    hop = probe_len // 2
    da = am.synth_uniform_device(0, len_a, seed=11, stream=0)
    db = am.synth_uniform_device(0, LEN_B, seed=11, stream=1)
    third = len_a // 3
    at = 1000 * SR + 321
    am.axpy_device(0, db, at, da.ptr + 4 * third, third, 2.0)          # A's middle third, twice as loud as B's noise
    dp = am.discover_params(probe_len, hop)
    P = am.discover_len(len_a, dp)
    out = np.zeros(P, dtype=am.PROBE_HIT_DTYPE)
    got = C.c_size_t(0)

    def discover():
        rc = L.am_discover_device(0, da.ptr, len_a, db.ptr, LEN_B, 0, C.byref(dp), out.ctypes.data, P, C.byref(got))
        assert rc == 0, L.am_last_error_string()

    n_scores = LEN_B - probe_len + 1
    tp = am.trace_params(1 << 30)
    assert n_scores <= 1 << 30
    rec = np.zeros(1, dtype=am.TRACE_BIN_DTYPE)
    places = np.zeros(P, dtype=np.int64)

    def composition():
        for i in range(P):
            h = C.c_void_p()
            assert L.am_needle_create_device(0, da.ptr + 4 * i * hop, probe_len, C.byref(h)) == 0
            assert L.am_needle_set_option(h, b"score_norm", 1) == 0
            rc = L.am_match_trace_device(h, db.ptr, LEN_B, 0, C.byref(tp), rec.ctypes.data, 1, C.byref(got))
            assert rc == 0, L.am_last_error_string()
            places[i] = rec[0]["argmax"]
            L.am_needle_destroy(h)

    t_disc = clock(discover, a.reps, a.warmup)
    t_comp = clock(composition, a.reps, a.warmup)
    with am.Profile(0) as p:
        discover()
        kern_ms, launches = p.query("discover")
    same = bool(np.array_equal(out["best"].astype(np.int64), places))
    inside = [i for i in range(P) if third <= i * hop and i * hop + probe_len <= 2 * third]
    found = bool(all(int(out[i]["best"]) - i * hop == at - third for i in inside))
    hours = LEN_B / SR / 3600.0
    res = dict(shape=dict(sr=SR, b_seconds=LEN_B // SR, a_seconds=a.a_seconds, probe_seconds=a.probe_seconds, hop_seconds=hop / SR, probes=P),
               unit="ms per probe per hour of B",
               **spread(t_disc, "discover", P * hours), **spread(t_comp, "composition", P * hours),
               discover_over_composition=round(float(np.median(t_disc)) / float(np.median(t_comp)), 3),
               discover_kernels_ms=round(kern_ms / (P * hours), 4), discover_kernel_launches=int(launches),
               same_best_places=same, planted_probes=len(inside), planted_found=found)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
