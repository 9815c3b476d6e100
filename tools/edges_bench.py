#!/usr/bin/env python3
"""Edge matching (am_match_edges_device) in milliseconds per haystack: a 10 s needle at 44.1 kHz against a resident hour
whose start lies 40 % into the needle and whose end lies 30 % into another occurrence (the call reads the two spans of
S - 1 samples only, so the hour's length does not enter), beside one am_match_device of the same hour at the CLI's
default parameters, for scale.  Both are timed by the host clock around calls that end in a device synchronise (median
and min of --reps); a profiled call gives the family's own kernels (class "edges": span passes, energy scans, the
normalising and the exact launches -- the engine's transforms and the record rule are counted in their own classes).

Also the largest observed coarse-score error ratio: |coarse(u) - ref(u)| over the bound 2 eps / sqrt(E_n(u) E_x(u)) + 2^-22
that tests/test_gpu_edges.py holds every candidate to (eps: the measured error of am_correlate over the span), over the
shapes of that test's largest needle and a few around AM_EDGE_TILE.  Prints one JSON line.

  python tools/edges_bench.py [--reps R] [--warmup W] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import audiomatch_amd as am  # noqa: E402
import edges_ref as er  # noqa: E402

SR = 44100
S, H = 10 * SR, 3600 * SR


def clock(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def error_ratio(s, length, seed):
    needle, pcm = er.case_signals(s, length, seed)
    x = er.downmix(pcm)
    h = am.HipConvolve(needle)
    worst = 0.0
    for edge in (er.HEAD, er.TAIL):
        t = er.edge_terms(needle, x, edge)
        span, _ = er.sanitise(np.asarray(er.span_of(x, s, edge), dtype=np.float32))
        a = h.correlate_with_sample(span.astype(np.float32), am.Mode.Full, False)
        eps = float(np.max(np.abs(a.astype(np.float64) - t["full"])))
        got = h.edge_scores(x, edge, am.edge_params(1, 0, 0.0)).astype(np.float64)
        ncc, _ = er.scores_of(t)
        den = np.sqrt(t["en"] * t["ex"])
        ok = den > 0
        worst = max(worst, float(np.max(np.abs(got[ok] - ncc[ok]) / (2.0 * eps / den[ok] + 2.0 ** -22))))
    h.close()
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    needle = am.synth_uniform_device(0, S, seed=7, stream=0)
    hay = am.synth_uniform_device(0, H, seed=7, stream=1)
    k_head, k_tail = 4 * S // 10, 3 * S // 10
    am.axpy_device(0, hay, 0, needle.ptr + 4 * k_head, S - k_head, 1.0)
    am.axpy_device(0, hay, H - k_tail, needle.ptr, k_tail, 1.0)
    am.axpy_device(0, hay, 1000 * SR, needle.ptr, S, 1.0)
    algo = am.HipConvolve.from_device(0, needle.ptr, S)
    ep = am.edge_params(SR // 2, 0, 0.05)
    recs = algo.match_edges_device(hay.ptr, H, ep)
    found = bool(int(recs[0]["start"]) == -k_head and int(recs[1]["start"]) == H - k_tail and int(recs[0]["flags"]) == 0 and int(recs[1]["flags"]) == 0)
    med, mn = clock(lambda: algo.match_edges_device(hay.ptr, H, ep), a.reps, a.warmup)
    with am.Profile(0) as p:
        algo.match_edges_device(hay.ptr, H, ep)
        kern_ms, launches = p.query("edges")
    prm = am.Config(overlap_length_s=10.0).params(SR, am.Scale.LIB)
    m_med, m_mn = clock(lambda: algo.match_device(hay.ptr, H, prm), a.reps, a.warmup)
    T = am.AM_EDGE_TILE
    ratios = {"%d/%d" % (s, n): round(error_ratio(s, n, 100 * s + n), 3)
              for s, n in ((T - 1, 3 * T), (T + 1, 2 * T), (2 * T + 1, 2 * T), (40000, 39999), (40000, 120000))}
    res = dict(shape=dict(sr=SR, needle_seconds=S // SR, haystack_seconds=H // SR, min_overlap=int(ep.min_overlap)),
               match_edges_ms=round(med, 3), match_edges_min_ms=round(mn, 3), edges_kernels_ms=round(kern_ms, 3), edges_kernel_launches=int(launches),
               match_device_default_ms=round(m_med, 3), match_device_default_min_ms=round(m_mn, 3), planted_found=found,
               head=dict(ncc=round(float(recs[0]["ncc"]), 4), second=round(float(recs[0]["ncc_second"]), 4), share=round(float(recs[0]["share"]), 4)),
               tail=dict(ncc=round(float(recs[1]["ncc"]), 4), second=round(float(recs[1]["ncc_second"]), 4), share=round(float(recs[1]["share"]), 4)),
               coarse_error_over_bound=ratios, coarse_error_over_bound_max=max(ratios.values()))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
