#!/usr/bin/env python3
"""Spectral whitening (am_fir_device, am_lag_products_device, am_needle_create_filtered) at the sizes users run.

  copy      one hour of 44.1 kHz f32 copied device to device (hipMemcpyAsync, host clock around the call): the 4 + 4
            bytes per sample the FIR kernel moves, at the rate this box gives a plain copy; run tools/membench beside it
            for the copy kernels of profiles/r01/membench_ceilings.txt
  fir       am_fir_device on that hour for 2, 9, 33 and 65 taps
  lag       am_lag_products_device on that hour for orders 8, 32 and 64
  match     am_match_device per hour of audio on the two non-white signals of bench.py --full (the speech-like AR(1)
            signal and the tone-and-drift signal), raw against whitened (order 8, noise_db 60), with the time of the
            filter's own steps (lag products, the haystack's FIR pass, the filtered needle) listed separately

Kernel times are device events around the launches (am_profile_*, the "other" class; median and min of --reps calls
after --warmup); call times are a host clock around the C entry point, which ends in a device synchronise.  Bytes are
what the algorithm needs: 4 per sample in, 4 per sample out (fir), 4 per sample in (lag).  Prints one JSON line.

  python tools/whiten_bench.py [--reps R] [--warmup W]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd"))
import audiomatch_amd as am  # noqa: E402

PEAK_BW = 8.0e12
DEV = 0
SR = 44100
HOUR = 3600 * SR


def median_min(v):
    v = sorted(v)
    return v[len(v) // 2], v[0]


def host_ms(call, reps, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return median_min(ts)


def timed_kernel(call, reps, warmup):
    """(kernel ms median, min, call ms median, min) of `call`"""
    for _ in range(warmup):
        call()
    ks, ts = [], []
    for _ in range(reps):
        with am.Profile(DEV) as prof:
            call()
        ks.append(prof.query("other")[0])
    for _ in range(reps):   # (host-clock calls without the profiling events)
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return (*median_min(ks), *median_min(ts))


def rate_row(case, nbytes, times, copy_ms, **extra):
    k_med, k_min, c_med, c_min = times
    row = {"case": case, **extra, "kernel_ms_median": k_med, "kernel_ms_min": k_min, "call_ms_median": c_med, "call_ms_min": c_min,
           "bytes": nbytes, "bytes_per_s_kernel": nbytes / (k_med * 1e-3), "fraction_of_8TBps_kernel": nbytes / (k_med * 1e-3) / PEAK_BW}
    if copy_ms:
        row["call_over_copy_call"] = c_med / copy_ms
    return row


def copy_row(n, reps, warmup):
    """a device-to-device hipMemcpyAsync of n f32 samples (am_resample_device at equal rates is exactly that), host clock
    around the call: 4 bytes in and 4 out per sample, what the runtime's own copy reaches on this box"""
    lib = am.lib()
    din = am.synth_uniform_device(DEV, n, 7, 2, amp=0.5)
    dout = am.DeviceBuffer(DEV, 4 * n)
    got = C.c_size_t(0)

    def call():
        rc = lib.am_resample_device(DEV, din.ptr, n, 0, SR, SR, dout.ptr, n, C.byref(got))
        assert rc == 0 and got.value == n, (rc, got.value)

    med, mn = host_ms(call, reps, warmup)
    din.free()
    dout.free()
    return {"case": "copy", "n": n, "bytes": 8.0 * n, "copy_ms_median": med, "copy_ms_min": mn, "bytes_per_s": 8.0 * n / (med * 1e-3),
            "fraction_of_8TBps": 8.0 * n / (med * 1e-3) / PEAK_BW}


def kernel_rows(reps, warmup, copy_ms):
    lib = am.lib()
    rows = []
    n = HOUR
    din = am.synth_uniform_device(DEV, n, 7, 2, amp=0.5)
    dout = am.DeviceBuffer(DEV, 4 * n)
    got = C.c_size_t(0)
    rng = np.random.default_rng(3)
    for n_taps in (2, 9, 33, 65):
        taps = np.ascontiguousarray(rng.uniform(-0.5, 0.5, n_taps), dtype=np.float32)
        tp = taps.ctypes.data_as(C.POINTER(C.c_float))

        def call():
            rc = lib.am_fir_device(DEV, din.ptr, n, 0, tp, n_taps, 0, dout.ptr, n, C.byref(got))
            assert rc == 0 and got.value == n, (rc, got.value)

        rows.append(rate_row("fir", 8.0 * n, timed_kernel(call, reps, warmup), copy_ms, n=n, n_taps=n_taps))
        rows[-1]["fma_per_s_kernel"] = float(n) * n_taps / (rows[-1]["kernel_ms_median"] * 1e-3)
    dout.free()
    r = (C.c_double * 65)()
    for order in (8, 32, 64):
        def call():
            rc = lib.am_lag_products_device(DEV, din.ptr, n, 0, order, r)
            assert rc == 0, rc

        rows.append(rate_row("lag", 4.0 * n, timed_kernel(call, reps, warmup), None, n=n, order=order))
        rows[-1]["f64_fma_per_s_kernel"] = float(n) * (order // 8 + 1) * 8 / (rows[-1]["kernel_ms_median"] * 1e-3)
    din.free()
    return rows


def match_rows(reps, warmup, order=8):
    import bench   # the signals of bench.py --full's non-white leg
    s, h = bench.NEEDLE_S * bench.SR, bench.HAY_S * bench.SR
    params = am.Config(chunk_size_s=bench.CHUNK_S, overlap_length_s=bench.NEEDLE_S, distance_s=480.0, prominence=0.13).params(bench.SR, am.Scale.LIB)
    rows = []
    for name, maker in (("non_white_speechlike", bench.make_speechlike), ("non_white_signal", bench.make_tonal)):
        nbuf, algo, hbuf, plants, note = maker(am, DEV, s, h)
        needle = nbuf.to_numpy(np.float32, s)
        row = {"case": "match", "signal": name, "note": note, "order": order, "hay_samples": h, "needle_samples": s}
        raw = algo.match_device(hbuf.ptr, h, params)
        row["raw_offsets_ok"] = [p.start for p in raw] == plants
        row["raw_n_peaks"] = len(raw)
        row["raw_match_ms_median"], row["raw_match_ms_min"] = host_ms(lambda: algo.match_device(hbuf.ptr, h, params), reps, warmup)
        # the filter's own steps
        row["lag_products_ms_median"], _ = host_ms(lambda: am.lag_products_device(DEV, hbuf.ptr, h, order), reps, warmup)
        taps = am.whiten_taps(am.lag_products_device(DEV, hbuf.ptr, h, order), 60.0)
        row["taps"] = [float(t) for t in taps]
        wbuf = am.DeviceBuffer(DEV, 4 * h)
        row["fir_haystack_ms_median"], _ = host_ms(lambda: am.fir_device(DEV, hbuf.ptr, h, taps, wbuf.ptr, h), reps, warmup)
        row["filtered_needle_ms_median"], _ = host_ms(lambda: am.HipConvolve.filtered(needle, taps).close(), reps, warmup)
        row["plain_needle_ms_median"], _ = host_ms(lambda: am.HipConvolve(needle).close(), reps, warmup)
        walgo = am.HipConvolve.filtered(needle, taps)
        white = walgo.match_device(wbuf.ptr, h, params)
        row["whitened_offsets_ok"] = [p.start for p in white] == plants
        row["whitened_n_peaks"] = len(white)
        row["whitened_match_ms_median"], row["whitened_match_ms_min"] = host_ms(lambda: walgo.match_device(wbuf.ptr, h, params), reps, warmup)
        rows.append(row)
        for b in (nbuf, hbuf, wbuf):
            b.free()
        algo.close()
        walgo.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if am.device_count() < 1:
        raise SystemExit("whiten_bench needs a HIP device")
    rows = [copy_row(HOUR, a.reps, a.warmup)]
    rows += kernel_rows(a.reps, a.warmup, rows[0]["copy_ms_median"])
    rows += match_rows(max(3, a.reps // 2), a.warmup)
    print(json.dumps({"bench": "whiten", "reps": a.reps, "warmup": a.warmup, "rows": rows}))


if __name__ == "__main__":
    main()
