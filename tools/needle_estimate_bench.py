#!/usr/bin/env python3
"""Needle estimation (am_needle_estimate_rows, am_needle_estimate_device) at the sizes users run.

  copy      a device-to-device hipMemcpyAsync of 16 x 4 410 000 f32 (host clock around the call): what this box gives a
            plain copy; run tools/membench beside it for the copy kernels of profiles/r01/membench_ceilings.txt
  rows      am_needle_estimate_rows: n rows of `length` f32 from host memory (the call's time holds their upload)
  device    am_needle_estimate_device: n hits at odd starts in one resident haystack, f32 mono and i16 stereo
            (--aligned: once more with every start a multiple of 64 bytes, cases "device_*_aligned")

for mean, median and trimmed (100 permille) at n = 8, 16, 32, 64 rows and length = 441 000 (10 s of 44.1 kHz) and
4 410 000.  Kernel times are device events around the launch (am_profile_*, the "other" class; median and min of --reps
calls after --warmup); call times are a host clock around the C entry point.  Bytes are what the algorithm needs:
n * length * 4 in, 4 * length out for the estimate alone ("est"); with the deviation and the count ("full", device f32
only) the rows are read a second time and three arrays are written.  Prints one JSON line.

  python tools/needle_estimate_bench.py [--reps R] [--warmup W] [--aligned] [--skip-rows]"""
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
NS = (8, 16, 32, 64)
LENGTHS = (441000, 4410000)
METHODS = (("mean", 0, 0), ("median", 1, 0), ("trimmed", 2, 100))


def median_min(v):
    v = sorted(v)
    return v[len(v) // 2], v[0]


def timed(call, reps, warmup):
    """(kernel ms median, min, call ms median, min) of `call`"""
    for _ in range(warmup):
        call()
    ks, ts = [], []
    for _ in range(reps):
        with am.Profile(DEV) as prof:
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        ks.append(prof.query("other")[0])
    return (*median_min(ks), *median_min(ts))


def row(form, method, n, length, outputs, times, copy_bps):
    k_med, k_min, c_med, c_min = times
    passes = 2 if outputs == "full" else 1
    nbytes = 4.0 * n * length * passes + 4.0 * length * (3 if outputs == "full" else 1)
    bps = nbytes / (k_med * 1e-3)
    return {"case": form, "method": method, "n": n, "length": length, "outputs": outputs, "kernel_ms_median": k_med, "kernel_ms_min": k_min,
            "call_ms_median": c_med, "call_ms_min": c_min, "bytes": nbytes, "bytes_per_s_kernel": bps,
            "fraction_of_8TBps_kernel": bps / PEAK_BW, "fraction_of_copy": bps / copy_bps}


def copy_row(n, reps, warmup):
    lib = am.lib()
    din = am.synth_uniform_device(DEV, n, 7, 2, amp=0.5)
    dout = am.DeviceBuffer(DEV, 4 * n)
    got = C.c_size_t(0)

    def call():
        rc = lib.am_resample_device(DEV, din.ptr, n, 0, 44100, 44100, dout.ptr, n, C.byref(got))
        assert rc == 0 and got.value == n, (rc, got.value)

    for _ in range(warmup):
        call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    med, mn = median_min(ts)
    din.free()
    dout.free()
    return {"case": "copy", "n": n, "bytes": 8.0 * n, "copy_ms_median": med, "copy_ms_min": mn, "bytes_per_s": 8.0 * n / (med * 1e-3),
            "fraction_of_8TBps": 8.0 * n / (med * 1e-3) / PEAK_BW}


def device_rows(reps, warmup, copy_bps, aligned=False):
    lib = am.lib()
    out = []
    total = max(NS) * max(LENGTHS) + 4096
    for fmt, name in ((am.Fmt.F32_MONO, "device_f32"), (am.Fmt.S16_STEREO, "device_s16")):
        buf = am.synth_uniform_device(DEV, total, 11, 3, amp=0.5) if fmt == am.Fmt.F32_MONO else am.synth_pcm16_stereo_device(DEV, total, 11, 3)
        ptrs = (C.c_void_p * 1)(buf.ptr)
        lens = (C.c_size_t * 1)(total)
        for length in LENGTHS:
            est = np.empty(length, np.float32)
            dev = np.empty(length, np.float32)
            cnt = np.empty(length, np.uint32)
            for n in NS:
                hits = (am.AmEstHit * n)(*[am.AmEstHit(i * length + (0 if aligned else 2 * i + 1), 0, 1.0 + 0.01 * i) for i in range(n)])
                for mname, method, trim in METHODS:
                    ep = am.AmEstimateParams(method, trim, 0, length)
                    for outputs in (("est", "full") if fmt == am.Fmt.F32_MONO else ("est",)):
                        dp, cp = (dev.ctypes.data, cnt.ctypes.data) if outputs == "full" else (None, None)

                        def call():
                            rc = lib.am_needle_estimate_device(DEV, ptrs, lens, 1, int(fmt), hits, n, C.byref(ep), est.ctypes.data, dp, cp)
                            assert rc == 0, (rc, lib.am_last_error_string())

                        out.append(row(name + ("_aligned" if aligned else ""), mname, n, length, outputs, timed(call, reps, warmup), copy_bps))
        buf.free()
    return out


def host_rows(reps, warmup, copy_bps):
    lib = am.lib()
    out = []
    rng = np.random.default_rng(4)
    for length in LENGTHS:
        data = rng.random((max(NS), length), dtype=np.float32) - np.float32(0.5)
        est = np.empty(length, np.float32)
        for n in NS:
            for mname, method, trim in METHODS:
                ep = am.AmEstimateParams(method, trim, 0, length)

                def call():
                    rc = lib.am_needle_estimate_rows(DEV, data.ctypes.data, n, C.byref(ep), est.ctypes.data, None, None)
                    assert rc == 0, (rc, lib.am_last_error_string())

                out.append(row("rows", mname, n, length, "est", timed(call, reps, warmup), copy_bps))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--aligned", action="store_true", help="the device form again with every hit's start a multiple of 64 bytes")
    ap.add_argument("--skip-rows", action="store_true", help="leave out the rows form (its calls upload up to 1.1 GB each)")
    a = ap.parse_args()
    if am.device_count() < 1:
        raise SystemExit("needle_estimate_bench needs a HIP device")
    rows = [copy_row(16 * max(LENGTHS), a.reps, a.warmup)]
    copy_bps = rows[0]["bytes_per_s"]
    rows += device_rows(a.reps, a.warmup, copy_bps)
    if a.aligned:
        rows += device_rows(a.reps, a.warmup, copy_bps, aligned=True)
    if not a.skip_rows:
        rows += host_rows(a.reps, a.warmup, copy_bps)
    print(json.dumps({"bench": "needle_estimate", "reps": a.reps, "warmup": a.warmup, "rows": rows}))


if __name__ == "__main__":
    main()
