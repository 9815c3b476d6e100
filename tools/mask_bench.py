#!/usr/bin/env python3
"""What the masked normalising pass costs against the ordinary score_norm pass, on the headline shape: a 10 s needle and
one 1 h 44.1 kHz f32 haystack through am_match_batch_device.

The pass is the two kernels normalise_scores launches (csrc/am_norm.hip): the block energies, once per signal, and
norm_scores / masked_norm_scores.  Both are of the profile class "other"; what is timed is that class's device-event time
per call with every other class masked out (option "profile_mask").  The call launches a few small kernels of the class
anyway: the variant "lib" (score_norm off) reports them (3 launches, about 0.05 ms on an MI355X, 2 % of the ordinary
pass); the ratios do NOT subtract them.  Variants: "ordinary", the ordinary handle of THIS build under score_norm -- the
baseline of every ratio; its kernel is the one before masked matching with the per-span assembly moved into a function,
not a build of an earlier commit --, and masked handles with 1, 4 and 16 kept spans of equal length (gaps of 1000 samples;
one kept span = one trailing gap).  The variants alternate inside every repetition; median, minimum, maximum and the
quartile spread are reported per variant, and each masked median over the ordinary one.  The planted offset is checked
in every timed call.  Prints one JSON line.

  python tools/mask_bench.py [--reps R] [--warmup W]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd"))
import audiomatch_amd as am  # noqa: E402

SR = 44100
S = 10 * SR
H = 3600 * SR
GAP = 1000
KN_OTHER = 5   # the class's bit in "profile_mask" (csrc/am_internal.h)
PLANT = 1800 * SR + 1234


def equal_spans(n_kept):
    """Gaps of GAP samples that leave n_kept spans of (almost) equal length; one span: a trailing gap."""
    if n_kept == 1:
        return [(S - GAP, S)]
    step = (S + GAP) // n_kept
    return [(k * step - GAP, k * step) for k in range(1, n_kept)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = 0
    needle = am.synth_uniform_device(dev, S, 1, 0)
    hay = am.synth_uniform_device(dev, H, 1, 1)
    am.axpy_device(dev, hay, PLANT, needle.ptr, S, 1.0)
    p = am.Config(chunk_size_s=60, overlap_length_s=10, distance_s=480.0, prominence=0.13).params(SR, am.Scale.LIB)
    variants = [("lib", None, 0), ("ordinary", None, 1)] + [("kept_%d" % k, equal_spans(k), 1) for k in (1, 4, 16)]
    algos = {}
    for name, gaps, norm in variants:
        h = am.HipConvolve.from_device(dev, needle.ptr, S, gaps=gaps)
        h.set_option("score_norm", norm)
        assert len(h.mask()) == (0 if gaps is None else len(gaps))
        algos[name] = h
    keep = am.get_option("profile_mask")
    am.set_option("profile_mask", 1 << KN_OTHER)
    times = {name: [] for name, _, _ in variants}
    launches = {}
    try:
        for rep in range(a.warmup + a.reps):
            for name, _, _ in variants:
                with am.Profile(dev) as prof:
                    res = algos[name].match_batch_device([hay.ptr], [H], p)
                    ms, n = prof.query("other")
                assert [q.start for q in res[0]] == [PLANT], (name, res[0])
                if rep >= a.warmup:
                    times[name].append(ms)
                    launches[name] = n
    finally:
        am.set_option("profile_mask", keep)
    out = {"shape": f"needle {S} samples, 1 x {H} samples (1 h at 44.1 kHz), am_match_batch_device", "reps": a.reps, "warmup": a.warmup,
           "timer": "device events around the launches of profile class 'other' (block_energy + the normalising kernel)"}
    for name, gaps, _ in variants:
        ts = sorted(times[name])
        q = len(ts) // 4
        out[name] = {"kept_spans": 1 if gaps is None else len(gaps) + (0 if name == "kept_1" else 1), "launches_per_call": launches[name],
                     "ms_median": ts[len(ts) // 2], "ms_min": ts[0], "ms_max": ts[-1], "ms_q1": ts[q], "ms_q3": ts[-1 - q]}
    base = out["ordinary"]["ms_median"]
    for k in (1, 4, 16):
        out["kept_%d_over_ordinary" % k] = out["kept_%d" % k]["ms_median"] / base if base > 0 else None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
