"""Argument refusals of the entry points that share the upload / residency / format / hand-back steps.

cases(gpu) yields (id, thunk) pairs; a thunk runs one refused (or trivially answered) call and returns
[return code, am_last_error_string()].  Every call is made right behind one fixed refusal (am_correlate_len with a null
pointer), so that a call that succeeds reports that refusal's text and not whatever ran before it.

`python tests/entry_refusals.py --record` writes tests/golden/entry_refusals.json from the library in the tree;
tests/test_gpu_entry_refusals.py replays the list against the current build and requires the same code and text.

Needle 257 samples, every buffer 4099 elements.  A host pointer goes only to the _device forms that check residency
(trace match, discover, probe_scores, the three envelope pairs): the other _device forms would read it.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entry_refusals.json")
S, N = 257, 4099
F32, S16 = 0, 1


class _Entry:
    """One entry point with a full set of good arguments (name -> value, in call order)."""

    def __init__(self, gpu, fn, **good):
        self.gpu, self.fn, self.good = gpu, fn, good

    def call(self, **over):
        L = self.gpu.lib()
        args = dict(self.good, **over)
        L.am_correlate_len(0, 0, 0, None)
        rc = getattr(L, self.fn)(*args.values())
        msg = L.am_last_error_string()
        return [int(rc), msg.decode() if msg else ""]

    def needed(self, cap, n_out):
        """What the call reports in *n_out when `cap` is ample."""
        rc, msg = self.call()
        assert rc == 0, (self.fn, rc, msg)
        n = int(self.good[n_out]._obj.value)
        assert n >= 1, (self.fn, n)
        return n

    def cases(self, tag, nulls=(), fmt=None, zeros=(), short=None, misaligned=(), host=(), other=()):
        """nulls / zeros: argument names; fmt: the sample-format argument; short: (cap, n_out) names, or (cap, value);
        misaligned: (name, device pointer) pairs; host: (name, host pointer) pairs; other: (label, overrides) pairs"""
        out = []

        def add(kind, over):
            out.append((f"{tag}:{kind}", lambda: self.call(**over)))
        for a in nulls:
            add("null:" + a, {a: None})
        if fmt:
            add("format7", {fmt: 7})
        for a in zeros:
            add("zero:" + a, {a: 0})
        if short:
            cap, n = short
            add("cap_short", {cap: (self.needed(cap, n) if isinstance(n, str) else n) - 1})
        for a, p in misaligned:
            add("misaligned:" + a, {a: p + 2})
        for a, p in host:
            add("host:" + a, {a: p})
        for label, over in other:
            add(label, over)
        return out


def cases(gpu):
    """The list; builds its needle and buffers on device 0 and keeps them alive in the thunks."""
    E = lambda fn, **good: _Entry(gpu, fn, **good)   # noqa: E731
    rng = np.random.default_rng(7)
    needle = rng.uniform(-1, 1, S).astype(np.float32)
    hay = rng.uniform(-0.05, 0.05, N).astype(np.float32)
    for t in (500, 2500):
        hay[t:t + S] += needle
    pcm = np.clip(np.round(hay * 65535.0), -32768, 32767).astype(np.int16).repeat(2).reshape(N, 2)
    d_hay, d_pcm = gpu.DeviceBuffer.from_numpy(0, hay), gpu.DeviceBuffer.from_numpy(0, pcm)
    d_out = gpu.DeviceBuffer(0, 8 * 4 * N)
    algo = gpu.HipConvolve(needle)
    h = algo._h
    hs = (C.c_void_p * 1)(h.value)
    keep = [needle, hay, pcm, d_hay, d_pcm, d_out, algo, hs]
    sz = lambda: C.byref(C.c_size_t(0))   # noqa: E731
    p = gpu.AmMatchParams(sr=1000, chunk=N, overlap=0, min_prominence=0.13, min_distance=300, overshadow_distance_s=0.3,
                          scale=int(gpu.Scale.LIB))
    pp = C.byref(p)
    peaks = (gpu.AmPeak * 64)()
    f32o = np.zeros(2 * N, np.float32)
    hp, pcmp, hayp, outp = d_hay.ptr, d_pcm.ptr, hay.ctypes.data, f32o.ctypes.data
    c = []

    # correlate, Valid
    nv = N - S + 1
    for tag, fn, w, o in (("correlate", "am_correlate", hayp, outp), ("correlate_device", "am_correlate_device", hp, d_out.ptr)):
        c += E(fn, h=h, within=w, w=N, mode=2, scale=1, out=o, cap=nv, out_len=sz()).cases(
            tag, nulls=("h", "within", "out", "out_len"), zeros=("w",), short=("cap", nv), other=(("mode9", {"mode": 9}), ("scale9", {"scale": 9})))
    # match, match_pcm16
    for tag, fn, src in (("match", "am_match", hayp), ("match_device", "am_match_device", hp), ("match_pcm16", "am_match_pcm16", pcm.ctypes.data),
                         ("match_pcm16_device", "am_match_pcm16_device", pcmp)):
        c += E(fn, h=h, hay=src, len=N, p=pp, out=peaks, cap=64, n_out=sz()).cases(
            tag, nulls=("h", "hay", "p", "out", "n_out"), zeros=("len",), short=("cap", "n_out"))
    # several needles
    ptrs, lens = (C.c_void_p * 1)(hp), (C.c_size_t * 1)(N)
    c += E("am_match_multi_batch_device", needles=hs, nn=1, hays=ptrs, lens=lens, n_hay=1, fmt=F32, p=pp, out=peaks, cap=64, n_out=sz()).cases(
        "match_multi_batch_device", nulls=("needles", "hays", "lens", "p", "out", "n_out"), fmt="fmt", zeros=("nn", "n_hay"))
    c += E("am_match_multi_varlen_batch_device", needles=hs, nn=1, overlaps=None, hays=ptrs, lens=lens, n_hay=1, fmt=F32, p=pp, out=peaks, cap=64,
           n_out=sz()).cases("match_multi_varlen_batch_device", nulls=("needles", "hays", "lens", "p", "out", "n_out"), fmt="fmt",
                             zeros=("nn", "n_hay"))
    c += E("am_match_multi_varlen", needles=hs, nn=1, overlaps=None, hay=hayp, len=N, fmt=F32, p=pp, out=peaks, cap=64, n_out=sz()).cases(
        "match_multi_varlen", nulls=("needles", "hay", "p", "out", "n_out"), fmt="fmt", zeros=("nn", "len"), short=("cap", "n_out"))
    # find_peaks, find_peaks_top, the k best
    sc = np.zeros(N, np.float32)
    sc[[100, 900, 1700, 3000]] = (1.0, 0.8, 0.9, 0.7)
    d_sc = gpu.DeviceBuffer.from_numpy(0, sc)
    keep += [sc, d_sc, ptrs, lens]
    c += E("am_find_peaks", device=0, scores=sc.ctypes.data, n=N, prom=0.1, dist=10, out=peaks, cap=64, n_out=sz()).cases(
        "find_peaks", nulls=("scores", "out", "n_out"), zeros=("n",), short=("cap", "n_out"))
    for tag, fn, src in (("find_peaks_top", "am_find_peaks_top", sc.ctypes.data), ("find_peaks_top_device", "am_find_peaks_top_device", d_sc.ptr)):
        c += E(fn, device=0, scores=src, n=N, prom=0.1, dist=10, k=3, out=peaks, n_out=sz()).cases(
            tag, nulls=("scores", "out", "n_out"), zeros=("n", "k"))
    bp = gpu.best_params(3)
    for tag, fn, src in (("match_best", "am_match_best", hayp), ("match_best_device", "am_match_best_device", hp)):
        c += E(fn, h=h, hay=src, len=N, fmt=F32, bp=C.byref(bp), out=peaks, n_out=sz()).cases(
            tag, nulls=("h", "hay", "bp", "out", "n_out"), fmt="fmt", zeros=("len",), other=(("k0", {"bp": C.byref(gpu.best_params(0))}),))
    c += E("am_match_best_batch_device", h=h, hays=ptrs, lens=lens, n_hay=1, fmt=F32, bp=C.byref(bp), out=peaks, n_out=sz()).cases(
        "match_best_batch_device", nulls=("h", "hays", "lens", "bp", "out", "n_out"), fmt="fmt", zeros=("n_hay",))
    # the down-mixes (host forms)
    c += E("am_pcm_s16_stereo_to_mono", device=0, src=pcm.ctypes.data, frames=N, out=outp).cases("pcm_to_mono", nulls=("src", "out"), zeros=("frames",))
    c += E("am_pcm_s16_stereo_mix", device=0, src=pcm.ctypes.data, frames=N, a=0.5, b=0.5, out=outp).cases(
        "pcm_mix", nulls=("src", "out"), zeros=("frames",))
    # traces
    bins = np.zeros(64, gpu.TRACE_BIN_DTYPE)
    keep += [bins, bp]
    for tag, fn, src, dev in (("trace_scores", "am_trace_scores", sc.ctypes.data, False), ("trace_scores_device", "am_trace_scores_device", d_sc.ptr, True)):
        c += E(fn, device=0, scores=src, n=N, bin=512, out=bins.ctypes.data, cap=64, n_out=sz()).cases(
            tag, nulls=("scores", "out", "n_out"), zeros=("n", "bin"), short=("cap", "n_out"), misaligned=(("scores", src),) if dev else ())
    tp = gpu.trace_params(512)
    for tag, fn, src, dev in (("match_trace", "am_match_trace", hayp, False), ("match_trace_device", "am_match_trace_device", hp, True)):
        c += E(fn, h=h, hay=src, len=N, fmt=F32, tp=C.byref(tp), out=bins.ctypes.data, cap=64, n_out=sz()).cases(
            tag, nulls=("h", "hay", "tp", "out", "n_out"), fmt="fmt", zeros=("len",), short=("cap", "n_out"), host=(("hay", hayp),) if dev else ())
    c += E("am_match_trace_batch_device", h=h, hays=ptrs, lens=lens, n_hay=1, fmt=F32, tp=C.byref(tp), out=bins.ctypes.data, cap=64, n_out=sz()).cases(
        "match_trace_batch_device", nulls=("h", "hays", "lens", "tp", "out", "n_out"), fmt="fmt", zeros=("n_hay",), short=("cap", 8))
    # discovery
    dp = gpu.discover_params(512, 256)
    rec = np.zeros(64, gpu.PROBE_HIT_DTYPE)
    keep += [tp, dp, rec]
    for tag, fn, a, dev in (("discover", "am_discover", hayp, False), ("discover_device", "am_discover_device", hp, True)):
        c += E(fn, device=0, a=a, len_a=N, b=a, len_b=N, fmt=F32, dp=C.byref(dp), out=rec.ctypes.data, cap=64, n_out=sz()).cases(
            tag, nulls=("a", "b", "dp", "out", "n_out"), fmt="fmt", zeros=("len_a", "len_b"), short=("cap", "n_out"),
            host=(("a", hayp), ("b", hayp)) if dev else ())
    for tag, fn, src, dev in (("probe_scores", "am_probe_scores", sc.ctypes.data, False), ("probe_scores_device", "am_probe_scores_device", d_sc.ptr, True)):
        c += E(fn, device=0, scores=src, n=N, ex_lo=0, ex_hi=0, sep=10, out=rec.ctypes.data).cases(
            tag, nulls=("scores", "out"), zeros=("n", "sep"), misaligned=(("scores", src),) if dev else (), host=(("scores", sc.ctypes.data),) if dev else ())
    hits = np.zeros(8, gpu.PROBE_HIT_DTYPE)
    hits["probe"] = np.arange(8) * 256
    hits["best"] = hits["probe"] + np.repeat([1000, 2000], 4).astype(np.uint64)
    hits["ncc"], hits["ncc_second"] = 0.9, 0.1
    rp = gpu.region_params(0.5, 4)
    regs = np.zeros(8, gpu.REGION_DTYPE)
    keep += [hits, rp, regs]
    c += E("am_discover_regions", hits=hits.ctypes.data, n=8, dp=C.byref(dp), rp=C.byref(rp), out=regs.ctypes.data, cap=8, n_out=sz()).cases(
        "discover_regions", nulls=("hits", "dp", "rp", "out", "n_out"), zeros=("n",), short=("cap", "n_out"))
    # envelopes
    LF, NB = 8, 4
    ep = gpu.env_params(gpu.band_edges_log(8000, LF, 150.0, 3000.0, NB))
    grid = gpu.env_grid(0.0, 0)   # (one drift: a needle of 257 samples holds one frame of 256)
    lev = np.zeros(NB * 64, np.uint16)
    keep += [ep, grid, lev]
    for tag, fn, src, dev in (("envelope", "am_envelope", hayp, False), ("envelope_device", "am_envelope_device", hp, True)):
        c += E(fn, device=0, signal=src, len=N, fmt=F32, ep=C.byref(ep), drift=0.0, out=lev.ctypes.data, cap=64, n_frames=sz()).cases(
            tag, nulls=("signal", "ep", "out", "n_frames"), fmt="fmt", zeros=("len",), short=("cap", "n_frames"), host=(("signal", hayp),) if dev else ())
    bank = (rng.integers(0, 1000, NB * 6)).astype(np.uint16)
    ehay = (rng.integers(0, 1000, NB * 40)).astype(np.uint16)
    frames = np.array([6], np.uint32)
    d_bank, d_ehay = gpu.DeviceBuffer.from_numpy(0, bank), gpu.DeviceBuffer.from_numpy(0, ehay)
    z, qi = np.zeros(64, np.float32), np.zeros(64, np.uint32)
    keep += [bank, ehay, frames, d_bank, d_ehay, z, qi]
    for tag, fn, nd, eh, dev in (("envelope_scores", "am_envelope_scores", bank.ctypes.data, ehay.ctypes.data, False),
                                 ("envelope_scores_device", "am_envelope_scores_device", d_bank.ptr, d_ehay.ptr, True)):
        c += E(fn, device=0, needles=nd, frames=frames.ctypes.data, nn=1, nb=NB, hay=eh, hay_frames=40, z=z.ctypes.data, qi=qi.ctypes.data, cap=64,
               n_out=sz()).cases(tag, nulls=("needles", "frames", "hay", "z", "qi", "n_out"), zeros=("nn", "nb", "hay_frames"), short=("cap", "n_out"),
                                 host=(("needles", bank.ctypes.data), ("hay", ehay.ctypes.data)) if dev else ())
    zz = np.zeros(64, np.float32)
    zz[[5, 30, 50]] = (0.9, 0.8, 0.7)
    picks = np.zeros(8, gpu.ENV_PICK_DTYPE)
    keep += [zz, picks]
    c += E("am_envelope_pick", z=zz.ctypes.data, qi=qi.ctypes.data, n=64, min_score=0.5, sep=4, out=picks.ctypes.data, cap=8, n_out=sz()).cases(
        "envelope_pick", nulls=("z", "qi", "out", "n_out"), zeros=("n",), short=("cap", "n_out"), other=(("nan", {"min_score": float("nan")}),))
    ehits = np.zeros(64, gpu.ENV_HIT_DTYPE)
    keep += [ehits]
    for tag, fn, src, dev in (("match_envelope", "am_match_envelope", hayp, False), ("match_envelope_device", "am_match_envelope_device", hp, True)):
        c += E(fn, h=h, hay=src, len=N, fmt=F32, ep=C.byref(ep), grid=C.byref(grid), min_score=-1.0, out=ehits.ctypes.data, cap=64, n_out=sz()).cases(
            tag, nulls=("h", "hay", "ep", "grid", "out", "n_out"), fmt="fmt", zeros=("len",), short=("cap", "n_out"), host=(("hay", hayp),) if dev else ())
    # whitening, resampling
    r = (C.c_double * 9)()
    taps = (C.c_float * 3)(1.0, -0.5, 0.25)
    new = lambda: C.byref(C.c_void_p())   # noqa: E731
    keep += [r, taps]
    for tag, fn, src in (("lag_products", "am_lag_products", hayp), ("lag_products_device", "am_lag_products_device", hp)):
        c += E(fn, device=0, src=src, n=N, fmt=F32, order=8, r=r).cases(tag, nulls=("src", "r"), fmt="fmt", zeros=("n", "order"))
    for tag, fn, src, o in (("fir", "am_fir", hayp, outp), ("fir_device", "am_fir_device", hp, d_out.ptr)):
        c += E(fn, device=0, src=src, n_in=N, fmt=F32, taps=taps, n_taps=3, lead=2, out=o, cap=N - 2, n_out=sz()).cases(
            tag, nulls=("src", "taps", "out", "n_out"), fmt="fmt", zeros=("n_in", "n_taps"), short=("cap", N - 2), other=(("lead_all", {"lead": N}),))
    c += E("am_needle_create_filtered", device=0, needle=needle.ctypes.data, n=S, fmt=F32, taps=taps, n_taps=3, out=new()).cases(
        "needle_create_filtered", nulls=("needle", "taps", "out"), fmt="fmt", zeros=("n", "n_taps"))
    no = gpu.resample_len(N, 44100, 48000)
    for tag, fn, src, o in (("resample", "am_resample", hayp, outp), ("resample_device", "am_resample_device", hp, d_out.ptr)):
        c += E(fn, device=0, src=src, n_in=N, fmt=F32, src_rate=44100, dst_rate=48000, out=o, cap=no, n_out=sz()).cases(
            tag, nulls=("src", "out", "n_out"), fmt="fmt", zeros=("n_in", "src_rate"), short=("cap", no))
    c += E("am_needle_create_resampled", device=0, needle=needle.ctypes.data, n=S, fmt=F32, src_rate=44100, dst_rate=48000, out=new()).cases(
        "needle_create_resampled", nulls=("needle", "out"), fmt="fmt", zeros=("n", "dst_rate"))
    c += E("am_needle_create_pcm16", device=0, src=pcm.ctypes.data, frames=S, out=new()).cases("needle_create_pcm16", nulls=("src", "out"), zeros=("frames",))
    # needle estimation from rows
    est = gpu.AmEstimateParams(method=int(gpu.Est.MEDIAN), trim_permille=0, lead=0, length=S)
    rows = np.zeros(3 * S, np.float32)
    keep += [est, rows]
    c += E("am_needle_estimate_rows", device=0, rows=rows.ctypes.data, n=3, ep=C.byref(est), est=outp, dev=None, count=None).cases(
        "needle_estimate_rows", nulls=("rows", "ep", "est"), zeros=("n",))
    ehit = (gpu.AmEstHit * 3)(gpu.AmEstHit(500, 0, 1.0), gpu.AmEstHit(2500, 0, 1.0), gpu.AmEstHit(1500, 0, 1.0))
    row = np.zeros(S, np.float32)
    keep += [ehit, row]
    c += E("am_needle_estimate_device", device=0, hays=ptrs, lens=lens, n_hay=1, fmt=F32, hits=ehit, n=3, ep=C.byref(est), est=outp, dev=None,
           count=None).cases("needle_estimate_device", nulls=("hays", "lens", "hits", "ep", "est"), fmt="fmt", zeros=("n", "n_hay"))
    c += E("am_hit_window", hay=hayp, len=N, fmt=F32, start=500, scale=1.0, lead=0, length=S, row=row.ctypes.data).cases(
        "hit_window", nulls=("hay", "row"), fmt="fmt", zeros=("length", "scale"))
    # the peak merge, parts, streams and pools: the hand-back and the format check
    two = (gpu.AmPeak * 2)(gpu.AmPeak(100, 0, 1.0, 1.0), gpu.AmPeak(3000, 0, 0.9, 0.9))
    keep += [two]
    c += E("am_merge_peaks", p=pp, peaks=two, n=2, out=peaks, cap=64, n_out=sz()).cases(
        "merge_peaks", nulls=("p", "peaks", "out", "n_out"), zeros=("n",), short=("cap", "n_out"))
    c += E("am_match_part_device", h=h, hay=hp, n=N, fmt=F32, p=pp, n_windows=1, first=0, out=peaks, cap=64, n_out=sz()).cases(
        "match_part_device", nulls=("h", "p", "out", "n_out"), fmt="fmt", zeros=("n", "n_windows"), short=("cap", "n_out"))
    c += E("am_match_stream_begin", h=h, fmt=F32, expected=N, p=pp, out=new()).cases("match_stream_begin", nulls=("h", "p", "out"), fmt="fmt")
    pool = gpu.Pool(needle, devices=[0])
    keep += [pool]
    c += E("am_pool_match_long", pool=pool._p, hay=hayp, len=N, fmt=F32, p=pp, out=peaks, cap=64, n_out=sz()).cases(
        "pool_match_long", nulls=("pool", "hay", "p", "out", "n_out"), fmt="fmt", zeros=("len",), short=("cap", "n_out"))
    hptrs, pcm_hptrs, pcm_ptrs = (C.c_void_p * 1)(hayp), (C.c_void_p * 1)(pcm.ctypes.data), (C.c_void_p * 1)(pcmp)
    keep += [hptrs, pcm_hptrs, pcm_ptrs]
    for tag, hays in (("pool_match_batch", hptrs), ("pool_match_batch_device", ptrs), ("pool_match_batch_pcm16", pcm_hptrs),
                      ("pool_match_batch_pcm16_device", pcm_ptrs)):
        c += E("am_" + tag, pool=pool._p, hays=hays, lens=lens, n_hay=1, p=pp, out=peaks, cap=64, n_out=sz()).cases(
            tag, nulls=("pool", "hays", "lens", "p", "out", "n_out"), zeros=("n_hay",), short=("cap", "n_out"))
    mpool = gpu.MultiPool([needle], devices=[0])
    keep += [mpool]
    for tag, hays in (("pool_match_multi_batch", hptrs), ("pool_match_multi_batch_device", ptrs)):
        c += E("am_" + tag, pool=mpool._p, hays=hays, lens=lens, n_hay=1, fmt=F32, p=pp, out=peaks, cap=64, n_out=sz()).cases(
            tag, nulls=("pool", "hays", "lens", "p", "out", "n_out"), fmt="fmt", zeros=("n_hay",))
    ids = [i for i, _ in c]
    assert len(set(ids)) == len(ids), "duplicate case id"
    return [(i, (lambda t=t, k=keep: t())) for i, t in c]


def run(gpu):
    return {i: t() for i, t in cases(gpu)}


if __name__ == "__main__":
    root = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.path.insert(0, os.path.join(root, "audio-matcher_amd", "python"))
    import audiomatch_amd
    got = run(audiomatch_amd)
    if "--record" in sys.argv:   # (--record [PATH]: the golden file unless a path follows)
        rest = sys.argv[sys.argv.index("--record") + 1:]
        with open(rest[0] if rest else GOLDEN, "w") as f:
            json.dump(got, f, indent=0, sort_keys=True)
            f.write("\n")
    for i, v in got.items():
        print(i, v)
