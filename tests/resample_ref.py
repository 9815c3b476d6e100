"""The f64 checker of sample-rate conversion (am_resample*, include/audiomatch.h): the filter and the output formula of
the header, in numpy, for the resampling tests; and, for test_gpu_resample_edges.py and test_resample_design_host.py, a
mirror of the kernel's launch geometry, the designed inputs placed with it and the pairs they run at."""
from math import gcd

import numpy as np

MAX_RATE, MAX_R = 768000, 8192


def ratio(src_rate: int, dst_rate: int):
    """(L, M, H): up factor, down factor, filter half length."""
    g = gcd(src_rate, dst_rate)
    L, M = dst_rate // g, src_rate // g
    return L, M, 10 * max(L, M)


def out_len(n_in: int, src_rate: int, dst_rate: int) -> int:
    L, M, _ = ratio(src_rate, dst_rate)
    return -(-n_in * L // M)


def taps(src_rate: int, dst_rate: int) -> np.ndarray:
    """h[j + H], j = -H .. H, in f64: L * w / sum(w), w = c sinc(c j) I0(5 sqrt(1 - (j/H)^2)) / I0(5), c = 1/R."""
    L, M, H = ratio(src_rate, dst_rate)
    c = 1.0 / max(L, M)
    j = np.arange(-H, H + 1, dtype=np.float64)
    w = c * np.sinc(c * j) * np.i0(5.0 * np.sqrt(1.0 - (j / H) ** 2)) / np.i0(5.0)
    return L * w / w.sum()


def resample(x, src_rate: int, dst_rate: int, k0: int = 0, k1=None, h=None, n0: int = 0, n_in=None) -> np.ndarray:
    """y[k] = sum over n in [0, n_in) with |k M - n L| <= H of x[n] h[k M - n L], for k in [k0, k1), in f64.
    Non-finite samples reach exactly the outputs whose support holds them.  x may be a window of a longer signal:
    samples n0 .. n0 + len(x) of n_in (it must hold every sample the outputs read)."""
    x = np.asarray(x, dtype=np.float64)
    L, M, H = ratio(src_rate, dst_rate)
    if n_in is None:
        n_in = n0 + x.size
    if k1 is None:
        k1 = out_len(n_in, src_rate, dst_rate)
    if h is None:
        h = taps(src_rate, dst_rate)
    k = np.arange(k0, k1, dtype=np.int64)
    a = k * M + H                       # h index of sample n: a - n L, in [0, 2H] on the support
    nh, p = a // L, a % L
    y = np.zeros(k.size, dtype=np.float64)
    if n_in == 0:
        return y
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(2 * H // L + 1):
            n = nh - t
            idx = p + t * L
            ok = (idx <= 2 * H) & (n >= 0) & (n < n_in)
            if not ok.any():
                continue
            assert (n[ok] >= n0).all() and (n[ok] < n0 + x.size).all(), "the window does not hold every sample read"
            y += np.where(ok, h[np.minimum(idx, 2 * H)] * x[np.clip(n - n0, 0, x.size - 1)], 0.0)
    return y


def downmix(interleaved) -> np.ndarray:
    """(l + r) * 0.5 * (1/65535) in f32, bit for bit as the library's down-mix."""
    a = np.asarray(interleaved, dtype=np.int16).reshape(-1, 2)
    s = a[:, 0].astype(np.float32) + a[:, 1].astype(np.float32)
    return (s * np.float32(0.5)) * np.float32(1.0 / 65535.0)


def resample_dot(x, src_rate: int, dst_rate: int, k0: int = 0, k1=None, h=None, n_in=None) -> np.ndarray:
    """The same formula as resample(), one f64 dot product per output instead of a loop over the taps: for pairs whose
    filter has tens of thousands of taps and whose outputs are few.  x holds the whole signal."""
    x = np.asarray(x, dtype=np.float64)
    L, M, H = ratio(src_rate, dst_rate)
    if n_in is None:
        n_in = x.size
    if k1 is None:
        k1 = out_len(n_in, src_rate, dst_rate)
    if h is None:
        h = taps(src_rate, dst_rate)
    y = np.zeros(max(0, k1 - k0), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, k in enumerate(range(k0, k1)):
            a = k * M + H
            lo, hi = max(0, -((2 * H - a) // L)), min(n_in - 1, a // L)      # a - n L in [0, 2H], n in [0, n_in)
            if hi >= lo:
                n = np.arange(lo, hi + 1, dtype=np.int64)
                y[i] = np.sum(x[n] * h[a - n * L])
    return y


# ---- the kernel's launch geometry (am_resample.hip), for placing designed inputs ---------------------------------------
# The constants of am_kernels.h and am_resample.hip; test_resample_design_host.py reads them out of the sources.
K_RS_THREADS, K_RS_J, K_RS_TC = 256, 8, 8
K_RS_XS_MAX, K_RS_TAB_MAX, K_RS_W_MAX = 8192, 8192, 2048

FORMS = ("both", "input", "table", "neither")


def geometry(src_rate: int, dst_rate: int) -> dict:
    """The launch geometry of a pair as am_resample.hip's rs_taps and rs_geometry compute it: L, M, H, the taps of the
    longest phase T, the table's row length ts, work items per workgroup W, floats of staged input xs_cap (0: not
    staged), tab_lds (the table is staged), outputs per workgroup bo = W kRsJ and the kernel form that runs.

    The mirror is used ONLY to place inputs (block edges, staged quads) and to word failures: every expectation is the
    f64 checker's.  Should the library's geometry change, the designed samples land elsewhere and stay correct."""
    L, M, H = ratio(src_rate, dst_rate)
    T = 2 * H // L + 1
    ts = (T + K_RS_TC - 1) // K_RS_TC * K_RS_TC

    def span(W):
        return ((L - 1 + (W * K_RS_J - 1) * M) // L + ts + 8 + 3) // 4 * 4

    best = best_x = 0
    best_eff = best_eff_x = -1.0
    for g in range(1, max(1, K_RS_W_MAX // L) + 1):
        W = L * g
        eff = W / (K_RS_THREADS * ((W + K_RS_THREADS - 1) // K_RS_THREADS))
        if eff >= best_eff:
            best_eff, best = eff, W
        if span(W) <= K_RS_XS_MAX and eff >= best_eff_x:
            best_eff_x, best_x = eff, W
    if best_eff_x < 0.5:
        best_x = 0
    W = best_x or best
    xs_cap = span(best_x) if best_x else 0
    tab_lds = L * (ts + 1) <= K_RS_TAB_MAX
    form = FORMS[(0 if xs_cap else 2) + (0 if tab_lds else 1)]
    return dict(src=src_rate, dst=dst_rate, L=L, M=M, H=H, T=T, ts=ts, W=W, xs_cap=xs_cap, tab_lds=tab_lds,
                bo=W * K_RS_J, form=form)


def support(g, k):
    """(lowest, highest) sample output k reads before clipping to the signal: nh(k) - cnt(p) + 1 and nh(k)."""
    a = k * g["M"] + g["H"]
    nh, p = a // g["L"], a % g["L"]
    return nh - ((2 * g["H"] - p) // g["L"] + 1) + 1, nh


def staged_quads(g, b):
    """First sample of the first and of the last quad that workgroup b stages (as the kernel computes xb and nq; for a
    form that does not stage its input, where they would lie)."""
    L, M, bo, ts = g["L"], g["M"], g["bo"], g["ts"]
    a0 = b * bo * M + g["H"]
    q0, r0 = a0 // L, a0 % L
    lo = q0 - (ts - 1)
    xb = lo - lo % 4
    hi = q0 + (r0 + (bo - 1) * M) // L
    nq = (hi - xb) // 4 + 1
    if g["xs_cap"]:
        nq = min(nq, g["xs_cap"] // 4)
    return xb, xb + 4 * (nq - 1)


def last_quad_carry(g) -> bool:
    """Whether a workgroup's highest sample opens a quad (only the first sample of its last staged quad is read) and
    lies there because of the carry of the workgroup's start phase r0: a quad count that is one short, or taken without
    r0, loses a live sample.  bo M is a multiple of 8 L, so this is the same for every workgroup of a pair."""
    L, M, bo = g["L"], g["M"], g["bo"]
    q0, r0 = g["H"] // L, g["H"] % L
    return bool(g["xs_cap"]) and (q0 + (r0 + (bo - 1) * M) // L) % 4 == 0 and r0 + (bo - 1) * M % L >= L


def design_len(g, extra: int = 0) -> int:
    """n_in of a designed input: two whole workgroups and a partial third (n_out = 2 bo plus about bo / 3), plus
    `extra` samples (0 .. 3, for the four residues of n_in mod 4)."""
    target = 2 * g["bo"] + (g["bo"] // 3 | 1)
    return -(-target * g["M"] // g["L"]) + extra


def edge_samples(g, n_in: int) -> np.ndarray:
    """The input positions that matter at the edges of workgroups 1 and 2: for the outputs b bo - 1 and b bo the lowest
    and highest sample each reads and the sample just outside each; the first and last quad a workgroup stages;
    samples 0 .. 3 and n_in - 4 .. n_in - 1.  Sorted, unique, inside [0, n_in)."""
    pos = [0, 1, 2, 3, n_in - 4, n_in - 3, n_in - 2, n_in - 1]
    for b in (1, 2):
        for k in (b * g["bo"] - 1, b * g["bo"]):
            lo, hi = support(g, k)
            pos += [lo - 1, lo, hi, hi + 1]
        first, last = staged_quads(g, b)
        pos += list(range(first, first + 4)) + list(range(last, last + 4))
    pos = np.unique(np.asarray(pos, dtype=np.int64))
    return pos[(pos >= 0) & (pos < n_in)]


def far_apart(g, positions, extra=()):
    """positions (and a few interior ones, `extra`) split into groups whose members are at least 2H/L + 2 samples
    apart: within one group no output's support holds two of them."""
    sep = 2 * g["H"] // g["L"] + 2
    groups = []
    for n in np.unique(np.concatenate([np.asarray(positions, np.int64), np.asarray(extra, np.int64)])):
        for grp in groups:
            if n - grp[-1] >= sep:
                grp.append(int(n))
                break
        else:
            groups.append([int(n)])
    return groups


AMPS = (1.0, -1.0, 0.5, -0.5, 2.0, -2.0)            # f32 impulses: powers of two, both signs
AMPS_I16 = (16384, -16384, 8192, -8192)             # i16 impulses: l = r = this


def impulse_designs(g, n_in: int, i16: bool = False):
    """The sparse designs of a pair: a list of (positions, amplitudes, x) with x zero but for x[positions] = amplitudes
    (f32), and for i16 (positions, amplitudes, x, lr) with lr the interleaved frames and x = downmix(lr).  Where the
    signal is long enough the last design holds one impulse twice, a workgroup apart: the same taps on the same
    amplitude at another place (short signals, the steep up-samplers, meet that among their edge samples anyway)."""
    interior = [g["bo"] * g["M"] // g["L"] // 2 + 1, 3 * g["bo"] * g["M"] // g["L"] // 2]
    interior = [n for n in interior if 0 <= n < n_in]
    groups = far_apart(g, edge_samples(g, n_in), interior)
    twin = interior[0] + (g["bo"] // g["L"] + 1) * g["M"]      # the same taps one workgroup and L outputs further on
    twins = twin < n_in and twin - interior[0] >= 2 * g["H"] // g["L"] + 2
    if twins:
        groups.append([interior[0], twin])
    out = []
    c = 0
    for gi, grp in enumerate(groups):
        pos = np.asarray(grp, np.int64)
        pick = [0] * pos.size if twins and gi == len(groups) - 1 else [c + i for i in range(pos.size)]
        if i16:
            v = np.asarray([AMPS_I16[i % len(AMPS_I16)] for i in pick], np.int16)
            lr = np.zeros((n_in, 2), np.int16)
            lr[pos, 0] = lr[pos, 1] = v
            x = downmix(lr)
            out.append((pos, x[pos].copy(), x, lr))
        else:
            a = np.asarray([AMPS[i % len(AMPS)] for i in pick], np.float32)
            x = np.zeros(n_in, np.float32)
            x[pos] = a
            out.append((pos, a, x))
        c += pos.size
    return out


def impulse_expectation(g, n_out: int, pos, amp, h=None):
    """What impulses amp[i] at pos[i] (far apart) give: (k, idx, a, want) over the outputs k inside a support, with
    idx = k M - n L + H the tap and want = a h[idx] in f64.  Every other output is 0."""
    L, M, H = g["L"], g["M"], g["H"]
    if h is None:
        h = taps(g["src"], g["dst"])
    ks, idxs, amps = [], [], []
    for n, a in zip(pos, amp):
        n = int(n)
        k_lo, k_hi = max(0, -((H - n * L) // M)), min(n_out - 1, (n * L + H) // M)     # |k M - n L| <= H
        if k_hi < k_lo:
            continue
        k = np.arange(k_lo, k_hi + 1, dtype=np.int64)
        ks.append(k)
        idxs.append(k * M - n * L + H)
        amps.append(np.full(k.size, float(a)))
    if not ks:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0), np.zeros(0)
    k, idx, a = np.concatenate(ks), np.concatenate(idxs), np.concatenate(amps)
    return k, idx, a, a * h[idx]


def where(g, k: int) -> str:
    """Names output k for a failure message: the pair, its form, the workgroup and the offset in it."""
    return "%d->%d (%s, W %d) block %d offset %d" % (g["src"], g["dst"], g["form"], g["W"], k // g["bo"], k % g["bo"])


# ---- the pairs of the designed tests ----------------------------------------------------------------------------------
EDGE_PAIRS = [(44100, 48000), (48000, 8000), (3, 2), (7, 6), (4, 3),      # both staged ((7, 6): T = ts; (4, 3): last_quad_carry)
              (11025, 384000), (409, 8192), (499, 500), (44100, 16000), (192000, 44100), (1, 8192), (44100, 32000),  # input only
              (300, 7), (401, 13),                                                                  # table staged only
              (32000, 11025), (384000, 11025), (8191, 8192), (8192, 8191)]                          # neither
LONG_PAIRS = [(8192, 1), (8191, 2), (768000, 100), (3000, 1), (384000, 8000)]    # the last one is the control (961 taps)


def long_inputs(g, n_full: int = 12):
    """The inputs of the long-filter test: n_in for n_full full-support outputs and both ends, and x = 1, the sign of
    the taps of one full-support output, and a sine of 5 periods over the filter's span (f32, max |x| = 1)."""
    L, M, H = g["L"], g["M"], g["H"]
    span = 2 * H // L + 1
    n_in = span + n_full * M // L
    h = taps(g["src"], g["dst"])
    k = out_len(n_in, g["src"], g["dst"]) // 2           # an output whose whole support lies inside the signal
    a = k * M + H
    n = np.arange(n_in, dtype=np.int64)
    idx = a - n * L
    sign = np.where((idx >= 0) & (idx <= 2 * H), np.where(h[np.clip(idx, 0, 2 * H)] < 0, -1.0, 1.0), 1.0)
    sine = np.sin(2 * np.pi * 5.0 * n / span)
    return n_in, {"ones": np.ones(n_in, np.float32), "sign": sign.astype(np.float32), "sine": sine.astype(np.float32)}


def sequential_f32(x, g, k: int, h=None) -> np.float32:
    """Output k as a plain sequential f32 sum of its taps in the order t = 0, 1, ... (one fma each) gives it, for x
    whose products with the f32 taps are exact (x = 1 or +-1): np.add.accumulate over the f32 products."""
    L, M, H = g["L"], g["M"], g["H"]
    if h is None:
        h = taps(g["src"], g["dst"])
    a = k * M + H
    nh, p = a // L, a % L
    t = np.arange((2 * H - p) // L + 1, dtype=np.int64)
    n = nh - t
    ok = (n >= 0) & (n < len(x))
    prod = h[p + t[ok] * L].astype(np.float32) * np.asarray(x, np.float32)[n[ok]]
    return np.add.accumulate(prod, dtype=np.float32)[-1]
