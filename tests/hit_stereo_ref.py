"""The checker of the per-hit stereo image (am_hit_stereo*, include/audiomatch.h) in plain numpy f64: c_L and c_R by
np.dot over the i16 values times k, the three energies as Python integers times k^2, the record by the header's
formulas.  Beside each record it returns, per channel, the margin between the best and the second-best |c|, so that a
test can state which of its cases decide the best lag.  mix_ref is am_pcm_s16_stereo_mix with its three f64 steps spelled
out."""
from dataclasses import dataclass

import numpy as np

UNREFINED, BELOW, NONFIN, EMPTY = 1, 2, 4, 8
LEFT_SILENT, RIGHT_SILENT, SIDE_SILENT, COLLINEAR, LEFT_UNREFINED, RIGHT_UNREFINED = 1024, 2048, 4096, 8192, 16384, 32768
MAX_RADIUS = 16
MIN_INDEPENDENCE = 1e-6
ABSENT, CENTRE, LEFT, RIGHT, PANNED, INVERTED = range(6)
KAPPA = np.float32(0.5) * (np.float32(1.0) / np.float32(65535.0))     # the f32 constant of the down-mix
K = float(np.float32(2.0) * KAPPA)                                    # k = (double)(2 kappa)
FLOATS = ("ncc_left", "ncc_right", "ncc_mid", "ncc_side", "ncc_best", "gain_left", "gain_right", "mix_left", "mix_right")


def bits(q):
    return bytes(q)


def downmix(lr):
    """The down-mix every other entry point applies to i16 stereo frames, bit for bit."""
    lr = np.asarray(lr).reshape(-1, 2)
    return ((lr[:, 0].astype(np.int32) + lr[:, 1]).astype(np.float32) * KAPPA).astype(np.float32)


def mix_ref(a, b, pcm):
    """out[i] = f32((f64(a) L[i] + f64(b) R[i]) k): two exact products, one f64 sum, one f64 product, one rounding."""
    lr = np.asarray(pcm, dtype=np.int16).reshape(-1, 2)
    a64, b64 = np.float64(np.float32(a)), np.float64(np.float32(b))
    pl = a64 * lr[:, 0].astype(np.float64)          # exact: 24 x 16 bits
    pr = b64 * lr[:, 1].astype(np.float64)
    s = pl + pr                                     # one rounding
    p = s * np.float64(K)                           # one rounding
    return p.astype(np.float32)                     # one rounding


@dataclass
class StereoRef:
    lag_left: float
    lag_right: float
    ncc_left: float
    ncc_right: float
    ncc_mid: float
    ncc_side: float
    ncc_best: float
    gain_left: float
    gain_right: float
    mix_left: float
    mix_right: float
    flags: int
    best_left: int = 0          # lambda* per channel
    best_right: int = 0
    margin_left: float = 1.0    # (best |c| - second-best |c|) / best |c| per channel; 1 where there is one lag only
    margin_right: float = 1.0
    det_ratio: float = 0.0      # det / (E_L E_R)


def _lag(c, r):
    """(lambda*, lag, unrefined, margin) of |c(-r .. r)| (c[l + r] = c(l)): the rule of am_hit_segments on |c|."""
    a = np.abs(c)
    ls = 0
    for k in range(1, r + 1):
        if a[r - k] > a[r + ls]:
            ls = -k
        if a[r + k] > a[r + ls]:
            ls = k
    rest = np.delete(a, r + ls)
    margin = 1.0 if rest.size == 0 or a[r + ls] == 0.0 else float((a[r + ls] - rest.max()) / a[r + ls])
    lag, unref = float(ls), True
    if r != 0 and abs(ls) != r:
        lo, mid, hi = a[r + ls - 1], a[r + ls], a[r + ls + 1]
        den = lo - 2.0 * mid + hi
        if den < 0.0:
            unref = False
            lag += min(max(0.5 * (lo - hi) / den, -0.5), 0.5)
    return ls, lag, unref, margin


def stereo_ref(lr, needle, t, r, floor_db=60.0):
    """The StereoRef of the hit at frame t of the i16 frames lr [(frames, 2)] against the f32 needle."""
    lr = np.asarray(lr, dtype=np.int16).reshape(-1, 2)
    n = np.asarray(needle, dtype=np.float32).astype(np.float64)
    s, ln = len(n), len(lr)
    nan = float("nan")
    if not np.isfinite(n).all():
        return StereoRef(0.0, 0.0, *([nan] * 9), NONFIN)
    en = float(np.dot(n, n))
    if en == 0.0:
        return StereoRef(0.0, 0.0, *([0.0] * 9), EMPTY)
    lo, hi = max(t - r, 0), min(t + s + r, ln)
    span = np.zeros((s + 2 * r, 2), dtype=np.int64)          # span[u + r] = frame t + u
    span[lo - (t - r):hi - (t - r)] = lr[lo:hi]
    fl, fr = span[:, 0].astype(np.float64), span[:, 1].astype(np.float64)
    cl = np.array([K * np.dot(fl[l + r:l + r + s], n) for l in range(-r, r + 1)])
    cr = np.array([K * np.dot(fr[l + r:l + r + s], n) for l in range(-r, r + 1)])
    w = span[r:r + s]
    sll, srr, slr = (int(np.dot(w[:, 0], w[:, 0])), int(np.dot(w[:, 1], w[:, 1])), int(np.dot(w[:, 0], w[:, 1])))
    k2 = K * K
    e_l, e_r, e_lr = float(sll) * k2, float(srr) * k2, float(slr) * k2
    e_m, e_d = float(sll + 2 * slr + srr) * k2 * 0.25, float(sll - 2 * slr + srr) * k2 * 0.25
    c_l, c_r = float(cl[r]), float(cr[r])
    flags = 0
    bl, lag_l, unref, ml = _lag(cl, r)
    flags |= LEFT_UNREFINED if unref else 0
    br, lag_r, unref, mr = _lag(cr, r)
    flags |= RIGHT_UNREFINED if unref else 0
    floor = en * 10.0 ** (-floor_db / 10.0)

    def silent(e):
        return e == 0.0 or e < floor

    ncc_l = ncc_r = ncc_m = ncc_s = ncc_b = m_l = m_r = 0.0
    if silent(e_l):
        flags |= LEFT_SILENT
    else:
        ncc_l = c_l / np.sqrt(en * e_l)
    if silent(e_r):
        flags |= RIGHT_SILENT
    else:
        ncc_r = c_r / np.sqrt(en * e_r)
    if silent(e_m):
        flags |= BELOW
    else:
        ncc_m = 0.5 * (c_l + c_r) / np.sqrt(en * e_m)
    if silent(e_d):
        flags |= SIDE_SILENT
    else:
        ncc_s = 0.5 * (c_l - c_r) / np.sqrt(en * e_d)
    det = e_l * e_r - e_lr * e_lr
    if silent(e_l) or silent(e_r) or det <= MIN_INDEPENDENCE * e_l * e_r:
        flags |= COLLINEAR
        if not (silent(e_l) and silent(e_r)):
            if e_l >= e_r:
                ncc_b, m_l = abs(c_l) / np.sqrt(en * e_l), c_l / e_l
            else:
                ncc_b, m_r = abs(c_r) / np.sqrt(en * e_r), c_r / e_r
    else:
        q = (c_l * c_l * e_r - 2.0 * c_l * c_r * e_lr + c_r * c_r * e_l) / det
        ncc_b = np.sqrt(max(q, 0.0) / en)
        m_l, m_r = (c_l * e_r - c_r * e_lr) / det, (c_r * e_l - c_l * e_lr) / det
    ratio = det / (e_l * e_r) if e_l > 0.0 and e_r > 0.0 else 0.0
    return StereoRef(lag_l, lag_r, float(ncc_l), float(ncc_r), float(ncc_m), float(ncc_s), float(ncc_b), c_l / en, c_r / en,
                     float(m_l), float(m_r), flags, bl, br, ml, mr, float(ratio))


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def assert_records(got, exp, who=""):
    """One record against the checker: the flags equal; lambda* equal wherever the channel's margin exceeds 1e-9 of the
    best |c|, and the lag then within 1e-9; each float within 2 f32 ulp or 1e-9 absolute of the checker, whichever is
    larger."""
    assert got.flags == exp.flags, (who, got, exp)
    if exp.flags & NONFIN:
        assert all(np.isnan(getattr(got, f)) for f in FLOATS) and got.lag_left == 0.0 and got.lag_right == 0.0, (who, got)
        return
    for side in ("left", "right"):
        if getattr(exp, "margin_" + side) > 1e-9:
            g, e = getattr(got, "lag_" + side), getattr(exp, "lag_" + side)
            assert abs(g - e) <= 1e-9 and abs(g - getattr(exp, "best_" + side)) <= 0.5, (who, side, got, exp)
    for f in FLOATS:
        g, e = float(getattr(got, f)), float(getattr(exp, f))
        assert abs(g - e) <= max(2.0 * ulp32(e), 1e-9), (who, f, g, e, got, exp)


def summary_ref(q, min_ncc):
    """(image, balance_db, delay, downmix_loss_db) by the rules of the header."""
    with np.errstate(divide="ignore", invalid="ignore"):
        balance = float(20.0 * np.log10(np.float64(abs(q.gain_left)) / np.float64(abs(q.gain_right))))
        loss = float(20.0 * np.log10(np.float64(q.ncc_best) / np.float64(abs(q.ncc_mid))))
    has_l, has_r = abs(q.ncc_left) >= min_ncc, abs(q.ncc_right) >= min_ncc
    delay = q.lag_left - q.lag_right if has_l and has_r else float("nan")
    if not q.ncc_best >= min_ncc:
        image = ABSENT
    elif has_l and not has_r:
        image = LEFT
    elif has_r and not has_l:
        image = RIGHT
    elif has_l and has_r and (q.ncc_left < 0) != (q.ncc_right < 0):
        image = INVERTED
    elif has_l and has_r and abs(balance) <= 3.0:
        image = CENTRE
    else:
        image = PANNED
    return image, balance, delay, loss
