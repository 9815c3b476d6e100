"""The per-hit call forms of the Python binding without a device or the library: hit_scores, hit_segments, hit_warp,
hit_bands and hit_significance, each as host method, _device method and *_batch_device function, against a recorder that
stands in for audiomatch_amd.lib().  Every am_hit_* callable of the recorder notes its arguments, writes r into a float
field of record r of the `out` array it was handed and returns 0; so the tests see what the binding passes down (format,
length, peak table, counts, cap, the parameter struct's bytes, the size of `out`) and which records it hands back where."""
import ctypes as C

import numpy as np
import pytest

import audiomatch_amd as am

# name -> (record type, the float field the recorder numbers, records per hit (None: one object per hit, not a list),
#          the public arguments after `peaks`, the parameter struct's bytes (None: the family has none))
WP = am.warp_params(200.0, 6, 3, 10.0)
BP = am.band_params(8, [1, 4, 9])
FAMILIES = {
    "scores": (am.AmHitScore, "ncc", None, (), None),
    "segments": (am.HitSegment, "ncc", 3, (3, 5), bytes(am.AmSegmentParams(3, 5))),
    "warp": (am.HitWarp, "ncc", None, (WP,), bytes(WP)),
    "bands": (am.HitBand, "ncc", 2, (BP,), bytes(BP)),
    "significance": (am.HitSignificance, "z", None, (7, 90), bytes(am.AmSignificanceParams(7, 90))),
}
SYMBOL = {"scores": "am_hit_scores", "segments": "am_hit_segments", "warp": "am_hit_warp", "bands": "am_hit_bands",
          "significance": "am_hit_significance"}
NAMES = sorted(FAMILIES)


def _table(buf):
    return [(int(p.start), int(p.end), float(p.height), float(p.prominence)) for p in buf]


class Recorder:
    """Stands in for the loaded library: am_hit_<family>[_device|_batch_device] record and fill, anything else is an
    AttributeError."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("am_hit_"):
            raise AttributeError(name)
        field = "z" if "significance" in name else "ncc"
        has_params = not name.startswith("am_hit_scores")

        def call(*args):
            out = args[-1]
            params = bytes(args[-2]._obj) if has_params else None       # C.byref(params) stands right ahead of `out`
            lead = args[:-2] if has_params else args[:-1]
            c = {"name": name, "params": params, "len_out": len(out), "out_type": out._type_}
            if name.endswith("_batch_device"):
                handles, nn, arr_p, arr_l, k, fmt, buf, cap, counts = lead
                c.update(handles=[handles[j] for j in range(nn)], nn=nn, ptrs=[arr_p[h] for h in range(k)],
                         lengths=[arr_l[h] for h in range(k)], k=k, fmt=fmt, table=_table(buf), cap=cap, counts=list(counts))
            else:
                h, ptr, length, fmt, buf, k = lead
                c.update(handle=h.value, ptr=ptr, length=length, fmt=fmt, table=_table(buf), k=k)
                if not name.endswith("_device"):                          # the host form: what the pointer holds
                    c["data"] = bytes((C.c_char * (4 * length)).from_address(ptr))   # 4 bytes a sample, and a frame
            for r in range(len(out)):
                setattr(out[r], field, r)
            self.calls.append(c)
            return 0
        return call


@pytest.fixture
def rig(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(am, "lib", lambda: rec)
    needles = []
    for j in range(2):
        n = am.HipConvolve.__new__(am.HipConvolve)
        n.device, n.sample_len, n._h = 0, 16, C.c_void_p(0x1000 + 0x10 * j)
        needles.append(n)
    yield rec, needles
    for n in needles:
        n._h = None              # nothing for close() to hand to the real am_needle_destroy


def _peaks(k, base=0):
    return [am.Peak(base + 10 * i, base + 10 * i + 3, 0.5 + i, 0.25 * (i + 1)) for i in range(k)]


def _as_tuples(peaks):
    return [(p.start, p.end, float(p.height), float(p.prominence)) for p in peaks]


def _numbers(result, field, per):
    """The record numbers of one form's result: [hit] for a family of one object per hit, [hit][record] otherwise."""
    if per is None:
        return [getattr(q, field) for q in result]
    return [[getattr(q, field) for q in hit] for hit in result]


def _expect(k, per, first=0):
    if per is None:
        return [float(first + i) for i in range(k)]
    return [[float((first + i) * per + j) for j in range(per)] for i in range(k)]


def _check_single(c, name, k, peaks, handle):
    rtype, field, per, extra, params = FAMILIES[name]
    assert c["handle"] == handle and c["k"] == k
    assert c["table"] == (_as_tuples(peaks) if k else [(0, 0, 0.0, 0.0)])      # max(1, k) rows
    assert c["params"] == params
    assert c["out_type"] is rtype and c["len_out"] == max(1, k * (per or 1))


HAYSTACKS = {
    "f32": np.linspace(-1.0, 1.0, 50, dtype=np.float32),
    "i16": (np.arange(60, dtype=np.int16) * 7 - 200).reshape(30, 2),
}


@pytest.mark.parametrize("kind", sorted(HAYSTACKS))
@pytest.mark.parametrize("k", [3, 0])
@pytest.mark.parametrize("name", NAMES)
def test_host_form(rig, name, k, kind):
    rec, needles = rig
    rtype, field, per, extra, params = FAMILIES[name]
    a = HAYSTACKS[kind]
    peaks = _peaks(k)
    result = getattr(needles[0], "hit_" + name)(a, peaks, *extra)
    assert len(rec.calls) == 1
    c = rec.calls[0]
    assert c["name"] == SYMBOL[name]
    if kind == "i16":
        assert (c["fmt"], c["length"]) == (int(am.Fmt.S16_STEREO), a.size // 2)
    else:
        assert (c["fmt"], c["length"]) == (int(am.Fmt.F32_MONO), a.size)
    assert c["data"] == a.tobytes()
    _check_single(c, name, k, peaks, needles[0]._h.value)
    assert _numbers(result, field, per) == _expect(k, per)
    if per is None and k:
        assert type(result[0]) is (am.HitScore if name == "scores" else rtype)


def test_host_form_takes_a_list_as_f32(rig):
    rec, needles = rig
    needles[0].hit_scores([0.5, -0.25, 1.0], _peaks(1))
    c = rec.calls[0]
    assert (c["fmt"], c["length"]) == (int(am.Fmt.F32_MONO), 3)
    assert c["data"] == np.array([0.5, -0.25, 1.0], dtype=np.float32).tobytes()


@pytest.mark.parametrize("k", [3, 0])
@pytest.mark.parametrize("name", NAMES)
def test_device_form(rig, name, k):
    rec, needles = rig
    rtype, field, per, extra, params = FAMILIES[name]
    peaks = _peaks(k, base=500)
    result = getattr(needles[1], "hit_" + name + "_device")(0xABC000, 4321, peaks, *extra, fmt=am.Fmt.S16_STEREO)
    assert len(rec.calls) == 1
    c = rec.calls[0]
    assert c["name"] == SYMBOL[name] + "_device"
    assert (c["ptr"], c["length"], c["fmt"]) == (0xABC000, 4321, int(am.Fmt.S16_STEREO))
    _check_single(c, name, k, peaks, needles[1]._h.value)
    assert _numbers(result, field, per) == _expect(k, per)
    # fmt defaults to f32 mono
    getattr(needles[1], "hit_" + name + "_device")(0xABC000, 4321, peaks, *extra)
    assert rec.calls[1]["fmt"] == int(am.Fmt.F32_MONO)


def test_negative_segments_reach_the_library(rig):
    """hit_segments sizes `out` with max(segments, 0) and passes the value on: the library refuses it, not Python."""
    rec, needles = rig
    peaks = _peaks(2)
    assert needles[0].hit_segments(HAYSTACKS["f32"], peaks, -1) == [[], []]
    assert needles[0].hit_segments_device(0x1, 50, peaks, -1) == [[], []]
    assert am.hit_segments_batch_device(needles[:1], [0x1], [50], [[peaks]], -1) == [[[[], []]]]
    for c in rec.calls:
        assert c["len_out"] == 1 and c["params"] == bytes(am.AmSegmentParams(0xFFFFFFFF, 4))


COUNTS = [[0, 1], [3, 2]]          # [haystack][needle]: ragged, one pair empty, cap = 3
CAP = 3


@pytest.mark.parametrize("name", NAMES)
def test_batch_form_ragged(rig, name):
    rec, needles = rig
    rtype, field, per, extra, params = FAMILIES[name]
    nn = k = 2
    ppp = [[_peaks(COUNTS[h][j], base=1000 * h + 100 * j) for j in range(nn)] for h in range(k)]
    result = getattr(am, "hit_" + name + "_batch_device")(needles, [0x7000, 0x8000], [111, 222], ppp, *extra,
                                                         fmt=am.Fmt.S16_STEREO)
    assert len(rec.calls) == 1
    c = rec.calls[0]
    assert c["name"] == SYMBOL[name] + "_batch_device"
    assert c["handles"] == [n._h.value for n in needles] and c["nn"] == nn
    assert (c["ptrs"], c["lengths"], c["k"], c["fmt"]) == ([0x7000, 0x8000], [111, 222], k, int(am.Fmt.S16_STEREO))
    assert c["cap"] == CAP and c["counts"] == [0, 1, 3, 2]
    table = [(0, 0, 0.0, 0.0)] * (CAP * k * nn)
    for h in range(k):
        for j in range(nn):
            for i, t in enumerate(_as_tuples(ppp[h][j])):
                table[(h * nn + j) * CAP + i] = t
    assert c["table"] == table
    assert c["params"] == params
    assert c["out_type"] is rtype and c["len_out"] == CAP * k * nn * (per or 1)
    assert len(result) == k and all(len(row) == nn for row in result)
    for h in range(k):
        for j in range(nn):
            assert _numbers(result[h][j], field, per) == _expect(COUNTS[h][j], per, first=(h * nn + j) * CAP)


@pytest.mark.parametrize("name", NAMES)
def test_batch_form_all_empty(rig, name):
    rec, needles = rig
    rtype, field, per, extra, params = FAMILIES[name]
    result = getattr(am, "hit_" + name + "_batch_device")(needles[:1], [0x7000], [111], [[[]]], *extra)
    assert result == [[[]]]
    assert len(rec.calls) == 1
    c = rec.calls[0]
    assert c["cap"] == 1 and c["counts"] == [0] and c["table"] == [(0, 0, 0.0, 0.0)]
    assert c["fmt"] == int(am.Fmt.F32_MONO) and c["params"] == params
    assert c["len_out"] == (per or 1)
