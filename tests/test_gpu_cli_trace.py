"""The CLI's --score-trace PREFIX[:BIN] on two WAV files and one snippet: each file's CSV reads back to the records of
am_match_trace (values written with %.9g), the 'Trace:' line is am_trace_summary of those records, and with
--normalize no bin's maximum lies above 1."""
import subprocess
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 8000
HEADER = "start_s,max,max_at_s,min,min_at_s,mean,rms,count"


def write_wav_stereo(path, lr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes(np.ascontiguousarray(lr, dtype="<i2").tobytes())


def make_case(tmp_path):
    """The snippet and two main files (its copies at 0.8 and 1.0, and at 0.6), as interleaved i16 stereo frames."""
    rng = np.random.default_rng(17)
    s = 2 * SR
    needle = rng.integers(-8000, 8000, size=(s, 2)).astype(np.int32)
    hays = []
    for secs, plants in ((30, ((5.0, 0.8), (21.25, 1.0))), (20, ((11.5, 0.6),))):
        hay = rng.integers(-8000, 8000, size=(secs * SR, 2)).astype(np.int32)
        for t, g in plants:
            off = int(t * SR)
            hay[off:off + s] += np.rint(g * needle).astype(np.int32)
        hays.append(np.clip(hay, -32768, 32767).astype(np.int16))
    needle = needle.astype(np.int16)
    write_wav_stereo(tmp_path / "needle.wav", needle)
    for i, h in enumerate(hays):
        write_wav_stereo(tmp_path / ("hay%d.wav" % i), h)
    return needle, hays


def csv_text(rec, D):
    """The file the CLI writes for the records `rec` of bins of D scores."""
    rows = [HEADER]
    for b, r in enumerate(rec):
        t0, c = float(b * D), float(r["count"])
        if r["count"]:
            vals = (t0 / SR, float(r["max"]), (t0 + float(r["argmax"])) / SR, float(r["min"]), (t0 + float(r["argmin"])) / SR,
                    float(r["sum"]) / c, float(np.sqrt(r["sumsq"] / c)))
        else:
            vals = (t0 / SR,) + (float("nan"),) * 6
        rows.append(",".join("%.9g" % v for v in vals) + ",%d" % r["count"])
    return "\n".join(rows) + "\n"


def trace_line(gpu, rec, D):
    st = gpu.trace_summary(rec, D)
    ms = int(float(st.argmax) * 1000.0 / SR)
    return "Trace: max %.9g at %02d:%02d:%02d.%03d, bin maxima median %.9g mad %.9g, peak z %.9g" % (
        st.max, ms // 3600000, ms // 60000 % 60, ms // 1000 % 60, ms % 1000, st.median_max, st.mad_max, st.peak_z)


def test_cli_score_trace(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    needle, hays = make_case(tmp_path)
    files = [str(tmp_path / "hay0.wav"), str(tmp_path / "hay1.wav")]
    base = [cli] + files + ["--snippet", str(tmp_path / "needle.wav"), "--best", "1", "--no-out", "-n"]
    monos = [gpu.pcm_s16_stereo_to_mono(h) for h in hays]
    for norm in (False, True):
        algo = gpu.HipConvolve(gpu.pcm_s16_stereo_to_mono(needle), score_norm=norm)
        for spec, D in (("", SR), (":250ms", SR // 4)):
            prefix = str(tmp_path / ("curve%d%s_" % (norm, spec.replace(":", "-"))))
            out = subprocess.run(base + ["--score-trace", prefix + spec] + (["--normalize"] if norm else []), capture_output=True, text=True)
            assert out.returncode == 0, out.stderr
            lines = [ln for ln in out.stdout.splitlines() if ln.startswith("Trace:")]
            assert len(lines) == 2, out.stdout
            for i, mono in enumerate(monos):
                rec = algo.match_trace(mono, D)
                text = open(prefix + "%d.csv" % i).read()
                assert text == csv_text(rec, D), (norm, spec, i)
                assert lines[i] == trace_line(gpu, rec, D), (norm, spec, i)
                # the values read back to the records' bits
                rows = [r.split(",") for r in text.splitlines()[1:]]
                assert len(rows) == rec.size == (mono.size - 2 * SR + 1 + D - 1) // D
                assert np.array_equal(np.array([r[1] for r in rows], dtype=np.float32), rec["max"])
                assert np.array_equal(np.array([r[3] for r in rows], dtype=np.float32), rec["min"])
                assert [int(r[7]) for r in rows] == [int(c) for c in rec["count"]]
                if norm:
                    assert float(rec["max"].max()) <= 1.0 + 4 * 2.0 ** -23
            # the trace line follows the file's offset lines
            body = out.stdout.splitlines()
            first = body.index(lines[0])
            assert any(ln.startswith("Offset") for ln in body[:first])
            assert "00:00:21.250" in lines[0] and "00:00:11.500" in lines[1]
        algo.close()
