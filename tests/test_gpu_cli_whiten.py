"""The CLI's --whiten and --preemphasis on coloured material: AR(1) noise (rho = 0.98) as the programme of two main
files, a snippet of the same colour planted twice in each.  Both flags report the planted offsets; --whiten over two
main files designs ONE filter, from the lag products of both, and finds the hits of both."""
import subprocess
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 8000
PLANTS = {"hay_a.wav": (6.0, 33.0), "hay_b.wav": (9.0, 37.5)}   # (away from the 20 s chunk boundaries)


def write_wav(path, mono_i16):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes(np.ascontiguousarray(np.repeat(mono_i16[:, None], 2, axis=1), dtype="<i2").tobytes())


def coloured(rng, n):
    signal = pytest.importorskip("scipy.signal")
    return signal.lfilter([1.0], [1.0, -0.98], rng.standard_normal(n + 2000))[2000:] * 800.0   # std about 4000


def make_case(tmp_path):
    rng = np.random.default_rng(12)
    snip = coloured(rng, 2 * SR)
    files = {"snip.wav": np.rint(snip).astype(np.int16)}
    for name, plants in PLANTS.items():
        hay = coloured(rng, 60 * SR)
        for t in plants:
            off = int(t * SR)
            hay[off:off + snip.size] += snip
        files[name] = np.clip(np.rint(hay), -32768, 32767).astype(np.int16)
    for name, data in files.items():
        write_wav(tmp_path / name, data)
    return files


def label_starts(text):
    """the segment boundaries of the label file: segment i runs from start_i + 7 s to start_{i+1}"""
    rows = [ln.split("\t") for ln in text.splitlines() if ln]
    return [float(r[0]) - 7.0 for r in rows] + ([float(rows[-1][1])] if rows else [])


def check_labels(tmp_path, names):
    for name in names:
        got = label_starts((tmp_path / name.replace(".wav", ".txt")).read_text())
        assert len(got) == 2 and np.allclose(got, PLANTS[name], atol=0.5 / SR), (name, got)


def clear_labels(tmp_path):
    for f in tmp_path.glob("*.txt"):
        f.unlink()


def offset_lines(stdout):
    return [ln for ln in stdout.splitlines() if ln.startswith("Offset")]


def test_cli_whiten_and_preemphasis(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    files = make_case(tmp_path)
    base = [cli, "--snippet", str(tmp_path / "snip.wav"), "--chunk-size", "20", "--distance", "10s", "-y"]
    hays = [str(tmp_path / name) for name in PLANTS]
    for flag in (["--whiten", "8"], ["--preemphasis", "0.95"]):
        clear_labels(tmp_path)
        out = subprocess.run(base + flag + hays[:1], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        lines = offset_lines(out.stdout)
        assert [ln.split(" with ")[0] for ln in lines] == ["Offset 1: 00:00:06", "Offset 2: 00:00:33"], out.stdout
        check_labels(tmp_path, ["hay_a.wav"])
    # two main files: one filter, designed from the lag products of both; the snippet is filtered once
    clear_labels(tmp_path)
    out = subprocess.run(base + ["--whiten", "8", "--debug"] + hays, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    shown = [ln for ln in out.stdout.splitlines() if ln.startswith("whitening filter:")]
    assert len(shown) == 1, out.stdout
    r = sum(gpu.lag_products(gpu.pcm_s16_stereo_to_mono(np.repeat(files[name][:, None], 2, axis=1)), 8) for name in PLANTS)
    taps = gpu.whiten_taps(r, 60.0)
    assert shown[0] == "whitening filter:" + "".join(" %.6g" % float(t) for t in taps)
    assert abs(taps[1] + 0.98) < 0.02
    assert [ln.split(" with ")[0] for ln in offset_lines(out.stdout)] == \
        ["Offset 1: 00:00:06", "Offset 2: 00:00:33", "Offset 1: 00:00:09", "Offset 2: 00:00:37"], out.stdout
    check_labels(tmp_path, list(PLANTS))
    # the flags are refused together and on a live feed
    out = subprocess.run(base + ["--whiten", "8", "--preemphasis", "0.9"] + hays[:1], capture_output=True, text=True)
    assert out.returncode == 2 and "mutually exclusive" in out.stderr
    out = subprocess.run([cli, "--snippet", str(tmp_path / "snip.wav"), "--live", "--rate", "8000", "--whiten", "8"],
                         capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert out.returncode == 2 and "--live: --whiten and --preemphasis do not apply" in out.stderr
    out = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--whiten P" in out.stdout and "--preemphasis A" in out.stdout
