"""The CLI's --resample: a 44.1 kHz snippet against a 48 kHz and a 44.1 kHz main file.  Without the flag the rate
mismatch stops the run as before; with it both files get labels at the planted times, and the 44.1 kHz file's label
file is byte-identical to a run without the flag."""
import subprocess
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SNIP_SR, OTHER_SR = 44100, 48000
PLANTS = {SNIP_SR: (6.0, 33.0), OTHER_SR: (9.0, 37.5)}   # (away from the 20 s chunk boundaries)


def write_wav(path, rate, lr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(lr, dtype="<i2").tobytes())


def tones(rate, n, freqs, phases):
    t = np.arange(n, dtype=np.float64) / rate
    return np.sin(2 * np.pi * freqs[None, :] * t[:, None] + phases[None, :]).sum(axis=1)


def make_case(tmp_path):
    rng = np.random.default_rng(9)
    freqs, phases = rng.uniform(100.0, 6000.0, 100), rng.uniform(0, 2 * np.pi, 100)
    peak = np.abs(tones(SNIP_SR, 2 * SNIP_SR, freqs, phases)).max()
    snip = tones(SNIP_SR, 2 * SNIP_SR, freqs, phases) / peak * 8000
    write_wav(tmp_path / "snip.wav", SNIP_SR, np.repeat(np.rint(snip)[:, None], 2, axis=1).astype(np.int16))
    for rate, name in ((OTHER_SR, "hay48.wav"), (SNIP_SR, "hay44.wav")):
        n = 60 * rate
        planted = tones(rate, 2 * rate, freqs, phases) / peak * 8000
        hay = rng.standard_normal(n) * 0.1 * np.sqrt(np.mean(planted ** 2))      # 20 dB below the snippet
        for t in PLANTS[rate]:
            off = int(t * rate)
            hay[off:off + planted.size] += planted
        write_wav(tmp_path / name, rate, np.repeat(np.clip(np.rint(hay), -32768, 32767)[:, None], 2, axis=1).astype(np.int16))


def label_starts(text):
    """the segment boundaries of the label file: segment i runs from start_i + 7 s to start_{i+1}"""
    rows = [ln.split("\t") for ln in text.splitlines() if ln]
    return [float(r[0]) - 7.0 for r in rows] + ([float(rows[-1][1])] if rows else [])


def test_cli_resample(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    make_case(tmp_path)
    base = [cli, "--snippet", str(tmp_path / "snip.wav"), "--chunk-size", "20", "--distance", "10s", "-y"]
    out = subprocess.run(base + [str(tmp_path / "hay48.wav"), "--no-out"], capture_output=True, text=True)
    assert out.returncode == 3
    assert out.stderr == "sample rate of snippet (44100) and main file (48000) don't match\n"
    # the 44.1 kHz file alone, without the flag: the parent's path
    out = subprocess.run(base + [str(tmp_path / "hay44.wav"), "-o", str(tmp_path / "plain44.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    plain = (tmp_path / "plain44.txt").read_bytes()
    out = subprocess.run(base + ["--resample", str(tmp_path / "hay48.wav"), str(tmp_path / "hay44.wav")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.count("Offset") == 4, out.stdout
    assert (tmp_path / "hay44.txt").read_bytes() == plain
    for rate, name in ((OTHER_SR, "hay48.txt"), (SNIP_SR, "hay44.txt")):
        got = label_starts((tmp_path / name).read_text())
        assert len(got) == 2 and np.allclose(got, PLANTS[rate], atol=1.5 / rate), (name, got)
    out = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--resample" in out.stdout
