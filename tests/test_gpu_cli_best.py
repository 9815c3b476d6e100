"""The CLI's --best N (am_match_best: the N best hits of each main file, no prominence threshold) on a WAV with three
planted copies of the snippet: the two strongest in start order, and with --normalize the copy in a quiet region."""
import subprocess
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 8000


def write_wav_stereo(path, lr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes(np.ascontiguousarray(lr, dtype="<i2").tobytes())


def make_case(tmp_path):
    rng = np.random.default_rng(7)
    s, h = 2 * SR, 70 * SR
    needle_lr = rng.integers(-8000, 8000, size=2 * s).astype(np.int32)
    hay_lr = rng.integers(-8000, 8000, size=2 * h).astype(np.int32)
    for t, g in ((5.0, 0.8), (31.0, 1.0), (55.5, 0.6)):
        off = int(t * SR)
        hay_lr[2 * off:2 * (off + s)] += np.rint(g * needle_lr).astype(np.int32)
    a, b = 2 * 25 * SR, 2 * 40 * SR             # the region of the copy at 31 s, 26 dB down
    hay_lr[a:b] = np.rint(hay_lr[a:b] * 10 ** (-26 / 20)).astype(np.int32)
    write_wav_stereo(tmp_path / "needle.wav", np.clip(needle_lr, -32768, 32767).astype(np.int16))
    write_wav_stereo(tmp_path / "hay.wav", np.clip(hay_lr, -32768, 32767).astype(np.int16))


def labels(path):
    """(start, end) of each label: label i runs from 7 s behind hit i to hit i + 1."""
    return [tuple(float(x) for x in row.split("\t")[:2]) for row in path.read_text().splitlines()]


def test_cli_best(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    make_case(tmp_path)
    base = [cli, str(tmp_path / "hay.wav"), "--snippet", str(tmp_path / "needle.wav"), "--distance", "10s", "-n"]
    out = subprocess.run(base + ["--best", "2", "-o", str(tmp_path / "raw.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.count("Offset") == 2
    assert labels(tmp_path / "raw.txt") == [(12.0, 55.5)]        # the copies at 5 s and 55.5 s, in start order
    out = subprocess.run(base + ["--best", "2", "--normalize", "-o", str(tmp_path / "ncc.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert labels(tmp_path / "ncc.txt") == [(12.0, 31.0)]        # by NCC the quiet copy at 31 s is among the best two
    out = subprocess.run(base + ["--best", "1", "--normalize", "-n", "--no-out"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.count("Offset") == 1 and "Offset 1: 00:00:31" in out.stdout, out.stdout   # ... and ranks first
    out = subprocess.run(base + ["--best", "3", "-o", str(tmp_path / "all.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert labels(tmp_path / "all.txt") == [(12.0, 31.0), (38.0, 55.5)]
    out = subprocess.run(base + ["--best", "0"], capture_output=True, text=True)
    assert out.returncode == 2 and "--best" in out.stderr
