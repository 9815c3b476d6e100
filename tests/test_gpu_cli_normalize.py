"""The CLI's --normalize (window-energy normalised scores, option "score_norm") on the WAV case of
test_gpu_cli.py with one hit's whole region -- jingle and background -- recorded 26 dB quieter."""
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
    rng = np.random.default_rng(5)
    s, h = 2 * SR, 70 * SR
    needle_lr = rng.integers(-8000, 8000, size=2 * s).astype(np.int16)
    hay_lr = rng.integers(-8000, 8000, size=2 * h).astype(np.int32)
    for t in (5.0, 31.0, 55.5):
        off = int(t * SR)
        hay_lr[2 * off:2 * (off + s)] += needle_lr
    g = 10 ** (-26 / 20)
    a, b = 2 * 25 * SR, 2 * 40 * SR             # the region of the hit at 31 s, 26 dB down
    hay_lr[a:b] = np.rint(hay_lr[a:b] * g).astype(np.int32)
    hay_lr = np.clip(hay_lr, -32768, 32767).astype(np.int16)
    write_wav_stereo(tmp_path / "needle.wav", needle_lr)
    write_wav_stereo(tmp_path / "hay.wav", hay_lr)


def labels(path):
    return [float(row.split("\t")[0]) for row in path.read_text().splitlines()]


def test_cli_normalize_finds_quiet_hit(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    make_case(tmp_path)
    base = [cli, str(tmp_path / "hay.wav"), "--snippet", str(tmp_path / "needle.wav"), "--chunk-size", "20", "--distance", "10s", "-n"]
    out = subprocess.run(base + ["-o", str(tmp_path / "lib.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    starts = labels(tmp_path / "lib.txt")            # label i starts 7 s behind hit i
    assert all(abs(x - 38.0) > 1e-3 for x in starts), starts     # the quiet hit is missed by the default scores
    out = subprocess.run(base + ["--normalize", "-o", str(tmp_path / "ncc.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.count("Offset") == 3
    starts = labels(tmp_path / "ncc.txt")
    assert any(abs(x - 38.0) < 1e-3 for x in starts), starts
    out = subprocess.run(base + ["--normalize", "--normalize-floor", "300"], capture_output=True, text=True)
    assert out.returncode == 2 and "--normalize-floor" in out.stderr
