"""The CLI's --segments (per-segment hit scoring, am_hit_segments) on a WAV with one whole plant of the snippet and one
that stops half way: each hit's offset line is followed by the presence mask of the snippet's parts."""
import subprocess
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 8000
WHOLE, HALF = 5.0, 31.0


def write_wav_stereo(path, lr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes(np.ascontiguousarray(lr, dtype="<i2").tobytes())


def make_case(tmp_path):
    rng = np.random.default_rng(8)
    s, h = 2 * SR, 50 * SR
    needle_lr = rng.integers(-300, 300, size=2 * s).astype(np.int16)
    hay_lr = rng.integers(-100, 100, size=2 * h).astype(np.int32)
    off = int(WHOLE * SR)
    hay_lr[2 * off:2 * (off + s)] += needle_lr
    off = int(HALF * SR)
    hay_lr[2 * off:2 * off + s] += needle_lr[:s]              # the first half of the snippet's frames only
    write_wav_stereo(tmp_path / "needle.wav", needle_lr)
    write_wav_stereo(tmp_path / "hay.wav", hay_lr.astype(np.int16))


def test_cli_segments_masks(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    make_case(tmp_path)
    base = [cli, str(tmp_path / "hay.wav"), "--snippet", str(tmp_path / "needle.wav"), "--chunk-size", "20", "--distance", "10s", "-n"]
    plain = subprocess.run(base + ["-o", str(tmp_path / "plain.txt")], capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    assert plain.stdout.count("Offset") == 2 and "segments" not in plain.stdout
    out = subprocess.run(base + ["--segments", "8", "-o", str(tmp_path / "seg.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    at = [i for i, ln in enumerate(lines) if "Offset" in ln]
    assert len(at) == 2
    after = [lines[i + 1] for i in at]
    assert after[0].startswith("  segments ######## coverage 1.000 drift_ppm "), after
    assert after[1].startswith("  segments ####.... coverage 0.500 drift_ppm "), after
    assert all(" start_lag " in ln for ln in after)
    assert [ln for ln in lines if "segments" not in ln] == plain.stdout.splitlines()   # nothing else changes
    assert (tmp_path / "seg.txt").read_bytes() == (tmp_path / "plain.txt").read_bytes()
    # several snippets: the same lines, prefixed by the snippet's name
    multi = subprocess.run(base + ["--snippet", str(tmp_path / "needle.wav"), "--segments", "8:2", "--no-out"], capture_output=True, text=True)
    assert multi.returncode == 0, multi.stderr
    assert multi.stdout.count("needle.wav:   segments ######## ") == 2 and multi.stdout.count("needle.wav:   segments ####.... ") == 2
    bad = subprocess.run(base + ["--segments", "8:17"], capture_output=True, text=True)
    assert bad.returncode == 2 and "--segments" in bad.stderr
