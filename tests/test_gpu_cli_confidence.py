"""The CLI's --min-confidence (per-hit scoring, am_hit_scores) on the WAV case of test_gpu_cli_normalize.py plus one
loud burst of uncorrelated noise: its LibConvolve height passes the default prominence, its exact NCC does not."""
import subprocess
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 8000
PLANTS = (5.0, 31.0, 55.5)


def write_wav_stereo(path, lr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes(np.ascontiguousarray(lr, dtype="<i2").tobytes())


def make_case(tmp_path):
    rng = np.random.default_rng(5)
    s, h = 2 * SR, 70 * SR
    needle_lr = rng.integers(-300, 300, size=2 * s).astype(np.int16)
    hay_lr = rng.integers(-300, 300, size=2 * h).astype(np.int32)
    for t in PLANTS:
        off = int(t * SR)
        hay_lr[2 * off:2 * (off + s)] += needle_lr
    a, b = 2 * 43 * SR, 2 * 44 * SR          # the decoy: one second of loud noise, more than 10 s from every plant
    hay_lr[a:b] = rng.integers(-30000, 30000, size=b - a)
    hay_lr = np.clip(hay_lr, -32768, 32767).astype(np.int16)
    write_wav_stereo(tmp_path / "needle.wav", needle_lr)
    write_wav_stereo(tmp_path / "hay.wav", hay_lr)
    return needle_lr, hay_lr


def label_text(starts):
    """format_labels(timelabel_from_peaks(...)) of the CLI: what the unfiltered run writes."""
    return "".join("%.6f\t%.6f\tSegment %d\n" % (starts[i] / SR + 7.0, starts[i + 1] / SR, i + 1)
                   for i in range(len(starts) - 1))


def test_cli_min_confidence_drops_decoy(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    needle_lr, hay_lr = make_case(tmp_path)
    # the parent's CLI logic: match, no filter
    needle = gpu.pcm_s16_stereo_to_mono(needle_lr)
    hay = gpu.pcm_s16_stereo_to_mono(hay_lr)
    p = gpu.Config(chunk_size_s=20.0, overlap_length_s=2.0, distance_s=10.0, prominence=0.13).params(SR, gpu.Scale.LIB)
    ref = [q.start for q in gpu.HipConvolve(needle).match(hay, p)]
    plants = [int(t * SR) for t in PLANTS]
    assert len(ref) == 4 and set(plants) < set(ref), ref          # the decoy passes the default prominence
    base = [cli, str(tmp_path / "hay.wav"), "--snippet", str(tmp_path / "needle.wav"), "--chunk-size", "20", "--distance", "10s", "-n"]
    out = subprocess.run(base + ["-o", str(tmp_path / "all.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.count("Offset") == 4 and "ncc" not in out.stdout
    assert (tmp_path / "all.txt").read_bytes() == label_text(ref).encode()
    out = subprocess.run(base + ["--min-confidence", "0.5", "-o", str(tmp_path / "conf.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.count("Offset") == 3
    assert (tmp_path / "conf.txt").read_bytes() == label_text(plants).encode()
    out = subprocess.run(base + ["--min-confidence", "0.5", "--debug", "--no-out"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("hit ")]
    assert len(lines) == 4 and sum("(dropped)" in ln for ln in lines) == 1, out.stdout
    assert all(" ncc " in ln and " gain " in ln and " dB" in ln for ln in lines)
    out = subprocess.run(base + ["--min-confidence", "1.5"], capture_output=True, text=True)
    assert out.returncode == 2 and "--min-confidence" in out.stderr
