"""The CLI's --min-significance (per-hit significance, am_hit_significance) on two small WAV files: a noise snippet
planted in noise, which stands hundreds of standard deviations above its surroundings, and a windowed 440 Hz snippet
planted at 0.3 gain over a faint steady 440 Hz tone, whose exact NCC is high but which stands only 4.4 standard
deviations above a background that oscillates with the tone (numpy f64: z = 4.44)."""
import subprocess
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 8000
S, H, T = SR, 24 * SR, 8 * SR      # snippet, main file, plant (440 Hz * 8 s: a whole number of periods)


def write_wav(path, mono):
    lr = np.repeat(np.asarray(mono, dtype=np.int16), 2)          # both channels the same
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes(np.ascontiguousarray(lr, dtype="<i2").tobytes())
    return lr


def plant_case(tmp_path):
    rng = np.random.default_rng(5)
    nd = rng.integers(-3000, 3000, S)
    hay = rng.integers(-600, 600, H)
    hay[T:T + S] += nd
    return write_wav(tmp_path / "noise_snip.wav", nd), write_wav(tmp_path / "noise_main.wav", hay)


def tonal_case(tmp_path):
    rng = np.random.default_rng(6)
    i, n = np.arange(S), np.arange(H)
    nd = np.round(8000 * (0.5 - 0.5 * np.cos(2 * np.pi * (i + 0.5) / S)) * np.sin(2 * np.pi * 440 * i / SR)).astype(np.int64)
    hay = np.round(840 * np.sin(2 * np.pi * 440 * n / SR)).astype(np.int64) + rng.integers(-40, 40, H)
    hay[T:T + S] += np.round(0.3 * nd).astype(np.int64)
    return write_wav(tmp_path / "tone_snip.wav", nd), write_wav(tmp_path / "tone_main.wav", hay)


def label_text(starts):
    """format_labels(timelabel_from_peaks(...)) of the CLI."""
    return "".join("%.6f\t%.6f\tSegment %d\n" % (starts[i] / SR + 7.0, starts[i + 1] / SR, i + 1)
                   for i in range(len(starts) - 1))


def library_hits(gpu, needle_lr, hay_lr):
    """What the CLI computes, through the binding: the matcher's hits, their exact NCC and their z."""
    needle, hay = gpu.pcm_s16_stereo_to_mono(needle_lr), gpu.pcm_s16_stereo_to_mono(hay_lr)
    algo = gpu.HipConvolve(needle)
    p = gpu.Config(chunk_size_s=20.0, overlap_length_s=1.0, distance_s=10.0, prominence=0.13).params(SR, gpu.Scale.LIB)
    hits = algo.match(hay, p)
    return hits, algo.hit_scores(hay, hits), algo.hit_significance(hay, hits, S - 1, 3 * S)


def test_cli_min_significance(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    tail = ["--chunk-size", "20", "--distance", "10s", "-n"]
    # the plant in noise: kept
    hits, ncc, sig = library_hits(gpu, *plant_case(tmp_path))
    assert [q.start for q in hits] == [T] and sig[0].z > 100 and sig[0].flags == 0, (hits, sig)
    base = [cli, str(tmp_path / "noise_main.wav"), "--snippet", str(tmp_path / "noise_snip.wav")] + tail
    out = subprocess.run(base + ["--min-significance", "50", "--debug", "-o", str(tmp_path / "noise.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.count("Offset") == 1
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("hit ")]
    assert len(lines) == 1 and "(dropped)" not in lines[0], out.stdout
    assert all(w in lines[0] for w in (" score ", " mean ", " std ", " z ", " side_max ", " lag ")), lines[0]
    assert abs(float(lines[0].split(" z ")[1].split()[0]) - sig[0].z) <= 0.01
    assert int(lines[0].split(" lag ")[1].split()[0]) == sig[0].side_lag
    assert (tmp_path / "noise.txt").read_bytes() == label_text([T]).encode()
    # the tonal bait: every hit passes --min-confidence 0.5 and none --min-significance 50
    hits, ncc, sig = library_hits(gpu, *tonal_case(tmp_path))
    starts = [q.start for q in hits]
    assert T in starts and all(q.ncc >= 0.5 for q in ncc) and all(q.z < 50 for q in sig), (hits, ncc, sig)
    assert abs(sig[starts.index(T)].z - 4.44) < 0.2, sig
    base = [cli, str(tmp_path / "tone_main.wav"), "--snippet", str(tmp_path / "tone_snip.wav")] + tail
    out = subprocess.run(base + ["--min-confidence", "0.5", "-o", str(tmp_path / "conf.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.count("Offset") == len(starts) >= 1
    assert (tmp_path / "conf.txt").read_bytes() == label_text(starts).encode()
    out = subprocess.run(base + ["--min-significance", "50", "--debug", "-o", str(tmp_path / "sig.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.count("Offset") == 0
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("hit ")]
    assert len(lines) == len(starts) and all("(dropped)" in ln for ln in lines), out.stdout
    assert (tmp_path / "sig.txt").read_bytes() == label_text([]).encode()
    # a lower bound keeps it; the zone is a duration
    out = subprocess.run(base + ["--min-significance", "3", "--significance-zone", "3s", "--no-out"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.count("Offset") >= 1 and " side_max " not in out.stdout
