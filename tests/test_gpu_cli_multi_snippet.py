"""The CLI with --snippet given several times (one am_match_multi_varlen per main file): the label file equals
timelabel_from_peaks over the merged hits of the single-snippet runs, with --resample and --min-confidence too; a
single --snippet writes what it always wrote."""
import subprocess
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 8000
# snippet frames and their plants (seconds, off the 20 s chunk edges); snippets 0 and 2 share the start at 41 s
SNIPS = ((1 * SR, (5.0, 25.0, 41.0)), (2 * SR, (12.0, 47.5)), (SR + SR // 2 + 1, (21.0, 41.0, 61.0)))


def write_wav_stereo(path, lr, sr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(lr, dtype="<i2").tobytes())


def make_case(tmp_path, decoy=False):
    rng = np.random.default_rng(17)
    h = 80 * SR
    hay = rng.integers(-300, 300, size=2 * h).astype(np.int32)
    snips = []
    for j, (s, plants) in enumerate(SNIPS):
        lr = rng.integers(-300, 300, size=2 * s).astype(np.int16)
        for t in plants:
            off = int(t * SR)
            hay[2 * off:2 * (off + s)] += lr
        write_wav_stereo(tmp_path / f"snip{j}.wav", lr, SR)
        snips.append(lr)
    if decoy:                                   # one second of loud noise, far from every plant
        a, b = 2 * 70 * SR, 2 * 71 * SR
        hay[a:b] = rng.integers(-30000, 30000, size=b - a)
    hay = np.clip(hay, -32768, 32767).astype(np.int16)
    write_wav_stereo(tmp_path / "hay.wav", hay, SR)
    return snips, hay


def label_text(starts):
    return "".join("%.6f\t%.6f\tSegment %d\n" % (starts[i] / SR + 7.0, starts[i + 1] / SR, i + 1)
                   for i in range(len(starts) - 1))


def params(gpu, overlap):
    p = gpu.Config(chunk_size_s=20.0, overlap_length_s=1.0, distance_s=10.0, prominence=0.13).params(SR, gpu.Scale.LIB)
    p.overlap = int(overlap)
    return p


def run(cli, tmp_path, hay_name, snips, *extra):
    args = [cli, str(tmp_path / hay_name)]
    for name in snips:
        args += ["--snippet", str(tmp_path / name)]
    out = subprocess.run(args + ["--chunk-size", "20", "--distance", "10s", "-n", *extra], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return out.stdout


def test_cli_several_snippets(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    snips, hay_lr = make_case(tmp_path)
    hay = gpu.pcm_s16_stereo_to_mono(hay_lr)
    algos = [gpu.HipConvolve(gpu.pcm_s16_stereo_to_mono(lr)) for lr in snips]
    single = [[q.start for q in a.match(hay, params(gpu, lr.size // 2))] for a, lr in zip(algos, snips)]
    for j, (_, plants) in enumerate(SNIPS):
        assert single[j] == [int(t * SR) for t in plants], (j, single[j])
    # one snippet: the label file of the single run, as always
    for j in range(3):
        run(cli, tmp_path, "hay.wav", [f"snip{j}.wav"], "-o", str(tmp_path / f"one{j}.txt"))
        assert (tmp_path / f"one{j}.txt").read_bytes() == label_text(single[j]).encode()
    # two and three snippets of different lengths: the merged hits
    for names in (["snip0.wav", "snip1.wav"], ["snip0.wav", "snip1.wav", "snip2.wav"], ["snip2.wav", "snip0.wav"]):
        idx = [int(n[4]) for n in names]
        labels = tmp_path / ("multi_" + "".join(map(str, idx)) + ".txt")   # (a fresh file: -n keeps an existing one)
        out = run(cli, tmp_path, "hay.wav", names, "-o", str(labels))
        merged = sorted(s for j in idx for s in single[j])
        assert labels.read_bytes() == label_text(merged).encode()
        for j in idx:
            assert sum(ln.startswith(f"snip{j}.wav: Offset ") for ln in out.splitlines()) == len(single[j]), out


def test_cli_several_snippets_resample_and_confidence(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    snips, hay_lr = make_case(tmp_path, decoy=True)
    hay = gpu.pcm_s16_stereo_to_mono(hay_lr)
    # snippet 1 at 16 kHz: --resample brings it to the main file's rate
    lr16 = np.repeat(snips[1].reshape(-1, 2), 2, axis=0).reshape(-1)
    write_wav_stereo(tmp_path / "snip1_16k.wav", lr16, 2 * SR)
    names = ["snip0.wav", "snip1_16k.wav", "snip2.wav"]
    algos = [gpu.HipConvolve(gpu.pcm_s16_stereo_to_mono(snips[0])),
             gpu.HipConvolve.resampled(gpu.pcm_s16_stereo_to_mono(lr16), 2 * SR, SR),
             gpu.HipConvolve(gpu.pcm_s16_stereo_to_mono(snips[2]))]
    hits = [a.match(hay, params(gpu, a.sample_len)) for a in algos]
    assert set(int(t * SR) for t in SNIPS[0][1]) <= set(q.start for q in hits[0])
    out = subprocess.run([cli, str(tmp_path / "hay.wav"), "--snippet", str(tmp_path / "snip0.wav"), "--snippet",
                          str(tmp_path / "snip1_16k.wav"), "--chunk-size", "20", "--distance", "10s", "-n", "--no-out"],
                         capture_output=True, text=True)
    assert out.returncode == 3 and "sample rate" in out.stderr
    run(cli, tmp_path, "hay.wav", names, "--resample", "-o", str(tmp_path / "rs.txt"))
    merged = sorted(q.start for h in hits for q in h)
    assert (tmp_path / "rs.txt").read_bytes() == label_text(merged).encode()
    # --min-confidence: each snippet's hits scored with that snippet's handle
    kept = []
    for a, h in zip(algos, hits):
        sc = a.hit_scores(hay, h)
        kept.append([q.start for q, s in zip(h, sc) if s.ncc >= 0.5])
    assert sum(len(k) for k in kept) < len(merged)     # the decoy is dropped
    run(cli, tmp_path, "hay.wav", names, "--resample", "--min-confidence", "0.5", "-o", str(tmp_path / "conf.txt"))
    assert (tmp_path / "conf.txt").read_bytes() == label_text(sorted(s for k in kept for s in k)).encode()
