"""The CLI's --learn-needle: three small main files with one planted occurrence of the snippet each, under different
material.  The run writes a mono float WAV of the snippet's length whose samples are estimate_needle on the rows of the
three hits (scale = 1 / gain of am_hit_scores); the option is refused on a live feed."""
import struct
import subprocess
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 8000
SNIP = SR             # one second
HAY = 10 * SR
PLANTS = {"hay_a.wav": (23457, 1.0), "hay_b.wav": (40001, 0.7), "hay_c.wav": (51234, 1.3)}   # (offset, gain)


def write_wav(path, mono_i16):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes(np.ascontiguousarray(np.repeat(mono_i16[:, None], 2, axis=1), dtype="<i2").tobytes())


def read_float_wav(path):
    """(format tag, channels, rate, bits, samples) of a RIFF/WAVE file, chunk by chunk"""
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:12] == b"WAVE" and struct.unpack("<I", b[4:8])[0] == len(b) - 8
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(b):
        cid, size = b[pos:pos + 4], struct.unpack("<I", b[pos + 4:pos + 8])[0]
        if cid == b"fmt ":
            fmt = struct.unpack("<HHIIHH", b[pos + 8:pos + 24])
        elif cid == b"data":
            data = np.frombuffer(b[pos + 8:pos + 8 + size], dtype="<f4")
        pos += 8 + size + (size & 1)
    return fmt[0], fmt[1], fmt[2], fmt[5], data


def make_case(tmp_path):
    rng = np.random.default_rng(8)
    snip = rng.uniform(-6000, 6000, SNIP)
    files = {"snip.wav": np.rint(snip).astype(np.int16)}
    for name, (off, gain) in PLANTS.items():
        hay = rng.uniform(-300, 300, HAY)
        hay[off:off + SNIP] += gain * snip
        over = off + int(rng.integers(0, SNIP // 2))          # a loud overlay on part of this occurrence
        hay[over:over + SNIP // 4] += rng.uniform(-6000, 6000, SNIP // 4)
        files[name] = np.clip(np.rint(hay), -32768, 32767).astype(np.int16)
    for name, data in files.items():
        write_wav(tmp_path / name, data)
    return files


def test_cli_learn_needle(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    files = make_case(tmp_path)
    out_wav = tmp_path / "learned.wav"
    base = [cli, "--snippet", str(tmp_path / "snip.wav"), "--chunk-size", "20", "--distance", "5s", "--no-out"]
    hays = [str(tmp_path / name) for name in PLANTS]
    run = subprocess.run(base + ["--learn-needle", f"{out_wav}:median", "--learn-margin", "0"] + hays, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    offsets = [ln for ln in run.stdout.splitlines() if ln.startswith("Offset")]
    assert [ln.split(" with ")[0] for ln in offsets] == ["Offset 1: 00:00:02", "Offset 1: 00:00:05", "Offset 1: 00:00:06"], run.stdout
    assert f"learned needle: 3 hits, {SNIP} samples at {SR} Hz" in run.stdout
    spread = [ln for ln in run.stdout.splitlines() if ln.startswith("  second ")]
    assert len(spread) == 1 and spread[0].startswith("  second 0: spread 0."), run.stdout
    tag, channels, rate, bits_, got = read_float_wav(out_wav)
    assert (tag, channels, rate, bits_) == (3, 1, SR, 32) and got.size == SNIP
    # the same rows through the binding: the files as the CLI reads them, the planted offsets, 1 / gain of am_hit_scores
    mono = {name: gpu.pcm_s16_stereo_to_mono(np.repeat(data[:, None], 2, axis=1)) for name, data in files.items()}
    algo = gpu.HipConvolve(mono["snip.wav"])
    rows = []
    try:
        for name, (off, _) in PLANTS.items():
            score = algo.hit_scores(mono[name], [gpu.Peak(off, off + 1, 1.0, 1.0)])[0]
            assert score.gain > 0 and score.flags & 6 == 0
            rows.append(gpu.hit_window(mono[name], off, np.float32(1.0) / np.float32(score.gain), 0, SNIP))
    finally:
        algo.close()
    est, dev, cnt = gpu.estimate_needle(np.stack(rows), gpu.Est.MEDIAN)
    assert np.array_equal(got.view(np.uint32), est.view(np.uint32))
    assert (cnt == 3).all()
    # the learned needle is a snippet the CLI reads: the next run finds the same offsets with it
    again = subprocess.run([cli, "--snippet", str(out_wav), "--chunk-size", "20", "--distance", "5s", "--no-out", hays[0]],
                           capture_output=True, text=True)
    assert again.returncode == 0 and "Offset 1: 00:00:02" in again.stdout, again.stderr + again.stdout
    # refused on a live feed, with --best and with several snippets
    live = subprocess.run([cli, "--snippet", str(tmp_path / "snip.wav"), "--live", "--rate", "8000", "--learn-needle", str(out_wav)],
                          capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert live.returncode == 2 and "--live: --learn-needle does not apply" in live.stderr
    best = subprocess.run(base + ["--learn-needle", str(out_wav), "--best", "2"] + hays[:1], capture_output=True, text=True)
    assert best.returncode == 2 and "--learn-needle and --best are mutually exclusive" in best.stderr
    two = subprocess.run(base + ["--snippet", str(tmp_path / "snip.wav"), "--learn-needle", str(out_wav)] + hays[:1], capture_output=True, text=True)
    assert two.returncode == 2 and "--learn-needle takes one --snippet only" in two.stderr
