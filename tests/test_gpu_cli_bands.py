"""The CLI's --bands (per-band hit scoring, am_hit_bands) on a WAV that holds the snippet once as it is and once
low-passed: each hit's offset line is followed by the presence mask of the snippet's frequency bands."""
import re
import subprocess
import wave

import numpy as np
import pytest

import hit_bands_ref as ref

pytestmark = pytest.mark.gpu

SR = 8000
WHOLE, LOWPASSED = 5.0, 31.0
CUTOFF = 362 / 2048          # cycles per sample: between the edges 342 and 592 of the eight bands at F = 2048


def write_wav_mono_as_stereo(path, mono):
    lr = np.repeat(np.asarray(mono, dtype="<i2"), 2)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes(lr.tobytes())


def make_case(tmp_path):
    rng = np.random.default_rng(8)
    s, h = 2 * SR, 50 * SR
    needle = rng.integers(-3000, 3000, size=s).astype(np.int16)
    k = np.arange(255) - 127
    taps = 2 * CUTOFF * np.sinc(2 * CUTOFF * k) * np.hamming(255)
    low = np.rint(np.convolve(needle.astype(np.float64), taps, mode="same")).astype(np.int32)
    hay = rng.integers(-1000, 1000, size=h).astype(np.int32)
    t1, t2 = int(WHOLE * SR), int(LOWPASSED * SR)
    hay[t1:t1 + s] += needle
    hay[t2:t2 + s] += low
    write_wav_mono_as_stereo(tmp_path / "needle.wav", needle)
    write_wav_mono_as_stereo(tmp_path / "hay.wav", hay.astype(np.int16))
    return needle.astype(np.float32), hay.astype(np.float32), t1, t2


def test_cli_bands_masks(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    needle, hay, t1, t2 = make_case(tmp_path)
    # what the checker says about the two plants (the level of the samples does not matter to a coherence): every band
    # is clearly present or clearly absent
    edges = ref.edges_log_ref(SR, 11, 50.0, 4000.0, 8)
    masks = []
    for t in (t1, t2):
        exp = ref.bands_ref(hay, needle, t, 11, edges)
        assert all(q.flags == 0 and not 0.35 <= q.coherence <= 0.65 for q in exp), exp
        masks.append("".join("#" if q.coherence >= 0.5 else "." for q in exp))
    assert masks == ["########", "######.."]
    base = [cli, str(tmp_path / "hay.wav"), "--snippet", str(tmp_path / "needle.wav"), "--chunk-size", "20", "--distance", "10s", "-n"]
    plain = subprocess.run(base + ["-o", str(tmp_path / "plain.txt")], capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    assert plain.stdout.count("Offset") == 2 and "bands" not in plain.stdout
    out = subprocess.run(base + ["--bands", "8", "-o", str(tmp_path / "bands.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    at = [i for i, ln in enumerate(lines) if "Offset" in ln]
    assert len(at) == 2
    after = [lines[i + 1] for i in at]
    assert after[0].startswith("  bands ######## coverage 1.000 coherence "), after
    assert after[1].startswith("  bands ######.. coverage "), after
    assert all(re.fullmatch(r"  bands [#.]{8} coverage \d\.\d{3} coherence \d\.\d{3} gain_db_spread \d+\.\d", ln) for ln in after), after
    assert [ln for ln in lines if "  bands " not in ln] == plain.stdout.splitlines()   # the offset lines are byte-identical
    assert (tmp_path / "bands.txt").read_bytes() == (tmp_path / "plain.txt").read_bytes()
    # with --segments both lines follow the offset line; several snippets: the same lines, prefixed by the snippet's name
    both = subprocess.run(base + ["--bands", "8:10", "--segments", "4", "--no-out"], capture_output=True, text=True)
    assert both.returncode == 0, both.stderr
    lines = both.stdout.splitlines()
    at = [i for i, ln in enumerate(lines) if "Offset" in ln]
    assert all(lines[i + 1].startswith("  segments ") and lines[i + 2].startswith("  bands ") for i in at), lines
    multi = subprocess.run(base + ["--snippet", str(tmp_path / "needle.wav"), "--bands", "8", "--no-out"], capture_output=True, text=True)
    assert multi.returncode == 0, multi.stderr
    assert multi.stdout.count("needle.wav:   bands ######## ") == 2 and multi.stdout.count("needle.wav:   bands ######.. ") == 2
    bad = subprocess.run(base + ["--bands", "8:13"], capture_output=True, text=True)
    assert bad.returncode == 2 and "--bands" in bad.stderr
