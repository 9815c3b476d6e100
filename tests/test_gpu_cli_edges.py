"""The CLI's --edges DUR[:MIN_NCC[:MAX_SECOND]] (am_match_edges) on a WAV that begins 40 % into the snippet and ends 30 %
into another occurrence, with two whole occurrences in between: both tagged offset lines and both labels appear with the
flag; without it the output is what it was before the flag existed, byte for byte."""
import re
import subprocess
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 8000
S, H = 4 * SR, 30 * SR
HEAD_MISSING, TAIL_KEPT = 4 * S // 10, 3 * S // 10


def write_wav_stereo(path, lr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes(np.ascontiguousarray(lr, dtype="<i2").tobytes())


def make_case(tmp_path):
    rng = np.random.default_rng(17)
    needle_lr = rng.integers(-8000, 8000, size=2 * S).astype(np.int32)
    hay_lr = rng.integers(-3000, 3000, size=2 * H).astype(np.int32)
    hay_lr[:2 * (S - HEAD_MISSING)] += needle_lr[2 * HEAD_MISSING:]          # the file begins 40 % into the snippet
    hay_lr[2 * (H - TAIL_KEPT):] += needle_lr[:2 * TAIL_KEPT]                  # ... and ends 30 % into another occurrence
    for t in (8.0, 19.0):
        off = int(t * SR)
        hay_lr[2 * off:2 * (off + S)] += needle_lr
    write_wav_stereo(tmp_path / "needle.wav", np.clip(needle_lr, -32768, 32767).astype(np.int16))
    write_wav_stereo(tmp_path / "hay.wav", np.clip(hay_lr, -32768, 32767).astype(np.int16))


def test_cli_edges(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    make_case(tmp_path)
    base = [cli, str(tmp_path / "hay.wav"), "--snippet", str(tmp_path / "needle.wav"), "--distance", "5s", "-n"]
    plain = subprocess.run(base + ["-o", str(tmp_path / "plain.txt")], capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    # the parent's format: offset lines only, and one label from 7 s behind the first hit to the second
    assert re.fullmatch(r"Offset 1: 00:00:08 with prominence \S+\nOffset 2: 00:00:19 with prominence \S+\n", plain.stdout), plain.stdout
    plain_labels = (tmp_path / "plain.txt").read_bytes()
    assert plain_labels == b"15.000000\t19.000000\tSegment 1\n"
    out = subprocess.run(base + ["--edges", "500ms", "-o", str(tmp_path / "edges.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith(plain.stdout)
    extra = out.stdout[len(plain.stdout):].splitlines()
    assert len(extra) == 2, out.stdout
    assert re.fullmatch(r"Offset head: -00:00:01\.600 with ncc 0\.\d{3} overlap 60 %", extra[0]), extra
    assert re.fullmatch(r"Offset tail: 00:00:28\.800 with ncc 0\.\d{3} overlap 30 %", extra[1]), extra
    assert all(float(ln.split("ncc ")[1].split()[0]) >= 0.8 for ln in extra), extra
    got = (tmp_path / "edges.txt").read_bytes()
    assert got == plain_labels + b"0.000000\t2.400000\thead 60 %\n28.800000\t30.000000\ttail 30 %\n", got
    # a threshold nothing reaches: the plain output again, byte for byte
    none = subprocess.run(base + ["--edges", "500ms:0.999", "-o", str(tmp_path / "none.txt")], capture_output=True, text=True)
    assert none.returncode == 0 and none.stdout == plain.stdout and (tmp_path / "none.txt").read_bytes() == plain_labels
    # an overlap longer than either edge holds
    long_ = subprocess.run(base + ["--edges", "3s", "--no-out"], capture_output=True, text=True)
    assert long_.returncode == 0 and long_.stdout == plain.stdout
    for bad in ("0s", "1s:2", "1s:0.5:-1", "x"):
        r = subprocess.run(base + ["--edges", bad, "--no-out"], capture_output=True, text=True)
        assert r.returncode == 2 and "--edges" in r.stderr, (bad, r.stderr)
    r = subprocess.run([cli, "--live", "--rate", "8000", "--snippet", str(tmp_path / "needle.wav"), "--edges", "1s"], capture_output=True, text=True,
                       stdin=subprocess.DEVNULL)
    assert r.returncode == 2 and "--edges" in r.stderr
