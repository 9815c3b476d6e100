"""`audiomatch --live`: the body of a WAV fed through a pipe gives the file mode's offsets and label file, and the first
hit's line arrives while the input is still open."""
import os
import select
import subprocess
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 8000
HITS = (5.0, 19.0, 31.5, 52.25)


def write_wav_stereo(path, lr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes(np.ascontiguousarray(lr, dtype="<i2").tobytes())


def split(line):
    """'Offset i: hh:mm:ss with prominence p' -> (the line up to p, p)"""
    head, p = line.rsplit(" ", 1)
    return head, float(p)


def test_live_matches_file_mode(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    rng = np.random.default_rng(9)
    s, h = SR, 60 * SR + 300
    needle_lr = rng.integers(-8000, 8000, size=2 * s).astype(np.int16)
    hay_lr = rng.integers(-8000, 8000, size=2 * h).astype(np.int32)
    for t in HITS:
        off = int(t * SR)
        hay_lr[2 * off:2 * (off + s)] += needle_lr
    hay_lr = np.clip(hay_lr, -32768, 32767).astype(np.int16)
    write_wav_stereo(tmp_path / "needle.wav", needle_lr)
    write_wav_stereo(tmp_path / "hay.wav", hay_lr)
    opts = ["--snippet", str(tmp_path / "needle.wav"), "--chunk-size", "4", "--distance", "3s"]
    ref = subprocess.run([cli, str(tmp_path / "hay.wav"), *opts, "-o", str(tmp_path / "file.txt"), "-y"],
                         capture_output=True, text=True, timeout=120)
    assert ref.returncode == 0, ref.stderr
    ref_lines = [l for l in ref.stdout.splitlines() if l.startswith("Offset")]
    assert len(ref_lines) == len(HITS)

    body = hay_lr.tobytes()
    proc = subprocess.Popen([cli, "--live", *opts, "--rate", str(SR), "--encoding", "s16le", "--channels", "2",
                             "-o", str(tmp_path / "live.txt")], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE)
    try:
        half = 4 * 30 * SR                     # 30 s: the hit at 5 s is final once 3 s of audio lie behind its group
        for a in range(0, half, 4 * 1152):
            proc.stdin.write(body[a:min(half, a + 4 * 1152)])
        proc.stdin.flush()
        ready, _, _ = select.select([proc.stdout], [], [], 60)
        assert ready, "no line while the input is still open"
        first = b""
        while not first.endswith(b"\n"):      # byte by byte from the pipe: nothing of the later lines is buffered here
            c = os.read(proc.stdout.fileno(), 1)
            assert c, "output ended before the first line"
            first += c
        first = first.decode().rstrip("\n")
        assert first.startswith("Offset 1: 00:00:05"), first
        rest, err = proc.communicate(input=body[half:], timeout=120)   # the rest, then end of input
    finally:
        if proc.poll() is None:
            proc.kill()
    assert proc.returncode == 0, err.decode()
    live_lines = [first] + [l for l in rest.decode().splitlines() if l.startswith("Offset")]
    assert len(live_lines) == len(ref_lines)
    for a, b in zip(live_lines, ref_lines):
        (ha, pa), (hb, pb) = split(a), split(b)
        assert ha == hb                        # number and time: exact
        assert abs(pa - pb) <= 1e-5 * max(1.0, abs(pb))   # prominence: f32 rounding (a group's blocks start at the group)
    assert (tmp_path / "live.txt").read_bytes() == (tmp_path / "file.txt").read_bytes()
    assert len((tmp_path / "live.txt").read_text().splitlines()) == len(HITS) - 1


def test_live_argument_errors(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    for args, msg in ((["--live", "--snippet", "a.wav"], "--rate"),
                      (["--live", "--snippet", "a.wav", "--rate", "8000", "x.wav"], "no FILE"),
                      (["--live", "--snippet", "a.wav", "--rate", "8000", "--encoding", "f32le"], "one channel"),
                      (["--live", "--snippet", "a.wav", "--rate", "8000", "--channels", "3"], "--channels")):
        r = subprocess.run([cli, *args], capture_output=True, text=True, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr)
    assert not os.path.exists(tmp_path / "live.txt")
