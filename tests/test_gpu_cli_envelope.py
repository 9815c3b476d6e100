"""The CLI's --envelope PCT[:STEPS[:MIN_SCORE]]: a snippet that occurs once 2 % short (played fast) and once as it is.  The
waveform match finds the second only (at a prominence of 50 %; at the default 13 % the fast one's first burst gives a weak
hit a second early); --envelope prints one line for each, the place played fast joins the label file,
and without the flag nothing changes."""
import re
import struct
import subprocess

import numpy as np
import pytest

import envelope_ref as er

pytestmark = pytest.mark.gpu

SR = 16000
AT_FAST, AT_PLAIN, DRIFT = 8 * SR + 77, 25 * SR, -20000.0
LINE = re.compile(r"^Envelope: (\d\d):(\d\d):(\d\d)\.(\d\d\d) speed ([+-]\d+\.\d\d) % score (-?\d\.\d\d\d)$")


def write_wav_f32(path, x):
    data = np.ascontiguousarray(x, dtype="<f4").tobytes()
    with open(str(path), "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 24 + 12 + 8 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 3, 1, SR, SR * 4, 4, 32))
        f.write(b"fact" + struct.pack("<II", 4, len(data) // 4))
        f.write(b"data" + struct.pack("<I", len(data)) + data)


def make_case(tmp_path):
    rng = np.random.default_rng(88)
    snip = er.burst_tones(rng, 4 * SR, SR)
    hay = 0.3 * er.burst_tones(rng, 40 * SR, SR) + 0.005 * rng.standard_normal(40 * SR)
    fast = er.stretch(snip, DRIFT)
    hay[AT_FAST:AT_FAST + len(fast)] += fast
    hay[AT_PLAIN:AT_PLAIN + len(snip)] += snip
    snip, hay = snip.astype(np.float32), hay.astype(np.float32)
    write_wav_f32(tmp_path / "snip.wav", snip)
    write_wav_f32(tmp_path / "hay.wav", hay)
    return snip, hay


def test_cli_envelope(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    snip, hay = make_case(tmp_path)
    labels, labels_env = tmp_path / "plain.txt", tmp_path / "env.txt"
    base = [cli, "--snippet", str(tmp_path / "snip.wav"), "--chunk-size", "20", "--distance", "10s", "-p", "50", "-y", str(tmp_path / "hay.wav")]
    plain = subprocess.run(base + ["-o", str(labels)], capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    assert [ln.split(" with ")[0] for ln in plain.stdout.splitlines() if ln.startswith("Offset")] == ["Offset 1: 00:00:25"], plain.stdout
    assert "Envelope" not in plain.stdout and labels.read_bytes() == b""             # one hit: no label, as before
    out = subprocess.run(base + ["-o", str(labels_env), "--envelope", "4:8"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines(keepends=True)
    env = [ln for ln in lines if ln.startswith("Envelope:")]
    # the flag adds its lines under the offset line and changes nothing else
    assert "".join(ln for ln in lines if ln not in env) == plain.stdout
    assert len(env) == 2 and lines.index(env[0]) == [i for i, ln in enumerate(lines) if ln.startswith("Offset")][-1] + 1, out.stdout
    # the lines are those of the library call
    ep = gpu.env_params(gpu.band_edges_log(SR, 10, 150.0, 6000.0, 8))
    algo = gpu.HipConvolve(snip)
    hits = algo.match_envelope(hay, ep, gpu.env_grid(40000.0, 8), 0.4)
    algo.close()
    assert hits.size == 2
    for ln, h in zip(env, hits):
        m = LINE.match(ln.rstrip("\n"))
        assert m, ln
        ms = int(int(h["start"]) * 1000.0 / SR)
        assert tuple(int(v) for v in m.groups()[:4]) == (ms // 3600000, ms // 60000 % 60, ms // 1000 % 60, ms % 1000)
        assert m.group(5) == "%+.2f" % (100.0 * (1.0 / (1.0 + float(h["drift_ppm"]) * 1e-6) - 1.0)) and m.group(6) == "%.3f" % float(h["score"])
    print("".join(env))
    # the place played fast: within 4 frames of the plant, its speed within two steps of +2.04 %
    assert abs(int(hits[0]["start"]) - AT_FAST) <= 4 * 512 and abs(float(hits[0]["drift_ppm"]) - DRIFT) <= 2 * 5000.0
    assert abs(int(hits[1]["start"]) - AT_PLAIN) <= 4 * 512
    # the label file: the place played fast joins the waveform hit, which is not listed twice
    rows = labels_env.read_text().splitlines()
    assert len(rows) == 1, rows
    start_s, end_s, name = rows[0].split("\t")
    assert start_s == "%.6f" % (int(hits[0]["start"]) / SR + 7.0) and abs(float(end_s) - AT_PLAIN / SR) <= 2.0 / SR and name == "Segment 1"
    # a bar above both scores: nothing printed, nothing added
    high = subprocess.run(base + ["--no-out", "--envelope", "4:8:0.99"], capture_output=True, text=True)
    assert high.returncode == 0 and "Envelope" not in high.stdout
    # refused values, on a live feed and with --discover
    for bad in ("0", "26", "4:0", "4:129", "4:8:2", "x"):
        r = subprocess.run(base + ["--no-out", "--envelope", bad], capture_output=True, text=True)
        assert r.returncode == 2 and "--envelope" in r.stderr, (bad, r.stderr)
    r = subprocess.run([cli, "--snippet", str(tmp_path / "snip.wav"), "--live", "--rate", "16000", "--envelope", "4"],
                       capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert r.returncode == 2 and "--live: --envelope does not apply" in r.stderr
    r = subprocess.run([cli, str(tmp_path / "hay.wav"), "--discover", "1s", "--envelope", "4"], capture_output=True, text=True)
    assert r.returncode == 2 and "--discover and --envelope are mutually exclusive" in r.stderr
    assert "--envelope PCT[:STEPS[:MIN_SCORE]]" in subprocess.run([cli, "--help"], capture_output=True, text=True).stdout
