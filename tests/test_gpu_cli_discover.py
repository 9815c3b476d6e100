"""The CLI's --discover DUR[:HOP] on the two noise designs of test_gpu_discover.py, written as 32-bit float WAV files at
8 kHz (256 ms = 2048 samples, 128 ms = 1024): the printed regions, the cut --discover-out writes, and that the cut works
as --snippet as it is -- with --normalize it finds the occurrence in B, and both occurrences in X."""
import re
import struct
import subprocess

import numpy as np
import pytest

import discover_ref as dr

pytestmark = pytest.mark.gpu

SR = 8000
LINE = re.compile(r"^Region: (\d\d:\d\d:\d\d\.\d\d\d) \+(\d+\.\d\d\d)s -> (.*) (\d\d:\d\d:\d\d\.\d\d\d), ncc mean (\d\.\d\d\d) min (\d\.\d\d\d), (\d+)/(\d+) probes$")


def write_wav_f32(path, x):
    data = np.ascontiguousarray(x, dtype="<f4").tobytes()
    with open(str(path), "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 24 + 12 + 8 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 3, 1, SR, SR * 4, 4, 32))
        f.write(b"fact" + struct.pack("<II", 4, len(data) // 4))
        f.write(b"data" + struct.pack("<I", len(data)) + data)


def read_wav_f32(path):
    raw = open(str(path), "rb").read()
    at = raw.index(b"data")
    n = struct.unpack("<I", raw[at + 4:at + 8])[0]
    assert raw[:4] == b"RIFF" and struct.unpack("<H", raw[20:22])[0] == 3 and struct.unpack("<I", raw[24:28])[0] == SR
    return np.frombuffer(raw[at + 8:at + 8 + n], dtype="<f4")


def stamp(sample):
    ms = int(sample * 1000.0 / SR)
    return "%02d:%02d:%02d.%03d" % (ms // 3600000, ms // 60000 % 60, ms // 1000 % 60, ms % 1000)


def regions_of(stdout):
    return [LINE.match(ln).groups() for ln in stdout.splitlines() if ln.startswith("Region:")]


def offsets(stdout):
    return [ln.split(" with ")[0] for ln in stdout.splitlines() if ln.startswith("Offset")]


def test_cli_discover_pair(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    a, b = dr.pair_design()
    fa, fb = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    write_wav_f32(fa, a)
    write_wav_f32(fb, b)
    prefix = str(tmp_path / "cut")
    out = subprocess.run([cli, fa, fb, "--discover", "256ms:128ms", "--discover-out", prefix], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert all(LINE.match(ln) for ln in out.stdout.splitlines() if ln.startswith("Region:")), out.stdout
    regs = regions_of(out.stdout)
    # A holds no repeat of its own; against B: the copy, exact to one hop
    assert len(regs) == 1, out.stdout
    t_a, length, name, t_b, mean, mn, good, count = regs[0]
    assert (t_a, length, name, t_b, good, count) == (stamp(9216), "1.024", fb, stamp(9216 + 31000), "7", "7")
    got = gpu.discover(a, b, gpu.discover_params(2048, 1024))
    reg = gpu.discover_regions(got, gpu.discover_params(2048, 1024), gpu.region_params(0.6, 128, 2, 1))
    assert (mean, mn) == ("%.3f" % reg[0]["mean_ncc"], "%.3f" % reg[0]["min_ncc"])
    assert list(p.name for p in tmp_path.iterdir() if p.name.startswith("cut")) == ["cut1_9216.wav"]     # no label file either
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.wav", "b.wav", "cut1_9216.wav"]
    cut = read_wav_f32(prefix + "1_9216.wav")
    assert cut.tobytes() == a[9216:9216 + 8192].tobytes()
    # the cut is a snippet as it is
    again = subprocess.run([cli, fb, "--snippet", prefix + "1_9216.wav", "--normalize", "--best", "1", "--no-out", "-n"], capture_output=True, text=True)
    assert again.returncode == 0, again.stderr
    assert offsets(again.stdout) == ["Offset 1: 00:00:05"], again.stdout          # (40216 / 8000 = 5.027 s)
    algo = gpu.HipConvolve(cut, score_norm=True)
    one = algo.match_trace(b, b.size)
    assert int(one[0]["argmax"]) == 9216 + 31000 and one[0]["max"] > 0.8    # (the cut's last 408 samples lie behind the copy)
    algo.close()
    # a higher bar: probe 15 (0.706) drops out, the region ends one hop earlier; too high a bar: no region, no file
    out = subprocess.run([cli, fa, fb, "--discover", "256ms:128ms", "--discover-min-ncc", "0.8"], capture_output=True, text=True)
    assert out.returncode == 0 and [(r[0], r[1], r[6]) for r in regions_of(out.stdout)] == [(stamp(9216), "0.896", "6")], out.stdout
    out = subprocess.run([cli, fa, fb, "--discover", "256ms:128ms", "--discover-min-ncc", "0.99", "--discover-out", str(tmp_path / "none")],
                         capture_output=True, text=True)
    assert out.returncode == 0 and regions_of(out.stdout) == [] and not [p for p in tmp_path.iterdir() if p.name.startswith("none")]


def test_cli_discover_self(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    x = dr.self_design()
    fx = str(tmp_path / "x.wav")
    write_wav_f32(fx, x)
    prefix = str(tmp_path / "rep")
    out = subprocess.run([cli, fx, "--discover", "256ms", "--discover-out", prefix], capture_output=True, text=True)   # (HOP = DUR / 2)
    assert out.returncode == 0, out.stderr
    regs = regions_of(out.stdout)
    assert len(regs) == 1, out.stdout                                               # the repeat is reported once
    assert (regs[0][0], regs[0][1], regs[0][2], regs[0][3], regs[0][6], regs[0][7]) == (stamp(5120), "0.768", fx, stamp(50120), "5", "5")
    cut = read_wav_f32(prefix + "0_5120.wav")
    assert cut.tobytes() == x[5120:5120 + 6144].tobytes()
    again = subprocess.run([cli, fx, "--snippet", prefix + "0_5120.wav", "--normalize", "--best", "2", "--distance", "1s", "--no-out", "-n"],
                           capture_output=True, text=True)
    assert again.returncode == 0, again.stderr
    assert offsets(again.stdout) == ["Offset 1: 00:00:00", "Offset 2: 00:00:06"], again.stdout   # (5120 and 50120 samples)
    algo = gpu.HipConvolve(cut, score_norm=True)
    best = algo.match_best(x, 2, min_distance=SR)
    assert sorted(int(p.start) for p in best) == [5120, 50120]
    algo.close()
