"""The CLI's --warp on an occurrence that runs 200 ppm slow: the drift, the refined lag and both NCCs beside the offset
line; --min-confidence then judges the corrected NCC; without the flag nothing changes."""
import re
import subprocess
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 8000
S, T, PPM = 30_000, 10 * SR + 123, 200.0


def write_wav(path, mono_i16):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes(np.ascontiguousarray(np.repeat(mono_i16[:, None], 2, axis=1), dtype="<i2").tobytes())


def make_case(tmp_path):
    rng = np.random.default_rng(21)
    snip = np.rint(np.convolve(rng.normal(0, 12_000, S + 7), np.ones(8) / 8, mode="valid")).astype(np.int16)   # smoothed noise
    hay = rng.normal(0, 40, 30 * SR)
    k = np.arange(int(S * (1 + PPM * 1e-6)) + 1)
    hay[T:T + len(k)] += np.interp(k / (1 + PPM * 1e-6), np.arange(S), snip.astype(np.float64), right=0.0)
    write_wav(tmp_path / "snip.wav", snip)
    write_wav(tmp_path / "hay.wav", np.clip(np.rint(hay), -32768, 32767).astype(np.int16))


WARP_LINE = re.compile(r"^  warp drift_ppm (-?[0-9.]+) lag (-?[0-9.]+) ncc (-?[0-9.]+) ncc_as_found (-?[0-9.]+)$")


def test_cli_warp(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    make_case(tmp_path)
    base = [cli, "--snippet", str(tmp_path / "snip.wav"), "--chunk-size", "20", "--distance", "10s", "-y", "--no-out", str(tmp_path / "hay.wav")]
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    assert [ln.split(" with ")[0] for ln in plain.stdout.splitlines() if ln.startswith("Offset")] == ["Offset 1: 00:00:10"], plain.stdout
    assert "warp" not in plain.stdout
    out = subprocess.run(base + ["--warp", "400:8:4"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines(keepends=True)
    warp = [ln for ln in lines if ln.startswith("  warp ")]
    # the flag adds its line behind the offset line and changes nothing else
    assert len(warp) == 1 and lines.index(warp[0]) == [i for i, ln in enumerate(lines) if ln.startswith("Offset")][0] + 1, out.stdout
    assert "".join(ln for ln in lines if ln not in warp) == plain.stdout
    m = WARP_LINE.match(warp[0].rstrip("\n"))
    assert m, warp[0]
    drift, lag, ncc, found = (float(v) for v in m.groups())
    print(warp[0])
    assert abs(drift - PPM) <= 2.0 and abs(lag) <= 4.5 and ncc >= 0.95 and found < ncc - 0.05
    # --min-confidence between the two NCCs: the hit is dropped as found, kept once the drift is taken out
    mid = "%.3f" % (0.5 * (ncc + found))
    dropped = subprocess.run(base + ["--min-confidence", mid], capture_output=True, text=True)
    kept = subprocess.run(base + ["--min-confidence", mid, "--warp", "400"], capture_output=True, text=True)
    assert dropped.returncode == 0 and kept.returncode == 0, (dropped.stderr, kept.stderr)
    assert not [ln for ln in dropped.stdout.splitlines() if ln.startswith("Offset")], dropped.stdout
    assert [ln for ln in kept.stdout.splitlines() if ln.startswith("  warp ")] == [warp[0].rstrip("\n")], kept.stdout
    # refused values, and on a live feed
    for bad in ("0", "60000", "400:0", "400:33", "400:8:17", "x"):
        r = subprocess.run(base + ["--warp", bad], capture_output=True, text=True)
        assert r.returncode == 2 and "--warp" in r.stderr, (bad, r.stderr)
    r = subprocess.run([cli, "--snippet", str(tmp_path / "snip.wav"), "--live", "--rate", "8000", "--warp", "400"],
                       capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert r.returncode == 2 and "--live: --warp does not apply" in r.stderr
    assert "--warp PPM[:STEPS[:RADIUS]]" in subprocess.run([cli, "--help"], capture_output=True, text=True).stdout
