"""The CLI's --channel on an occurrence that went through a short filter: the channel line beside the offset line;
--residual writes what am_hit_residual gives through the binding; --residual without --channel is a usage error."""
import re
import subprocess
import wave

import numpy as np
import pytest

from test_hit_channel_host import G, downmix

pytestmark = pytest.mark.gpu

SR = 8000
S, T, P = 12_000, 10 * SR + 123, 8


def write_wav(path, mono_i16):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes(np.ascontiguousarray(np.repeat(mono_i16[:, None], 2, axis=1), dtype="<i2").tobytes())


def make_case(tmp_path):
    """(needle, haystack) as the CLI's down-mix sees the two files."""
    rng = np.random.default_rng(23)
    snip = np.rint(rng.normal(0, 6000, S)).astype(np.int16)
    hay = rng.normal(0, 40, 30 * SR)
    for l, g in G.items():
        hay[T + l:T + l + S] += g * snip.astype(np.float64)
    hay = np.clip(np.rint(hay), -32768, 32767).astype(np.int16)
    write_wav(tmp_path / "snip.wav", snip)
    write_wav(tmp_path / "hay.wav", hay)
    return downmix(np.repeat(snip[:, None], 2, axis=1)), downmix(np.repeat(hay[:, None], 2, axis=1))


CHANNEL_LINE = re.compile(r"^  channel ncc (-?[0-9.]+) ncc_eq (-?[0-9.]+) gain_db (-?[0-9.]+) residual_db (-?[0-9.]+) main_tap (-?[0-9]+) "
                          r"main_share ([0-9.]+)$")


def test_cli_channel(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    needle, mono = make_case(tmp_path)
    base = [cli, "--snippet", str(tmp_path / "snip.wav"), "--chunk-size", "20", "--distance", "10s", "-y", "--no-out", str(tmp_path / "hay.wav")]
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    assert [ln.split(" with ")[0] for ln in plain.stdout.splitlines() if ln.startswith("Offset")] == ["Offset 1: 00:00:10"], plain.stdout
    assert "channel" not in plain.stdout
    prefix = str(tmp_path / "left_")
    out = subprocess.run(base + ["--channel", "%d:200" % P, "--residual", prefix], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines(keepends=True)
    chan = [ln for ln in lines if ln.startswith("  channel ")]
    # the flag adds its line behind the offset line and changes nothing else
    assert len(chan) == 1 and lines.index(chan[0]) == [i for i, ln in enumerate(lines) if ln.startswith("Offset")][0] + 1, out.stdout
    assert "".join(ln for ln in lines if ln not in chan) == plain.stdout
    m = CHANNEL_LINE.match(chan[0].rstrip("\n"))
    assert m, chan[0]
    ncc, ncc_eq, gain_db, residual_db, main_tap, main_share = (float(v) for v in m.groups())
    print(chan[0])
    assert ncc < 0.9 and ncc_eq > 0.99 and ncc_eq > ncc + 0.05 and main_tap == 0 and abs(main_share - 1 / 1.3125) < 0.01 and residual_db < -15
    # the residual file holds am_hit_residual's resid of the same hit, absent samples as 0
    recs, taps = gpu.HipConvolve(needle).hit_channel(mono, [gpu.Peak(T, T + 1, 0.0, 0.0)], gpu.channel_params(P, 200.0))
    assert abs(recs[0].ncc_eq - ncc_eq) < 1e-5
    _, resid = gpu.hit_residual(mono, T, needle, taps[0])
    want = np.where(np.isfinite(resid), resid, np.float32(0)).astype(np.float32)
    raw = open(prefix + "0_%d.wav" % T, "rb").read()
    assert raw[:4] == b"RIFF" and raw[36:40] == b"fact" and raw[48:52] == b"data"
    got = np.frombuffer(raw[56:], dtype="<f4")
    assert got.shape == want.shape == (S + 2 * P,) and got.tobytes() == want.tobytes()
    # what is left is the noise under the jingle: far below the span
    assert np.sqrt(np.mean(got.astype(np.float64) ** 2)) < 0.05 * np.sqrt(np.mean(mono[T:T + S].astype(np.float64) ** 2))
    # usage errors
    r = subprocess.run(base + ["--residual", prefix], capture_output=True, text=True)
    assert r.returncode == 2 and "--residual needs --channel" in r.stderr, r.stderr
    for bad in ("129", "-1", "8:201", "8:x", "x", ""):
        r = subprocess.run(base + ["--channel", bad], capture_output=True, text=True)
        assert r.returncode == 2 and "--channel" in r.stderr, (bad, r.stderr)
    r = subprocess.run([cli, "--snippet", str(tmp_path / "snip.wav"), "--live", "--rate", "8000", "--channel", "8"],
                       capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert r.returncode == 2 and "--live: --channel does not apply" in r.stderr
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True).stdout
    assert "--channel P[:NOISE_DB]" in usage and "--residual PREFIX" in usage
