"""The CLI's --mix and --stereo on a two-channel WAV that holds the snippet once in phase and once polarity-inverted
between the channels: the down-mix finds the first only, --mix side the second only; --stereo prints the checker's values
under the offset line; the refusals; and without the new options the output is the parent's, byte for byte."""
import re
import subprocess
import wave

import numpy as np
import pytest

import hit_stereo_ref as ref

pytestmark = pytest.mark.gpu

SR = 8000
S, T_BOTH, T_INV, FRAMES = 12_000, 5 * SR + 77, 20 * SR + 123, 30 * SR
# What the parent commit's CLI printed for `--snippet snip.wav --chunk-size 20 --distance 10s -y --no-out hay.wav` on the
# files of make_case (recorded on an MI355X from a build of the parent): the new options change nothing where they are absent.
PARENT_STDOUT = "Offset 1: 00:00:05 with prominence 1.0294031\n"


def write_wav(path, frames_i16, channels=2):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes(np.ascontiguousarray(frames_i16, dtype="<i2").tobytes())


def make_case(tmp_path):
    """snip.wav: the snippet in the left channel, silence in the right (its mid and its side are the same signal);
    hay.wav: noise, the snippet at +0.5 in both channels at T_BOTH, at +0.5 in L and -0.5 in R at T_INV."""
    rng = np.random.default_rng(29)
    snip = np.rint(rng.normal(0, 6000, S)).astype(np.int64)
    snip_lr = np.stack([snip, np.zeros(S, dtype=np.int64)], axis=1).astype(np.int16)
    hay = rng.integers(-1500, 1501, size=(FRAMES, 2)).astype(np.int64)
    hay[T_BOTH:T_BOTH + S, 0] += snip // 2
    hay[T_BOTH:T_BOTH + S, 1] += snip // 2
    hay[T_INV:T_INV + S, 0] += snip // 2
    hay[T_INV:T_INV + S, 1] -= snip // 2
    assert np.abs(hay).max() <= 32767
    hay = hay.astype(np.int16)
    write_wav(tmp_path / "snip.wav", snip_lr)
    write_wav(tmp_path / "hay.wav", hay)
    write_wav(tmp_path / "mono.wav", hay[:, 0], channels=1)
    return snip_lr, hay


STEREO_LINE = re.compile(r"^  stereo image (\w+) ncc_left (-?[0-9.]+) ncc_right (-?[0-9.]+) ncc_side (-?[0-9.]+) ncc_best (-?[0-9.]+) "
                         r"balance_db (-?[0-9.]+|-?inf|-?nan) delay (-?[0-9.]+|-?nan) downmix_loss_db (-?[0-9.]+|-?inf|-?nan)$")
IMAGES = ("absent", "centre", "left", "right", "panned", "inverted")


def offsets(stdout):
    return [ln.split(" with ")[0] for ln in stdout.splitlines() if ln.startswith("Offset")]


def check_stereo_line(line, exp, min_ncc=0.5):
    m = STEREO_LINE.match(line.rstrip("\n"))
    assert m, line
    image, balance, delay, loss = ref.summary_ref(exp, min_ncc)
    assert m.group(1) == IMAGES[image], (line, exp)
    for text, want in zip(m.groups()[1:5], (exp.ncc_left, exp.ncc_right, exp.ncc_side, exp.ncc_best)):
        assert abs(float(text) - want) <= 1e-6, (line, exp)           # (six decimals printed, of an f32 within 2 ulp)
    assert abs(float(m.group(6)) - balance) <= 0.006 and abs(float(m.group(7)) - delay) <= 0.0006 and abs(float(m.group(8)) - loss) <= 0.006, (line, balance, delay, loss)


def test_cli_mix_and_stereo(gpu, tmp_path):
    import build as am_build
    cli = am_build.build_cli()
    snip_lr, hay = make_case(tmp_path)
    base = [cli, "--snippet", str(tmp_path / "snip.wav"), "--chunk-size", "20", "--distance", "10s", "-y", "--no-out", str(tmp_path / "hay.wav")]
    # without the new options: the parent's bytes; the down-mix finds the plant that is in phase, not the inverted one
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    print(repr(plain.stdout))
    assert offsets(plain.stdout) == ["Offset 1: 00:00:05"], plain.stdout
    assert plain.stdout == PARENT_STDOUT
    mid = subprocess.run(base + ["--mix", "mid"], capture_output=True, text=True)
    assert mid.returncode == 0 and mid.stdout == plain.stdout, mid.stderr
    # --mix side finds the inverted plant, and only that
    side = subprocess.run(base + ["--mix", "side"], capture_output=True, text=True)
    assert side.returncode == 0, side.stderr
    assert offsets(side.stdout) == ["Offset 1: 00:00:20"], side.stdout
    assert "stereo" not in side.stdout
    # --stereo: one line behind the offset line, with the checker's values; nothing else changes
    for mix, t, needle, image in (([], T_BOTH, ref.downmix(snip_lr), "centre"), (["--mix", "side"], T_INV, ref.mix_ref(0.5, -0.5, snip_lr), "inverted")):
        without = subprocess.run(base + mix, capture_output=True, text=True).stdout
        out = subprocess.run(base + mix + ["--stereo", "4"], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines(keepends=True)
        st = [ln for ln in lines if ln.startswith("  stereo ")]
        assert len(st) == 1 and lines.index(st[0]) == [i for i, ln in enumerate(lines) if ln.startswith("Offset")][0] + 1, out.stdout
        assert "".join(ln for ln in lines if ln not in st) == without
        print(st[0])
        exp = ref.stereo_ref(hay, needle, t, 4)
        assert IMAGES[ref.summary_ref(exp, 0.5)[0]] == image, exp          # (the input is what the case says, by the checker)
        check_stereo_line(st[0], exp)
        assert st[0].startswith("  stereo image " + image + " "), st[0]
        q = gpu.HipConvolve(needle).hit_stereo(hay, [gpu.Peak(t, t + 1, 0.0, 0.0)], 4)[0]
        ref.assert_records(q, exp, image)
    # a higher MIN_NCC than the channels reach: absent
    out = subprocess.run(base + ["--stereo", "4:0.999"], capture_output=True, text=True)
    assert out.returncode == 0 and "  stereo image absent " in out.stdout, out.stdout + out.stderr
    # refusals: a mono file, --live, --whiten (and its kin), malformed values
    mono = [cli, "--snippet", str(tmp_path / "snip.wav"), "--chunk-size", "20", "--distance", "10s", "-y", "--no-out", str(tmp_path / "mono.wav")]
    r = subprocess.run(mono + ["--stereo", "4"], capture_output=True, text=True)
    assert r.returncode != 0 and "--stereo: the main file is not a 16-bit two-channel file" in r.stderr, r.stderr
    r = subprocess.run(mono + ["--mix", "left"], capture_output=True, text=True)
    assert r.returncode != 0 and "--mix:" in r.stderr and "not a 16-bit two-channel file" in r.stderr, r.stderr
    assert subprocess.run(mono, capture_output=True, text=True).returncode == 0
    for extra in (["--whiten", "8"], ["--preemphasis", "0.9"], ["--resample"]):
        r = subprocess.run(base + ["--stereo", "4"] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "--stereo does not apply with" in r.stderr, (extra, r.stderr)
    for opt, val in (("--stereo", "4"), ("--mix", "side")):
        r = subprocess.run([cli, "--snippet", str(tmp_path / "snip.wav"), "--live", "--rate", "8000", opt, val],
                           capture_output=True, text=True, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and "--live: " + opt + " does not apply" in r.stderr, r.stderr
    for opt, bad in (("--stereo", "17"), ("--stereo", "4:2"), ("--mix", "centre"), ("--mix", "1,")):
        r = subprocess.run(base + [opt, bad], capture_output=True, text=True)
        assert r.returncode == 2 and opt in r.stderr, (opt, bad, r.stderr)
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True).stdout
    assert "--mix M" in usage and "--stereo R[:MIN_NCC]" in usage
