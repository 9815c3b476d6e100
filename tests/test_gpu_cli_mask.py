"""The CLI's --ignore FROM-TO and --mask-report on the WAV case of test_gpu_cli_normalize.py with one occurrence whose
middle 40 % is overwritten by noise 23 dB above the jingle (an episode title spoken over the theme)."""
import os
import re
import subprocess
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 8000
S = 2 * SR
PLANTS = (5.0, 31.0, 55.5)
GAP_S = (0.6, 1.4)   # of the snippet, seconds


def write_wav_stereo(path, lr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes(np.ascontiguousarray(lr, dtype="<i2").tobytes())


def make_case(tmp_path):
    """Jingle and background of amplitude 2000 (NCC of a clean occurrence: 0.71); the occurrence at 31 s has the snippet's
    0.6 s .. 1.4 s replaced by noise of amplitude 30000: as the zero-filled snippet under the whole window's energy it
    scores 0.6 / sqrt(1.2 + 0.4 * 226) = 0.06, below the default prominence of 0.13."""
    rng = np.random.default_rng(6)
    h = 70 * SR
    needle_lr = rng.integers(-2000, 2000, size=2 * S).astype(np.int16)
    hay_lr = rng.integers(-2000, 2000, size=2 * h).astype(np.int32)
    for t in PLANTS:
        off = int(t * SR)
        hay_lr[2 * off:2 * (off + S)] += needle_lr
    a, b = round((31.0 + GAP_S[0]) * SR), round((31.0 + GAP_S[1]) * SR)
    hay_lr[2 * a:2 * b] = rng.integers(-30000, 30000, size=2 * (b - a))
    hay_lr = np.clip(hay_lr, -32768, 32767).astype(np.int16)
    write_wav_stereo(tmp_path / "needle.wav", needle_lr)
    write_wav_stereo(tmp_path / "hay.wav", hay_lr)
    return needle_lr, hay_lr


def labels(path):
    return [float(row.split("\t")[0]) for row in path.read_text().splitlines()]


@pytest.fixture
def cli():
    import build as am_build
    return am_build.build_cli()


def test_ignore_finds_the_occurrence_the_plain_run_misses(gpu, cli, tmp_path):
    needle_lr, hay_lr = make_case(tmp_path)
    base = [cli, str(tmp_path / "hay.wav"), "--snippet", str(tmp_path / "needle.wav"), "--chunk-size", "20", "--distance", "10s", "-n", "--normalize"]
    out = subprocess.run(base + ["-o", str(tmp_path / "plain.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    starts = labels(tmp_path / "plain.txt")            # label i starts 7 s behind hit i
    assert out.stdout.count("Offset") == 2 and all(abs(x - 38.0) > 1e-3 for x in starts), (out.stdout, starts)
    assert "mask" not in out.stdout
    ignore = ["--ignore", "600ms-1s400ms"]
    out = subprocess.run(base + ignore + ["--mask-report", "-o", str(tmp_path / "masked.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    starts = labels(tmp_path / "masked.txt")
    assert out.stdout.count("Offset") == 3 and any(abs(x - 38.0) < 1e-3 for x in starts), (out.stdout, starts)
    # the report: one line per hit, am_hit_mask's record of that hit
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("  mask ")]
    assert len(lines) == 3, out.stdout
    needle, hay = gpu.pcm_s16_stereo_to_mono(needle_lr), gpu.pcm_s16_stereo_to_mono(hay_lr)
    gaps = [(round(GAP_S[0] * SR), round(GAP_S[1] * SR))]
    recs = gpu.HipConvolve(needle, gaps=gaps).hit_mask(hay, [gpu.Peak(int(t * SR), int(t * SR) + 1, 0.0, 0.0) for t in PLANTS])
    for ln, r in zip(lines, recs):
        m = re.match(r"  mask ncc (\S+) gain (\S+) kept_db (\S+) ncc_gaps (\S+) gaps_db (\S+) flags (\d+)", ln)
        assert m, ln
        ncc, gain, kept_db, ncc_gaps, gaps_db = (float(x) for x in m.groups()[:5])
        assert int(m.group(6)) == r.flags == 0
        assert abs(ncc - r.ncc) <= 1e-6 and abs(gain - r.gain) <= 1e-6 and abs(ncc_gaps - r.ncc_gaps) <= 1e-6, (ln, r)
        assert abs(kept_db - r.kept_db) <= 6e-3 and abs(gaps_db - r.gaps_db) <= 6e-3, (ln, r)
    assert recs[0].ncc_gaps > 0.6 and recs[2].ncc_gaps > 0.6 and abs(recs[1].ncc_gaps) < 0.1   # the original twice, something else once
    assert recs[1].gaps_db > 15.0 and all(r.ncc > 0.6 for r in recs)
    # --ignore with --best, as an ordinary snippet
    out = subprocess.run(base + ignore + ["--best", "3", "--no-out"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.count("Offset") == 3, (out.stdout, out.stderr)
    # ... with --min-confidence: the filter reads the masked NCC (0.70 for all three); am_hit_scores' NCC over the whole
    # window, which the filter takes without --ignore, would drop the occurrence with the loud span (0.06)
    out = subprocess.run(base + ignore + ["--min-confidence", "0.6", "--debug", "--no-out"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.count("Offset") == 3, (out.stdout, out.stderr)
    shown = [float(x) for x in re.findall(r"hit \d+: masked ncc (\S+)", out.stdout)]
    assert len(shown) == 3 and all(abs(x - r.ncc) <= 1e-6 for x, r in zip(shown, recs)) and "(dropped)" not in out.stdout
    out = subprocess.run(base + ignore + ["--min-confidence", "0.8", "--no-out"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.count("Offset") == 0, (out.stdout, out.stderr)
    # ... with --score-trace: the curve is that of the masked scores, its maximum the best masked hit
    out = subprocess.run(base + ignore + ["--score-trace", str(tmp_path / "curve"), "--no-out"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.count("Offset") == 3, (out.stdout, out.stderr)
    rows = (tmp_path / "curve0.csv").read_text().splitlines()
    assert rows[0].startswith("start_s,max,") and len(rows) > 1
    y = gpu.HipConvolve(needle, gaps=gaps, score_norm=True).correlate_with_sample(hay, gpu.Mode.Valid, True)
    top = max(float(row.split(",")[1]) for row in rows[1:] if row.split(",")[1] != "nan")
    assert abs(top - float(y.max())) <= 1e-6, (top, float(y.max()))


# ---- without --ignore: the parent's output, byte for byte --------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_mask")
COMMON = ["hay.wav", "--snippet", "needle.wav", "--chunk-size", "20", "--distance", "10s", "-n"]
# name -> the options of a run without --ignore: the default scores, NCC, and every per-hit report line the hit loop prints
GOLDEN_RUNS = {
    "plain": [],
    "normalize": ["--normalize"],
    "report": ["--normalize", "--min-confidence", "0.5", "--segments", "4", "--stereo", "2", "--warp", "200", "--channel", "4", "--bands", "4"],
}


def run_golden(cli, workdir, name):
    """(stdout, label file) of run `name` on the files of make_case in `workdir`, as bytes; relative file names, so that
    no line depends on where the files are."""
    out = subprocess.run([cli] + COMMON + GOLDEN_RUNS[name] + ["-o", name + ".txt"], cwd=str(workdir), capture_output=True)
    assert out.returncode == 0, out.stderr
    return out.stdout, (workdir / (name + ".txt")).read_bytes()


@pytest.mark.parametrize("name", sorted(GOLDEN_RUNS))
def test_without_ignore_output_is_the_parents(gpu, cli, tmp_path, name):
    """tests/golden/cli_mask holds what the CLI of the commit before masked matching printed and wrote for these runs on
    the files of make_case (recorded with this module's record mode, see the README there): a run without --ignore still
    gives those bytes -- the same lines in the same order, the same digits."""
    make_case(tmp_path)
    stdout, labels_ = run_golden(cli, tmp_path, name)
    assert stdout == open(os.path.join(GOLDEN, name + ".stdout"), "rb").read()
    assert labels_ == open(os.path.join(GOLDEN, name + ".labels"), "rb").read()
    assert stdout.count(b"Offset") >= 2


if __name__ == "__main__":
    # record mode: python tests/test_gpu_cli_mask.py CLI OUT_DIR -- the fixtures of test_without_ignore_output_is_the_parents
    # from the CLI binary given (the one of the commit to compare with), on a device
    import pathlib
    import sys
    import tempfile
    cli_, out_dir = os.path.abspath(sys.argv[1]), pathlib.Path(sys.argv[2])
    out_dir.mkdir(parents=True, exist_ok=True)
    with tempfile.TemporaryDirectory() as d:
        make_case(pathlib.Path(d))
        for name_ in sorted(GOLDEN_RUNS):
            stdout_, labels_ = run_golden(cli_, pathlib.Path(d), name_)
            (out_dir / (name_ + ".stdout")).write_bytes(stdout_)
            (out_dir / (name_ + ".labels")).write_bytes(labels_)
            print(name_, len(stdout_), "bytes of stdout,", len(labels_), "bytes of labels")


def test_refused_combinations(cli, tmp_path):
    base = [cli, "hay.wav", "--snippet", "a.wav", "--ignore", "1s-2s"]
    for extra, word in ((["--resample"], "--resample"), (["--whiten", "8"], "--whiten"), (["--envelope", "3"], "--envelope"),
                        (["--edges", "1s"], "--edges"), (["--snippet", "b.wav"], "several --snippet")):
        r = subprocess.run(base + extra, capture_output=True, text=True, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and "--ignore and " + word + " are mutually exclusive" in r.stderr, (extra, r.stderr)
    r = subprocess.run([cli, "--live", "--rate", "8000", "--snippet", "a.wav", "--ignore", "1s-2s"], capture_output=True, text=True,
                       stdin=subprocess.DEVNULL)
    assert r.returncode == 2 and "--ignore and --live are mutually exclusive" in r.stderr
    for bad in (["--ignore", "2s-1s"], ["--ignore", "1s"], ["--ignore", "x-2s"], ["--ignore", "1s-1s"]):
        r = subprocess.run([cli, "hay.wav", "--snippet", "a.wav"] + bad, capture_output=True, text=True, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and "--ignore" in r.stderr, (bad, r.stderr)
    r = subprocess.run([cli, "hay.wav", "--snippet", "a.wav", "--mask-report"], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert r.returncode == 2 and "--mask-report needs --ignore" in r.stderr
    r = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--ignore FROM-TO" in r.stdout and "--mask-report" in r.stdout
