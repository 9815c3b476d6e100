"""csrc/am_spans.h, the span merger of the per-hit host forms, through a g++ probe with its own main: the merged spans,
span_of and the staged total against an interval union written here, on designed and seeded random cases; once more
with the probe built under AddressSanitizer and UBSan."""
import os
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "audio-matcher_amd", "csrc")
PROBE = r"""
#include "am_spans.h"
#include <cstdio>
int main() {   // per case: n, then n pairs lo hi; prints "lo hi off ... | span_of ... | total"
    size_t n;
    while (scanf("%zu", &n) == 1) {
        std::vector<am::HitRange> r(n);
        for (auto& q : r) if (scanf("%zu %zu", &q.lo, &q.hi) != 2) return 1;
        std::vector<am::Span> spans;
        std::vector<size_t> span_of;
        const size_t total = am::merge_spans(r.data(), n, spans, span_of);
        for (const am::Span& s : spans) printf("%zu %zu %zu ", s.lo, s.hi, s.off);
        printf("|");
        for (size_t i : span_of) printf(" %zu", i);
        printf(" | %zu\n", total);
    }
    return 0;
}
"""
DESIGNED = [
    [(7, 19)],                          # one hit
    [(0, 10), (10, 15)],                # touching: one span
    [(0, 10), (11, 15)],                # a gap of one element: two spans
    [(0, 100), (20, 30)],               # contained
    [(5, 9), (5, 30), (5, 6)],          # equal starts, different ends
    [(50, 60), (30, 40), (35, 52), (0, 3)],   # descending input
    [(5, 5)], [(3, 5), (5, 5), (9, 9)], [(5, 5), (5, 8)],   # empty spans
]


def cases():
    rng = np.random.default_rng(15)
    rnd = []
    for _ in range(200):
        lo = rng.integers(0, 60, size=int(rng.integers(1, 13)))
        rnd.append([(int(a), int(a + rng.integers(0, 9))) for a in lo])
    return DESIGNED + rnd


def union_ref(r):
    """Components of 'overlap or touch' (closed intervals meet), ascending, with running offsets."""
    comp = list(range(len(r)))
    for _ in r:   # label propagation to a fixed point
        for i, (a, b) in enumerate(r):
            for j, (c, d) in enumerate(r):
                if a <= d and c <= b:
                    comp[i] = comp[j] = min(comp[i], comp[j])
    groups = sorted({k: (min(r[i][0] for i in range(len(r)) if comp[i] == k), max(r[i][1] for i in range(len(r)) if comp[i] == k))
                     for k in set(comp)}.items(), key=lambda kv: kv[1])
    spans, off = [], 0
    for _, (lo, hi) in groups:
        spans.append((lo, hi, off))
        off += hi - lo
    index = {k: n for n, (k, _) in enumerate(groups)}
    return spans, [index[k] for k in comp], off


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_merge_spans_against_interval_union(tmp_path, flags):
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I", CSRC, "-o", str(exe), str(src)])
    cs = cases()
    text = "".join(f"{len(r)} " + " ".join(f"{a} {b}" for a, b in r) + "\n" for r in cs)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(cs)
    for r, ln in zip(cs, lines):
        a, b, c = ln.split("|")
        v = [int(x) for x in a.split()]
        got = ([tuple(v[i:i + 3]) for i in range(0, len(v), 3)], [int(x) for x in b.split()], int(c))
        assert got == union_ref(r), (r, got)
    assert [len(ln.split("|")[0].split()) // 3 for ln in lines[:4]] == [1, 1, 2, 1]   # the designed merges, spelled out
