#!/usr/bin/env python3
"""The raw output bytes of the library's kernels on a fixed list of small cases, for comparing two builds of the library
byte for byte (a refactor of the kernels must not move a bit).

  python tools/hit_records_dump.py OUT.npz        every case's output, as uint8 arrays keyed by the case's name
  python tools/hit_records_dump.py --compare A.npz B.npz
                                                  one JSON line: the case count, equal or not, the differing cases

The inputs are seeded numpy arrays; the tool reads nothing but the library of the tree it stands in.  Run it once in
each tree, each in a process of its own, then compare the files.

The cases are those of tests/kernel_bytes_cases.py (its head lists them): the per-hit families, significance,
score_norm and a needle's energy, bands, the envelope levels and scores, the lag products, discovery and the score
traces.  tests/test_gpu_kernel_bytes.py checks the same cases against the digests in tests/golden/kernel_bytes.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "audio-matcher_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kernel_bytes_cases as cases   # (tests/: the case list, shared with tests/test_gpu_kernel_bytes.py)


def dump(path):
    import audiomatch_amd as am
    out = {}
    for fam in cases.FAMILIES:
        for name, (_, data) in cases.run_family(am, fam).items():
            out[name] = np.frombuffer(data, dtype=np.uint8).copy()
    np.savez(path, **out)
    print(json.dumps({"cases": len(out), "bytes": int(sum(a.size for a in out.values())), "file": path}))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    names = sorted(set(a.files) | set(b.files))
    differing = [n for n in names if n not in a.files or n not in b.files or a[n].shape != b[n].shape or not np.array_equal(a[n], b[n])]
    errors = [n for n in a.files if bytes(a[n][:5]) == b"error"]
    print(json.dumps({"cases": len(names), "equal": not differing, "differing": differing, "refused_calls": errors}))
    return 0 if not differing else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("paths", nargs="+")
    a = ap.parse_args()
    if a.compare:
        if len(a.paths) != 2:
            ap.error("--compare takes two files")
        sys.exit(compare(*a.paths))
    if len(a.paths) != 1:
        ap.error("one output file")
    dump(a.paths[0])


if __name__ == "__main__":
    main()
