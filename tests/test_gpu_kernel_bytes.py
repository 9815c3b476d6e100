"""The raw output bytes of the library's kernels on the fixed cases of kernel_bytes_cases.py, against the SHA-256 digests of
tests/golden/kernel_bytes.json.  The record was taken on an MI355X from the library of the parent of the commit that
added it (and is taken again from a parent only when a change means to move bits): a refactor of the kernels must leave
every case equal.  Per case the record holds the digest of the input bytes as well, so that a changed random stream is
told apart from a changed library; either fails the test.  tools/hit_records_dump.py dumps the same cases to a file and
compares two files, for finding which bytes of a case moved."""
import json
import os

import pytest

import kernel_bytes_cases as cases

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_bytes.json")) as f:
    GOLDEN = json.load(f)


def test_record_covers_every_family():
    assert sorted(GOLDEN) == sorted(cases.FAMILIES)


@pytest.mark.parametrize("family", sorted(cases.FAMILIES))
def test_kernel_bytes(gpu, family):
    got, want = cases.digests(gpu, family), GOLDEN[family]
    assert sorted(got) == sorted(want), "the case list and the record differ"
    moved_inputs = [k for k in sorted(want) if got[k]["in"] != want[k]["in"]]
    assert not moved_inputs, "the inputs of %d cases are not the recorded ones (numpy's stream?): %s" % (len(moved_inputs), moved_inputs[:8])
    moved = [k for k in sorted(want) if got[k]["out"] != want[k]["out"]]
    assert not moved, "%d of %d cases differ from the record: %s" % (len(moved), len(want), moved[:16])
