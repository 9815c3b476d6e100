"""The argument refusals of tests/entry_refusals.py, replayed: return code and message of every case equal what
tests/golden/entry_refusals.json holds (recorded once with `python tests/entry_refusals.py --record`, from the library
as it was before the entry points' shared steps were written once)."""
import json

import pytest

import entry_refusals

pytestmark = pytest.mark.gpu


def test_every_refusal_answers_as_recorded(gpu):
    with open(entry_refusals.GOLDEN) as f:
        golden = json.load(f)
    got = entry_refusals.run(gpu)
    assert sorted(got) == sorted(golden), "the case list and the recording differ: record again"
    differ = {i: {"got": got[i], "recorded": golden[i]} for i in golden if got[i] != golden[i]}
    assert not differ, differ
