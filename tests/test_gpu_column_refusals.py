"""The fifteen entry points that take witness or selector columns refuse a bad call -- one mistake, or two at once -- with
the code and the message recorded in tests/golden/column_refusals.json, and still work afterwards.  The fixture was recorded
from the library before the columns of a call were stated once (ColumnsOf / admit_columns in csrc/host.hpp); it is the
contract for which refusal wins.  Integers and strings: every comparison is exact."""
import json
import os

import pytest

import column_refusal_cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "column_refusals.json")


def test_every_refusal_is_the_recorded_one(ctx):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = column_refusal_cases.run_cases(ctx)
    assert sorted(got) == sorted(want)
    wrong = {name: (got[name], want[name]) for name in want if got[name] != want[name]}
    assert not wrong, f"{len(wrong)} of {len(want)} cases differ, the first: {sorted(wrong.items())[0]}"
