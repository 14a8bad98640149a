"""The training convolutions send the C ABI exactly the launches recorded in tests/golden/train_conv_launch_plan.json (written by
tools/record_train_conv_launches.py on the commit the file names): the same entries in the same order with the same integers, and
the same pointers null.  An equality — no tolerance; a change of the dispatch in train_ops / ops that moves a launch shows here
before it shows in a number.  (The *_supported / *_rows queries go through _lib.lib(), not K: how often they are asked is free.)"""
import json
import os

import pytest

import train_conv_cases as tc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_conv_launch_plan.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_every_case_is_recorded(golden):
    assert list(golden) == list(tc.CASES)
    for case in tc.CASES:
        assert list(golden[case]) == [key for key, _, _ in tc.settings(case)]
        assert all(golden[case][key] for key in golden[case]), case  # (no setting without a launch)


@pytest.mark.parametrize("case", list(tc.CASES))
def test_launch_plan_is_the_recorded_one(dev, golden, case):
    for key, groups, epi in tc.settings(case):
        got = json.loads(json.dumps(tc.launches(case, groups, epi)))
        want = golden[case][key]
        assert [c[0] for c in got] == [c[0] for c in want], (case, key)
        for n, (g, w) in enumerate(zip(got, want)):
            assert g == w, (case, key, n, g, w)
