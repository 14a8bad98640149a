"""The entries of csrc/pw_x3.hip — the pointwise, lateral and chained plane-pair kernels and the training form in its three modes — give
bit for bit what they gave on the commit tests/golden/pw_x3_bits.json names (written there by tools/record_wgrad_bits.py with
pw_bits_cases named): per key of tests/pw_bits_cases.py, the SHA-256 over the whole of every output buffer.  An equality — no
tolerance: a change of the file that keeps the arithmetic and its order keeps every hash; one that moves a single rounding, or
stores one element outside its slice, shows here."""
import json
import os

import pytest

import pw_bits_cases as pb

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pw_x3_bits.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["sha256"]


def test_every_key_is_recorded(golden):
    assert list(golden) == list(pb.KEYS)


@pytest.mark.parametrize("key", pb.KEYS)
def test_pointwise_bits_are_the_recorded_ones(dev, golden, key):
    assert pb.digest(key) == golden[key], key
