"""The weight gradients come out bit for bit as on the commit tests/golden/wgrad_x3_bits.json names (written there by
tools/record_wgrad_bits.py): per key of tests/wgrad_bits_cases.py, the SHA-256 of dW's bytes.  An equality — no tolerance: a change
of csrc/wgrad_x3.hip that keeps the arithmetic and its order keeps every hash, and one that moves a single rounding shows here.  (What
the hashes cannot cover — launches of more than two chunks on the atomic path, whose order of addition is the hardware's — stays with
the tolerances of test_gpu_train_conv.py.)"""
import json
import os

import pytest

import wgrad_bits_cases as wb

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_x3_bits.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["sha256"]


def test_every_key_is_recorded(golden):
    assert list(golden) == list(wb.KEYS)


@pytest.mark.parametrize("key", wb.KEYS)
def test_weight_gradient_bits_are_the_recorded_ones(dev, golden, key):
    assert wb.digest(key) == golden[key], key
