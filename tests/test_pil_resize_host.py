"""Pillow's 8-bit resize without a GPU: the NumPy restatement (tests/pil_resize_ref.py) equals live `Image.resize` and the committed
fixture bit for bit, and the C ABI's host tables (avt_resize_u8_ksize / avt_resize_u8_tables) equal the restatement's exactly."""
import os

import numpy as np
import pytest

import pil_resize_ref as ref

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "pil_resize.npz"))
REAL = ((360, 640), (352, 640))  # one real extent: only the vertical pass runs
PAIRS = [(45, 32), (70, 64), (95, 64), (33, 32), (32, 45), (64, 70), (360, 352), (37, 32)]
FILTERS = [ref.LANCZOS, ref.BILINEAR]


@pytest.mark.parametrize("name,big,small", ref.CASES + [("real",) + REAL], ids=[c[0] for c in ref.CASES] + ["real"])
def test_restatement_equals_live_pillow(name, big, small):
    pytest.importorskip("PIL")
    x = ref.noisy_frames(7 + len(name), big + (3,))
    down = ref.resize(x, small, ref.LANCZOS)
    assert np.array_equal(down, ref.pil_resize(x, small, ref.LANCZOS))
    assert down.min() == 0 and down.max() == 255  # both ends of the clamp are reached
    assert np.array_equal(ref.resize(down, big, ref.BILINEAR), ref.pil_resize(down, big, ref.BILINEAR))
    # ... and the other filter in each direction
    assert np.array_equal(ref.resize(x, small, ref.BILINEAR), ref.pil_resize(x, small, ref.BILINEAR))
    assert np.array_equal(ref.resize(down, big, ref.LANCZOS), ref.pil_resize(down, big, ref.LANCZOS))


@pytest.mark.parametrize("name,big,small", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_restatement_equals_the_fixture(name, big, small):
    x = GOLD[name + "_in"]
    assert x.shape == big + (3,) and np.array_equal(x, ref.noisy_frames(100 + [c[0] for c in ref.CASES].index(name), big + (3,)))
    down = ref.resize(x, small, ref.LANCZOS)
    assert np.array_equal(down, GOLD[name + "_down"])
    assert np.array_equal(ref.resize(down, big, ref.BILINEAR), GOLD[name + "_up"])


def test_restatement_equals_the_fixture_batch():
    batch = np.stack([GOLD[c[0] + "_down"] for c in ref.CASES if c[2] == (32, 64)][:ref.UP_BATCH])
    assert np.array_equal(ref.resize(batch, (45, 70), ref.BILINEAR), GOLD["up4"])


def test_same_size_is_a_copy():
    x = ref.noisy_frames(1, (9, 11, 3))
    y = ref.resize(x, (9, 11), ref.LANCZOS)
    assert np.array_equal(x, y) and y is not x


@pytest.mark.parametrize("filt", FILTERS, ids=["lanczos", "bilinear"])
@pytest.mark.parametrize("n_in,n_out", PAIRS, ids=["%d-%d" % p for p in PAIRS])
def test_abi_host_tables_equal_the_restatement(avt, n_in, n_out, filt):
    k, bounds = avt.ops.resize_u8_tables(n_in, n_out, filt)
    rk, rb = ref.tables(n_in, n_out, filt)
    assert k.dtype == np.int32 and bounds.dtype == np.int32 and k.shape == rk.shape and bounds.shape == (n_out, 2)
    assert np.array_equal(bounds, rb) and np.array_equal(k, rk)
    # a row's taps stay inside the input, fill no more than ksize, and sum to 1 in fixed point up to their roundings
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= n_in).all() and (bounds[:, 1] <= k.shape[1]).all()
    assert (np.abs(k.sum(1) - (1 << 22)) <= k.shape[1]).all()
    if (n_in, n_out, filt) == (37, 32, ref.LANCZOS):  # edge outputs with clipped bounds: fewer taps than inside
        assert bounds[0, 0] == 0 and bounds[0, 1] < bounds[16, 1] and bounds[-1].sum() == n_in and bounds[-1, 1] < bounds[16, 1]


def test_abi_host_tables_refuse_what_they_cannot_do(avt):
    lib = avt._lib.lib()
    AVT_ERR_ARG = -1
    assert lib.avt_resize_u8_ksize(0, 32, 1) == AVT_ERR_ARG and lib.avt_resize_u8_ksize(32, 0, 1) == AVT_ERR_ARG
    assert lib.avt_resize_u8_ksize(45, 32, 2) == AVT_ERR_ARG
    assert lib.avt_resize_u8_ksize(45, 32, 1) == 11 and lib.avt_resize_u8_ksize(32, 45, 0) == 3 and lib.avt_resize_u8_ksize(95, 64, 1) == 11
    k, b = np.zeros((32, 11), np.int32), np.zeros((32, 2), np.int32)
    assert lib.avt_resize_u8_tables(45, 32, 1, 9, k.ctypes.data, b.ctypes.data) == AVT_ERR_ARG  # buffers made for another ksize
    assert b"11 taps" in lib.avt_last_error()
    assert lib.avt_resize_u8_tables(45, 32, 1, 11, None, b.ctypes.data) == AVT_ERR_ARG
    with pytest.raises(avt._lib.AvtError):
        avt.ops.resize_u8_tables(45, 0, 1)


def test_resize_refuses_host_tensors(avt):
    import torch
    with pytest.raises(avt._lib.AvtError):
        avt.ops.resize_u8(torch.zeros((1, 45, 70, 3), dtype=torch.uint8), (32, 64), "lanczos")
