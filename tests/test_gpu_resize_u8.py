"""ops.resize_u8 (csrc/resize_u8.hip) against Pillow's `Image.resize`, bit for bit: the committed fixture (tests/golden/pil_resize.npz,
written from Pillow by tools/gen_pil_resize_golden.py), the NumPy restatement that test_pil_resize_host.py holds equal to Pillow, and
Pillow itself where it can be imported.  Inputs are random bytes with a block of 0 / 255 rows, where Lanczos overshoots into the clamp."""
import os

import numpy as np
import pytest
import torch

import pil_resize_ref as ref

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "pil_resize.npz"))
DEV = "cuda:0"
FILTER = {ref.LANCZOS: "lanczos", ref.BILINEAR: "bilinear"}


def _resize(x, size, filt):
    """x uint8 numpy [H, W, 3] or [B, H, W, 3] -> what the device gives, as numpy, same rank"""
    from avtex import ops
    t = torch.from_numpy(x).to(DEV)
    out = ops.resize_u8(t if t.dim() == 4 else t[None], size, FILTER[filt])
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and out.is_contiguous()
    out = out.cpu().numpy()
    return out if x.ndim == 4 else out[0]


def _equals_pillow_if_importable(got, x, size, filt):
    try:
        import PIL  # noqa: F401
    except ImportError:
        return
    assert np.array_equal(got, ref.pil_resize(x, size, filt))


# both_odd_bytes: both passes, 210-byte rows; taps11: 11 horizontal taps; vertical_only / horizontal_only: one launch;
# wide_clipped: clipped bounds at both edges, 111-byte rows on the way up; square: scale 1.97, 13 taps on both axes
@pytest.mark.parametrize("name,big,small", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_lanczos_down_equals_pillow(dev, name, big, small):
    x = GOLD[name + "_in"]
    got = _resize(x, small, ref.LANCZOS)
    assert got.shape == small + (3,) and np.array_equal(got, GOLD[name + "_down"])
    assert got.min() == 0 and got.max() == 255
    _equals_pillow_if_importable(got, x, small, ref.LANCZOS)


@pytest.mark.parametrize("name,big,small", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_bilinear_up_equals_pillow(dev, name, big, small):
    x = GOLD[name + "_down"]
    got = _resize(x, big, ref.BILINEAR)
    assert got.shape == big + (3,) and np.array_equal(got, GOLD[name + "_up"])
    _equals_pillow_if_importable(got, x, big, ref.BILINEAR)


def test_bilinear_up_of_a_batch_of_four(dev):
    """The SF - 1 frames of a jump, 32 x 64 -> 45 x 70 in one call."""
    batch = np.stack([GOLD[c[0] + "_down"] for c in ref.CASES if c[2] == (32, 64)][:ref.UP_BATCH])
    got = _resize(batch, (45, 70), ref.BILINEAR)
    assert got.shape == (4, 45, 70, 3) and np.array_equal(got, GOLD["up4"])
    _equals_pillow_if_importable(got, batch, (45, 70), ref.BILINEAR)


def test_lanczos_down_of_a_batch_of_two(dev):
    """The two frames of a jump in one call: each equals its own single-frame result."""
    a, b = GOLD["both_odd_bytes_in"], GOLD["both_odd_bytes_in"][::-1, ::-1].copy()
    got = _resize(np.stack((a, b)), (32, 64), ref.LANCZOS)
    assert np.array_equal(got[0], GOLD["both_odd_bytes_down"]) and np.array_equal(got[1], ref.resize(b, (32, 64), ref.LANCZOS))


def test_same_size_is_a_copy(dev):
    from avtex import ops
    x = torch.from_numpy(GOLD["both_odd_bytes_in"]).to(DEV)[None]
    y = ops.resize_u8(x, (45, 70), "lanczos")
    assert y.data_ptr() != x.data_ptr() and torch.equal(x, y)


def test_real_extent_down_and_back(dev):
    """360 x 640 -> 352 x 640 (only the vertical pass runs, 1920-byte rows) and back."""
    x = ref.noisy_frames(5, (360, 640, 3))
    down = _resize(x, (352, 640), ref.LANCZOS)
    assert np.array_equal(down, ref.resize(x, (352, 640), ref.LANCZOS))
    _equals_pillow_if_importable(down, x, (352, 640), ref.LANCZOS)
    up = _resize(down, (360, 640), ref.BILINEAR)
    assert np.array_equal(up, ref.resize(down, (360, 640), ref.BILINEAR))
    _equals_pillow_if_importable(up, down, (360, 640), ref.BILINEAR)


@pytest.mark.parametrize("filt", [ref.LANCZOS, ref.BILINEAR], ids=["lanczos", "bilinear"])
def test_rows_wider_than_one_block(dev, filt):
    """40 x 700 <-> 32 x 690: 6 blocks of output pixels per row in the horizontal pass; 2070- and 2100-byte rows are 130 and 132 16-byte
    chunks in the vertical pass, more than one block's 128, the last one a 6- / 4-byte tail."""
    x = ref.noisy_frames(11, (2, 40, 700, 3))
    down = _resize(x, (32, 690), filt)
    assert np.array_equal(down, ref.resize(x, (32, 690), filt))
    _equals_pillow_if_importable(down, x, (32, 690), filt)
    up = _resize(down, (40, 700), filt)
    assert np.array_equal(up, ref.resize(down, (40, 700), filt))


def test_what_the_kernel_cannot_do_is_refused(dev):
    from avtex import ops
    from avtex._lib import AvtError
    ok = torch.zeros((1, 45, 70, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(AvtError, match="3 channels"):
        ops.resize_u8(torch.zeros((1, 45, 70, 4), dtype=torch.uint8, device=DEV), (32, 64), "lanczos")
    with pytest.raises(AvtError, match="device"):
        ops.resize_u8(ok.cpu(), (32, 64), "lanczos")
    for size in ((0, 64), (32, 0), (0, 0)):
        with pytest.raises(AvtError):
            ops.resize_u8(ok, size, "lanczos")
    with pytest.raises(AvtError):
        ops.resize_u8(torch.zeros((1, 0, 70, 3), dtype=torch.uint8, device=DEV), (32, 64), "lanczos")
    with pytest.raises(AvtError):
        ops.resize_u8(ok.float(), (32, 64), "lanczos")
    with pytest.raises(AvtError):
        ops.resize_u8(ok[0], (32, 64), "lanczos")
    with pytest.raises(AvtError):
        ops.resize_u8(ok, (32, 64), "nearest")
    torch.cuda.synchronize()
