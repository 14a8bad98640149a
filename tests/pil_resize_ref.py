"""Pillow's 8-bit `Image.resize` (filters BILINEAR and LANCZOS, mode RGB) restated in NumPy: the coefficient tables of
precompute_coeffs / normalize_coeffs_8bpc and the two integer passes of ImagingResampleHorizontal_8bpc / ...Vertical_8bpc
(libImaging/Resample.c).  tests/test_pil_resize_host.py holds it equal to live Pillow and to the committed fixture bit for bit;
the GPU tests and the C ABI's host tables (avt_resize_u8_tables) are then compared with it.  `math.sin` is libm's sin, the call
Pillow makes (NumPy's vectorised sin may round differently)."""
import math

import numpy as np

BILINEAR, LANCZOS = 0, 1      # include/avt.h AVT_RESIZE_*
PRECISION_BITS = 32 - 8 - 2

# (name, (H, W) in, (h, w) out): the small cases of tests/golden/pil_resize.npz — Lanczos down, then bilinear back up from the result
CASES = [("both_odd_bytes", (45, 70), (32, 64)),   # both passes, 210-byte rows
         ("taps11", (33, 95), (32, 64)),           # 11 horizontal taps, 285-byte rows
         ("vertical_only", (45, 64), (32, 64)),
         ("horizontal_only", (32, 70), (32, 64)),
         ("wide_clipped", (100, 37), (96, 32)),    # 37 -> 32: edge outputs with clipped bounds
         ("square", (63, 63), (32, 32))]
UP_BATCH = 4                                       # the SF - 1 frames that go back up, 32 x 64 -> 45 x 70


def _bilinear(x):
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def tables(in_size, out_size, filt):
    """-> (k int32 [out, ksize], bounds int32 [out, 2] = (first tap, taps)) of one axis."""
    f, fsupport = (_lanczos, 3.0) if filt == LANCZOS else (_bilinear, 1.0)
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = fsupport * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fscale
    k, bounds = np.zeros((out_size, ksize), np.int32), np.zeros((out_size, 2), np.int32)
    for i in range(out_size):
        center = (i + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - first
        w = [f((x + first - center + 0.5) * ss) for x in range(n)]
        total = 0.0
        for v in w:
            total += v
        for x, v in enumerate(w):
            if total != 0.0:
                v = v / total
            k[i, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[i] = first, n
    return k, bounds


def _pass(img, k, bounds, axis):
    """One pass along `axis` of a uint8 [..., H, W, 3] array."""
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((k.shape[0],) + src.shape[1:], np.uint8)
    for i in range(k.shape[0]):
        first, n = bounds[i]
        acc = np.tensordot(k[i, :n], src[first:first + n], axes=(0, 0)).astype(np.int32) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, size, filt):
    """uint8 [..., H, W, 3] -> uint8 [..., h, w, 3], size = (h, w): horizontal pass, then vertical; an unchanged axis is skipped."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    assert img.ndim >= 3 and img.shape[-1] == 3
    h, w = size
    if w != img.shape[-2]:
        img = _pass(img, *tables(img.shape[-2], w, filt), axis=img.ndim - 2)
    if h != img.shape[-3]:
        img = _pass(img, *tables(img.shape[-3], h, filt), axis=img.ndim - 3)
    return img.copy()


def noisy_frames(seed, shape):
    """Random bytes with a third of the rows (the middle third) set to 0 / 255 noise: Lanczos overshoots there, both ends of the clamp are hit."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=shape, dtype=np.uint8)
    h = shape[-3]
    x[..., h // 3:h // 3 + max(h // 3, 1), :, :] = rng.integers(0, 2, size=x[..., h // 3:h // 3 + max(h // 3, 1), :, :].shape, dtype=np.uint8) * 255
    return x


def pil_resize(img, size, filt):
    """The oracle itself: Image.resize frame by frame."""
    from PIL import Image
    flt = Image.LANCZOS if filt == LANCZOS else Image.BILINEAR
    flat = img.reshape((-1,) + img.shape[-3:])
    out = np.stack([np.array(Image.fromarray(f).resize((size[1], size[0]), flt)) for f in flat])
    return out.reshape(img.shape[:-3] + out.shape[1:])
