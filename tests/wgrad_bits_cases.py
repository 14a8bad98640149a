"""The cases of tests/test_gpu_wgrad_bits.py and tools/record_wgrad_bits.py: the weight-gradient entries of csrc/wgrad_x3.hip (and the
patch-resident stems' deterministic entry, which shares wgrad_reduce with them) on inputs built on the host, dW hashed byte for byte.

Why an ATOMIC result can be hashed: dW is zeroed and every chunk adds one partial tile into it, so with at most two chunks an element
is 0 + a + b, and fp32 addition is commutative.  pick_chunks never returns more than nslab / min_slabs chunks — ceil(M / 64) / 16 for
the phase-serial tile, ceil(M / 32) / 32 for the pipelined one — so M = B * To * Ho * Wo <= 3008 keeps every case at two chunks or
fewer; the pipelined tile also refuses M < 2048.  Both are asserted below for every case, on the host.  The deterministic entries fix
their order by construction and take any M."""
import hashlib
import zlib

import numpy as np

DEV = "cuda:0"
MAX_M, XL_MIN_M = 3008, 2048
S1, P0, P011 = (1, 1, 1), (0, 0, 0), (0, 1, 1)

# name: cin, cout, kernel, stride, pad, x dims (B, T, H, W) — the smallest shapes that reach each instantiation and ragged edge
SERIAL = {  # the phase-serial tile (set_xl(0)), with buffer loads and without; the same cases go through the deterministic entry
    "bn64-ragged-27-taps": (24, 40, (3, 3, 3), (1, 2, 2), (1, 1, 1), (2, 3, 29, 31)),
    "bn128-several-r-tiles": (64, 136, (1, 3, 3), S1, P011, (2, 3, 21, 19)),
    "bn32": (8, 8, (1, 3, 3), S1, P011, (2, 3, 20, 21)),
    "swapped-bn128-pointwise": (136, 264, (1, 1, 1), S1, P0, (1, 2, 33, 35)),
    "swapped-bn64": (16, 136, (3, 1, 1), S1, (1, 0, 0), (2, 6, 14, 15)),
    "swapped-bn32": (8, 32, (1, 1, 1), S1, P0, (2, 3, 20, 21)),
    "temporal-stride": (8, 16, (7, 1, 1), (4, 1, 1), (3, 0, 0), (1, 32, 9, 9)),
    "less-than-one-slab": (16, 8, (1, 1, 1), S1, P0, (1, 1, 5, 7)),
}
PIPELINED = {  # the pipelined tile at the S width that fits (set_xl(2))
    "sw128": (64, 136, (1, 3, 3), S1, P011, (2, 3, 21, 19)),
    "swapped-sw128": (264, 520, (1, 1, 1), S1, P0, (3, 2, 20, 20)),
    "sw64": (64, 64, (1, 3, 3), S1, P011, (2, 3, 21, 19)),
    "swapped-sw64": (64, 256, (1, 1, 1), S1, P0, (2, 2, 25, 25)),
    "sw32": (8, 8, (1, 3, 3), S1, P011, (2, 3, 20, 21)),
    "swapped-sw32": (8, 32, (1, 1, 1), S1, P0, (2, 3, 20, 21)),
    "strided-odd-extents": (136, 256, (1, 3, 3), (1, 2, 2), P011, (2, 2, 51, 53)),
    "27-taps": (16, 48, (3, 3, 3), S1, (1, 1, 1), (1, 5, 21, 23)),
}
# the stems' sub-problem as train_ops._conv_wgrad issues it: cin 4 inside 8-channel rows, kt slices of [1,7,7] (49 taps: the
# one-workgroup-per-CU LDS size), stride (1,2,2), explicit output extent, pt - dt per slice, ldw = kt * 49 * 4, accumulator zeroed by
# the caller.  name: cout, kt
STEM_SUB = {"stem-sub-cout64-kt1": (64, 1), "stem-sub-cout8-kt5": (8, 5)}
STEM_SUB_DIMS = (1, 4, 44, 46)
# the patch-resident stems' deterministic entry (csrc/stem_train.hip), shapes of tests/test_gpu_wgrad_deterministic.py.  name: kt, cout, clip
STEM_PATCH = {"stem-patch-fast": (5, 8, (2, 8, 64, 64)), "stem-patch-slow": (1, 64, (2, 3, 64, 64))}


def out_dims(kernel, stride, pad, dims):
    return tuple((n + 2 * p - k) // s + 1 for n, k, s, p in zip(dims[1:], kernel, stride, pad))


def positions(kernel, stride, pad, dims):
    to, ho, wo = out_dims(kernel, stride, pad, dims)
    return dims[0] * to * ho * wo


for _c in SERIAL.values():
    assert positions(*_c[2:]) <= MAX_M, _c
for _c in PIPELINED.values():
    assert XL_MIN_M <= positions(*_c[2:]) <= MAX_M, _c
assert positions((1, 7, 7), (1, 2, 2), (0, 3, 3), STEM_SUB_DIMS) <= MAX_M  # (every slice has the whole filter's output extent)

KEYS = (["serial/%s/buf%d" % (n, b) for n in SERIAL for b in (1, 0)] + ["serial/%s/buf%d" % (n, b) for n in STEM_SUB for b in (1, 0)] +
        ["pipelined/%s" % n for n in PIPELINED] +
        ["det/%s/buf%d" % (n, b) for n in list(SERIAL) + list(STEM_SUB) for b in (1, 0)] + ["det/%s" % n for n in STEM_PATCH])


def hashed(shape, salt):
    """fp32 in (-0.5, 0.5) from integer arithmetic on the flat index (a multiplicative hash, its top 23 bits): the same bits on every
    commit and machine, whatever the device's random generator does."""
    n = int(np.prod(shape))
    k = ((np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(41)
    return ((k.astype(np.float64) + 0.5) / float(1 << 23) - 0.5).astype(np.float32).reshape(shape)


_INPUTS = {}


def _pair(name, x_shape, dy_shape):
    """(x, dy) of a case on the device: built once, shared by its settings, never written to."""
    import torch
    if name not in _INPUTS:
        salt = zlib.crc32(name.encode())
        _INPUTS[name] = tuple(torch.from_numpy(hashed(s, salt + i)).to(DEV) for i, s in enumerate((x_shape, dy_shape)))
    return _INPUTS[name]


def _conv(name, cases, det):
    import torch
    from avtex import ops
    cin, cout, kernel, stride, pad, dims = cases[name]
    x, dy = _pair(name, dims + (cin,), (dims[0],) + out_dims(kernel, stride, pad, dims) + (cout,))
    dw = torch.zeros(cout, kernel[0] * kernel[1] * kernel[2] * cin, device=DEV)
    if det:
        ops.conv3d_wgrad_x3_det_sub_f32(dy, x, dw, dims, cin, cout, kernel, stride, pad, (0, 0, 0), cin, cout, dw.shape[1])
    else:
        ops.conv3d_wgrad_x3_f32(dy, x, dw, dims, cin, cout, kernel, stride, pad, cin, cout)
    return dw


def _stem_sub(name, det):
    import torch
    from avtex import ops
    cout, kt = STEM_SUB[name]
    dims, stride, pad = STEM_SUB_DIMS, (1, 2, 2), (kt // 2, 3, 3)
    extent = out_dims((kt, 7, 7), stride, pad, dims)
    x, dy = _pair(name, dims + (8,), (dims[0],) + extent + (cout,))
    acc = torch.zeros(cout, kt, 49, 4, device=DEV)
    for dt in range(kt):
        args = (dy, x, acc[:, dt], dims, 4, cout, (1, 7, 7), stride, (pad[0] - dt, pad[1], pad[2]), extent, 8, cout, kt * 49 * 4)
        if det:
            ops.conv3d_wgrad_x3_det_sub_f32(*args)
        else:
            ops.conv3d_wgrad_x3_sub_f32(*args, False)
    return acc


def _stem_patch(name):
    from avtex import ops
    kt, cout, (b, t, h, w) = STEM_PATCH[name]
    x, dy = _pair(name, (b, 3, t, h, w), (b, t, h // 2, w // 2, cout))
    xh, xl = ops.clip_planes_f32(x, ops.X3_BF16)
    return ops.stem_wgrad_x3_det(xh, xl, dy, b, t, h, w // 2, cout, kt, kt // 2)


def digest(key):
    """SHA-256 of dW's bytes for one key of KEYS; the tile switches are back at their defaults afterwards."""
    import torch
    from avtex import _lib
    family, name, buf = (key.split("/") + [""])[:3]
    set_xl = _lib.lib().avt_wgrad_x3_set_xl
    try:
        if name in STEM_PATCH:
            dw = _stem_patch(name)
        else:
            set_xl(2 if family == "pipelined" else 0)
            set_xl(5 if buf == "buf0" else 6)
            if name in STEM_SUB:
                dw = _stem_sub(name, family == "det")
            else:
                dw = _conv(name, PIPELINED if family == "pipelined" else SERIAL, family == "det")
        torch.cuda.synchronize()
    finally:
        set_xl(1)
        set_xl(6)
    return hashlib.sha256(dw.contiguous().cpu().numpy().tobytes()).hexdigest()
