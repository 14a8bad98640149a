"""The training MaxPool3d(3, stride 2, padding 1) pair on fp32 NDHWC rows (csrc/stem_train.hip: avt_maxpool3d_train_fwd / _bwd, the
3D-ResNet stems' pool under train_ops.max_pool3d) against torch's own max_pool3d on the same channels-last tensor: values bit for
bit, NaN in exactly torch's windows, and the gradient bit for bit with integer-valued dy (sums of up to 8 terms are exact in any
order) — which pins the tie rule on post-ReLU inputs full of exact zeros."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(2, 20, 112, 112, 64),  # the production stem output of a clip pair
          (3, 5, 7, 9, 8),        # odd extents
          (1, 1, 4, 4, 4)]        # one frame
SENTINEL = -12345.0


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _run_pair(avt, x, dy):
    """x, dy: [b, c, t, h, w] channels_last_3d fp32 on the device -> (y, tap, dx) of the HIP pair; dx starts as a sentinel."""
    lib = avt._lib.lib()
    b, c, t, h, w = x.shape
    y = torch.empty(dy.shape, dtype=torch.float32, device=x.device, memory_format=torch.channels_last_3d)
    tap = torch.full((y.numel(),), 255, dtype=torch.uint8, device=x.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    avt._lib.check(lib.avt_maxpool3d_train_fwd(_ptr(x), _ptr(y), _ptr(tap), b, t, h, w, c, 0, stream), "avt_maxpool3d_train_fwd")
    dx = torch.full(x.shape, SENTINEL, dtype=torch.float32, device=x.device).contiguous(memory_format=torch.channels_last_3d)
    avt._lib.check(lib.avt_maxpool3d_train_bwd(_ptr(dy), _ptr(tap), _ptr(dx), b, t, h, w, c, 0, stream), "avt_maxpool3d_train_bwd")
    torch.cuda.synchronize()
    return y, tap, dx


def _inputs(shape, kind, dev):
    b, t, h, w, c = shape
    g = torch.Generator().manual_seed(11 + t * h)
    x = torch.randn((b, c, t, h, w), generator=g)
    if kind == "relu":
        x = torch.relu(x)  # half the values are exact zeros: windows tie all the time
    x = x.to(dev).contiguous(memory_format=torch.channels_last_3d)
    to, ho, wo = (t - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dy = torch.randint(-4, 5, (b, c, to, ho, wo), generator=g).float().to(dev).contiguous(memory_format=torch.channels_last_3d)
    return x, dy


@pytest.mark.parametrize("kind", ["randn", "relu"])
@pytest.mark.parametrize("shape", SHAPES)
def test_pair_is_bit_equal_to_torch(avt, dev, shape, kind):
    x, dy = _inputs(shape, kind, dev)
    y, tap, dx = _run_pair(avt, x, dy)
    xr = x.detach().clone().requires_grad_(True)
    ref = F.max_pool3d(xr, 3, 2, 1)
    assert ref.shape == y.shape  # (n - 1) / 2 + 1 per axis
    assert torch.equal(y, ref.detach())
    assert int(tap.max()) <= 26
    ref.backward(dy)
    assert not bool((dx == SENTINEL).any())  # dx is fully written: no memset needed
    assert torch.equal(dx, xr.grad)


@pytest.mark.parametrize("shape", SHAPES)
def test_nan_lands_in_torchs_windows(avt, dev, shape):
    x, dy = _inputs(shape, "relu", dev)
    b, c, t, h, w = x.shape
    x[0, 1, t // 2, h // 2, w // 2] = float("nan")
    y, tap, dx = _run_pair(avt, x, dy)
    xr = x.detach().clone().requires_grad_(True)
    ref = F.max_pool3d(xr, 3, 2, 1)
    assert ref.isnan().any() and torch.equal(y.isnan(), ref.detach().isnan())
    fin = ~ref.detach().isnan()
    assert torch.equal(y[fin], ref.detach()[fin])
    assert int(tap.max()) <= 26
    ref.backward(dy)
    assert torch.equal(dx, xr.grad)


def test_train_ops_dispatch_and_autograd(avt, dev):
    """train_ops.max_pool3d: the HIP pair for the stem's pool in train mode (counted), the module for anything else; gradients through
    autograd equal torch's."""
    from avtex import train_ops

    pool = torch.nn.MaxPool3d(3, stride=2, padding=1).train()
    x, dy = _inputs((3, 5, 7, 9, 8), "relu", dev)
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    before = train_ops.CALLS["maxpool3d_hip"]
    y = train_ops.max_pool3d(a, pool)
    assert train_ops.CALLS["maxpool3d_hip"] == before + 1
    ref = pool(b)
    assert torch.equal(y, ref) and y.is_contiguous(memory_format=torch.channels_last_3d)
    y.backward(dy)
    ref.backward(dy)
    assert torch.equal(a.grad, b.grad)
    # not the stem's window / eval mode / no gradient: the module itself
    for other, inp in ((torch.nn.MaxPool3d(3, stride=2, padding=0).train(), a), (torch.nn.MaxPool3d(3, stride=2, padding=1).eval(), a),
                       (pool, x)):
        before = train_ops.CALLS["maxpool3d_hip"]
        assert torch.equal(train_ops.max_pool3d(inp, other), other(inp))
        assert train_ops.CALLS["maxpool3d_hip"] == before
