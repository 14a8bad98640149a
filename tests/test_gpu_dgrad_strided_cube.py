"""The stride-(2,2,2) input gradients of the 3D-ResNets' training step (train_ops._dgrad_strided: 8 residue classes, odd extents on a
grid rounded up to even extents and cropped) against torch's fp32 Conv3d through autograd, layer by layer: the form and the bounds of
test_gpu_train_conv.test_conv_forward_and_gradients_match_fp32_autograd, on the shapes layers 2-4 meet at W = 20 (T = 10, 5, 3) and on
odd H / W.  No case may fall back to MIOpen's bwd_data."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last_3d)


@pytest.mark.parametrize("cin,cout,kernel,pad,dims", [
    (64, 128, (3, 3, 3), (1, 1, 1), (2, 10, 16, 16)),   # layer2 conv1 at 64^2: every extent even
    (64, 128, (1, 1, 1), (0, 0, 0), (2, 10, 16, 16)),   # layer2 projection: one class, seven of zeros
    (128, 256, (3, 3, 3), (1, 1, 1), (2, 5, 8, 8)),     # layer3: T = 5
    (128, 256, (1, 1, 1), (0, 0, 0), (2, 5, 8, 8)),
    (256, 512, (3, 3, 3), (1, 1, 1), (3, 3, 4, 4)),     # layer4: T = 3
    (256, 512, (1, 1, 1), (0, 0, 0), (3, 3, 4, 4)),
    (16, 32, (3, 3, 3), (1, 1, 1), (2, 5, 7, 9)),       # every extent odd
    (16, 32, (1, 1, 1), (0, 0, 0), (1, 3, 9, 7)),
    (8, 16, (3, 3, 3), (1, 1, 1), (1, 1, 5, 6)),        # one frame
    (64, 128, (3, 3, 3), (1, 1, 1), (1, 5, 14, 14)),    # layer3's input at 224^2
])
def test_cube_strided_input_gradient_matches_fp32_autograd(cin, cout, kernel, pad, dims):
    from avtex import train_ops
    torch.manual_seed(cin + cout + dims[1])
    b, t, h, w = dims
    conv = nn.Conv3d(cin, cout, kernel, stride=2, padding=pad, bias=False).to(DEV).to(memory_format=torch.channels_last_3d).train()
    x0 = _cl(torch.randn(b, cin, t, h, w, device=DEV))
    assert train_ops.conv_fusable(x0, conv)

    def run(fused):
        conv.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = train_ops.conv3d(x, conv) if fused else conv(x)
        gy = _cl(torch.randn(y.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(7)))
        y.backward(gy)
        return y.detach(), x.grad, conv.weight.grad.clone()

    before = dict(train_ops.CALLS)
    ya, dxa, dwa = run(True)
    assert train_ops.CALLS["miopen_dgrad"] == before["miopen_dgrad"]
    assert train_ops.CALLS["dgrad_strided_x3"] == before["dgrad_strided_x3"] + 1
    ye, dxe, dwe = run(False)
    rel = lambda u, v: float((u - v).norm()) / (float(v.norm()) + 1e-30)
    assert ya.shape == ye.shape and dxa.shape == dxe.shape == x0.shape
    assert dxa.is_contiguous(memory_format=torch.channels_last_3d)
    print("conv %s stride 2 on %s: fwd %.2e dx %.2e dw %.2e" % ((cin, cout, kernel), dims, rel(ya, ye), rel(dxa, dxe), rel(dwa, dwe)))
    assert rel(ya, ye) < 2e-6, rel(ya, ye)
    assert rel(dxa, dxe) < 2e-5, rel(dxa, dxe)
    assert rel(dwa, dwe) < 1e-4, rel(dwa, dwe)
    if kernel == (1, 1, 1):  # the positions no tap reaches are exact zeros
        mask = torch.ones_like(dxa, dtype=torch.bool)
        mask[:, :, ::2, ::2, ::2] = False
        assert float(dxa[mask].abs().max()) == 0.0
