"""Host side of the 3D-ResNet encoders on the split-plane kernels (fused_resnet3d): the layer plan against the module's own shapes,
the batch cap, and the new pool entry in the C ABI.  No GPU."""
import re

import pytest
import torch

GRID = [(224, 20), (64, 8), (48, 8), (112, 16), (96, 5), (40, 3), (256, 32), (72, 17)]


def _module_extents(avt, arch, hw, window):
    """Per-layer output extents of a CPU forward of the module (on the meta device: shapes only)."""
    with torch.device("meta"):
        net = avt.resnet3d.build(arch, hw, window).eval()
        x = torch.empty((1, 3, window, hw, hw))
    got = []
    hooks = [getattr(net, n).register_forward_hook(lambda m, i, o, n=n: got.append((n, tuple(o.shape[1:]))))
             for n in ("conv1", "maxpool")]
    for k in range(1, 5):
        for i, blk in enumerate(getattr(net, "layer%d" % k)):
            hooks.append(blk.register_forward_hook(lambda m, i_, o, n="layer%d.%d" % (k, i): got.append((n, tuple(o.shape[1:])))))
    with torch.no_grad():
        out = net(x)
    for h in hooks:
        h.remove()
    return got, tuple(net.avgpool.kernel_size), tuple(out.shape[1:])


@pytest.mark.parametrize("arch", ["resnet10", "resnet18", "resnet34", "resnet50"])
def test_layer_plan_matches_module_forward(avt, arch):
    from avtex.fused_resnet3d import layer_plan

    for hw, window in GRID:
        plan = layer_plan(arch, hw, window)
        got, kernel, out = _module_extents(avt, arch, hw, window)
        assert [(n, (c,) + e) for n, e, c in plan[:-1]] == got, (arch, hw, window)
        # the head: layer4's extent IS the module's AvgPool3d kernel, so its output is one position per channel
        assert plan[-1] == ("avgpool", kernel, 512) and plan[-2][1] == kernel and out == (512, 1, 1, 1), (arch, hw, window)


def test_plan_refuses_a_head_that_is_not_a_global_mean(avt):
    """A module built for another sample size has an AvgPool3d kernel smaller than layer4's extent: its head is not the mean over
    layer4's positions, and the encoder says so instead of computing something else."""
    from avtex.fused_resnet3d import ResNet3dMFMA

    torch.manual_seed(0)
    enc = ResNet3dMFMA(torch.nn.Sequential(avt.resnet3d.build("resnet10", 112, 8), torch.nn.AdaptiveAvgPool3d(1)), "cpu")
    assert enc.plan(112, 8)[-1] == ("avgpool", (1, 4, 4), 512)
    with pytest.raises(avt._lib.AvtError, match="AvgPool3d kernel"):
        enc.plan(224, 8)
    with pytest.raises(avt._lib.AvtError):
        ResNet3dMFMA(avt.resnet3d.build("resnet10", 112, 8), "cpu", precision="bf16")


def test_max_enc_batch_resnet3d(avt):
    from avtex.texture import max_enc_batch_resnet3d

    assert max_enc_batch_resnet3d(224, 20) == 133
    for hw, window in GRID:
        n = max_enc_batch_resnet3d(hw, window)
        h2 = -(-hw // 2)
        assert n * window * h2 * h2 * 64 < 2 ** 31 and (n + 1) * window * h2 * h2 * 64 >= 2 ** 31 - 64 or n == 1


def test_maxpool3d_entry_declared_and_bound(avt):
    src = re.sub(r"/\*.*?\*/", "", open(avt._lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"int avt_maxpool3d_k3s2_ndhwc_x3\(([^)]*)\);", src)
    assert m, "avt_maxpool3d_k3s2_ndhwc_x3 is not declared in include/avt.h"
    n_args = len(m.group(1).split(","))
    assert len(avt._lib.SIGNATURES["avt_maxpool3d_k3s2_ndhwc_x3"]) == n_args == 13
    assert hasattr(avt._lib.lib(), "avt_maxpool3d_k3s2_ndhwc_x3")
