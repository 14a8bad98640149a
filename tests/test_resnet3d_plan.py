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


def _fused(avt, case, x3):
    from avtex.fused_slowfast import FusedConv

    conv = torch.nn.Conv3d(case.cin, case.cout, case.kernel, stride=case.stride, padding=case.pad, bias=False)
    return FusedConv(conv, torch.nn.BatchNorm3d(case.cout).eval(), case.relu, "cpu", x3=x3)


def test_resnet3d_shape_cases_name_their_paths(avt):
    """Every case of tests/resnet3d_cases.py lands on the kernel it names (the host dispatcher rule, both plane types): a later
    dispatcher change fails here before the GPU comparison quietly tests another path."""
    from resnet3d_cases import CASES, bare_symbol, m_out

    assert len({c.name for c in CASES}) == len(CASES)
    for case in CASES:
        for x3 in (avt.ops.X3_BF16, avt.ops.X3_F16):
            fc = _fused(avt, case, x3)
            assert bare_symbol(fc.kernel_symbol(m_out(case))) == case.symbol, case.name
            assert fc.pw is None and fc.lat is None, case.name
            if case.blocked is not None:
                assert (fc.wblk is not None) == case.blocked, case.name


@pytest.mark.parametrize("arch", ["resnet10", "resnet18", "resnet34"])
def test_resnet3d_shape_cases_cover_every_encoder_path(avt, arch):
    """Every path class (kernel symbol, kernel, stride, tap table in global memory, K % 32 == 0) a ResNet3dMFMA convolution runs
    at these sizes, at batch 1 and at the batch cap, has a case in tests/resnet3d_cases.py (the float64 comparison on the GPU)."""
    from avtex.fused_resnet3d import ResNet3dMFMA
    from avtex.texture import max_enc_batch_resnet3d
    from resnet3d_cases import CASES, case_class, path_class

    pinned = {case_class(c) for c in CASES}
    seen = set()
    for hw, window in [(224, 20), (64, 8), (48, 8), (112, 16)]:
        torch.manual_seed(0)
        enc = ResNet3dMFMA(torch.nn.Sequential(avt.resnet3d.build(arch, hw, window), torch.nn.AdaptiveAvgPool3d(1)), "cpu")
        blocks = [p for p in enc.plan(hw, window) if p[0].startswith("layer")]
        assert len(blocks) == len(enc.blocks)
        for batch in (1, max_enc_batch_resnet3d(hw, window)):
            for (name, (t, h, w), _), convs in zip(blocks, enc.blocks):
                for fc in convs:
                    if fc is None:
                        continue
                    cls = path_class(fc.kernel_symbol(batch * t * h * w), fc.cin, fc.kernel, fc.stride)
                    assert cls in pinned, "%s %d^2 W=%d batch %d %s: path %s has no case" % (arch, hw, window, batch, name, cls)
                    seen.add(cls)
    # the production batch reaches the XL tile (layer3 at 224^2, layer4.0's downsample at 48^2) and the global tap table
    assert any(c[0] == "conv_x3_xl_kernel" and c[1] == (1, 1, 1) for c in seen)
    assert any(c[0] == "conv_x3_xl_kernel" and c[2] == (2, 2, 2) and c[1] == (3, 3, 3) for c in seen)
    assert any(c[3] for c in seen)
